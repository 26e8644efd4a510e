"""Detrended exposures without a device: the host harness of the index arithmetic and the column functions
(tests/helpers/detrend_host.cpp, a stand-alone program, plain and sanitized), observation.filter_weights and
observation.sysrem, the float64 reference of the filter (tests/helpers/detrend_ref.py) and its bound, and the refusals
of observation.Detrend and Transit.expose(detrend=...) that come before a device is needed."""
import os
import subprocess
import types

import numpy as np
import pytest

from helpers import detrend_ref as dref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "prometheus_amd", "csrc")
HOST = os.path.join(REPO, "tests", "helpers", "detrend_host.cpp")
U = 2.0 ** -53


# ---- the harness -------------------------------------------------------------------------------------------------
def _column_file(path, M, Ub, W):
    """One column (n_pix = 1) with filter_f64's answer, as hexadecimal floats."""
    out, ok = dref.filter_f64(M[:, None, None], Ub, W[:, :, None])
    vals = lambda a: " ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel())
    with open(path, "w") as f:
        f.write("%d %d\n%s\n%s\n%s\n%d\n%s\n" % (Ub.shape[0], Ub.shape[1], vals(M), vals(Ub), vals(W), int(ok[0, 0]),
                                               vals(out[:, 0, 0])))
    return out[:, 0, 0], bool(ok[0, 0])


def _column_cases(tmp_path):
    rng = np.random.default_rng(17)
    cases = []
    for i, (n_exp, n_comp) in enumerate([(1, 1), (5, 2), (7, 6), (9, 16)]):
        M = 1.0 - 0.01 * rng.random(n_exp)
        Ub = rng.normal(size=(n_exp, n_comp))
        W = rng.normal(size=(n_comp, n_exp))
        W[:, n_exp // 2] = 0.0                                    # an exposure no component reads
        W[0, 0] = 0.0
        cases.append(("plain%d" % i, M, Ub, W))
    n_exp, n_comp = 6, 3
    M = 1.0 - 0.01 * rng.random(n_exp)
    Ub, W = rng.normal(size=(n_exp, n_comp)), rng.normal(size=(n_comp, n_exp))
    W[:, 2] = 0.0
    Mp = M.copy()
    Mp[2] = np.nan                                                # NaN under W = 0: padding, the column stands
    cases.append(("padding", Mp, Ub, W))
    Mu = M.copy()
    Mu[4] = np.nan                                                # NaN under W != 0: not filterable
    cases.append(("unfilterable", Mu, Ub, W))
    cases.append(("zero basis", M, np.zeros((n_exp, n_comp)), W))
    files = []
    for name, M, Ub, W in cases:
        path = tmp_path / (name.replace(" ", "_") + ".txt")
        out, ok = _column_file(path, M, Ub, W)
        files.append((name, path, out, ok, M))
    return files


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_harness_walks_every_index_and_matches_the_reference_bitwise(tmp_path, which):
    """The walk over eight shapes (one and several tiles, chunks, trial groups and batches, n_comp 1 to 16) finds every
    index inside and every model value, flag and record written once; dt_coefficients / dt_apply give filter_f64's
    bits on seven columns, the padding rule, an unfilterable column and U = 0 among them."""
    flags = {"plain": ("-O2",), "sanitized": ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")}
    exe = tmp_path / "detrend_host"
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags[which], "-I" + CSRC, HOST, "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert r.stdout.count("_oor=0") == 6 * 8 and r.stdout.count("visit_err=0") == 8
    assert "batches=3" in r.stdout and "batches=2" in r.stdout and "batches=1" in r.stdout
    for name, path, out, ok, M in _column_cases(tmp_path):
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        print(name, r.stdout, r.stderr)
        assert r.returncode == 0 and "mismatches=0" in r.stdout, name
        if name == "padding":
            assert ok and np.isnan(out[2]) and np.isfinite(np.delete(out, 2)).all()
        if name == "unfilterable":
            assert not ok and np.isnan(out).all()
        if name == "zero basis":
            assert ok and np.array_equal(out, M)


# ---- filter_weights ----------------------------------------------------------------------------------------------
def _basis(n_exp, n_comp, seed=1):
    rng = np.random.default_rng(seed)
    Ub = rng.normal(size=(n_exp, n_comp))
    Ub[:, 0] = 1.0
    return Ub


def test_filter_weights_invert_the_basis():
    """W_p U = I within cond(N_p) (2 n_exp + n_comp^2) u: the normal matrix N_p and U^T L_p are sums of n_exp
    products (relative error n_exp u each in magnitude, which the inverse carries over at cond(N_p)), and the solve is
    backward stable to about n_comp^2 u cond(N_p)."""
    from prometheus_amd import observation as obs
    n_exp, n_comp, n_pix = 12, 4, 40
    Ub = _basis(n_exp, n_comp)
    ivar = 1e4 * (0.1 + np.random.default_rng(2).random((n_exp, n_pix)))
    ivar[3, 5] = 0.0
    ivar[7, 5] = 0.0
    ivar[:, 9] = 0.0                       # no weight at all: singular
    ivar[n_comp - 1:, 11] = 0.0            # n_comp - 1 weighted exposures: singular
    ivar[2, 13] = np.nan
    W = obs.filter_weights(Ub, ivar)
    assert W.shape == (n_comp, n_exp, n_pix) and np.isfinite(W).all()
    assert np.all(W[:, 3, 5] == 0) and np.all(W[:, 7, 5] == 0) and np.all(W[:, 2, 13] == 0)
    assert np.all(W[:, :, 9] == 0) and np.all(W[:, :, 11] == 0)
    worst = 0.0
    for p in range(n_pix):
        if p in (9, 11):
            continue
        iv = np.where(np.isfinite(ivar[:, p]), ivar[:, p], 0.0)
        N = (Ub.T * iv) @ Ub
        tol = np.linalg.cond(N) * (2 * n_exp + n_comp * n_comp) * U
        err = np.abs(W[:, :, p] @ Ub - np.eye(n_comp)).max()
        worst = max(worst, err / tol)
        assert np.any(W[:, :, p] != 0)
    print("filter_weights: W U - I at most %.3f of cond(N) (2 n_exp + n_comp^2) u" % worst)
    assert worst <= 1.0
    with pytest.raises(ValueError):
        obs.filter_weights(Ub, ivar[:5])
    with pytest.raises(ValueError):
        obs.filter_weights(np.where(Ub == 1.0, np.nan, Ub), ivar)


# ---- the reference -----------------------------------------------------------------------------------------------
def test_filter_annihilates_the_basis_and_keeps_the_model_when_the_basis_is_zero():
    """A column M = U x is what the basis spans: the filter leaves nothing of it within the bound of detrend_ref with
    eps_e = 0 (M is given exactly).  With U = 0 it returns M bit for bit."""
    from prometheus_amd import observation as obs
    n_exp, n_comp, n_pix, n_trial = 10, 3, 37, 4
    rng = np.random.default_rng(4)
    Ub = _basis(n_exp, n_comp, seed=3)
    ivar = 1e4 * (0.1 + rng.random((n_exp, n_pix)))
    ivar[4, 6] = 0.0
    W = obs.filter_weights(Ub, ivar)
    x = rng.normal(size=(n_comp, n_trial, n_pix))
    M = np.einsum("ek,kjp->ejp", Ub, x)
    out, ok = dref.filter_f64(M, Ub, W)
    assert ok.all()
    exact, _ = dref.filter_ld(M, Ub, W)
    bound = dref.model_bound(M, Ub, W, 0.0)
    # the longdouble filter of the float64 M = fl(U x) against zero: W_p U = I only within filter_weights' own error
    cond = max(np.linalg.cond((Ub.T * ivar[:, p]) @ Ub) for p in range(n_pix))
    slack = cond * (2 * n_exp + n_comp * n_comp) * U * np.abs(np.einsum("ek,kjp->ejp", np.abs(Ub), np.abs(x))).max()
    frac = dref.model_fraction(out, exact, bound)
    print("filter_f64 against filter_ld on M = U x: %.4f of the bound; |M'| <= %.3g (slack %.3g)"
          % (frac, np.abs(out).max(), slack))
    assert frac <= 1.0
    assert np.abs(out).max() <= bound.max() + slack and np.abs(out).max() < 1e-9 * np.abs(M).max()
    out0, ok0 = dref.filter_f64(M, np.zeros_like(Ub), W)
    assert ok0.all() and np.array_equal(out0, M)


def test_float64_orders_stay_far_below_the_bound():
    """filter_f64 forwards and with the exposures reversed against filter_ld: measured at 0.034 of the bound at most
    (the print), asserted below 0.1, so the bound of the GPU tests is not tight."""
    from prometheus_amd import observation as obs
    n_exp, n_comp, n_pix, n_trial = 24, 6, 50, 3
    rng = np.random.default_rng(8)
    Ub = _basis(n_exp, n_comp, seed=9)
    ivar = 1e4 * (0.1 + rng.random((n_exp, n_pix)))
    W = obs.filter_weights(Ub, ivar)
    M = 1.0 - 0.02 * rng.random((n_exp, n_trial, n_pix))
    exact, _ = dref.filter_ld(M, Ub, W)
    bound = dref.model_bound(M, Ub, W, 0.0)
    worst = 0.0
    for rev in (False, True):
        s = slice(None, None, -1) if rev else slice(None)
        out, _ = dref.filter_f64(M[s], Ub[s], W[:, s])
        worst = max(worst, dref.model_fraction(out[s], exact, bound))
    print("float64 orders: %.4f of the bound" % worst)
    assert worst < 0.1


# ---- sysrem ------------------------------------------------------------------------------------------------------
def test_sysrem_removes_planted_systematics_down_to_the_noise():
    """Two planted a[e] c[p] terms plus seeded noise: after two components the residual variance is the noise's.  A
    fit of K rank-one terms takes about K (n_exp + n_pix) degrees of freedom out of the n_exp n_pix noise values, so
    the residual variance lies between var(noise) (1 - 2 K (n_exp + n_pix) / (n_exp n_pix)) and var(noise) itself, up
    to the planted terms' own remainder, bounded here by 1 % of the noise."""
    from prometheus_amd import observation as obs
    n_exp, n_pix, K = 40, 300, 2
    rng = np.random.default_rng(5)
    noise = 1e-3 * rng.normal(size=(n_exp, n_pix))
    sysm = sum(0.05 / (i + 1) * rng.normal(size=n_exp)[:, None] * rng.normal(size=n_pix)[None, :] for i in range(K))
    data = sysm + noise
    Ub, clean = obs.sysrem(data, 1e-3, K)
    assert Ub.shape == (n_exp, K) and clean.shape == data.shape
    assert np.allclose((Ub * Ub).sum(axis=0), 1.0)
    v, vn = clean.var(), noise.var()
    lo = vn * (1.0 - 2.0 * K * (n_exp + n_pix) / (n_exp * n_pix))
    print("sysrem: residual variance %.4g, noise %.4g, lower margin %.4g; raw %.4g" % (v, vn, lo, data.var()))
    assert lo <= v <= 1.01 * vn and data.var() > 100 * vn
    # one component is not enough
    assert obs.sysrem(data, 1e-3, 1)[1].var() > 10 * vn
    # a leading column of ones on request, for a pixel-wise mean
    U1, clean1 = obs.sysrem(data + 1.0, 1e-3, K, ones=True)
    assert U1.shape == (n_exp, K + 1) and np.all(U1[:, 0] == 1.0) and clean1.var() <= 1.01 * vn
    # masked entries carry no weight and come back as they were
    d2 = data.copy()
    d2[3, 4] = np.nan
    U2, clean2 = obs.sysrem(d2, 1e-3, K)
    assert np.isnan(clean2[3, 4]) and np.isfinite(np.delete(clean2.ravel(), 3 * n_pix + 4)).all()
    assert np.isfinite(U2).all()
    with pytest.raises(ValueError):
        obs.sysrem(data[0], 1e-3, 1)
    with pytest.raises(ValueError):
        obs.sysrem(data, 1e-3, 0)


# ---- Detrend and Transit.expose(detrend=...) without a device ------------------------------------------------------
def _bare_transit(n_wav, n_orb):
    """A Transit with a grid and phases and nothing a device could run: expose must refuse before it needs one."""
    from prometheus_amd import gasProperties as gp
    tr = gp.Transit.__new__(gp.Transit)
    tr.wavelength = 5880e-8 + 1e-11 * np.arange(n_wav)
    tr.spatialGrid = types.SimpleNamespace(constructOrbphaseAxis=lambda: np.linspace(-0.03, 0.03, n_orb))
    tr.atmosphere = types.SimpleNamespace(densityDistributionList=[])
    tr.last_stats, tr.collect_stats = [], False
    return tr


def test_detrend_and_expose_refuse_before_touching_a_device(monkeypatch):
    from prometheus_amd import _native
    from prometheus_amd import observation as obs

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_native, "get_device", no_device)
    monkeypatch.setattr(_native, "device_count", no_device)
    tr = _bare_transit(20000, 3)
    ins = obs.Instrument(tr.wavelength[[300, 100, 200]], resolving_power=140000.0)
    rows, a, F = np.array([[0, 1], [1, 2], [0, 2]]), np.full((3, 2), 0.5), np.ones((3, 4, 2))
    data, err = np.ones((3, 3)), np.full((3, 3), 1e-3)
    err[1, 2] = np.nan
    ex = obs.Exposures(ins, rows, a, F, data, err)
    Ub = np.stack([np.ones(3), np.array([-1.0, 0.0, 1.0])], axis=1)
    dt = obs.Detrend(ex, Ub)
    assert (dt.n_exp, dt.n_comp) == (3, 2) and dt.W.shape == (2, 3, 3) and dt.exposures_key == ex.key
    assert np.array_equal(dt.W, obs.filter_weights(Ub, ex.ivar))
    # (the caller's pixel 2 is the device's pixel 1: its masked exposure carries W = 0, and the pixel, left with two
    # weighted exposures for two components, is still regular)
    assert np.all(dt.W[:, 1, ins.sort(np.arange(3.0)) == 2.0] == 0) and np.any(dt.W[:, 0] != 0)
    # W in the caller's order is sorted for the device
    Wc = np.arange(18.0).reshape(2, 3, 3)
    assert np.array_equal(obs.Detrend(ex, Ub, Wc).W, ins.sort(Wc))
    assert obs.Detrend(ex, Ub).key == dt.key and obs.Detrend(ex, Ub, Wc).key != dt.key
    assert obs.Detrend(ex, Ub * (1 + 1e-15)).key != dt.key
    for bad in (dict(U=Ub[:2]), dict(U=Ub[:, :0]), dict(U=np.ones((3, 17))), dict(U=Ub[:, 0]),
                dict(U=np.where(Ub == 0.0, np.nan, Ub)), dict(U=np.where(Ub == 0.0, np.inf, Ub)),
                dict(W=Wc[:1]), dict(W=Wc[:, :2]), dict(W=Wc[:, :, :2]), dict(W=np.where(Wc == 4.0, np.nan, Wc))):
        args = dict(U=Ub, W=None)
        args.update(bad)
        with pytest.raises(ValueError):
            obs.Detrend(ex, **args)
    with pytest.raises(TypeError):
        obs.Detrend(ins, Ub)
    with pytest.raises(TypeError, match="observation.Detrend"):
        tr.expose(ex, detrend=Ub)
    other = obs.Exposures(ins, rows, a, F, data * 1.5, err)
    with pytest.raises(ValueError, match="made for other exposures"):
        tr.expose(other, detrend=dt)
    with pytest.raises(ValueError, match="not additive over wavelength partials"):    # the plain refusals stand
        tr.expose(ex, detrend=dt, devices=[0, 1])
