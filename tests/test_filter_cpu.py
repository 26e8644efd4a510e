"""The filter's weights without a device: the host harness of the index arithmetic and the per-pixel function
(tests/helpers/filter_host.cpp, a stand-alone program, plain and sanitized), the numpy restatement of the definition
(tests/helpers/filter_ref.py) against observation.filter_weights and its longdouble twin, and the refusals of
observation.Detrend(on_device=True) and Transit.recover that come before a device is needed."""
import os
import subprocess

import numpy as np
import pytest

from helpers import filter_ref as fref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "prometheus_amd", "csrc")
HOST = os.path.join(REPO, "tests", "helpers", "filter_host.cpp")


# ---- the harness -------------------------------------------------------------------------------------------------
def edge_case(n_exp, K, n_pix, seed=3):
    """(U, ivar) with, where the shape has room, a pixel without weight, one with exactly K and one with K - 1
    weighted exposures, and ivar entries that are NaN, +inf, negative and -0."""
    rng = np.random.default_rng(seed + 100 * n_exp + 10 * K + n_pix)
    U = rng.normal(size=(n_exp, K))
    iv = rng.uniform(0.5, 2.0, (n_exp, n_pix))
    iv[rng.random((n_exp, n_pix)) < 0.1] = 0.0
    iv[:, 0] = 0.0
    if n_pix > 2 and n_exp >= K:
        iv[:, 1] = 0.0
        iv[rng.permutation(n_exp)[:K], 1] = 1.5
        iv[:, 2] = 0.0
        iv[rng.permutation(n_exp)[:K - 1], 2] = 0.75
    if n_pix > 7:
        for p, v in ((3, np.nan), (4, np.inf), (5, -1.0), (6, -0.0)):
            iv[n_exp // 2, p] = v
    return U, iv


def _columns_file(path, U, iv):
    W = fref.weights_f64(U, iv)
    vals = lambda a: " ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel())
    with open(path, "w") as f:
        f.write("%d %d %d\n%s\n%s\n%s\n" % (U.shape[0], U.shape[1], iv.shape[1], vals(U), vals(iv), vals(W)))
    return W


def _column_cases():
    cases = [("edge_%d_%d" % (n_exp, K), *edge_case(n_exp, K, 9)) for n_exp, K in ((1, 1), (2, 2), (7, 6), (70, 11),
                                                                                    (70, 16), (7, 11))]
    U, iv = edge_case(12, 4, 9)
    Uz = U.copy()
    Uz[:, 2] = 0.0
    cases.append(("zero_column", Uz, iv))
    Ud = U.copy()
    Ud[:, 3] = Ud[:, 1]
    cases.append(("duplicated_column", Ud, iv))
    Uh = U.copy()
    Uh[:, 0] *= 1e200                                            # N_00 overflows: the pixel is singular
    cases.append(("overflow", Uh, iv))
    return cases


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_harness_walks_every_index_and_matches_the_reference_bitwise(tmp_path, which):
    """The walk over 5 x 4 x 5 shapes (one lane, a wave's edge, the tail of the last wave, two waves; K from 1 to 16)
    finds every index inside, every W entry written exactly once and no thread past n_pix at work, and fw_weights
    itself stays inside arrays of exactly those lengths; on nine sets of columns it gives weights_f64's bits."""
    flags = {"plain": ("-O2",), "sanitized": ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")}
    exe = tmp_path / "filter_host"
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags[which], "-I" + CSRC, HOST, "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr)
    assert r.returncode == 0
    assert r.stdout.count("_oor=0") == 3 * 100 and r.stdout.count("visit_err=0 untouched=0") == 100
    for name, U, iv in _column_cases():
        path = tmp_path / (name + ".txt")
        W = _columns_file(path, U, iv)
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        print(name, r.stdout, r.stderr)
        assert r.returncode == 0 and "mismatches=0" in r.stdout, name
        if name in ("zero_column", "overflow") or name == "edge_7_11":       # (7 exposures cannot carry 11 components)
            assert not W.any() and not np.signbit(W).any()
        if name.startswith("edge") and name != "edge_7_11":
            assert W.any()


# ---- the definition ----------------------------------------------------------------------------------------------
def test_the_definition_agrees_with_filter_weights_and_with_its_longdouble_twin():
    """On the four prototype designs the definition zeroes the pixels observation.filter_weights zeroes (the planted
    ones without weight, with K - 1 and with fewer weighted exposures) and no others.  On the regular pixels both
    stand within cond(N_p) (2 n_exp + K^2) u max|W_p| of the longdouble evaluation, the bound test_detrend_cpu.py
    uses for filter_weights: N_p and U^T L_p are sums of n_exp products (relative error n_exp u each in magnitude,
    which the inverse carries over at cond(N_p)), and a Cholesky or LU solve is backward stable to about K^2 u
    cond(N_p).  A wrong pivot, order or skipped exposure errs at order 1.  The fractions of the bound and the errors
    in units of u max|W_p| are printed."""
    from prometheus_amd import observation as obs
    u = 2.0 ** -53
    for (n_exp, K, n_pix), (U, iv) in zip(fref.DESIGNS, fref.designs()):
        W = fref.weights_f64(U, iv)
        Wh = obs.filter_weights(U, iv)
        Wl = fref.weights_ld(U, iv)
        reg = fref.regular_f64(U, iv)
        assert np.array_equal(reg, Wh.any(axis=(0, 1))) and np.array_equal(reg, (Wl != 0).any(axis=(0, 1)))
        assert not reg[:2].any() and reg[5:].all()
        assert np.all(W[:, iv == 0] == 0) and not np.signbit(W[:, iv == 0]).any()
        lam = np.linalg.eigvalsh(np.einsum("ei,ep,ej->pij", U, iv, U)[reg])
        bound = (lam[:, -1] / lam[:, 0]) * (2 * n_exp + K * K) * u
        scale = np.abs(Wl).max(axis=(0, 1))[reg].astype(np.float64)
        for name, X in (("definition", W), ("filter_weights", Wh)):
            d = (np.abs(X - Wl).max(axis=(0, 1))[reg] / scale).astype(np.float64)
            print("n_exp=%d K=%d n_pix=%d %s: %.1f u max|W_p|, %.3f of the bound" % (n_exp, K, n_pix, name, d.max() / u,
                                                                                 (d / bound).max()))
            assert np.all(d <= bound)


# ---- refusals that need no device --------------------------------------------------------------------------------
def test_detrend_on_device_and_recover_refuse_before_touching_a_device(monkeypatch):
    from prometheus_amd import _native
    from prometheus_amd import observation as obs
    from test_sysrem_cpu import _bare_transit

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_native, "get_device", no_device)
    monkeypatch.setattr(_native, "device_count", no_device)
    tr = _bare_transit(20000, 3)
    ins = obs.Instrument(tr.wavelength[[300, 100, 200]], resolving_power=140000.0)
    rows, a, F = np.array([[0, 1], [1, 2], [0, 2]]), np.full((3, 2), 0.5), np.ones((3, 4, 2))
    data, err = np.ones((3, 3)), np.full((3, 3), 1e-3)
    ex = obs.Exposures(ins, rows, a, F, data, err)
    other = obs.Exposures(ins, rows, a, F, data * 1.5, err)
    Ub = np.stack([np.ones(3), np.array([-1.0, 0.0, 1.0])], axis=1)
    # Detrend(on_device=True): no W on the host, a key of the exposures and U alone; the default is unchanged
    dt = obs.Detrend(ex, Ub, on_device=True)
    assert dt.W is None and dt.on_device and (dt.n_exp, dt.n_comp) == (3, 2) and dt.exposures_key == ex.key
    host = obs.Detrend(ex, Ub)
    assert not host.on_device and np.array_equal(host.W, obs.filter_weights(Ub, ex.ivar)) and host.key != dt.key
    assert host.key == obs.Detrend(ex, Ub, None, False).key
    assert obs.Detrend(ex, Ub.copy(), on_device=True).key == dt.key
    assert obs.Detrend(ex, Ub * (1 + 1e-15), on_device=True).key != dt.key
    assert obs.Detrend(other, Ub, on_device=True).key != dt.key
    with pytest.raises(ValueError, match="give no W"):
        obs.Detrend(ex, Ub, np.zeros((2, 3, 3)), on_device=True)
    for bad in (Ub[:2], Ub[:, :0], np.ones((3, 17)), np.where(Ub == 0.0, np.nan, Ub)):
        with pytest.raises(ValueError):
            obs.Detrend(ex, bad, on_device=True)
    with pytest.raises(ValueError, match="made for other exposures"):
        tr.expose(other, detrend=dt)
    # Transit.filter_weights
    with pytest.raises(TypeError):
        tr.filter_weights(ins, Ub)
    for bad in (Ub[:2], np.ones((3, 17)), np.where(Ub == 0.0, np.inf, Ub)):
        with pytest.raises(ValueError):
            tr.filter_weights(ex, bad)
    with pytest.raises(ValueError, match="one device"):
        tr.filter_weights(ex, Ub, devices=[0, 1])
    # Transit.recover: inject's and expose's checks
    inj = obs.Injection(ex, np.arange(9.0).reshape(3, 3))
    hp, od = obs.HighPass(ex, obs.box_taps(1)), obs.Orders(ex, None)
    with pytest.raises(TypeError, match="observation.Injection"):
        tr.recover(ex, 0)
    for kw, err_t in ((dict(trial=1.0), TypeError), (dict(trial=True), TypeError), (dict(trial=4), ValueError),
                      (dict(trial=-1), ValueError), (dict(scale="x"), TypeError), (dict(scale=np.inf), ValueError),
                      (dict(n_comp=0), ValueError), (dict(n_comp=16, ones=True), ValueError),
                      (dict(n_comp=2.0), TypeError), (dict(n_iter=0), ValueError), (dict(ones=1), TypeError),
                      (dict(highpass=Ub), TypeError), (dict(orders=Ub), TypeError), (dict(broaden=Ub), TypeError),
                      (dict(highpass=obs.HighPass(other, obs.box_taps(1))), ValueError),
                      (dict(orders=obs.Orders(other, None)), ValueError), (dict(devices=[0, 1]), ValueError),
                      (dict(max_memory_gb=1e-9), ValueError)):
        args = dict(trial=0, highpass=hp, orders=od)
        args.update(kw)
        with pytest.raises(err_t, match="recover"):
            tr.recover(inj, **args)
    rows_far = obs.Exposures(ins, rows + 5, a, F, data, err)
    with pytest.raises(ValueError, match="the transit has 3 phases"):
        tr.recover(obs.Injection(rows_far, np.ones((3, 3))), 0)
