"""Injection and SYSREM without a device: the host harness of prometheus_amd/csrc/sysrem_index.h (every index of the
kernels and the row shape's bits, plain and under sanitizers), the float64 reference of the definition
(tests/helpers/sysrem_ref.py) against observation.sysrem and its longdouble self, the accuracy designs' margin, the
planted planet in the all-numpy pipeline, and the refusals of observation.Injection, Transit.clean and Transit.inject
that come before a device is needed."""
import json
import os
import subprocess
import types

import numpy as np
import pytest

from helpers import expose_ref as eref
from helpers import sysrem_ref as sref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "prometheus_amd", "csrc")
HOST = os.path.join(REPO, "tests", "helpers", "sysrem_host.cpp")
T = sref.TILE
ACCURACY = [(7, T + 1, 1), (70, 3 * T + 5, 2), (70, T - 1, 3)]      # (n_exp, n_pix, seed) of the accuracy designs


def _hex(v):
    return " ".join("nan" if x != x else float(x).hex() for x in np.asarray(v, dtype=np.float64).ravel())


def _step_cases(tmp_path):
    """Files for sysrem_host <file>: shapes about the tile, NaN, infinities and ivar = 0 sprinkled in, a pixel and an
    exposure without any weight."""
    out = []
    for i, (n_exp, n_pix) in enumerate([(1, 1), (2, T - 1), (7, T), (7, T + 1), (5, 3 * T + 5), (3, 64 * T + 1)]):
        rng = np.random.default_rng(20 + i)
        D = 1.0 + 0.1 * rng.normal(size=(n_exp, n_pix))
        iv = 1e4 * (0.1 + rng.random((n_exp, n_pix)))
        if n_pix > 4:
            D[rng.random(D.shape) < 0.03] = np.nan
            D[rng.random(D.shape) < 0.01] = np.inf
            iv[rng.random(D.shape) < 0.03] = 0.0
            iv[rng.random(D.shape) < 0.01] = np.inf
            iv[:, 2] = 0.0
            iv[n_exp - 1, :] = -1.0 if n_exp > 2 else iv[n_exp - 1, :]
        a = rng.normal(size=n_exp)
        w, r = sref.weights_of(D, iv)
        c = sref.fit_c(w, r, a)
        a2 = sref.fit_a(w, r, c)
        norm = sref.norm_of(a2)
        r2 = np.where(w > 0, r - a[:, None] * c[None, :], r)
        path = tmp_path / ("step%d.txt" % i)
        path.write_text("%d %d\n%s\n%s\n%s\n%s\n%s\n%s\n%s\n" % (n_exp, n_pix, _hex(D), _hex(iv), _hex(a), _hex(c),
                                                                  _hex(a2), _hex([norm]), _hex(r2)))
        out.append(path)
    return out


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_harness_walks_every_index_and_matches_the_reference_bitwise(tmp_path, which):
    """The walk over n_pix in {1, T - 1, T, T + 1, 3 T + 5, 64 T + 1} x n_exp in {1, 2, 7, 70} finds every index of
    k_sysrem_prep, k_sysrem_step, k_sysrem_rows and k_sysrem_finish inside its buffer and every work entry, partial,
    a, U and cleaned entry written exactly once; the header's entry functions in the kernels' order give fit_c, fit_a,
    the norm and the residual of sysrem_ref bit for bit on six cases."""
    flags = {"plain": ("-O2",), "sanitized": ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")}
    exe = tmp_path / "sysrem_host"
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags[which], "-I" + CSRC, HOST, "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "shapes=24 tile=%d" % T in r.stdout
    assert r.stdout.count("_oor=0") == 5 * 24 and r.stdout.count("visit_err=0") == 24
    for path in _step_cases(tmp_path):
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        print(path.name, r.stdout, r.stderr)
        assert r.returncode == 0 and "mismatches=0" in r.stdout, path.name


def test_reference_is_sysrem_and_keeps_the_definitions_clauses():
    """sysrem_f64 is observation.sysrem up to rounding on a planted design, with and without ones; entries without
    weight come back as they came and influence nothing; a pixel and an exposure without weight give a zero row of U
    and no NaN; all-masked data end every component with U = 0."""
    from prometheus_amd import observation as obs
    D, ivar = sref.planted(7, T + 1, 1)
    err = np.where(ivar > 0, 1e-3, np.nan)
    for ones in (False, True):
        U, cl = sref.sysrem_f64(D, ivar, 3, 30, ones)
        U0, cl0 = obs.sysrem(D, err, 3, 30, ones=ones)
        w, _ = sref.weights_of(D, ivar)
        assert U.shape == U0.shape and np.abs(U - U0).max() < 1e-9
        assert np.array_equal(np.isnan(cl), np.isnan(cl0)) and np.abs(cl - cl0)[w > 0].max() < 1e-9
        assert np.array_equal(cl[w == 0], D[w == 0], equal_nan=True)
        assert not ones or np.all(U[:, 0] == 1.0)
        # what an entry without weight holds changes no other bit
        iv2 = np.where(w == 0, 0.0, ivar)
        for Dx in (np.where(w == 0, 1e300, D), np.where(w == 0, np.nan, D)):
            Ux, clx = sref.sysrem_f64(Dx, iv2, 3, 30, ones)
            assert np.array_equal(Ux, U) and np.array_equal(clx[w > 0], cl[w > 0])
            assert np.array_equal(clx[w == 0], Dx[w == 0], equal_nan=True)
    # a pixel masked in every exposure and an exposure masked in every pixel
    D, ivar = sref.planted(7, T + 1, 2)
    D = np.where(np.isnan(D), 1.0, D)
    ivar = np.where(ivar == 0, 1e6, ivar)
    ivar[:, 5] = 0.0
    ivar[2, :] = 0.0
    U, cl = sref.sysrem_f64(D, ivar, 3, 4)
    assert np.all(U[2] == 0) and np.isfinite(U).all() and np.isfinite(cl).all()
    assert np.array_equal(cl[:, 5], D[:, 5]) and np.array_equal(cl[2], D[2])
    # nothing weighted at all
    U, cl = sref.sysrem_f64(D, np.zeros_like(D), 2, 3, True)
    assert np.all(U[:, 0] == 1) and np.all(U[:, 1:] == 0) and np.array_equal(cl, D)
    U, cl = sref.sysrem_f64(np.full_like(D, np.nan), ivar, 2, 3)
    assert np.all(U == 0) and np.isnan(cl).all()


@pytest.mark.parametrize("n_exp,n_pix,seed", ACCURACY)
def test_accuracy_designs_stay_inside_the_margin(n_exp, n_pix, seed):
    """The yardstick of the device's accuracy test is d(observation.sysrem), the host function's own distance from the
    longdouble run, with the floor n_pix 2^-53 max |D| and the factor 4.  Two float64 runs of equal quality, sysrem_f64
    and observation.sysrem on pixel-reversed input, must stay inside it: a design where they do not is no yardstick."""
    from prometheus_amd import observation as obs
    D, ivar = sref.planted(n_exp, n_pix, seed)
    err = np.where(ivar > 0, 1e-3, np.nan)
    w, _ = sref.weights_of(D, ivar)
    _, cld = sref.sysrem_ld(D, ivar, 3, 30)
    d_host = sref.distance(obs.sysrem(D, err, 3, 30)[1], cld, w)
    d_ref = sref.distance(sref.sysrem_f64(D, ivar, 3, 30)[1], cld, w)
    d_rev = sref.distance(obs.sysrem(D[:, ::-1], err[:, ::-1], 3, 30)[1][:, ::-1], cld, w)
    bound = 4.0 * max(d_host, sref.margin(D, n_pix))
    print("SYSREM_ERR cpu n_exp=%d n_pix=%d: host %.3g, float64 definition %.3g, host reversed %.3g, bound %.3g"
          % (n_exp, n_pix, d_host, d_ref, d_rev, bound))
    assert d_ref <= bound and d_rev <= bound
    # a wrong algorithm misses by the noise level
    assert sref.distance(obs.sysrem(D, err, 2, 30)[1], cld, w) > 1e6 * bound


def test_numpy_pipeline_finds_the_planted_planet():
    """The all-numpy pipeline on the planted-planet design (the oracle's R of the reduced C1 problem, the longdouble
    exposures' model, numpy injection, observation.high_pass, observation.sysrem, the filter and the likelihood) peaks
    at the injected trial: the design the device test uses is a fair one."""
    from oracle import prom_oracle as O
    from prometheus_amd import celestialBodies as bodies
    from prometheus_amd import observation as obs
    g = np.load(os.path.join(REPO, "tests", "golden", "transit_C1.npz"))
    cfg = json.loads(str(g["config"]))
    cfg["Grids"].update(sref.PLANET_CFG)
    wav, orb, R = O.run_setup(cfg)
    d = sref.planet_design(bodies.AvailablePlanets().findPlanet(cfg["Architecture"]["planetName"]), orb)
    ins = d["ins"]
    ex = obs.Exposures(ins, d["rows"], d["a"], d["F"], d["raw"], d["err"])
    M = eref.expose(wav, R, ins.lam, ins.sig, ins.truncate, d["rows"], d["a"], d["F"], ex.data, ex.ivar)[2]
    M = ins.unsort(M.astype(np.float64))
    assert M.shape == (12, 9, 400) and np.isnan(M).any() and np.nanmin(M) < 0.99
    D = sref.inject_f64(d["raw"], M[:, sref.PLANET_TRIAL], 1.0)
    flat = obs.high_pass(D, d["taps"], orders=d["orders"], mode=d["mode"])
    Ub, clean = obs.sysrem(flat, d["err"], d["n_comp"], d["n_iter"], ones=d["ones"])
    ll = sref.numpy_recovery(d, M, clean, Ub)
    print("planted planet, numpy: logL - max per trial", ll - ll.max())
    assert int(np.argmax(ll)) == sref.PLANET_TRIAL
    # the raw data alone do not put the peak there: it is the injection that the pipeline finds
    flat0 = obs.high_pass(d["raw"], d["taps"], orders=d["orders"], mode=d["mode"])
    U0, clean0 = obs.sysrem(flat0, d["err"], d["n_comp"], d["n_iter"], ones=d["ones"])
    assert int(np.argmax(sref.numpy_recovery(d, M, clean0, U0))) != sref.PLANET_TRIAL


# ---- Injection, Transit.clean and Transit.inject without a device --------------------------------------------------
def _bare_transit(n_wav, n_orb):
    """A Transit with a grid and phases and nothing a device could run: the calls must refuse before they need one."""
    from prometheus_amd import gasProperties as gp
    tr = gp.Transit.__new__(gp.Transit)
    tr.wavelength = 5880e-8 + 1e-11 * np.arange(n_wav)
    tr.spatialGrid = types.SimpleNamespace(constructOrbphaseAxis=lambda: np.linspace(-0.03, 0.03, n_orb))
    tr.atmosphere = types.SimpleNamespace(densityDistributionList=[])
    tr.last_stats, tr.collect_stats = [], False
    return tr


def test_injection_clean_and_inject_refuse_before_touching_a_device(monkeypatch):
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
    ex = obs.Exposures(ins, rows, a, F, data, err)
    raw = np.arange(9.0).reshape(3, 3)
    raw[1, 1] = np.nan                                                    # any value is allowed
    inj = obs.Injection(ex, raw)
    assert inj.exposures is ex and inj.exposures_key == ex.key and np.array_equal(inj.raw, ins.sort(raw), equal_nan=True)
    assert obs.Injection(ex, raw).key == inj.key and obs.Injection(ex, raw + 1.0).key != inj.key
    raw[0, 0] = 5.0
    assert inj.raw[0, 2] == 0.0                                           # (copied; the caller's pixel 0 is the device's 2)
    with pytest.raises(TypeError):
        obs.Injection(ins, raw)
    with pytest.raises(TypeError):
        obs.Injection(ex, [["a", "b", "c"]] * 3)
    for bad in (raw[:2], raw[:, :2], raw[0], raw[None]):
        with pytest.raises(ValueError):
            obs.Injection(ex, bad)
    hp = obs.HighPass(ex, obs.box_taps(1))
    other = obs.Exposures(ins, rows, a, F, data * 1.5, err)
    hp_other = obs.HighPass(other, obs.box_taps(1))
    for call in (lambda **k: tr.clean(inj, **k), lambda **k: tr.inject(inj, 1, **k)):
        for bad, exc in ((dict(n_comp=0), ValueError), (dict(n_comp=-1, ones=True), ValueError),
                         (dict(n_comp=17), ValueError), (dict(n_comp=16, ones=True), ValueError),
                         (dict(n_comp=2, n_iter=0), ValueError), (dict(n_comp=2.5), TypeError),
                         (dict(n_comp=2, n_iter=3.0), TypeError), (dict(n_comp=2, ones=1), TypeError),
                         (dict(n_comp=2, highpass=obs.box_taps(1)), TypeError),
                         (dict(n_comp=2, highpass=hp_other), ValueError),
                         (dict(n_comp=2, devices=[0, 1]), ValueError)):
            with pytest.raises(exc):
                call(**bad)
    with pytest.raises(TypeError, match="observation.Injection"):
        tr.clean(ex, n_comp=2)
    with pytest.raises(TypeError, match="observation.Injection"):
        tr.inject(raw, 0, n_comp=2)
    for trial in (-1, 4):
        with pytest.raises(ValueError, match="trial"):
            tr.inject(inj, trial, n_comp=2)
    with pytest.raises(TypeError):
        tr.inject(inj, 1.0, n_comp=2)
    for scale in (np.nan, np.inf):
        with pytest.raises(ValueError, match="scale"):
            tr.inject(inj, 1, scale=scale, n_comp=2)
    with pytest.raises(TypeError, match="observation.Broadening"):
        tr.inject(inj, 1, n_comp=2, broaden=np.ones(3))
    with pytest.raises(ValueError, match="split"):
        tr.inject(inj, 1, n_comp=2, highpass=hp, max_memory_gb=1e-9)
    rows_bad = obs.Injection(obs.Exposures(ins, rows + 1, a, F, data, err), raw)
    with pytest.raises(ValueError, match="phases"):
        tr.inject(rows_bad, 1, n_comp=2)
