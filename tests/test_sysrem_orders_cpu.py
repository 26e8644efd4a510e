"""SYSREM per echelle order without a device: the host harness of prometheus_amd/csrc/order_sysrem_index.h (every
thread of k_sysrem_prep_orders and k_sysrem_finish_orders, the padding lemma on values, the sub-batch planner; plain
and under sanitizers, as a stand-alone program), the lemma once more on the float64 reference, the host per-order
observation.sysrem / observation.filter_weights against the loop over column subsets, and the refusals of the
``sysrem_orders`` keyword that come before a device is needed."""
import os
import subprocess

import numpy as np
import pytest

from helpers import sysrem_ref as sref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "prometheus_amd", "csrc")
HOST = os.path.join(REPO, "tests", "helpers", "order_sysrem_host.cpp")
T = sref.TILE


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_harness_walks_the_order_kernels_checks_the_lemma_and_the_planner(tmp_path, which):
    """Five tables (orders of 1, T - 1, T, T + 1 and 3 T + 5 pixels mixed and interleaved, among others) x n_exp in
    {1, 2, 7, 70} x 1 and 3 injections: every index of the two kernels lies inside its buffer, every work entry of
    every item (padding included), every D entry and every cleaned entry is visited exactly once; an order's row sums
    at width n_s and at width n_max have equal bits; the planner keeps the byte cap and the 65,535-item cap."""
    flags = {"plain": ("-O2",), "sanitized": ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")}
    exe = tmp_path / "order_sysrem_host"
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags[which], "-I" + CSRC, HOST, "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "shapes=40 tile=%d" % T in r.stdout
    assert r.stdout.count("_oor=0") == 3 * 40 and r.stdout.count("visit_err=0") == 40
    assert "n_seg=5 n_pix=%d n_max=%d n_exp=70 n_inj=3" % (6 * T + 6, 3 * T + 5) in r.stdout
    assert "mismatches=0" in r.stdout and "lemma cases=0" not in r.stdout
    assert "errors=0" in r.stdout


def test_the_lemma_on_the_float64_reference():
    """sysrem_f64 on a table padded with columns without weight gives the unpadded table's U and cleaned data bit for
    bit, whatever the padding's width: the row sums' shape is a function of the weighted prefix alone."""
    for n_exp, n_s, seed in ((7, T + 1, 1), (2, 1, 2), (7, T - 1, 3), (5, 3 * T + 5, 4)):
        D, ivar = sref.planted(n_exp, n_s, seed)
        for ones in (False, True):
            U, cl = sref.sysrem_f64(D, ivar, 2, 3, ones)
            for n_max in (n_s + 1, T + 1, 3 * T + 5, 66 * T):
                if n_max <= n_s:
                    continue
                Dp = np.concatenate([D, np.full((n_exp, n_max - n_s), 7.0)], axis=1)
                ip = np.concatenate([ivar, np.zeros((n_exp, n_max - n_s))], axis=1)
                Up, clp = sref.sysrem_f64(Dp, ip, 2, 3, ones)
                assert np.array_equal(Up, U) and not np.signbit(Up[Up == 0]).any(), (n_s, n_max)
                assert np.array_equal(clp[:, :n_s], cl, equal_nan=True) and np.all(clp[:, n_s:] == 7.0)


def _orders_design(seed=0):
    rng = np.random.default_rng(seed)
    n_exp, n_pix = 9, 90
    labels = rng.permutation(np.repeat([7, -2, 30], [40, 1, 49]))     # interleaved, labels not 0 .. n - 1
    data = (1.0 + 0.02 * rng.normal(size=(n_exp, n_pix))
            + 0.3 * rng.normal(size=n_exp)[:, None] * rng.normal(size=n_pix)[None, :] * (1 + (labels == 30)))
    err = np.full((n_exp, n_pix), 1e-2)
    data[2, 5] = np.nan
    err[4, 11] = 0.0
    return data, err, labels


def test_host_sysrem_per_order_is_the_loop_over_column_subsets():
    from prometheus_amd import observation as obs
    data, err, labels = _orders_design()
    for ones in (False, True):
        U, cleaned = obs.sysrem(data, err, 2, 5, ones=ones, orders=labels)
        assert U.shape == (3, 9, 2 + ones) and cleaned.shape == data.shape
        for s, label in enumerate(np.unique(labels)):
            idx = np.flatnonzero(labels == label)
            Us, cs = obs.sysrem(data[:, idx], err[:, idx], 2, 5, ones=ones)
            assert np.array_equal(U[s], Us) and np.array_equal(cleaned[:, idx], cs, equal_nan=True), label
    # one order: the existing call with the order dimension in front (to rounding only: the order in which numpy adds
    # depends on the memory layout of a column subset)
    U1, c1 = obs.sysrem(data, err, 2, 5, orders=np.zeros(90, dtype=int))
    U0, c0 = obs.sysrem(data, err, 2, 5)
    assert U1.shape == (1,) + U0.shape and np.allclose(U1[0], U0, rtol=0, atol=1e-12)
    assert np.allclose(c1, c0, rtol=0, atol=1e-12, equal_nan=True)
    # a scalar err broadcasts as before
    assert np.array_equal(obs.sysrem(data, 1e-2, 2, 5, orders=labels)[0],
                          obs.sysrem(data, np.full_like(data, 1e-2), 2, 5, orders=labels)[0])
    with pytest.raises(ValueError):
        obs.sysrem(data, err, 2, 5, orders=labels[:-1])
    with pytest.raises(TypeError):
        obs.sysrem(data, err, 2, 5, orders=labels + 0.5)


def test_host_filter_weights_per_order_is_the_loop_over_column_subsets():
    from prometheus_amd import observation as obs
    data, err, labels = _orders_design(1)
    U, _ = obs.sysrem(data, err, 2, 5, ones=True, orders=labels)
    ivar = np.where(err > 0, 1.0 / np.where(err > 0, err, 1.0) ** 2, 0.0)
    W = obs.filter_weights(U, ivar, orders=labels)
    assert W.shape == (3, 9, 90)
    for s, label in enumerate(np.unique(labels)):
        idx = np.flatnonzero(labels == label)
        assert np.array_equal(W[:, :, idx], obs.filter_weights(U[s], ivar[:, idx])), label
    assert np.any(W != obs.filter_weights(U[0], ivar))                      # the orders' bases differ
    for bad in (U[0], U[:2], U[:, :-1]):
        with pytest.raises(ValueError):
            obs.filter_weights(bad, ivar, orders=labels)


def test_sysrem_orders_refusals_before_touching_a_device(monkeypatch):
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
    inj = obs.Injection(ex, np.arange(9.0).reshape(3, 3))
    od_other = obs.Orders(obs.Exposures(ins, rows, a, F, data * 1.5, err), [0, 1, 0])
    calls = (lambda **k: tr.clean(inj, n_comp=2, **k), lambda **k: tr.inject(inj, 1, n_comp=2, **k),
             lambda **k: tr.inject_grid(inj, [0, 1], [1.0, 0.5], n_comp=2, **k))
    for call in calls:
        with pytest.raises(TypeError, match="sysrem_orders"):
            call(sysrem_orders=[0, 1, 0])
        with pytest.raises(ValueError, match="sysrem_orders"):
            call(sysrem_orders=od_other)
    # the keyword is looked at before the run would be split
    with pytest.raises(ValueError, match="split"):
        tr.inject(inj, 1, n_comp=2, sysrem_orders=obs.Orders(ex, [0, 1, 0]), max_memory_gb=1e-9)


def test_numpy_per_order_pipeline_finds_the_planted_planet():
    """The all-numpy per-order pipeline on the planted-planet design (two interleaved orders): numpy injection,
    observation.high_pass, observation.sysrem(orders=), the filter of every order's own basis
    (observation.filter_weights(orders=)) and the likelihood peak at the injected trial: the design the device test
    uses is a fair one.  observation.Detrend(orders=) forms the same W."""
    import json
    from helpers import detrend_ref as dref
    from helpers import expose_ref as eref
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
    D = sref.inject_f64(d["raw"], M[:, sref.PLANET_TRIAL], 1.0)
    flat = obs.high_pass(D, d["taps"], orders=d["orders"], mode=d["mode"])
    Ub, clean = obs.sysrem(flat, d["err"], d["n_comp"], d["n_iter"], ones=d["ones"], orders=d["orders"])
    assert Ub.shape == (2, 12, 3)
    ex2 = obs.Exposures(ins, d["rows"], d["a"], d["F"], clean, d["err"])
    Mh = ins.sort(obs.high_pass(M, d["taps"], orders=d["orders"], mode=d["mode"]))
    labels = ins.sort(d["orders"].astype(np.float64)).astype(np.int64)   # the orders in the device's pixel order
    W = obs.filter_weights(Ub, ex2.ivar, orders=labels)
    Mf = np.empty_like(Mh)
    for s, label in enumerate(np.unique(labels)):
        idx = np.flatnonzero(labels == label)
        Mf[:, :, idx] = dref.filter_f64(np.ascontiguousarray(Mh[:, :, idx]), Ub[s], np.ascontiguousarray(W[:, :, idx]))[0]
    mom, nu, _ = dref.moments_ld(Mf, ex2.data, ex2.ivar)
    ll = obs.VelocityMap(mom.astype(np.float64), nu, d["F"]).loglike.sum(axis=0)
    print("planted planet per order, numpy: logL - max per trial", ll - ll.max())
    assert int(np.argmax(ll)) == sref.PLANET_TRIAL
    od = obs.Orders(ex2, d["orders"])
    dt = obs.Detrend(ex2, Ub, orders=od)
    assert np.array_equal(dt.W, W) and np.array_equal(np.unique(labels)[dt.seg_of], labels)
    assert obs.Detrend(ex2, Ub, orders=od).key == dt.key and obs.Detrend(ex2, Ub[::-1], orders=od).key != dt.key
    assert obs.Detrend(ex2, Ub, orders=od, on_device=True).W is None
    for bad, exc in ((dict(U=Ub[0], orders=od), ValueError), (dict(U=Ub, orders=d["orders"]), TypeError),
                     (dict(U=Ub, orders=obs.Orders(ex, d["orders"])), ValueError),
                     (dict(U=Ub, orders=od, W=W, on_device=True), ValueError), (dict(U=Ub, orders=od, W=W[:2]), ValueError)):
        with pytest.raises(exc):
            obs.Detrend(ex2, **bad)
