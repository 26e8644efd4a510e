"""Injection grids without a device: the host harness of prometheus_amd/csrc/grid_index.h (every index of every batched
kernel, the flags' rows and the sub-batch planner, plain and under sanitizers; a batch evaluated launch by launch in
the kernels' order against sysrem_ref, filter_ref and detrend_ref per entry, bit for bit), the design of the device's
flag test on its numpy model, observation.injection_grid, and the refusals of Transit.inject_grid /
Transit.recover_grid that come before a device is needed."""
import os
import subprocess

import numpy as np
import pytest

from helpers import detrend_ref as dref
from helpers import expose_ref as eref
from helpers import filter_ref as fref
from helpers import grid_design as gd
from helpers import sysrem_ref as sref
from test_sysrem_cpu import _bare_transit, _hex

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "prometheus_amd", "csrc")
HOST = os.path.join(REPO, "tests", "helpers", "grid_host.cpp")
T = sref.TILE
SHAPES = [(B, n_pix, n_exp) for B in (1, 2, 5) for n_pix in (1, T - 1, T, T + 1, 3 * T + 5) for n_exp in (1, 2, 7)]


def _batch_cases(tmp_path):
    """Files for grid_host <file>: shapes about the tile, 1, 2 and 5 injections with a duplicate and a scale of 0, NaN,
    infinities and ivar = 0 sprinkled in, model values missing, with and without ones; in the last case the second
    injection's scale overflows D everywhere, so every one of its components ends while its neighbours' do not."""
    out = []
    cases = [(1, 1, 1, 1, 2, False), (2, 2, T - 1, 2, 3, True), (5, 7, T + 1, 2, 4, False), (5, 2, 3 * T + 5, 0, 2, True),
             (3, 7, T, 2, 4, False)]
    for i, (B, n_exp, n_pix, n_comp, n_iter, ones) in enumerate(cases):
        rng = np.random.default_rng(40 + i)
        n_trial = 3
        raw = 1.0 + 0.1 * rng.normal(size=(n_exp, n_pix)) + 0.3 * rng.normal(size=(n_exp, 1)) * rng.normal(size=(1, n_pix))
        iv = 1e4 * (0.1 + rng.random((n_exp, n_pix)))
        Tm = 1.0 - 0.2 * rng.random((n_exp, n_trial, n_pix))
        points = [gd.LIST[b % len(gd.LIST)] for b in range(B)]
        if n_pix > 4:
            raw[rng.random(raw.shape) < 0.03] = np.nan
            raw[rng.random(raw.shape) < 0.01] = np.inf
            iv[rng.random(raw.shape) < 0.03] = 0.0
            Tm[:, :, 3] = np.nan
            Tm[rng.random(Tm.shape) < 0.01] = np.nan
        if i == 4:
            raw = np.where(np.isfinite(raw), raw, 1.0) * 1e10
            Tm = np.where(np.isnan(Tm), 0.9, Tm)
            points = [(0, 0.7), (1, 1e305), (2, -0.5)]
        model = np.stack([Tm[:, t] for t, _ in points], axis=1)          # [n_exp][B][n_pix], as k_expose lays it out
        U, cl, W, Tf = [], [], [], []
        for b, (t, s) in enumerate(points):
            Ub, c = sref.sysrem_f64(sref.inject_f64(raw, model[:, b], s), iv, n_comp, n_iter, ones)
            Wb = fref.weights_f64(Ub, iv)
            U.append(Ub), cl.append(c), W.append(Wb), Tf.append(dref.filter_f64(Tm, Ub, Wb)[0])
        if i == 4:
            assert not U[1].any() and all(U[b][:, k].any() for b in (0, 2) for k in range(2))
        path = tmp_path / ("batch%d.txt" % i)
        path.write_text("%d %d %d %d %d %d %d\n%s\n" % (B, n_exp, n_pix, n_comp, n_iter, ones, n_trial, "\n".join(
            _hex(x) for x in (raw, iv, model, [s for _, s in points], Tm, np.stack(U), np.stack(cl), np.stack(W),
                              np.stack(Tf)))))
        out.append((path, 2 if i == 4 else None))
    return out


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_harness_walks_every_batched_kernel_and_matches_the_references_bitwise(tmp_path, which):
    """Over n_inj in {1, 2, 5} x n_pix in {1, T - 1, T, T + 1, 3 T + 5} x n_exp in {1, 2, 7} every index of the gather,
    the injection, prep, fill, step, rows, finish, the filter's weights and the out-of-place detrend lies inside its
    buffer and inside its own injection's slice (the `ended` flags: its own row), every entry of every per-injection
    buffer is written exactly once, and the planner covers the list exactly once under caps that give 1, 2 and n_inj
    sub-batches without exceeding them; five batches evaluated launch by launch give sysrem_ref, filter_ref and
    detrend_ref per entry bit for bit."""
    flags = {"plain": ("-O2",), "sanitized": ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")}
    exe = tmp_path / "grid_host"
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags[which], "-I" + CSRC, HOST, "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "shapes=%d tile=%d flags=%d" % (len(SHAPES), T, gd.FLAGS) in r.stdout
    for name in ("oor", "foreign", "visit_err", "plan_err"):
        assert r.stdout.count(" %s=0" % name) == len(SHAPES), name
    cols = (1, 3, 16)
    for i, (B, n_pix, n_exp) in enumerate(SHAPES):                         # the byte count the tests' caps rely on
        line = "n_inj=%d n_exp=%d n_pix=%d n_cols=%d:" % (B, n_exp, n_pix, cols[i % 3])
        want = " bytes=%d/%d" % tuple(gd.injection_bytes(n_exp, n_pix, cols[i % 3], 2, rec) for rec in (False, True))
        assert [ln for ln in r.stdout.splitlines() if ln.startswith(line)][0].endswith(want)
    for path, ended in _batch_cases(tmp_path):
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        print(path.name, r.stdout, r.stderr)
        assert r.returncode == 0 and "mismatches=0" in r.stdout, path.name
        assert ended is None or "ended=%d " % ended in r.stdout


def test_the_flag_design_ends_the_middle_entry_alone():
    """The condition the device's flag test puts on its design, on the numpy model of the same design: at scale 1e305
    the middle point's D is infinite wherever raw is not NaN, so SYSREM finds no weight and both columns of its U are
    zero, while both columns of its neighbours' U are not."""
    d, points = gd.overflow_design()
    M = np.asarray(eref.expose(d["wav"], d["R"], d["lam"], d["sig"], d["k"], d["rows"], d["a"], d["F"], d["data"],
                               d["ivar"])[2], dtype=np.float64)
    assert M.shape == (7, 3, 129) and not np.isnan(M).any() and M.max() < 1.0
    for b, (t, s) in enumerate(points):
        with np.errstate(over="ignore", invalid="ignore"):
            D = sref.inject_f64(d["raw"], M[:, t], s)
        U, _ = sref.sysrem_f64(D, d["ivar"], 2, 4)
        if b == 1:
            assert not np.isfinite(D).any() and not U.any()
        else:
            assert np.isfinite(D).sum() > 800 and U[:, 0].any() and U[:, 1].any()


def test_injection_grid_is_the_cross_product_trial_major():
    from prometheus_amd import observation as obs
    t, s = obs.injection_grid([4, 1, 4], [0.5, 1.0])
    assert t.tolist() == [4, 4, 1, 1, 4, 4] and s.tolist() == [0.5, 1.0, 0.5, 1.0, 0.5, 1.0]
    assert t.dtype == np.int64 and s.dtype == np.float64
    t, s = obs.injection_grid([], [1.0])
    assert len(t) == len(s) == 0
    with pytest.raises(TypeError):
        obs.injection_grid([1.5], [1.0])
    with pytest.raises(ValueError):
        obs.injection_grid([[1]], [1.0])
    # the containers: grid[b] is the single call's result
    U, data = np.arange(12.0).reshape(2, 3, 2), np.arange(24.0).reshape(2, 3, 4)
    cg = obs.CleanedGrid(np.array([1, 2]), np.array([0.5, 1.0]), U, data)
    assert len(cg) == 2 and isinstance(cg[1], obs.Cleaned) and np.array_equal(cg[1].U, U[1])
    assert np.array_equal(cg[-1].data, data[1]) and cg[0].injected is None
    assert obs.CleanedGrid(np.array([1]), np.array([0.5]), U[:1])[0].data is None
    mom, nu = np.ones((2, 3, 5, 7)), np.full((2, 3, 5), 4)
    rg = obs.RecoveryGrid(np.array([1, 2]), np.array([0.5, 1.0]), mom, nu, U, np.ones((3, 5, 2)), np.ones((2, 3, 5, 4)))
    assert isinstance(rg[0], obs.VelocityMap) and rg.total("chi2").shape == (2, 5) and rg[1].order_totals.chi2.shape == (3, 5)
    assert np.array_equal(rg[1].U, U[1]) and rg[0].by_order is None
    with pytest.raises(IndexError):
        rg[2]


def test_grid_calls_refuse_before_touching_a_device(monkeypatch):
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
    inj = obs.Injection(ex, raw)
    hp = obs.HighPass(ex, obs.box_taps(1))
    other = obs.Exposures(ins, rows, a, F, data * 1.5, err)
    hp_other, od_other = obs.HighPass(other, obs.box_taps(1)), obs.Orders(other, np.zeros(3, dtype=int))
    for call in (lambda *p, **k: tr.inject_grid(inj, *p, **k), lambda *p, **k: tr.recover_grid(inj, *p, **k)):
        for bad, exc in ((dict(n_comp=0), ValueError), (dict(n_comp=-1, ones=True), ValueError),
                         (dict(n_comp=17), ValueError), (dict(n_comp=16, ones=True), ValueError),
                         (dict(n_comp=2, n_iter=0), ValueError), (dict(n_comp=2.5), TypeError),
                         (dict(n_comp=2, n_iter=3.0), TypeError), (dict(n_comp=2, ones=1), TypeError),
                         (dict(n_comp=2, highpass=obs.box_taps(1)), TypeError),
                         (dict(n_comp=2, highpass=hp_other), ValueError),
                         (dict(n_comp=2, broaden=np.ones(3)), TypeError),
                         (dict(n_comp=2, devices=[0, 1]), ValueError),
                         (dict(n_comp=2, highpass=hp, max_memory_gb=1e-9), ValueError)):
            with pytest.raises(exc):
                call([1, 2], [1.0, 0.5], **bad)
        # the list: lengths (scalars broadcast), the trials' range and type, the scales
        for t, s, exc in (([1, 2], [1.0], ValueError), ([1], [1.0, 0.5, 0.2], ValueError), ([[1, 2]], [[1.0, 0.5]], ValueError),
                          ([1, 4], [1.0, 1.0], ValueError), ([-1], [1.0], ValueError), ([1.0], [1.0], TypeError),
                          ([1, 2], [1.0, np.nan], ValueError), (1, np.inf, ValueError), ([1], ["a"], TypeError)):
            with pytest.raises(exc):
                call(t, s, n_comp=2)
        with pytest.raises(ValueError, match="entry 1"):
            call([0, 7], 1.0, n_comp=2)
    t, s = obs._check_grid_list("x", inj, 2, [0.5, 1.0])                  # a scalar is broadcast against the other
    assert t.tolist() == [2, 2] and s.tolist() == [0.5, 1.0]
    t, s = obs._check_grid_list("x", inj, [0, 3], 1.5)
    assert t.tolist() == [0, 3] and s.tolist() == [1.5, 1.5]
    with pytest.raises(TypeError, match="observation.Injection"):
        tr.inject_grid(ex, [1], [1.0], n_comp=2)
    with pytest.raises(TypeError, match="observation.Orders"):
        tr.recover_grid(inj, [1], [1.0], n_comp=2, orders=np.zeros(3))
    with pytest.raises(ValueError, match="Orders"):
        tr.recover_grid(inj, [1], [1.0], n_comp=2, orders=od_other)
    rows_bad = obs.Injection(obs.Exposures(ins, rows + 1, a, F, data, err), raw)
    with pytest.raises(ValueError, match="phases"):
        tr.recover_grid(rows_bad, [1], [1.0], n_comp=2)
