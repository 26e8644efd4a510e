"""The median high-pass without a device: the host harness of k_median's index arithmetic and selection function
(tests/helpers/median_host.cpp, a stand-alone program, plain and sanitized), the two references of
tests/helpers/median_ref.py against each other, observation.high_pass with a median_window against both, and the
refusals of observation.median_window and observation.HighPass."""
import os
import subprocess

import numpy as np
import pytest

from helpers import highpass_ref as href
from helpers import median_ref as mref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "prometheus_amd", "csrc")
HOST = os.path.join(REPO, "tests", "helpers", "median_host.cpp")
HALVES = (0, 1, 3, 255, 256, 512)


def special_row(rng, n, nan_every=11):
    """A row about 1 with NaN, both zeros, both infinities, subnormals and many ties."""
    x = 1.0 - 0.05 * rng.random(n)
    x[::3] = np.floor(x[::3] * 32.0) / 32.0                      # ties
    pick = lambda k: rng.choice(n, size=max(n // k, 1), replace=False)
    x[pick(17)] = 0.0
    x[pick(17)] = -0.0
    x[pick(29)] = np.inf
    x[pick(29)] = -np.inf
    x[pick(23)] = 5e-324 * rng.integers(1, 9)
    x[pick(nan_every)] = np.nan
    return x


# ---- the harness -----------------------------------------------------------------------------------------------------
def _row_cases():
    """(name, row, h, mode)."""
    rng = np.random.default_rng(29)
    row = lambda n: 1.0 - 0.05 * rng.random(n)
    cases = []
    a = row(40)
    a[[0, 1, 39]] = np.nan
    cases.append(("edge NaN", a, 5, 0))
    b = row(300)
    b[[100, 101, 170]] = np.nan
    cases.append(("middle NaN", b, 12, 0))
    cases.append(("middle NaN divide", b, 12, 1))
    c = row(50)
    c[17:24] = np.nan
    c[20] = 0.9731                                   # a valid centre whose whole window (h = 3) is NaN but itself
    cases.append(("lone centre", c, 3, 0))
    cases.append(("lone centre divide", c, 3, 1))
    d = row(64)
    d[30:41] = 0.0                                   # B = 0 under division
    cases.append(("zero stretch divide", d, 2, 1))
    cases.append(("specials", special_row(rng, 700), 40, 0))
    cases.append(("specials divide", special_row(rng, 700), 7, 1))
    cases.append(("three tiles", special_row(rng, 2600, nan_every=400), 300, 0))
    cases.append(("ties", np.floor(row(1500) * 64.0) / 64.0, 160, 0))
    cases.append(("h = 0", row(7), 0, 0))
    cases.append(("h beyond the row", row(9), 512, 1))
    return cases


def _row_file(path, M, h, mode):
    seg, perm = href.one_segment(len(M))
    want = mref.median_f64(M, seg, perm, h, mode)
    vals = lambda a: " ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel())
    with open(path, "w") as f:
        f.write("%d %d %d\n%s\n%s\n" % (len(M), h, mode, vals(M), vals(want)))
    return want


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_harness_walks_every_index_and_matches_the_reference_bitwise(tmp_path, which):
    """The walk over the segment lengths {1, 2, 3, T - 1, T, T + 1, 2 T + 5} (interleaved through perm) x
    h in {0, 1, 3, 255, 256, 512} x both modes finds every ring slot, index and rank entry, perm entry and model value
    inside, every slot read holding the original of the position intended, every sort ascending, no value read after
    it was overwritten, every model value written once and every result equal to the definition evaluated directly;
    the clean path is taken at every half width and even counts occur wherever h > 0.  The given rows agree with
    median_f64 bit for bit."""
    flags = {"plain": ("-O2",), "sanitized": ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")}
    exe = tmp_path / "median_host"
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags[which], "-I" + CSRC, HOST, "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    lines = [l for l in r.stdout.splitlines() if l.startswith("h=")]
    assert len(lines) == 2 * len(HALVES)
    for h in HALVES:
        for mode in (0, 1):
            (line,) = [l for l in lines if l.startswith("h=%d mode=%d " % (h, mode))]
            for name in ("ring_oor", "lds_oor", "perm_oor", "model_oor", "slot_err", "sort_err", "stale_read",
                         "visit_err", "mismatch"):
                assert " %s=0" % name in line, line
            assert "clean_waves=0 " not in line, line
            assert ("even_counts=0 " in line) == (h == 0), line
            assert "workgroups=7 " in line and "outputs=5131 " in line
    for name, M, h, mode in _row_cases():
        path = tmp_path / (name.replace(" ", "_").replace("=", "") + ".txt")
        want = _row_file(path, M, h, mode)
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        print(name, r.stdout, r.stderr)
        assert r.returncode == 0 and " mismatch=0" in r.stdout and " visit_err=0" in r.stdout, name
        if name == "lone centre":
            assert want[20] == 0.0 and not np.signbit(want[20])        # B = M: its own value is all the window has
        if name == "lone centre divide":
            assert want[20] == 1.0
        if name == "zero stretch divide":
            assert np.isnan(want[32:39]).all() and np.isfinite(np.delete(want, np.arange(30, 41))).all()
        if name == "h = 0":
            assert np.all(want == 0.0) and not np.signbit(want).any()


# ---- the references ----------------------------------------------------------------------------------------------------
def test_the_two_references_agree_and_the_key_order_adds_the_sign_of_zero():
    rng = np.random.default_rng(41)
    lengths = [1, 2, 77, 300]
    seg, perm = href.interleaved(lengths, seed=3)
    M = np.stack([special_row(rng, sum(lengths)) for _ in range(3)])
    for h in (0, 1, 2, 9, 160, 512):
        for mode in (0, 1):
            a, b = mref.median_f64(M, seg, perm, h, mode), mref.median_np(M, seg, perm, h, mode)
            zero_B = (mref.median_B(M, seg, perm, h) == 0) & (mode == 1)      # (its sign shows in M / B)
            assert zero_B.any() or mode == 0 or h > 2
            assert mref.median_equal(np.where(zero_B, 0.0, a), np.where(zero_B, 0.0, b)), (h, mode)
            assert np.isnan(a[np.isnan(M)]).all() and np.isfinite(a).any()
    # the order among ties: the median of (-0, +0) windows carries the sign the key order gives
    seg1, perm1 = href.one_segment(3)
    z = np.array([[0.0, -0.0, 0.0], [-0.0, 0.0, -0.0]])
    B = mref.running_median_f64(z, 1)
    # (a window of two: fl(fl(-0 + +0) 0.5) = +0; of three: the middle one of (-0, +0, +0) and of (-0, -0, +0))
    assert np.array_equal(np.signbit(B), [[False, False, False], [False, True, False]])
    assert mref.same_bits(mref.median_f64(z, seg1, perm1, 1, 0), z - B)
    # keys: monotone, -0 below +0, the infinities the ends, a round trip
    v = np.array([-np.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.inf])
    k = mref.keys_of(v)
    assert np.all(np.diff(k.astype(object)) > 0) and mref.same_bits(mref.values_of(k), v)
    assert mref.keys_of(np.array([np.nan]))[0] == mref.NO_KEY
    # h = 0 and n = 1: B = M
    one = np.array([[0.5, np.nan, -0.0, np.inf]])
    assert mref.same_bits(mref.running_median_f64(one, 0), one)
    with np.errstate(invalid="ignore"):
        assert mref.same_bits(mref.median_f64(one, np.arange(5), np.arange(4), 7, 1), one / one)


# ---- observation.high_pass with a window -------------------------------------------------------------------------------
def test_high_pass_with_a_window_equals_both_references_on_permuted_overlapping_orders():
    from prometheus_amd import observation as obs
    rng = np.random.default_rng(9)
    n_pix = 700
    orders = rng.permutation(np.repeat([7, 2, 5], [300, 250, 150]))
    px = 5890e-8 + 1e-10 * rng.permutation(n_pix)
    ins = obs.Instrument(px, resolving_power=1e5)
    ex = obs.Exposures(ins, [[0]], [[1.0]], np.ones((1, 1, 1)), np.ones(n_pix), np.full(n_pix, 1e-3))
    a = np.stack([special_row(rng, n_pix) for _ in range(6)]).reshape(2, 3, n_pix)
    a[0, 1, 50:60] = np.nan
    a[1, :, 699] = np.nan
    for h, mode in ((12, "subtract"), (40, "divide"), (0, "subtract"), (1, "divide"), (512, "subtract")):
        win = obs.median_window(h)
        hp = obs.HighPass(ex, win, orders=orders, mode=mode)
        assert hp.kind == "median" and hp.taps is None and hp.half_width == h
        assert hp.n_seg == 3 and list(np.diff(hp.seg_first)) == [250, 150, 300]
        got = obs.high_pass(a, win, orders=orders, mode=mode)
        want = mref.median_f64(ins.sort(a), hp.seg_first, hp.perm, h, hp.mode_id)
        assert mref.same_bits(ins.sort(got), want), (h, mode)
        zero_B = (mref.median_B(ins.sort(a), hp.seg_first, hp.perm, h) == 0) & (hp.mode_id == 1)
        other = mref.median_np(ins.sort(a), hp.seg_first, hp.perm, h, hp.mode_id)
        assert mref.median_equal(np.where(zero_B, 0.0, ins.sort(got)), np.where(zero_B, 0.0, other))
        assert np.isnan(got[np.isnan(a)]).all()
    # one order, a plain row, against the loop directly
    row = special_row(rng, 90)
    assert mref.same_bits(obs.high_pass(row, obs.median_window(4)), row - mref.running_median_f64(row, 4))
    # the mean stands as it was
    assert np.array_equal(obs.high_pass(a, obs.box_taps(3), orders=orders),
                          ins.unsort(href.highpass_f64(ins.sort(a), hp.seg_first, hp.perm, np.ones(4), 0)),
                          equal_nan=True)


def test_median_window_and_highpass_refusals_and_keys():
    from prometheus_amd import observation as obs
    assert obs.median_window(0).half_width == 0 and obs.median_window(np.int64(512)).half_width == 512
    assert isinstance(obs.median_window(3), obs.MedianWindow)
    for bad in (-1, 513, 1.5, 3.0, "3", None, True, np.nan):
        with pytest.raises(ValueError):
            obs.median_window(bad)
    px = 5890e-8 + 1e-10 * np.arange(4)
    ins = obs.Instrument(px, resolving_power=1e5)
    rows, w, F = np.array([[0, 1], [1, 2], [0, 2]]), np.full((3, 2), 0.5), np.ones((3, 4, 2))
    ex = obs.Exposures(ins, rows, w, F, np.ones((3, 4)), np.full((3, 4), 1e-3))
    win = obs.median_window(1)
    hp = obs.HighPass(ex, win, orders=[1, 0, 1, 0], mode="divide")
    assert (hp.kind, hp.taps, hp.n_seg, hp.half_width, hp.mode_id) == ("median", None, 2, 1, 1)
    assert hp.exposures_key == ex.key and list(hp.seg_first) == [0, 2, 4] and list(hp.perm) == [1, 3, 0, 2]
    mean = obs.HighPass(ex, obs.box_taps(1), orders=[1, 0, 1, 0], mode="divide")
    assert mean.kind == "mean" and mean.taps is not None and mean.key != hp.key
    assert obs.HighPass(ex, obs.median_window(1), orders=[1, 0, 1, 0], mode="divide").key == hp.key
    assert obs.HighPass(ex, obs.median_window(2), orders=[1, 0, 1, 0], mode="divide").key != hp.key
    assert obs.HighPass(ex, win, orders=[1, 0, 1, 0]).key != hp.key
    assert obs.HighPass(ex, win, orders=[1, 0, 0, 1], mode="divide").key != hp.key
    assert "median" in hp.key and 1 in hp.key
    for bad in (dict(orders=[0, 1, 0]), dict(mode="median"), dict(mode=0)):
        args = dict(taps=win, orders=None, mode="subtract")
        args.update(bad)
        with pytest.raises(ValueError):
            obs.HighPass(ex, **args)
        with pytest.raises(ValueError):
            obs.high_pass(np.ones((2, 4)), **args)
    with pytest.raises(TypeError):
        obs.HighPass(ex, win, orders=[0.5, 1.0, 0.0, 1.0])
    with pytest.raises(TypeError):
        obs.HighPass(ins, win)
    with pytest.raises(TypeError):
        obs.high_pass(np.ones((2, 4)), win, orders=np.linspace(0.0, 1.0, 4))


def test_numpy_pipeline_finds_the_planted_planet_with_a_median_continuum():
    """test_sysrem_cpu's all-numpy pipeline on the planted-planet design with a running median over 33 pixels divided
    out of data and model in the place of the Gaussian mean: it peaks at the injected trial, and the raw data alone do
    not.  (The window is several line widths and a sixth of an order: half widths of 24 and more begin to follow the
    blaze's curvature less well than SYSREM's two components absorb, and the peak moves to the last trial.)"""
    import json
    from helpers import expose_ref as eref
    from helpers import sysrem_ref as sref
    from oracle import prom_oracle as O
    from prometheus_amd import celestialBodies as bodies
    from prometheus_amd import observation as obs
    g = np.load(os.path.join(REPO, "tests", "golden", "transit_C1.npz"))
    cfg = json.loads(str(g["config"]))
    cfg["Grids"].update(sref.PLANET_CFG)
    wav, orb, R = O.run_setup(cfg)
    d = sref.planet_design(bodies.AvailablePlanets().findPlanet(cfg["Architecture"]["planetName"]), orb)
    d = dict(d, taps=obs.median_window(16))
    ins = d["ins"]
    ex = obs.Exposures(ins, d["rows"], d["a"], d["F"], d["raw"], d["err"])
    M = eref.expose(wav, R, ins.lam, ins.sig, ins.truncate, d["rows"], d["a"], d["F"], ex.data, ex.ivar)[2]
    M = ins.unsort(M.astype(np.float64))
    D = sref.inject_f64(d["raw"], M[:, sref.PLANET_TRIAL], 1.0)
    flat = obs.high_pass(D, d["taps"], orders=d["orders"], mode=d["mode"])
    Ub, clean = obs.sysrem(flat, d["err"], d["n_comp"], d["n_iter"], ones=d["ones"])
    ll = sref.numpy_recovery(d, M, clean, Ub)
    print("planted planet, median, numpy: logL - max per trial", ll - ll.max())
    assert int(np.argmax(ll)) == sref.PLANET_TRIAL
    flat0 = obs.high_pass(d["raw"], d["taps"], orders=d["orders"], mode=d["mode"])
    U0, clean0 = obs.sysrem(flat0, d["err"], d["n_comp"], d["n_iter"], ones=d["ones"])
    assert int(np.argmax(sref.numpy_recovery(d, M, clean0, U0))) != sref.PLANET_TRIAL
