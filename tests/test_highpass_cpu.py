"""High-pass filtered exposures without a device: the host harness of k_highpass's index arithmetic and window function
(tests/helpers/highpass_host.cpp, a stand-alone program, plain and sanitized), the float64 reference of the filter
(tests/helpers/highpass_ref.py) and its bound, observation.high_pass / gaussian_taps / box_taps, and the refusals of
observation.HighPass and Transit.expose(highpass=...) that come before a device is needed."""
import os
import subprocess
import types

import numpy as np
import pytest

from helpers import highpass_ref as href

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "prometheus_amd", "csrc")
HOST = os.path.join(REPO, "tests", "helpers", "highpass_host.cpp")
U = 2.0 ** -53
HALVES = (0, 3, 255, 256, 300, 512)


# ---- the harness -------------------------------------------------------------------------------------------------
def _row_cases():
    """(name, row, taps, mode): rows with NaN at an edge, NaN in the middle, an all-NaN window about a valid centre's
    neighbours, a zero under division, and a row longer than a tile with a long half width."""
    rng = np.random.default_rng(23)
    row = lambda n: 1.0 - 0.05 * rng.random(n)
    gauss = lambda h, s: np.exp(-0.5 * (np.arange(h + 1) / s) ** 2)
    cases = []
    a = row(40)
    a[[0, 1, 39]] = np.nan
    cases.append(("edge NaN", a, gauss(5, 2.0), 0))
    b = row(300)
    b[[100, 101, 170]] = np.nan
    cases.append(("middle NaN", b, gauss(12, 5.0), 0))
    cases.append(("middle NaN divide", b, gauss(12, 5.0), 1))
    c = row(50)
    c[17:24] = np.nan
    c[20] = 0.9731                                   # a valid centre whose whole window (h = 3) is NaN but itself
    cases.append(("lone centre", c, np.ones(4), 0))
    cases.append(("lone centre divide", c, np.ones(4), 1))
    d = row(64)
    d[30:41] = 0.0                                   # B = 0 under division: inf and NaN by IEEE
    cases.append(("zero stretch divide", d, np.ones(3), 1))
    e = row(2600)
    e[[5, 1023, 1024, 2599]] = np.nan
    cases.append(("three tiles", e, gauss(300, 90.0), 0))
    cases.append(("h = 0", row(7), np.ones(1), 0))
    cases.append(("taps with zeros", row(90), np.array([1.0, 0.0, 0.5, 0.0, 0.25]), 1))
    return cases


def _row_file(path, M, g, mode):
    seg, perm = href.one_segment(len(M))
    want = href.highpass_f64(M, seg, perm, g, mode)
    vals = lambda a: " ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel())
    with open(path, "w") as f:
        f.write("%d %d %d\n%s\n%s\n%s\n" % (len(M), len(g) - 1, mode, vals(g), vals(M), vals(want)))
    return want


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_harness_walks_every_index_and_matches_the_reference_bitwise(tmp_path, which):
    """The walk over the segment lengths {1, 2, 255, 256, 257, 515} and one tile less one, one tile, one tile and
    one, three tiles and 452 (interleaved through perm) x h in {0, 3, 255, 256, 300, 512} x both modes finds every
    ring slot, perm entry and model value inside, every slot read holding the original of the position intended, no
    value read after it was overwritten, every model value written once and every result equal to the definition
    evaluated directly; the clean path is taken (and its claim holds) at every half width.  The given rows agree with
    highpass_f64 bit for bit."""
    flags = {"plain": ("-O2",), "sanitized": ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")}
    exe = tmp_path / "highpass_host"
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
            for name in ("ring_oor", "perm_oor", "model_oor", "slot_err", "stale_read", "visit_err", "mismatch"):
                assert " %s=0" % name in line, line
            assert "clean_waves=0 " not in line, line
            assert "workgroups=10 " in line
    for name, M, g, mode in _row_cases():
        path = tmp_path / (name.replace(" ", "_").replace("=", "") + ".txt")
        want = _row_file(path, M, g, mode)
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        print(name, r.stdout, r.stderr)
        assert r.returncode == 0 and " mismatch=0" in r.stdout and " visit_err=0" in r.stdout, name
        assert np.array_equal(np.isnan(want), np.isnan(M)) or name == "zero stretch divide", name
        if name == "lone centre":
            assert want[20] == 0.0 and not np.signbit(want[20])        # B = M: its own value is all the window has
        if name == "lone centre divide":
            assert want[20] == 1.0
        if name == "zero stretch divide":
            # (0 / 0 where the whole window is 0; a zero beside a non-zero value gives 0 / B = 0)
            assert np.isnan(want[32:39]).all() and np.all(want[[30, 31, 39, 40]] == 0.0)
            assert np.isfinite(np.delete(want, np.arange(32, 39))).all()
        if name == "h = 0":
            assert np.all(want == 0.0) and not np.signbit(want).any()


# ---- the reference and its bound -----------------------------------------------------------------------------------
def test_float64_orders_stay_inside_the_bound():
    """highpass_f64 forwards and with every window summed in reverse against highpass_ld, eps_e = 0 (M is given
    exactly), both modes, on overlapping orders with NaN: inside the derived bound; the print shows how far."""
    rng = np.random.default_rng(5)
    lengths = [1, 2, 77, 300, 620]
    seg, perm = href.interleaved(lengths, seed=3)
    M = 1.0 - 0.05 * rng.random((3, sum(lengths)))
    M[0, ::41] = np.nan
    M[1, 400:430] = np.nan
    for h, sigma in ((0, 1.0), (3, 1.5), (160, 40.0), (512, 200.0)):
        g = np.exp(-0.5 * (np.arange(h + 1) / sigma) ** 2)
        for mode in (0, 1):
            exact, bound, live = href.model_bound(M, seg, perm, g, mode, 0.0)
            assert live.sum() == (~np.isnan(M)).sum()
            worst = 0.0
            for fn in (href.highpass_f64, href.highpass_f64_reversed):
                worst = max(worst, href.model_fraction(fn(M, seg, perm, g, mode), exact, bound, live))
            print("float64 orders, h = %d mode %d: %.4f of the bound" % (h, mode, worst))
            assert worst <= 1.0


def test_reference_degenerate_cases_and_renormalisation():
    """h = 0 and segments of length 1 give +0 / 1; a constant row gives +0 / 1 for any taps whose partial sums are
    exact (a box); the window renormalises over a NaN: the neighbours of a NaN in a constant row are still +0."""
    seg1 = np.arange(6, dtype=np.int32)
    perm1 = np.array([3, 0, 4, 1, 2], dtype=np.int32)
    M = np.array([[0.5, np.nan, 2.0, 0.0, 1.25]])
    for g in (np.ones(1), np.ones(4)):
        segs = [(seg1, perm1)] + ([href.one_segment(5)] if len(g) == 1 else [])
        for seg, perm in segs:
            sub = href.highpass_f64(M, seg, perm, g, 0)
            div = href.highpass_f64(M, seg, perm, g, 1)
            ok = ~np.isnan(M)
            assert np.array_equal(np.isnan(sub), ~ok) and np.all(sub[ok] == 0.0) and not np.signbit(sub[ok]).any()
            assert np.all(div[ok & (M != 0)] == 1.0) and np.isnan(div[M == 0]).all()
    seg, perm = href.one_segment(40)
    C = np.full((1, 40), 0.75)
    C[0, 11] = np.nan
    sub = href.highpass_f64(C, seg, perm, np.ones(6), 0)
    assert np.isnan(sub[0, 11]) and np.all(np.delete(sub[0], 11) == 0.0)


# ---- observation.high_pass and the taps ----------------------------------------------------------------------------
def test_high_pass_equals_the_reference_bitwise_on_permuted_overlapping_orders():
    """The library's high_pass in the caller's pixel order against highpass_f64 in the device's: three orders whose
    wavelengths overlap, given in descending wavelength with the orders' pixels shuffled together."""
    from prometheus_amd import observation as obs
    rng = np.random.default_rng(9)
    n_pix = 700
    orders = rng.permutation(np.repeat([7, 2, 5], [300, 250, 150]))
    px = 5890e-8 + 1e-10 * rng.permutation(n_pix)                    # any order: overlapping echelle orders
    ins = obs.Instrument(px, resolving_power=1e5)
    ex = obs.Exposures(ins, [[0]], [[1.0]], np.ones((1, 1, 1)), np.ones(n_pix), np.full(n_pix, 1e-3))
    a = 1.0 - 0.05 * rng.random((2, 3, n_pix))
    a[0, 1, 50:60] = np.nan
    a[1, :, 699] = np.nan
    for taps, mode in ((obs.gaussian_taps(12.0), "subtract"), (obs.box_taps(40), "divide"), (obs.box_taps(0), "subtract")):
        hp = obs.HighPass(ex, taps, orders=orders, mode=mode)
        assert hp.n_seg == 3 and list(np.diff(hp.seg_first)) == [250, 150, 300]      # ascending label: 2, 5, 7
        assert sorted(hp.perm) == list(range(n_pix)) and hp.perm.dtype == np.int32 and hp.seg_first.dtype == np.int32
        want = href.highpass_f64(ins.sort(a), hp.seg_first, hp.perm, hp.taps, hp.mode_id)
        got = obs.high_pass(a, taps, orders=orders, mode=mode)
        assert np.array_equal(ins.sort(got), want, equal_nan=True)
        assert np.array_equal(np.isnan(got), np.isnan(a))
    # position inside an order is the rank in the caller's order
    hp = obs.HighPass(ex, obs.box_taps(1), orders=orders)
    first = np.flatnonzero(orders == 2)[:3]
    assert np.array_equal(ins.order[hp.perm[:3]], first)
    # one order: the caller's order as it stands
    hp1 = obs.HighPass(ex, obs.box_taps(1))
    assert hp1.n_seg == 1 and np.array_equal(ins.order[hp1.perm], np.arange(n_pix))


def test_taps():
    from prometheus_amd import observation as obs
    g = obs.gaussian_taps(40.0)
    assert len(g) == 161 and g[0] == 1.0 and np.all(np.diff(g) < 0) and abs(g[160] - np.exp(-8.0)) < 1e-15
    assert len(obs.gaussian_taps(0.1)) == 1 and len(obs.gaussian_taps(128.0)) == 513
    assert np.array_equal(obs.box_taps(3), np.ones(4)) and np.array_equal(obs.box_taps(0), np.ones(1))
    for bad in (lambda: obs.gaussian_taps(0.0), lambda: obs.gaussian_taps(np.nan), lambda: obs.gaussian_taps(129.0),
                lambda: obs.gaussian_taps(10.0, truncate=-1.0), lambda: obs.box_taps(513), lambda: obs.box_taps(-1),
                lambda: obs.box_taps(1.5)):
        with pytest.raises(ValueError):
            bad()
    a = np.ones((2, 9))
    for bad in (dict(taps=np.ones(514)), dict(taps=np.ones((2, 2))), dict(taps=[0.0, 1.0]), dict(taps=[1.0, -0.5]),
                dict(taps=[1.0, np.nan]), dict(taps=[]), dict(mode="high"), dict(orders=np.zeros(8, dtype=int))):
        args = dict(taps=np.ones(2), orders=None, mode="subtract")
        args.update(bad)
        with pytest.raises(ValueError):
            obs.high_pass(a, **args)
    with pytest.raises(TypeError):
        obs.high_pass(a, np.ones(2), orders=np.linspace(0.0, 1.0, 9))


# ---- HighPass and Transit.expose(highpass=...) without a device ----------------------------------------------------
def _bare_transit(n_wav, n_orb):
    """A Transit with a grid and phases and nothing a device could run: expose must refuse before it needs one."""
    from prometheus_amd import gasProperties as gp
    tr = gp.Transit.__new__(gp.Transit)
    tr.wavelength = 5880e-8 + 1e-11 * np.arange(n_wav)
    tr.spatialGrid = types.SimpleNamespace(constructOrbphaseAxis=lambda: np.linspace(-0.03, 0.03, n_orb))
    tr.atmosphere = types.SimpleNamespace(densityDistributionList=[])
    tr.last_stats, tr.collect_stats = [], False
    return tr


def test_highpass_and_expose_refuse_before_touching_a_device(monkeypatch):
    from prometheus_amd import _native
    from prometheus_amd import observation as obs

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_native, "get_device", no_device)
    monkeypatch.setattr(_native, "device_count", no_device)
    tr = _bare_transit(20000, 3)
    ins = obs.Instrument(tr.wavelength[[300, 100, 200, 150]], resolving_power=140000.0)
    rows, a, F = np.array([[0, 1], [1, 2], [0, 2]]), np.full((3, 2), 0.5), np.ones((3, 4, 2))
    data, err = np.ones((3, 4)), np.full((3, 4), 1e-3)
    ex = obs.Exposures(ins, rows, a, F, data, err)
    hp = obs.HighPass(ex, obs.box_taps(1), orders=[1, 0, 1, 0], mode="divide")
    assert (hp.n_seg, hp.half_width, hp.mode_id) == (2, 1, 1) and hp.exposures_key == ex.key
    # the caller's pixels 1 and 3 (order 0) are the device's 0 and 1, pixels 0 and 2 (order 1) the device's 3 and 2
    assert list(hp.seg_first) == [0, 2, 4] and list(hp.perm) == [0, 1, 3, 2]
    assert obs.HighPass(ex, obs.box_taps(1), orders=[1, 0, 1, 0], mode="divide").key == hp.key
    assert obs.HighPass(ex, obs.box_taps(1), orders=[1, 0, 1, 0]).key != hp.key
    assert obs.HighPass(ex, obs.box_taps(2), orders=[1, 0, 1, 0], mode="divide").key != hp.key
    assert obs.HighPass(ex, obs.box_taps(1), orders=[1, 0, 0, 1], mode="divide").key != hp.key
    for bad in (dict(taps=np.ones(514)), dict(taps=[0.0, 1.0]), dict(taps=[1.0, np.inf]), dict(taps=[1.0, -1.0]),
                dict(taps=np.ones((2, 2))), dict(orders=[0, 1, 0]), dict(orders=np.zeros((2, 2), dtype=int)),
                dict(mode="median"), dict(mode=0)):
        args = dict(taps=obs.box_taps(1), orders=None, mode="subtract")
        args.update(bad)
        with pytest.raises(ValueError):
            obs.HighPass(ex, **args)
    with pytest.raises(TypeError):
        obs.HighPass(ex, obs.box_taps(1), orders=[0.5, 1.0, 0.0, 1.0])
    with pytest.raises(TypeError):
        obs.HighPass(ins, obs.box_taps(1))
    with pytest.raises(TypeError, match="observation.HighPass"):
        tr.expose(ex, highpass=obs.box_taps(1))
    other = obs.Exposures(ins, rows, a, F, data * 1.5, err)
    with pytest.raises(ValueError, match="HighPass was made for other exposures"):
        tr.expose(other, highpass=hp)
    dt = obs.Detrend(ex, np.ones((3, 1)))
    with pytest.raises(ValueError, match="Detrend was made for other exposures"):
        tr.expose(other, highpass=obs.HighPass(other, obs.box_taps(1)), detrend=dt)
    with pytest.raises(ValueError, match="not additive over wavelength partials"):    # the plain refusals stand
        tr.expose(ex, highpass=hp, detrend=dt, devices=[0, 1])
