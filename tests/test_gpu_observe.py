"""The observation on the device (prom_observe_set / prom_spectrum_observe / prom_transit_observe, Transit.observe)
against the longdouble reference of tests/helpers/observe_ref.py.  Marked ``gpu``.

Tolerance for M = num / den (ref.m_tolerance, derived from the definition, not from the kernel): the terms are
non-negative, so a sum of n terms in any order errs by at most (n - 1) u; z is exact up to two roundings and the
exponent is at most k^2 / 2, so with the 1-ulp exp of the device library a weight is off by at most about
(1.5 k^2 + 2) u; a ratio of positively weighted sums moves by at most twice the weights' relative error:
|M_dev - M_ref| <= (3 k^2 + 2 n_max + 16) 2^-53 |M_ref|, n_max the largest support count of the case.  den alone is
one such sum: half the bound holds for it, the whole is asserted.

Every test prints its largest error as a fraction of its bound (``OBSERVE_ERR``; profiles/observe_errors.txt).
"""
import json
import os
import re

import numpy as np
import pytest

from helpers import observe_ref as ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
LD = np.longdouble
_hdr = open(os.path.join(REPO, "prometheus_amd", "csrc", "obs_index.h")).read()
TILE = int(re.search(r"kObsTile = (\d+)", _hdr).group(1))
STAGE = int(re.search(r"kObsStage = (\d+)", _hdr).group(1))
E_ARG, E_STATE = "PROM_E_ARG", "PROM_E_STATE"


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


def observe(dev, wav, R, lam, sig, k, f=None, data=None, ivar=None, edges=(np.nan, np.nan), partials=True, chi2=False):
    R = np.atleast_2d(R)
    dev.observe_set(lam, sig, k, R.shape[0], f, data, ivar)
    return dev.spectrum_observe(wav, R, edges[0], edges[1], partials=partials, chi2=chi2)


def report(name, frac):
    print("OBSERVE_ERR %s %.4f of the bound" % (name, frac))


def check(name, out, want, k, extra=""):
    """Device (num, den) against the reference's: equal NaN / coverage masks, M and den within the bound.  Returns
    the largest error as a fraction of the bound."""
    num, den = out[0], out[1]
    rnum, rden, cnt = want
    assert num.shape == rnum.shape and den.shape == rden.shape
    Md, Mr = ref.model(num, den), ref.model(rnum, rden)
    assert np.array_equal(den == 0, rden == 0), name     # (a one-point grid without edges has q = 0: den is 0)
    assert np.array_equal(np.isnan(Md), np.isnan(Mr)), name
    ok = ~np.isnan(Mr)
    frac = 0.0
    if ok.any():
        tol = ref.m_tolerance(k, cnt.max())
        eM = np.abs(Md[ok].astype(LD) - Mr[ok]) / np.abs(Mr[ok])
        eD = np.abs(den[ok].astype(LD) - rden[ok]) / rden[ok]
        frac = float(max(eM.max(), eD.max()) / tol)
    report(name + extra, frac)
    assert frac <= 1.0, (name, frac)
    return frac


# ---- smallest shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_wav", [1, 2, 63, 64, 65, STAGE - 1, STAGE, STAGE + 1])
def test_smallest_shapes(dev, n_wav):
    """A non-uniform grid with 10x spacing jumps inside the supports and duplicated points, duplicated pixels, pixels
    beyond both ends and widths too small to reach a node; n_pix 0, 1 and about the tile, n_orb 1, 3, 17."""
    wav = ref.grid_nonuniform(n_wav)
    worst = 0.0
    for n_orb in (1, 3, 17):
        R = ref.spectrum(wav, n_orb)
        for n_pix in (0, 1, TILE - 1, TILE, TILE + 1):
            lam = ref.pixels_over(wav, n_pix)
            sig = np.full(n_pix, 2.5e-10)
            sig[::7] = 1e-13
            out = observe(dev, wav, R, lam, sig, 5.0)
            assert out[0].shape == (n_orb, n_pix)
            if n_pix:
                worst = max(worst, check("shapes", out, ref.observe(wav, R, lam, sig, 5.0), 5.0,
                                         " n_wav=%d n_orb=%d n_pix=%d" % (n_wav, n_orb, n_pix)))
    # the same grid as a shard between two neighbours (a one-point grid then has a weight)
    edges = (wav[0] - 3e-11, wav[-1] + 7e-11)
    lam, sig = ref.pixels_over(wav, TILE + 1), np.full(TILE + 1, 2.5e-10)
    want = ref.observe(wav, R, lam, sig, 5.0, None, *edges)
    assert (want[1] > 0).any()
    worst = max(worst, check("shapes", observe(dev, wav, R, lam, sig, 5.0, edges=edges), want, 5.0,
                             " n_wav=%d with edges" % n_wav))
    report("test_smallest_shapes[%d]" % n_wav, worst)


# ---- truncation boundary ---------------------------------------------------------------------------------------
def test_truncation_boundary_is_inclusive(dev):
    """Dyadic grid, pixels on nodes, k = 4 and sig = 2 spacings: c is exactly 8 spacings, the points at +-8 spacings
    are in (17 points); with sig one ulp smaller they are out (15).  A boundary point carries e^-8 of the central
    weight, 7e-5 of den: den within the bound of the reference's tells the counts are equal."""
    wav = ref.grid_dyadic(400)
    R = ref.spectrum(wav, 3)
    lam = wav[[8, 9, 100, 101, 250, 390, 391]]
    for sig0, n in ((2 * ref.DYADIC_STEP, 17), (np.nextafter(2 * ref.DYADIC_STEP, 0.0), 15)):
        sig = np.full(len(lam), sig0)
        want = ref.observe(wav, R, lam, sig, 4.0)
        assert np.all(want[2] == n)
        out = observe(dev, wav, R, lam, sig, 4.0)
        check("test_truncation_boundary_is_inclusive[%d]" % n, out, want, 4.0)
    # the two references differ by far more than the bound, so the check above tells 17 from 15
    a = ref.observe(wav, R, lam, np.full(len(lam), 2 * ref.DYADIC_STEP), 4.0)[1]
    assert np.all(np.abs(a - want[1]) / a > 1e3 * ref.m_tolerance(4.0, 17))


# ---- empty supports --------------------------------------------------------------------------------------------
def test_empty_supports_give_zero_and_nan(dev):
    wav = ref.grid_coarse_fine(300, 40)
    R = ref.spectrum(wav, 3)
    lam = np.sort(np.concatenate([[wav[0] - 1e-7, wav[0] - 1e-9, wav[-1] + 1e-9, wav[-1] + 1e-6],
                                  0.5 * (wav[5:30] + wav[6:31]), wav[35:45]]))
    sig = np.full(len(lam), 1e-11)     # k sig = 0.5e-10: between the coarse nodes (2e-9 apart) nothing
    want = ref.observe(wav, R, lam, sig, 5.0)
    assert (want[2] == 0).sum() >= 3 * 29 and (want[2] > 0).any()
    out = observe(dev, wav, R, lam, sig, 5.0)
    check("test_empty_supports_give_zero_and_nan", out, want, 5.0)
    empty = want[2] == 0
    assert np.all(out[0][empty] == 0) and np.all(out[1][empty] == 0)


# ---- wide supports ---------------------------------------------------------------------------------------------
def test_wide_supports_fall_back_to_global_reads(dev):
    """A width that makes the whole grid one pixel's support (far more than the stage holds) beside ordinary pixels of
    the same tile, and a tile that spans the coarse / fine boundary."""
    wav = ref.grid_coarse_fine(1200, 150)
    assert len(wav) > 2 * STAGE
    R = ref.spectrum(wav, 9)
    lam = ref.pixels_over(wav, 2 * TILE + 3, outside=False)
    sig = lam / (140000.0 * 2.3548)
    sig[5] = 1.0
    sig[TILE + 1] = 2e-9
    want = ref.observe(wav, R, lam, sig, 5.0)
    assert want[2][0, 5] == len(wav) and STAGE < want[2][0, TILE + 1] < len(wav)
    assert ((want[2][0] > 0) & (want[2][0] <= STAGE)).sum() > TILE
    check("test_wide_supports_fall_back_to_global_reads", observe(dev, wav, R, lam, sig, 5.0), want, 5.0)


# ---- NaN in R --------------------------------------------------------------------------------------------------
def test_nan_in_r_reaches_exactly_its_pixels(dev):
    wav = ref.grid_nonuniform(800)
    R = ref.spectrum(wav, 3)
    R[1, 417] = np.nan
    lam = ref.pixels_over(wav, 3 * TILE)
    sig = np.full(len(lam), 2.5e-10)
    sig[::5] = 1.0     # fallback pixels hold it too
    want = ref.observe(wav, R, lam, sig, 5.0)
    hit = np.isnan(want[0])
    assert hit[1].any() and not hit[1].all() and not hit[0].any() and not hit[2].any()
    out = observe(dev, wav, R, lam, sig, 5.0)
    assert np.array_equal(np.isnan(out[0]), hit) and not np.isnan(out[1]).any()
    check("test_nan_in_r_reaches_exactly_its_pixels", out, want, 5.0)


# ---- frame factors ---------------------------------------------------------------------------------------------
def test_frame_factors(dev):
    wav = ref.grid_nonuniform(1500)
    n_orb = 5
    R = ref.spectrum(wav, n_orb)
    lam = ref.pixels_over(wav, 2 * TILE + 1)
    sig = np.full(len(lam), 2.5e-10)
    a = observe(dev, wav, R, lam, sig, 5.0)
    b = observe(dev, wav, R, lam, sig, 5.0, f=np.ones(n_orb))
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])
    f = 1.0 + 1e-4 * np.linspace(-1.0, 1.0, n_orb)
    want = ref.observe(wav, R, lam, sig, 5.0, f)
    assert len({tuple(c) for c in want[2]}) == n_orb     # the supports differ per phase
    check("test_frame_factors", observe(dev, wav, R, lam, sig, 5.0, f=f), want, 5.0)


# ---- determinism -----------------------------------------------------------------------------------------------
def test_two_calls_agree_bitwise(dev):
    wav = ref.grid_coarse_fine(1200, 150)
    R = ref.spectrum(wav, 17)
    lam = ref.pixels_over(wav, 5 * TILE + 7)
    sig = lam / (140000.0 * 2.3548)
    sig[::11] = 1.0
    rng = np.random.default_rng(9)
    data, ivar = 1.0 - 0.2 * rng.random((17, len(lam))), 1e4 * rng.random((17, len(lam)))
    a = observe(dev, wav, R, lam, sig, 5.0, data=data, ivar=ivar, chi2=True)
    b = observe(dev, wav, R, lam, sig, 5.0, data=data, ivar=ivar, chi2=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


# ---- sharding --------------------------------------------------------------------------------------------------
def test_chunks_with_edges_combine(dev):
    """The same grid as 1, 2, 3 and 7 chunks, each passing its neighbours' grid points as edges: the combined M is
    within the tolerance of the one-chunk M, and of the reference."""
    from prometheus_amd import _native
    wav = ref.grid_nonuniform(1300)
    R = ref.spectrum(wav, 3)
    lam = ref.pixels_over(wav, 2 * TILE + 5)
    sig = np.full(len(lam), 2.5e-10)
    f = np.array([1.0 - 2e-5, 1.0, 1.0 + 1e-5])
    want = ref.observe(wav, R, lam, sig, 5.0, f)
    one = observe(dev, wav, R, lam, sig, 5.0, f=f)
    M1 = ref.model(one[0], one[1])
    tol = ref.m_tolerance(5.0, want[2].max())
    worst = 0.0
    for n in (1, 2, 3, 7):
        cuts = np.linspace(0, len(wav), n + 1).astype(int)
        num, den = np.zeros_like(one[0]), np.zeros_like(one[1])
        for a, b in zip(cuts[:-1], cuts[1:]):
            part = dev.spectrum_observe(wav[a:b], R[:, a:b], wav[a - 1] if a else np.nan,
                                        wav[b] if b < len(wav) else np.nan)
            num += part[0]
            den += part[1]
        M = ref.model(num, den)
        assert np.array_equal(np.isnan(M), np.isnan(M1))
        ok = ~np.isnan(M1)
        worst = max(worst, float(np.max(np.abs(M[ok] - M1[ok]) / np.abs(M1[ok])) / tol))
        assert worst <= 1.0
        check("chunks", (num, den), want, 5.0, " n=%d" % n)
    report("test_chunks_with_edges_combine", worst)
    data = np.ones_like(one[0])
    dev.observe_set(lam, sig, 5.0, 3, f, data, data)
    with pytest.raises(_native.NativeError, match=E_ARG):
        dev.spectrum_observe(wav[:700], R[:, :700], np.nan, wav[700], chi2=True)
    with pytest.raises(_native.NativeError, match=E_ARG):
        dev.spectrum_observe(wav[700:], R[:, 700:], wav[699], np.nan, partials=False, chi2=True)


# ---- chi-square ------------------------------------------------------------------------------------------------
def test_chi_square(dev):
    """chi2 and n_used against the longdouble sum formed from the device's own M: the terms are non-negative, so
    any order of the n_used terms (each with 3 roundings) stays within (n_used + 4) 2^-53 relative.  Masked pixels:
    ivar 0, negative, infinite and NaN, NaN and infinite data, den 0.  A used NaN M gives NaN."""
    wav = ref.grid_nonuniform(900)
    n_orb = 4
    R = ref.spectrum(wav, n_orb)
    R[3, 300] = np.nan
    lam = ref.pixels_over(wav, 10 * TILE + 3)
    sig = np.full(len(lam), 2.5e-10)
    sig[::7] = 1e-13
    rng = np.random.default_rng(4)
    data = 0.9 + 0.05 * rng.standard_normal((n_orb, len(lam)))
    ivar = 1e4 * (0.1 + rng.random((n_orb, len(lam))))
    ivar[0, 3], ivar[0, 12], ivar[1, 5], ivar[1, 9] = 0.0, -1.0, np.nan, np.inf
    data[2, 8], data[2, 20] = np.nan, np.inf
    num, den, c2, nu = observe(dev, wav, R, lam, sig, 5.0, data=data, ivar=ivar, chi2=True)
    assert (den == 0).any()
    M = ref.model(num, den)
    want, nwant = ref.chi2(M, den, data, ivar)
    assert np.array_equal(nu, nwant) and nu.dtype == np.int64
    assert np.isnan(c2[3]) and np.isnan(want[3])
    frac = 0.0
    for o in range(3):
        frac = max(frac, float(abs(c2[o] - want[o]) / want[o]) / ((nwant[o] + 4) * ref.U))
    report("test_chi_square", frac)
    assert frac <= 1.0
    # chi-square alone: nothing else is copied back, the same bits
    _, _, c2b, nub = dev.spectrum_observe(wav, R, partials=False, chi2=True)
    assert np.array_equal(c2b, c2, equal_nan=True) and np.array_equal(nub, nu)


# ---- argument and state errors ---------------------------------------------------------------------------------
def test_argument_errors(dev):
    from prometheus_amd import _native
    wav = ref.grid_nonuniform(100)
    R = ref.spectrum(wav, 2)
    lam, sig = wav[[10, 20, 30]], np.full(3, 2e-10)
    for bad in (dict(lam=lam[::-1]), dict(sig=np.array([2e-10, 0.0, 2e-10])), dict(sig=-sig), dict(k=0.0),
                dict(k=-5.0), dict(f=np.array([1.0, 0.0])), dict(lam=np.array([1.0, np.nan, 2.0]))):
        a = dict(lam=lam, sig=sig, k=5.0, n_orb=2, f=None)
        a.update(bad)
        with pytest.raises(_native.NativeError, match=E_ARG):
            dev.observe_set(a["lam"], a["sig"], a["k"], a["n_orb"], a["f"])
    # a failed set leaves no observation behind
    with pytest.raises(_native.NativeError, match=E_STATE):
        dev.spectrum_observe(wav, R)
    dev.observe_set(lam, sig, 5.0, 2)
    with pytest.raises(_native.NativeError, match=E_ARG):
        dev.spectrum_observe(wav, R[:1])                      # another n_orb
    with pytest.raises(_native.NativeError, match=E_ARG):
        dev.spectrum_observe(wav[::-1], R)                    # descending grid
    with pytest.raises(_native.NativeError, match=E_ARG):
        dev.spectrum_observe(wav, R, chi2=True)               # no data on the context
    assert dev.spectrum_observe(wav, R)[0].shape == (2, 3)


def test_state_errors():
    """Observe before set (a fresh context), and an observation dropped by a prom_transit_set with another n_orb."""
    from prometheus_amd import _native, configs, setupfile
    d = _native.Device(0)
    try:
        wav = ref.grid_nonuniform(100)
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.spectrum_observe(wav, ref.spectrum(wav, 2))
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.transit_observe()
        d.observe_set(wav[[3, 4]], np.full(2, 2e-10), 5.0, 2)
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.transit_observe()                               # no run yet
    finally:
        d.close()
    dev = _native.get_device(0)
    tr = setupfile.build_transit(configs.get("C1"))
    n_orb = tr.sumOverChords(devices=[0]).shape[0]
    dev.observe_set(tr.wavelength[[3, 4]], np.full(2, 2e-10), 5.0, n_orb)
    assert dev.transit_observe()[0].shape == (n_orb, 2)
    dev.observe_set(tr.wavelength[[3, 4]], np.full(2, 2e-10), 5.0, n_orb + 2)
    with pytest.raises(_native.NativeError, match=E_STATE):
        dev.transit_observe()                                 # the run has another n_orb
    tr.sumOverChords(devices=[0])                             # prom_transit_set drops the observation
    wav = ref.grid_nonuniform(100)
    with pytest.raises(_native.NativeError, match=E_STATE):
        dev.spectrum_observe(wav, ref.spectrum(wav, n_orb + 2))


# ---- end to end ------------------------------------------------------------------------------------------------
def _product_transit(cfg):
    from oracle import prom_oracle as O
    from prometheus_amd import gasProperties as gp
    from prometheus_amd import setupfile
    gp.register_molecular_table("H2O", O.synthetic_molecular_table(n_nu=2001))
    return setupfile.build_transit(cfg)


CHUNK = 4096      # the smallest chunk of Transit._integrate (what max_memory_gb = 1e-9 gives), in wavelengths
LEGS = (("one", dict(devices=[0])), ("two", dict(devices=[0, 0])), ("chunks", dict(devices=[0], max_memory_gb=1e-9)),
        ("two+chunks", dict(devices=[0, 0], max_memory_gb=1e-9)))


def _cuts(n_wav, kw):
    """Where a leg cuts the grid (first index of every shard and chunk but the first) and its number of runs."""
    from prometheus_amd.sharding import split
    cuts, runs = [], 0
    for lo, hi in split(n_wav, len(kw["devices"])):
        for a in range(lo, hi, CHUNK if "max_memory_gb" in kw else hi - lo):
            runs += 1
            if a > 0:
                cuts.append(a)
    return cuts, runs


def _pieces(wav, R, ins, frame, cuts, edges):
    """The reference summed over the pieces between ``cuts``, with the neighbours as edges or (wrongly) without."""
    num = den = 0
    for a, b in zip([0] + cuts, cuts + [len(wav)]):
        lo = wav[a - 1] if a and edges else np.nan
        hi = wav[b] if b < len(wav) and edges else np.nan
        n, d, _ = ref.observe(wav[a:b], R[:, a:b], ins.lam, ins.sig, ins.truncate, frame, lo, hi)
        num, den = num + n, den + d
    return num, den


@pytest.mark.parametrize("name", ["C1", "C3r", "C2r", "C3x"])
def test_transit_observe_end_to_end(name):
    """Transit.observe on the reduced golden problems C1, C3r (Doppler, 4 phases), C2r and on C3x, a reduced C3 of
    9,322 wavelengths (Doppler, 4 phases), in the model's frame and the planet's: one device, two shards, the smallest
    chunks, and both.  Each leg is compared with the reference applied to sumOverChords' R on the host (model and
    coverage), and the one-device chi-square (from the device) with the host chi-square of the cut runs.

    What the public interface can cut (asserted through the number of runs): C1 (219 wavelengths) is one shard and
    one chunk in every leg, so its legs repeat the one-device run; C3r (3,880) has two shards and one chunk; C2r
    (4,448) two shards or two chunks (a shard of it is below one chunk); C3x three chunks, or two shards of two chunks.  At every cut of every leg, in
    every phase's frame, a pixel sits between the two grid points the cut separates, wide enough to reach several
    points on either side: its num and den depend on the edges the neighbouring runs pass.  The reference's den summed
    over the same pieces WITHOUT edges misses the bound a thousandfold (asserted), and the coverage, den over the
    kernel's full weight, is held to the bound: a wrong edge cannot pass.

    The chi-square bound follows from M's: with |dM| <= 2 tol |M| between two runs,
    |d chi2| <= sum ivar (2 |M - data| |dM| + dM^2), plus the (n_used + 4) u of either sum."""
    from prometheus_amd import _native, configs
    from prometheus_amd import observation as obs
    if name == "C3x":
        tr = _product_transit(configs.reduced(configs.get("C3"), orbphase_steps=4, res_low=4e-9, res_high=2.5e-10))
    else:
        d = np.load(os.path.join(G, "transit_" + name + ".npz"))
        tr = _product_transit(json.loads(str(d["config"])))
    R = np.array(tr.sumOverChords(devices=[0]))
    wav = np.asarray(tr.wavelength)
    n_orb, n_wav = R.shape
    legs = [(key, kw) + _cuts(n_wav, kw) for key, kw in LEGS]
    assert [runs for _, _, _, runs in legs] == {"C1": [1, 1, 1, 1], "C3r": [1, 2, 1, 2], "C2r": [1, 2, 2, 2],
                                                "C3x": [1, 2, 3, 4]}[name]
    all_cuts = sorted({c for _, _, cuts, _ in legs for c in cuts})
    shifts = obs.planet_frame_shifts(tr.planet, tr.spatialGrid.constructOrbphaseAxis())
    rng = np.random.default_rng(11)
    core = wav[np.argmin(np.diff(wav))]                      # unsorted pixels: the whole range, some outside, and
    px = np.concatenate([wav[0] - 2e-9 + (wav[-1] - wav[0] + 4e-9) * rng.random(TILE),     # the finest stretch
                         core + 1e-8 * (2 * rng.random(TILE + 9) - 1)])
    sg = px / (140000.0 * obs.FWHM_PER_SIGMA)
    for c in all_cuts:                                       # ... and the pixels across the cuts, in every frame
        mid = 0.5 * (wav[c - 1] + wav[c])
        at = np.concatenate([[mid], mid / shifts])
        px = np.concatenate([px, at])
        sg = np.concatenate([sg, np.full(len(at), (wav[min(c + 3, n_wav - 1)] - wav[max(c - 4, 0)]) / 5.0)])
    order = rng.permutation(len(px))
    ins = obs.Instrument(px[order], sigma=sg[order], truncate=5.0)
    worst = 0.0
    for frame in (None, shifts):
        want = ref.observe(wav, R, ins.lam, ins.sig, ins.truncate, frame)
        Mr = ins.unsort(ref.model(want[0], want[1]))
        cov_r = ins.unsort(want[1]) / ins.full_weight(frame)
        tol = ref.m_tolerance(ins.truncate, want[2].max())
        ok = ~np.isnan(Mr)
        err = np.full(Mr.shape, 1e-3)
        data = np.where(np.isnan(Mr), 1.0, Mr.astype(np.float64)) + err * rng.standard_normal(Mr.shape)
        data[0, 1] = np.nan
        runs = {}
        for key, kw, cuts, n_runs in legs:
            o = tr.observe(ins, frame_shifts=frame, data=data, err=err, **kw)
            assert len(tr.last_stats) == n_runs, (name, key)
            runs[key] = o
            assert np.array_equal(np.isnan(o.model), np.isnan(Mr)), (name, key)
            assert np.array_equal(o.coverage == 0, cov_r == 0)
            if ok.any():
                worst = max(worst, float(np.max(np.abs(o.model[ok].astype(LD) - Mr[ok]) / np.abs(Mr[ok])) / tol),
                            float(np.max(np.abs(o.coverage[ok].astype(LD) - cov_r[ok]) / cov_r[ok]) / tol))
            assert worst <= 1.0, (name, key, worst)
            if cuts:
                # the same pieces without edges are off by more than the bound: the edges are what is tested
                wd = _pieces(wav, R, ins, frame, cuts, edges=False)[1]
                gd = _pieces(wav, R, ins, frame, cuts, edges=True)[1]
                live = want[1] > 0
                assert np.max(np.abs(gd[live] - want[1][live]) / want[1][live]) <= tol
                assert np.max(np.abs(wd[live] - want[1][live]) / want[1][live]) > 1e3 * tol, (name, key)
        one = runs["one"]
        ivar = 1.0 / (err * err)
        used = np.isfinite(data) & ~np.isnan(Mr)
        dM = 2 * tol * np.where(used, np.abs(one.model), 0.0)
        bound = np.sum(np.where(used, ivar * (2 * np.abs(np.where(used, one.model - data, 0.0)) * dM + dM * dM), 0.0), axis=1)
        bound += (one.n_used + 4) * ref.U * np.abs(one.chi2) * 2
        for key in ("two", "chunks", "two+chunks"):
            assert np.array_equal(one.n_used, runs[key].n_used)
            assert np.all(np.abs(one.chi2 - runs[key].chi2) <= bound), (name, key, one.chi2, runs[key].chi2, bound)
        # an Observation prepared once: chi-square alone crosses the bus, the same bits
        prepared = obs.Observation(ins, n_orb, frame, data, err)
        only = tr.observe(prepared, devices=[0], return_model=False)
        assert only.model is None and np.array_equal(only.chi2, one.chi2) and np.array_equal(only.n_used, one.n_used)
        assert _native.get_device(0).observe_key == prepared.key
    report("test_transit_observe_end_to_end[%s]" % name, worst)
