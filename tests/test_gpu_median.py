"""Median high-pass on the device (prom_highpass_set_median, observation.median_window) against the references of
tests/helpers/median_ref.py.  Marked ``gpu``.

The running median is a selection, so every comparison is bit for bit: the device's filtered model must be median_f64
of prom_spectrum_expose's own model_out, NaN pattern included, and n_used exact; every chain that runs the resident
high-pass (the SYSREM filter, the per-order moments, clean, inject, recover and the grids) must give with a median what
the numpy route through observation.high_pass and the existing references gives.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import detrend_ref as dref
from helpers import highpass_ref as href
from helpers import median_ref as mref
from helpers import order_ref as oref
from helpers import sysrem_ref as sref
from test_gpu_highpass import design, gauss, same, table, upload
import test_gpu_sysrem as ts

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_STATE = "PROM_E_ARG", "PROM_E_STATE"
TILE = 1024              # outputs of a k_median tile (highpass_index.h's)
HALVES = (0, 1, 3, 255, 256, 512)
LENGTHS = (1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 5)
PLANET_HALF = 16         # the planted planet's window: 33 of an order's 200 pixels, several line widths


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


planet = ts.planet   # (the module's fixture: reduced C1 and the planted-planet design)


def both(dev, d, seg, perm, h, mode, filt=None):
    """(prom_spectrum_expose's, prom_spectrum_expose_highpass's with the median resident) outputs of design d."""
    upload(dev, d)
    plain = dev.spectrum_expose(d["wav"], d["R"], model=True)
    dev.highpass_set_median(seg, perm, h, mode)
    if filt is not None:
        dev.detrend_set(*filt)
    return plain, dev.spectrum_expose_highpass(d["wav"], d["R"], detrend=filt is not None, model=True)


def check(name, d, seg, perm, h, mode, plain, out, filt=None):
    """The device's model bit for bit against median_f64 (then filter_f64) of the unfiltered model, n_used exact, no
    NaN moment."""
    mom, nu, model = out
    want = mref.median_f64(plain[2], seg, perm, h, mode)
    ok = np.ones(want.shape[1:], dtype=bool)
    if filt is not None:
        want, ok = dref.filter_f64(want, *filt)
    assert model.shape == want.shape and nu.dtype == np.int64
    assert np.array_equal(np.isnan(model), np.isnan(want)), name
    assert mref.same_bits(model, want), name
    with np.errstate(invalid="ignore"):
        good = np.isfinite(d["ivar"]) & (d["ivar"] > 0) & np.isfinite(d["data"])
    used = good[:, None, :] & ok[None, :, :] & ~np.isnan(want)
    assert np.array_equal(nu, used.sum(axis=2)), name
    assert not np.isnan(mom).any() or not np.isfinite(want[used]).all(), name
    return want


# ---- 1: the sweep over the lengths x half widths x modes -------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep(dev):
    """One design whose segments have the harness' lengths, dealt over the device's pixel order at random (every second
    one reversed), some pixels without a model: the plain exposures once, shared by the sweep."""
    d = design(3, sum(LENGTHS), 3)
    seg, perm = href.interleaved(LENGTHS, seed=4)
    upload(dev, d)
    plain = dev.spectrum_expose(d["wav"], d["R"], model=True)
    assert np.isnan(plain[2]).any() and np.isfinite(plain[2]).any()
    return d, seg, perm, plain


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("h", HALVES)
def test_model_bitwise_over_lengths_and_half_widths(dev, sweep, h, mode):
    d, seg, perm, plain = sweep
    plain2, out = both(dev, d, seg, perm, h, mode)
    assert same(plain2, plain)
    want = check("sweep h=%d mode=%d" % (h, mode), d, seg, perm, h, mode, plain, out)
    if h == 0:       # B = M: +0 or 1 wherever M is valid (and not 0)
        valid = ~np.isnan(plain[2])
        assert np.all(want[valid] == (0.0, 1.0)[mode]) and not np.signbit(want[valid]).any()


# ---- 2: other designs ---------------------------------------------------------------------------------------------------
def test_orders_interleaved_and_reversed_with_nan_in_R_bitwise(dev):
    """Two orders interleaved pixel by pixel, then one order reversed; NaN sprinkled in R makes pixels without a
    model in the interior, so windows with an even count occur there as well as at the ends."""
    n = 2 * 350
    d = design(3, n, 3, outside=False)
    Rn = d["R"].copy()
    Rn[:, np.random.default_rng(2).choice(Rn.shape[1], 25, replace=False)] = np.nan
    d = dict(d, R=Rn)
    seg = np.array([0, n // 2, n], dtype=np.int32)
    perm = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)]).astype(np.int32)
    plain, out = both(dev, d, seg, perm, 20, 0)
    hit = np.isnan(plain[2])
    assert hit[..., 40:-40].any() and not hit.all()
    check("two interleaved orders", d, seg, perm, 20, 0, plain, out)
    seg1, fwd = href.one_segment(n)
    rev = fwd[::-1].copy()
    plain, out_r = both(dev, d, seg1, rev, 7, 1)
    check("one reversed order", d, seg1, rev, 7, 1, plain, out_r)
    # a median does not know the direction: the forward order gives the same values at the same pixels
    out_f = both(dev, d, seg1, fwd, 7, 1)[1]
    assert mref.same_bits(out_f[2], out_r[2])


def test_ties_dominate_bitwise(dev):
    """R quantised to a few values: the model holds few distinct values and most windows are full of ties."""
    d = design(3, 1500, 3, outside=False)
    d = dict(d, R=np.round(d["R"] * 4.0) / 4.0)
    seg, perm = href.interleaved((1100, 400), seed=6)
    for h, mode in ((160, 0), (5, 1)):
        plain, out = both(dev, d, seg, perm, h, mode)
        assert len(np.unique(plain[2])) < plain[2].size // 4          # (most values have a twin)
        check("ties h=%d" % h, d, seg, perm, h, mode, plain, out)


def test_zeros_and_infinities_planted_through_R_bitwise(dev):
    """A hand-made R with stretches of +0, -0, +inf and -inf: the model holds zeros and both infinities (and NaN where
    a support meets both), and the filtered model is the definition's with what IEEE gives for inf - inf and 0 / 0."""
    d = design(3, 600, 3, outside=False)
    Rs = d["R"].copy()
    Rs[:, 200:330] = 0.0
    Rs[:, 330:420] = -0.0
    Rs[:, 600:700] = np.inf
    Rs[:, 900:1000] = -np.inf
    Rs[0, 1200:1210] = np.inf
    Rs[0, 1210:1220] = -np.inf
    d = dict(d, R=Rs)
    seg, perm = href.interleaved((450, 150), seed=7)
    for h, mode in ((3, 0), (30, 1), (300, 0)):
        plain, out = both(dev, d, seg, perm, h, mode)
        M = plain[2]
        assert (M == 0).any() and np.isposinf(M).any() and np.isneginf(M).any() and np.isfinite(M).any()
        check("specials h=%d mode=%d" % (h, mode), d, seg, perm, h, mode, plain, out)


def test_a_window_that_is_all_nan_but_its_centre_bitwise(dev):
    """The positions of one order are arranged so that a pixel with a model stands between pixels without one (they lie
    beyond the grid's ends): its window holds its own value alone, B = M, so M' is +0 or 1."""
    d = design(3, 300, 3)
    upload(dev, d)
    M = dev.spectrum_expose(d["wav"], d["R"], model=True)[2]
    gone = np.flatnonzero(np.isnan(M).all(axis=(0, 1)))
    live = np.flatnonzero(~np.isnan(M).any(axis=(0, 1)))
    h = 2
    assert len(gone) >= 2 * h and len(live) > 10
    head = np.concatenate([gone[:h], live[:1], gone[h:2 * h]])
    perm = np.concatenate([head, np.setdiff1d(np.arange(300), head)]).astype(np.int32)
    seg = np.array([0, 300], dtype=np.int32)
    for mode in (0, 1):
        plain, out = both(dev, d, seg, perm, h, mode)
        check("lone centre mode=%d" % mode, d, seg, perm, h, mode, plain, out)
        lone = out[2][..., live[0]]
        assert np.all(lone == (0.0, 1.0)[mode]) and not np.signbit(lone).any()


def test_zero_stretch_under_division_bitwise(dev):
    """R = 0 over a stretch wider than a support plus the window: M = 0 and B = 0 there, 0 / 0 is NaN and the pixel is
    unused.  No moment is NaN."""
    d = design(3, 400, 3, outside=False)
    Rz = d["R"].copy()
    Rz[:, 500:1000] = 0.0
    dz = dict(d, R=Rz)
    seg, perm = href.one_segment(400)
    plain, out = both(dev, dz, seg, perm, 2, 1)
    want = check("zero stretch", dz, seg, perm, 2, 1, plain, out)
    assert not np.isnan(plain[2]).any() and (plain[2] == 0).any()
    gone = np.isnan(want)
    assert gone.any() and np.all(plain[2][gone] == 0) and np.array_equal(out[1], 400 - gone.sum(axis=2))
    assert not np.isnan(out[0]).any()


# ---- 3: independence -------------------------------------------------------------------------------------------------------
def _indep_design():
    d = design(3, 1300, 17, n_tap=2, seed=7)
    seg, perm = href.interleaved((1100, 200), seed=8)
    return d, seg, perm, 60


@pytest.fixture(scope="module")
def indep(dev):
    d, seg, perm, h = _indep_design()
    plain, out = both(dev, d, seg, perm, h, 0)
    return d, seg, perm, h, plain, out


def test_two_calls_and_trials_alone_bitwise(dev, indep):
    d, seg, perm, h, plain, base = indep
    assert np.isnan(base[2]).any() and np.all(base[1].max(axis=1) > 0)
    assert same(dev.spectrum_expose_highpass(d["wav"], d["R"], model=True), base)           # two calls in a row
    for j in (0, 8, 16):
        dj = dict(d, F=np.ascontiguousarray(d["F"][:, j:j + 1]))
        assert same(both(dev, dj, seg, perm, h, 0)[1], tuple(x[:, j:j + 1] for x in base)), j


_BATCHED = """
import hashlib, json, sys
sys.path.insert(0, %r)
import numpy as np
from prometheus_amd import _native
from test_gpu_median import _indep_design, both
d, seg, perm, h = _indep_design()
out = both(_native.get_device(0), d, seg, perm, h, 0)[1]
print(json.dumps([hashlib.sha256(x.tobytes()).hexdigest() for x in out]))
"""


def test_batches_under_a_small_scratch_cap_bitwise(indep):
    """PROM_VMAP_SCRATCH_MB is read at context creation, so the case runs in a process of its own: 0.0001 MB is below
    one trial group's records, so every group of the 17 trials is a batch of its own: three batches."""
    base = indep[5]
    env = dict(os.environ, PROM_VMAP_SCRATCH_MB="0.0001", PROM_DEBUG="1")
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _BATCHED % os.path.join(REPO, "tests")],
                       env=env, cwd=REPO, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = [l for l in p.stderr.splitlines() if "detrended moments:" in l]
    assert lines and "3 groups, 3 batches of up to 1 groups" in lines[-1], p.stderr[-2000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("[")][-1])
    assert out == [hashlib.sha256(x.tobytes()).hexdigest() for x in base]


# ---- 4: composition -----------------------------------------------------------------------------------------------------
def test_composition_with_the_sysrem_filter_bitwise(dev):
    """detrend = 1: the model is filter_f64(median_f64(plain)) bit for bit and n_used exact; detrend = 0 on the same
    context still gives the median alone; prom_highpass_kernel_ms times the resident kind."""
    n_exp, n_pix = 3, 300
    d = design(n_exp, n_pix, 3)
    seg, perm = href.interleaved((100, 200), seed=5)
    rng = np.random.default_rng(31)
    Ub, W = rng.normal(size=(n_exp, 2)), rng.normal(size=(2, n_exp, n_pix)) / n_exp
    W[:, 0, ::7] = 0.0
    plain, out = both(dev, d, seg, perm, 30, 1, filt=(Ub, W))
    check("composition", d, seg, perm, 30, 1, plain, out, filt=(Ub, W))
    alone = dev.spectrum_expose_highpass(d["wav"], d["R"], detrend=False, model=True)
    assert dev.highpass_kernel_ms(2) > 0.0
    check("composition, median alone", d, seg, perm, 30, 1, plain, alone)
    assert not mref.same_bits(alone[2], out[2])
    assert same(dev.spectrum_expose(d["wav"], d["R"], model=True), plain)                  # the plain call stands


def test_composition_with_the_per_order_moments_bitwise(dev):
    """orders = with highpass = 1: the final model is the median's, the lumped moments are the high-pass call's and the
    records are order_moments_f64 of that model."""
    d = design(3, 300, 3)
    seg, perm = href.interleaved((100, 200), seed=5)
    oseg, operm = href.interleaved((40, 260), seed=3)
    plain, hp_out = both(dev, d, seg, perm, 12, 0)
    dev.orders_set(oseg, operm, np.ones(2, dtype=np.uint8))
    mom, nu, rmom, rnu, tot, model = dev.spectrum_expose_orders(d["wav"], d["R"], highpass=True, detrend=False,
                                                                model=True)
    assert mref.same_bits(model, mref.median_f64(plain[2], seg, perm, 12, 0))
    assert same((mom, nu, model), hp_out)
    want_mom, want_nu = oref.order_moments_f64(model, d["data"], d["ivar"], None, oseg, operm)
    assert np.array_equal(rnu, want_nu) and np.array_equal(rmom, want_mom) and (want_nu > 0).any()


def _sysrem_upload(dev, d, h, mode, orders=False, data=None):
    """test_gpu_sysrem's upload, then the median over its two orders (and those orders for the per-order moments)."""
    ts.upload(dev, d if data is None else dict(d, data=data))
    seg, perm, _ = ts.two_orders(len(d["lam"]))
    dev.highpass_set_median(seg, perm, h, mode)
    if orders:
        dev.orders_set(seg, perm, np.ones(len(seg) - 1, dtype=np.uint8))


def test_clean_and_inject_are_the_numpy_route_bitwise(dev):
    """U, cleaned and injected of prom_spectrum_inject and prom_sysrem_clean with the median resident equal sysrem_f64
    of observation.high_pass (with the window) of the numpy injection."""
    from prometheus_amd import observation as obs
    d = ts.design(7, 129, seed=136)
    h, mode = 9, 1
    _sysrem_upload(dev, d, h, mode)
    hp = (obs.median_window(h), mode)
    args = dict(n_comp=2, n_iter=4, ones=True, highpass=True, injected=True)
    ts.same(dev.spectrum_inject(d["wav"], d["R"], 1, 0.7, **args), ts.expected(dev, d, 1, 0.7, 2, 4, True, hp), "inject")
    ts.same(dev.sysrem_clean(**args), ts.expected(dev, d, None, 0.0, 2, 4, True, hp), "clean")
    plain = dev.sysrem_clean(n_comp=2, n_iter=4, ones=True, highpass=False, injected=True)
    assert np.array_equal(plain[2], d["raw"], equal_nan=True)                                # highpass = 0: untouched


def _separate(dev, d, trial, scale, n_comp, n_iter, ones, h, mode, orders):
    """The recovery by separate calls with the median resident (test_gpu_recover's route)."""
    _sysrem_upload(dev, d, h, mode)
    U, cleaned, _ = dev.spectrum_inject(d["wav"], d["R"], trial, scale, n_comp=n_comp, n_iter=n_iter, ones=ones,
                                        highpass=True)
    _sysrem_upload(dev, d, h, mode, orders, data=cleaned)
    dev.detrend_set(U, dev.filter_weights(U, d["ivar"]))
    if orders:
        out = dev.spectrum_expose_orders(d["wav"], d["R"], highpass=True, detrend=True, model=True)
    else:
        mom, nu, model = dev.spectrum_expose_highpass(d["wav"], d["R"], detrend=True, model=True)
        out = (mom, nu, None, None, None, model)
    return out + (U,)


@pytest.mark.parametrize("orders", [False, True])
def test_recover_is_the_route_of_separate_calls_bitwise(dev, orders):
    import test_gpu_recover as tr_
    d = ts.design(7, 129, seed=136)
    h, mode = 9, 0
    want = _separate(dev, d, 1, 0.7, 2, 4, True, h, mode, orders)
    _sysrem_upload(dev, d, h, mode, orders)
    got = dev.spectrum_recover(d["wav"], d["R"], 1, 0.7, 2, n_iter=4, ones=True, highpass=True, orders=orders,
                               model=True)
    tr_.same(got, want, "recover orders=%d" % orders)
    assert got[1].sum() > 0
    # and the model is the numpy route's: the median of the plain model, then the filter of (U, W)
    plain = dev.spectrum_expose(d["wav"], d["R"], moments=False, model=True)[2]
    seg, perm, _ = ts.two_orders(129)
    U = got[6]
    Mf = dref.filter_f64(mref.median_f64(plain, seg, perm, h, mode), U, dev.filter_weights(U, d["ivar"]))[0]
    assert mref.same_bits(got[5], Mf)


def test_grid_calls_are_loops_of_the_single_calls_bitwise(dev):
    import test_gpu_inject_grid as tg
    d = ts.design(7, 129, seed=136)
    h, mode = 9, 1
    kw = dict(n_comp=2, n_iter=4, ones=True, highpass=True)
    _sysrem_upload(dev, d, h, mode, True)
    want_i = tg.inject_loop(dev, d, tg.LIST, **kw)
    want_r = tg.recover_loop(dev, d, tg.LIST, True, **kw)
    tg.eq(dev.spectrum_inject_grid(d["wav"], d["R"], tg.TRIALS, tg.SCALES, injected=True, **kw), want_i, "inject grid")
    tg.eq(dev.spectrum_recover_grid(d["wav"], d["R"], tg.TRIALS, tg.SCALES, orders=True, **kw), want_r, "recover grid")
    assert want_r[1].any()
    # the loop's first entry is the numpy route's (the grid is then, too)
    from prometheus_amd import observation as obs
    t0, s0 = tg.LIST[0]
    exp = ts.expected(dev, d, t0, s0, 2, 4, True, (obs.median_window(h), mode))
    ts.same(tuple(x[0] for x in want_i), exp, "first entry")


# ---- 5: both kinds on one table ------------------------------------------------------------------------------------------
def test_mean_then_median_then_mean_on_one_table_bitwise(dev):
    d = design(3, 300, 3)
    seg, perm = href.interleaved((100, 200), seed=5)
    g = gauss(12, 4.0)
    upload(dev, d)
    plain = dev.spectrum_expose(d["wav"], d["R"], model=True)
    want_mean = href.highpass_f64(plain[2], seg, perm, g, 0)
    want_med = mref.median_f64(plain[2], seg, perm, 12, 0)
    assert not mref.same_bits(want_mean, want_med)
    dev.highpass_set(seg, perm, g, 0, key="mean")
    assert mref.same_bits(dev.spectrum_expose_highpass(d["wav"], d["R"], model=True)[2], want_mean)
    dev.highpass_set_median(seg, perm, 12, 0, key="median")
    assert dev.highpass_key == "median"
    assert mref.same_bits(dev.spectrum_expose_highpass(d["wav"], d["R"], model=True)[2], want_med)
    dev.highpass_set(seg, perm, g, 0, key="mean")
    assert dev.highpass_key == "mean"
    assert mref.same_bits(dev.spectrum_expose_highpass(d["wav"], d["R"], model=True)[2], want_mean)


# ---- 6: errors -----------------------------------------------------------------------------------------------------------
def test_errors():
    from prometheus_amd import _native
    from helpers import observe_ref as ref
    wav = ref.grid_nonuniform(100)
    R = ref.spectrum(wav, 2)
    lam, sig = wav[[10, 20, 30, 40]], np.full(4, 2e-10)
    rng = np.random.default_rng(6)
    data, ivar = 0.9 + 0.05 * rng.random((4, 4)), 1e4 * (0.1 + rng.random((4, 4)))
    rows, a, _ = table(4, 3, 2, n_orb=2)
    F = 1.0 + 1e-6 * np.arange(24.0).reshape(4, 3, 2)
    seg, perm = np.array([0, 1, 4]), np.array([2, 0, 3, 1])
    d = _native.Device(0)
    try:
        with pytest.raises(_native.NativeError, match=E_STATE):          # no exposure table on the context
            d.highpass_set_median(seg, perm, 1)
        d.observe_set(lam, sig, 5.0, 2)
        d.expose_set(rows, a, F, data, ivar)
        with pytest.raises(_native.NativeError, match=E_STATE):          # a table, but no high-pass
            d.spectrum_expose_highpass(wav, R)
        bad_sets = [
            (seg, perm, -1, 0), (seg, perm, 513, 0),                      # the half width
            (seg, perm[:3], 1, 0),                                        # n_pix other than the observation's
            ([1, 2, 4], perm, 1, 0),                                      # seg_first does not start at 0
            ([0, 1, 3], perm, 1, 0),                                      # ... or end at n_pix
            ([0, 2, 2, 4], perm, 1, 0),                                   # an empty segment
            ([0, 3, 2, 4], perm, 1, 0),                                   # descending
            (seg, [2, 0, 3, 3], 1, 0),                                    # no permutation
            (seg, [2, 0, 4, 1], 1, 0), (seg, [2, 0, -1, 1], 1, 0),        # out of range
            (seg, perm, 1, 2), (seg, perm, 1, -1),                        # mode
        ]
        for args in bad_sets:
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.highpass_set_median(*args)
        with pytest.raises(_native.NativeError, match=E_STATE):          # a failed set leaves no high-pass behind
            d.spectrum_expose_highpass(wav, R)
        d.highpass_set(seg, perm, np.ones(2), 0, key="mean")
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.highpass_set_median(seg, perm, 600)
        assert d.highpass_key is None                                     # ... and none that was there before
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.spectrum_expose_highpass(wav, R)
        for h in (0, 512):
            d.highpass_set_median(seg, perm, h, 1, key="m")
            assert d.highpass_key == "m"
            mom, nu, model = d.spectrum_expose_highpass(wav, R, model=True)
            assert model.shape == (4, 3, 4) and np.all(nu == 4)
        assert d.highpass_kernel_ms(2) > 0.0
        d.expose_set(rows, a, F, data, ivar)                              # drops the median
        assert d.highpass_key is None
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.spectrum_expose_highpass(wav, R)
        d.observe_set(lam[:0], sig[:0], 5.0, 2)                           # no pixel: zeros
        d.expose_set(rows, a, F, data[:, :0], ivar[:, :0])
        d.highpass_set_median([0, 0], [], 3)
        mom, nu, model = d.spectrum_expose_highpass(wav, R, model=True)
        assert np.all(mom == 0) and np.all(nu == 0) and model.shape == (4, 3, 0)
    finally:
        d.close()


# ---- 7: a planted planet, through the Python path ------------------------------------------------------------------------
def test_planted_planet_is_recovered_with_a_median_continuum(planet):
    """The sysrem tests' design (12 exposures, 400 pixels in two orders, 9 trials) with a running median divided out of
    data and model: Transit.recover peaks at the injected trial, and so does the all-numpy pipeline (observation.high_pass
    with the window, observation.sysrem, the filter and the likelihood) on the device's plain model.  Transit.expose with
    the median HighPass gives observation.high_pass of the plain model bit for bit."""
    from prometheus_amd import _native
    from prometheus_amd import observation as obs
    tr, d, ex, inj, _ = planet
    win = obs.median_window(PLANET_HALF)
    hp = obs.HighPass(ex, win, orders=d["orders"], mode=d["mode"])
    kw = dict(n_comp=d["n_comp"], n_iter=d["n_iter"], ones=d["ones"], highpass=hp, devices=[0])
    vm = tr.recover(inj, sref.PLANET_TRIAL, 1.0, **kw)
    assert _native.get_device(0).highpass_key == hp.key
    ll = vm.loglike.sum(axis=0)
    print("planted planet, median, device: logL - max per trial", ll - ll.max())
    assert int(np.argmax(ll)) == sref.PLANET_TRIAL
    plain = tr.expose(ex, return_model=True, devices=[0])
    out = tr.expose(ex, return_model=True, devices=[0], highpass=hp)
    assert mref.same_bits(out.model, obs.high_pass(plain.model, win, orders=d["orders"], mode=d["mode"]))
    D = sref.inject_f64(d["raw"], plain.model[:, sref.PLANET_TRIAL], 1.0)
    flat = obs.high_pass(D, win, orders=d["orders"], mode=d["mode"])
    Ub, clean = obs.sysrem(flat, d["err"], d["n_comp"], d["n_iter"], ones=d["ones"])
    ll_np = sref.numpy_recovery(dict(d, taps=win), plain.model, clean, Ub)
    print("planted planet, median, numpy: logL - max per trial", ll_np - ll_np.max())
    assert int(np.argmax(ll_np)) == sref.PLANET_TRIAL
