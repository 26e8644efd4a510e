"""High-pass filtered exposures on the device (prom_highpass_set / prom_spectrum_expose_highpass /
prom_transit_expose_highpass, Transit.expose(highpass=...)) against the references of tests/helpers/highpass_ref.py.
Marked ``gpu``.

The device's filtered model must be highpass_f64 of prom_spectrum_expose's own model_out bit for bit, NaN pattern
included, and n_used exact.  The moments lie within (n_used + 4) u sum |term| of the longdouble sums of the device's own
model, and the model within the derived bound of the longdouble filter of the exposures' longdouble model
(highpass_ref's derivation, from the definition and not from the kernel).  Orders, the degenerate cases, the
independence clause and the composition with the SYSREM filter are tested bitwise.  The tests print the largest
fractions of the bounds they reached (``HIGHPASS_ERR``; profiles/highpass_errors.txt).
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import detrend_ref as dref
from helpers import expose_ref as eref
from helpers import highpass_ref as href
from helpers import observe_ref as ref
from helpers import vmap_ref as vref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
E_ARG, E_STATE = "PROM_E_ARG", "PROM_E_STATE"
TILE = 1024              # outputs of a k_highpass tile (highpass_index.h)
HALVES = (0, 3, 255, 256, 300, 512)
# the harness' lengths: about a wave and a workgroup's threads, and about the tile (one, one and a bit, four)
LENGTHS = (1, 2, 255, 256, 257, 515, TILE - 1, TILE, TILE + 1, 3 * TILE + 452)


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


def gauss(h, sigma=None):
    return np.exp(-0.5 * (np.arange(h + 1) / (sigma or max(h / 4.0, 1.0))) ** 2)


def table(n_exp, n_trial, n_tap, n_orb=3, seed=11):
    """Rows over n_orb, weights that sum to 1, factors a few km/s about 1 that differ per exposure, trial and tap."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_orb, (n_exp, n_tap)).astype(np.int32)
    a = 0.2 + rng.random((n_exp, n_tap))
    a /= a.sum(axis=1, keepdims=True)
    v = np.linspace(-8.0, 8.0, n_trial) if n_trial > 1 else np.array([1.0])
    F = (vref.doppler(1e5 * v)[None, :, None] * (1.0 + 1e-5 * np.arange(n_tap))[None, None, :]
         * (1.0 - 2e-6 * np.arange(n_exp))[:, None, None])
    return rows, a, np.ascontiguousarray(F)


def design(n_exp=3, n_pix=300, n_trial=5, n_tap=2, outside=True, seed=3):
    """The spectrum entries' inputs on observe_ref.grid_nonuniform(1500); with ``outside`` some pixels lie beyond the
    grid's ends and have no model; without, they lie over the middle 80 % of the grid, further from either end than
    the trials' shifts (0.16 A at 8 km/s) and a support's half width (0.125 A) together, so every pixel has a model in
    every trial."""
    wav = ref.grid_nonuniform(1500)
    rng = np.random.default_rng(seed)
    if outside:
        lam = ref.pixels_over(wav, n_pix)
    else:
        lam = np.sort(wav[0] + (wav[-1] - wav[0]) * (0.1 + 0.8 * rng.random(n_pix)))
    data, ivar = 0.9 + 0.05 * rng.random((n_exp, n_pix)), 1e4 * (0.1 + rng.random((n_exp, n_pix)))
    rows, a, F = table(n_exp, n_trial, n_tap)
    return dict(wav=wav, R=ref.spectrum(wav, 3), lam=lam, sig=np.full(n_pix, 2.5e-10), k=5.0, rows=rows, a=a, F=F,
                data=data, ivar=ivar)


def upload(dev, d):
    dev.observe_set(d["lam"], d["sig"], d["k"], d["R"].shape[0])
    dev.expose_set(d["rows"], d["a"], d["F"], d["data"], d["ivar"])


def both(dev, d, seg, perm, g, mode, filt=None, model=True):
    """(prom_spectrum_expose's, prom_spectrum_expose_highpass's) (moments, n_used, model) of design d."""
    upload(dev, d)
    plain = dev.spectrum_expose(d["wav"], d["R"], model=True)
    dev.highpass_set(seg, perm, g, mode)
    if filt is not None:
        dev.detrend_set(*filt)
    return plain, dev.spectrum_expose_highpass(d["wav"], d["R"], detrend=filt is not None, model=model)


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def check(name, d, seg, perm, g, mode, plain, out, filt=None, exact=None):
    """The definition on the device's output: the model bitwise against highpass_f64 (then filter_f64) of the unfiltered
    model, n_used exact, no NaN moment, the moments within their summation bounds, on request the model within the
    derived bound of the exact reference (``exact``: the exposures' longdouble model and its bound eps_e)."""
    mom, nu, model = out
    want = href.highpass_f64(plain[2], seg, perm, g, mode)
    ok = np.ones(want.shape[1:], dtype=bool)
    if filt is not None:
        want, ok = dref.filter_f64(want, *filt)
    assert model.shape == want.shape and nu.dtype == np.int64
    assert np.array_equal(np.isnan(model), np.isnan(want)), name
    assert np.array_equal(model, want, equal_nan=True), name
    with np.errstate(invalid="ignore"):
        good = np.isfinite(d["ivar"]) & (d["ivar"] > 0) & np.isfinite(d["data"])
    used = good[:, None, :] & ok[None, :, :] & ~np.isnan(want)
    assert np.array_equal(nu, used.sum(axis=2)), name
    mld, nld, ald = dref.moments_ld(model, d["data"], d["ivar"])
    assert np.array_equal(nu, nld) and not np.isnan(mom).any(), name
    assert np.all(mom[nu == 0] == 0), name
    frac = dref.moment_fractions(mom, mld, nu, ald)
    mfrac = None
    if exact is not None:
        rM, eps_e = exact
        rMf, bound, live = href.model_bound(rM, seg, perm, g, mode, eps_e)
        assert live.any(), name
        mfrac = href.model_fraction(model, rMf, bound, live)
    print("HIGHPASS_ERR %s %s of the bounds (m0 .. m6), model %s" %
          (name, " ".join("%.4f" % f for f in frac), "-" if mfrac is None else "%.4f" % mfrac))
    assert np.all(frac <= 1.0), (name, frac)
    assert mfrac is None or mfrac <= 1.0, (name, mfrac)
    return want


# ---- 1, 2: the model bitwise and the moments over the lengths x half widths ----------------------------------------
@pytest.fixture(scope="module")
def sweep(dev):
    """One design whose segments have the harness' lengths, dealt over the device's pixel order at random (every second
    one reversed), some pixels without a model: the plain exposures once, shared by the sweep."""
    d = design(2, sum(LENGTHS), 5)
    seg, perm = href.interleaved(LENGTHS, seed=4)
    upload(dev, d)
    plain = dev.spectrum_expose(d["wav"], d["R"], model=True)
    assert np.isnan(plain[2]).any() and np.isfinite(plain[2]).any()
    return d, seg, perm, plain


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("h", HALVES)
def test_model_bitwise_and_moments_over_lengths_and_half_widths(dev, sweep, h, mode):
    d, seg, perm, plain = sweep
    plain2, out = both(dev, d, seg, perm, gauss(h), mode)
    assert same(plain2, plain)
    check("sweep h=%d mode=%d" % (h, mode), d, seg, perm, gauss(h), mode, plain, out)


# ---- 3: the model against the exact reference ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact_design():
    """The exposures' longdouble model of one design, computed once."""
    d = design(3, 300, 5)
    rmom, rnu, rM, n_max, k_live = eref.expose(d["wav"], d["R"], d["lam"], d["sig"], d["k"], d["rows"], d["a"], d["F"],
                                               d["data"], d["ivar"])
    return d, (rM, eref.model_tolerance(d["k"], n_max, k_live))


@pytest.mark.parametrize("mode", [0, 1])
def test_model_within_the_derived_bound_of_the_exact_reference(dev, exact_design, mode):
    d, exact = exact_design
    seg, perm = href.interleaved((1, 2, 120, 177), seed=2)
    for h in (3, 40, 300):
        plain, out = both(dev, d, seg, perm, gauss(h), mode)
        check("exact h=%d mode=%d" % (h, mode), d, seg, perm, gauss(h), mode, plain, out, exact=exact)


# ---- 4: orders -------------------------------------------------------------------------------------------------------
def test_orders_interleaved_and_reversed_bitwise(dev):
    """Two orders interleaved pixel by pixel in the device's order, then one order reversed in position; both against
    the reference, and the reversed one against the forward one mirrored (the taps are symmetric, but the sums run the
    other way, so only the reference decides the bits)."""
    n = 2 * 700
    d = design(2, n, 5)
    g = gauss(40, 12.0)
    seg = np.array([0, n // 2, n], dtype=np.int32)
    perm = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)]).astype(np.int32)
    plain, out = both(dev, d, seg, perm, g, 0)
    check("two interleaved orders", d, seg, perm, g, 0, plain, out)
    seg1, fwd = href.one_segment(n)
    plain, out_r = both(dev, d, seg1, fwd[::-1].copy(), g, 1)
    check("one reversed order", d, seg1, fwd[::-1].copy(), g, 1, plain, out_r)
    out_f = both(dev, d, seg1, fwd, g, 1)[1]
    ok = ~np.isnan(out_f[2])
    assert np.allclose(out_r[2][ok], out_f[2][ok], rtol=1e-13, atol=0)


def test_clean_tiles_of_a_long_order_bitwise(dev):
    """Every pixel has a model and the order is 2,500 long: its second tile's window lies inside and holds no NaN, so
    the path without validity tests runs; h = 160 and the largest."""
    d = design(2, 2500, 5, outside=False)
    seg, perm = href.one_segment(2500)
    for h, mode in ((160, 0), (512, 1)):
        plain, out = both(dev, d, seg, perm, gauss(h), mode)
        assert not np.isnan(plain[2]).any() and np.all(out[1] == 2500)
        check("clean tiles h=%d" % h, d, seg, perm, gauss(h), mode, plain, out)


def test_nan_in_R_reaches_its_pixels_and_neighbours_renormalise(dev):
    d = design(3, 400, 5, outside=False)
    seg, perm = href.interleaved((150, 250), seed=6)
    g = gauss(25, 8.0)
    clean_plain, clean = both(dev, d, seg, perm, g, 0)
    Rn = d["R"].copy()
    Rn[:, 700] = np.nan
    dn = dict(d, R=Rn)
    plain, out = both(dev, dn, seg, perm, g, 0)
    check("NaN in R", dn, seg, perm, g, 0, plain, out)
    hit = np.isnan(plain[2])
    assert hit.any() and not np.isnan(clean_plain[2]).any()
    assert np.array_equal(np.isnan(out[2]), hit)                        # exactly the pixels with it in a support
    assert np.array_equal(out[1], clean[1] - hit.sum(axis=2))
    # a value whose window holds a NaN changes (it renormalises over what is left), one whose window holds none stands
    changed = ~hit & (out[2] != clean[2])
    assert changed.any() and np.isfinite(out[2][changed]).all()
    near = np.zeros_like(hit)
    for s in range(2):
        idx = perm[seg[s]:seg[s + 1]]
        h_seg = hit[..., idx]
        reach = np.zeros_like(h_seg)
        for dd in range(-25, 26):
            src = h_seg[..., max(0, dd):h_seg.shape[-1] + min(0, dd)]
            reach[..., max(0, -dd):h_seg.shape[-1] - max(0, dd)] |= src
        near[..., idx] = reach
    assert not changed[~near].any()
    assert np.array_equal(out[2][~near], clean[2][~near])


def test_zero_stretch_under_division_bitwise(dev):
    """R = 0 over a stretch wider than a support plus the window: M = 0 and B = 0 there, 0 / 0 is NaN and the pixel is
    unused; at the stretch's rim 0 / B = 0 stays used.  No moment is NaN."""
    d = design(2, 400, 5, outside=False)
    Rz = d["R"].copy()
    Rz[:, 500:1000] = 0.0
    dz = dict(d, R=Rz)
    seg, perm = href.one_segment(400)
    plain, out = both(dev, dz, seg, perm, np.ones(3), 1)
    want = check("zero stretch", dz, seg, perm, np.ones(3), 1, plain, out)
    assert not np.isnan(plain[2]).any() and (plain[2] == 0).any()
    gone = np.isnan(want)
    assert gone.any() and np.all(plain[2][gone] == 0) and np.array_equal(out[1], 400 - gone.sum(axis=2))
    assert (want == 0).any()


# ---- 5: the degenerate cases -------------------------------------------------------------------------------------------
def test_degenerate_cases_bitwise_with_the_sign_of_zero(dev):
    """Every segment of length 1 with h = 7, and h = 0 on one segment: mode 0 gives +0 wherever M is valid, mode 1
    gives 1 wherever M is valid and not 0."""
    n = 70
    d = design(2, n, 5)
    Rz = d["R"].copy()
    Rz[:, 600:900] = 0.0
    d = dict(d, R=Rz)
    singles = (np.arange(n + 1, dtype=np.int32), np.random.default_rng(1).permutation(n).astype(np.int32), gauss(7))
    flat = href.one_segment(n) + (np.ones(1),)
    for name, (seg, perm, g) in (("length 1", singles), ("h = 0", flat)):
        for mode in (0, 1):
            plain, out = both(dev, d, seg, perm, g, mode)
            check("degenerate %s mode=%d" % (name, mode), d, seg, perm, g, mode, plain, out)
            M, Mf = plain[2], out[2]
            valid = ~np.isnan(M)
            assert valid.any() and (~valid).any() and (M == 0).any()
            assert np.array_equal(np.isnan(Mf), ~valid | ((M == 0) & (mode == 1)))
            if mode == 0:
                assert np.all(Mf[valid] == 0.0) and not np.signbit(Mf[valid]).any()
                assert np.all(out[0][..., 1] == 0) and np.all(out[0][..., 3] == 0)      # sum iv M', sum iv M'^2
            else:
                assert np.all(Mf[valid & (M != 0)] == 1.0)


# ---- 6: independence ---------------------------------------------------------------------------------------------------
def _indep_design():
    d = design(4, 1300, 17, n_tap=2, seed=7)
    seg, perm = href.interleaved((1100, 200), seed=8)
    return d, seg, perm, gauss(60, 20.0)


@pytest.fixture(scope="module")
def indep(dev):
    d, seg, perm, g = _indep_design()
    plain, out = both(dev, d, seg, perm, g, 0)
    return d, seg, perm, g, plain, out


def test_two_calls_and_trials_alone_bitwise(dev, indep):
    d, seg, perm, g, plain, base = indep
    check("independence base", d, seg, perm, g, 0, plain, base)
    assert np.isnan(base[2]).any() and np.all(base[1].max(axis=1) > 0)
    assert same(dev.spectrum_expose_highpass(d["wav"], d["R"], model=True), base)           # two calls in a row
    for j in (0, 7, 8, 16):
        dj = dict(d, F=np.ascontiguousarray(d["F"][:, j:j + 1]))
        assert same(both(dev, dj, seg, perm, g, 0)[1], tuple(x[:, j:j + 1] for x in base)), j
    pj = np.random.default_rng(12).permutation(d["F"].shape[1])
    dp = dict(d, F=np.ascontiguousarray(d["F"][:, pj]))
    assert same(both(dev, dp, seg, perm, g, 0)[1], tuple(x[:, pj] for x in base))


_BATCHED = """
import hashlib, json, sys
sys.path.insert(0, %r)
import numpy as np
from prometheus_amd import _native
from test_gpu_highpass import _indep_design, both
d, seg, perm, g = _indep_design()
out = both(_native.get_device(0), d, seg, perm, g, 0)[1]
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


# ---- 7: composition with the SYSREM filter -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_composition_with_the_sysrem_filter_bitwise(dev, mode):
    """detrend = 1: the model is filter_f64(highpass_f64(plain)) bit for bit, n_used exact, the moments within their
    bounds; detrend = 0 on the same context still gives the high-pass alone, and the detrended entry its own."""
    n_exp, n_pix = 5, 300
    d = design(n_exp, n_pix, 7)
    seg, perm = href.interleaved((100, 200), seed=5)
    g = gauss(30, 10.0)
    rng = np.random.default_rng(31)
    Ub, W = rng.normal(size=(n_exp, 3)), rng.normal(size=(3, n_exp, n_pix)) / n_exp
    W[:, 0, ::7] = 0.0
    plain, out = both(dev, d, seg, perm, g, mode, filt=(Ub, W))
    check("composition mode=%d" % mode, d, seg, perm, g, mode, plain, out, filt=(Ub, W))
    alone = dev.spectrum_expose_highpass(d["wav"], d["R"], detrend=False, model=True)
    check("composition, high-pass alone mode=%d" % mode, d, seg, perm, g, mode, plain, alone)
    assert not np.array_equal(alone[2], out[2], equal_nan=True)
    only_dt = dev.spectrum_expose_detrended(d["wav"], d["R"], model=True)
    assert np.array_equal(only_dt[2], dref.filter_f64(plain[2], Ub, W)[0], equal_nan=True)
    assert same(dev.spectrum_expose(d["wav"], d["R"], model=True), plain)                  # the plain call stands
    mom, nu, model = dev.spectrum_expose_highpass(d["wav"], d["R"], detrend=True, model=False)    # moments alone
    assert model is None and same((mom, nu), out[:2])
    none, none2, model = dev.spectrum_expose_highpass(d["wav"], d["R"], detrend=True, moments=False, model=True)
    assert none is None and none2 is None and np.array_equal(model, out[2], equal_nan=True)
    assert dev.highpass_kernel_ms(2) > 0.0


# ---- 8: state and argument errors --------------------------------------------------------------------------------------
def test_errors():
    from prometheus_amd import _native
    wav = ref.grid_nonuniform(100)
    R = ref.spectrum(wav, 2)
    lam, sig = wav[[10, 20, 30, 40]], np.full(4, 2e-10)
    rng = np.random.default_rng(6)
    data, ivar = 0.9 + 0.05 * rng.random((4, 4)), 1e4 * (0.1 + rng.random((4, 4)))
    rows, a, _ = table(4, 3, 2, n_orb=2)
    F = 1.0 + 1e-6 * np.arange(24.0).reshape(4, 3, 2)
    seg, perm, g = np.array([0, 1, 4]), np.array([2, 0, 3, 1]), np.array([1.0, 0.5])
    Ub, W = rng.normal(size=(4, 2)), rng.normal(size=(2, 4, 4))
    d = _native.Device(0)
    try:
        for call in (lambda: d.highpass_set(seg, perm, g), lambda: d.spectrum_expose_highpass(wav, R),
                     d.transit_expose_highpass, d.highpass_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):      # no exposure table on the context
                call()
        d.observe_set(lam, sig, 5.0, 2)
        d.expose_set(rows, a, F, data, ivar)
        for call in (lambda: d.spectrum_expose_highpass(wav, R), d.transit_expose_highpass, d.highpass_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):      # a table, but no high-pass
                call()
        bad_sets = [
            (seg, perm[:3], g, 0),                                        # n_pix other than the observation's
            ([0, 1, 3], [2, 0, 1], g, 0),
            ([1, 2, 4], perm, g, 0),                                      # seg_first does not start at 0
            ([0, 1, 3], perm, g, 0),                                      # ... or end at n_pix
            ([0, 2, 2, 4], perm, g, 0),                                   # an empty segment
            ([0, 3, 2, 4], perm, g, 0),                                   # descending
            (seg, [2, 0, 3, 3], g, 0),                                    # no permutation
            (seg, [2, 0, 4, 1], g, 0),                                    # out of range
            (seg, [2, 0, -1, 1], g, 0),
            (seg, perm, np.ones(514), 0),                                 # half_width 513
            (seg, perm, [1.0, np.nan], 0), (seg, perm, [1.0, np.inf], 0), (seg, perm, [1.0, -0.5], 0),
            (seg, perm, [0.0, 1.0], 0),                                   # g[0] = 0
            (seg, perm, g, 2), (seg, perm, g, -1),                        # mode
        ]
        for args in bad_sets:
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.highpass_set(*args)
        with pytest.raises(_native.NativeError, match=E_STATE):          # a failed set leaves no high-pass behind
            d.spectrum_expose_highpass(wav, R)
        d.highpass_set(seg, perm, g, 1, key="h")
        assert d.highpass_key == "h"
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.transit_expose_highpass()                                   # no run yet
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.spectrum_expose_highpass(wav, R, detrend=True)              # detrend = 1 without a filter
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_expose_highpass(wav, R, detrend=2)                 # detrend is 0 or 1
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_expose_highpass(wav, ref.spectrum(wav, 3))         # another n_orb
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_expose_highpass(wav[::-1], R)                      # descending grid
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.highpass_kernel_ms()                                        # no high-pass call yet
        mom, nu, model = d.spectrum_expose_highpass(wav, R, model=True)
        assert mom.shape == (4, 3, 7) and nu.shape == (4, 3) and model.shape == (4, 3, 4) and np.all(nu == 4)
        assert d.highpass_kernel_ms(2) > 0.0
        d.detrend_set(Ub, W)
        assert d.highpass_key == "h"                                      # a filter leaves the high-pass alone
        assert np.all(d.spectrum_expose_highpass(wav, R, detrend=True)[1] == 4)
        d.expose_set(rows, a, F, data, ivar)                              # drops the high-pass (and the filter)
        assert d.highpass_key is None
        for call in (lambda: d.spectrum_expose_highpass(wav, R), d.highpass_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):
                call()
        d.highpass_set(seg, perm, g, 0, key="h")
        d.observe_set(lam, sig, 5.0, 2)                                   # drops the table and the high-pass with it
        assert d.highpass_key is None and d.expose_key is None
        for call in (lambda: d.spectrum_expose_highpass(wav, R), lambda: d.highpass_set(seg, perm, g)):
            with pytest.raises(_native.NativeError, match=E_STATE):
                call()
        d.observe_set(lam[:0], sig[:0], 5.0, 2)                           # no pixel: zeros
        d.expose_set(rows, a, F, data[:, :0], ivar[:, :0])
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.highpass_set([0, 1], [], g)
        d.highpass_set([0, 0], [], g)
        mom, nu, model = d.spectrum_expose_highpass(wav, R, model=True)
        assert np.all(mom == 0) and np.all(nu == 0) and model.shape == (4, 3, 0)
    finally:
        d.close()


# ---- 9: the Python path --------------------------------------------------------------------------------------------------
def test_transit_expose_highpass_end_to_end(monkeypatch):
    """Transit.expose(ex, highpass=hp[, detrend=dt]) on the reduced C1 problem, 60 pixels about Na D2 in two overlapping
    orders given in descending wavelength: the spectrum entry's numbers on that transit's R, in the caller's pixel
    order; a second call uploads nothing; highpass=None is today's expose bit for bit."""
    from oracle import prom_oracle as O
    from prometheus_amd import _native
    from prometheus_amd import constants as const
    from prometheus_amd import gasProperties as gp
    from prometheus_amd import lightcurve as lc
    from prometheus_amd import observation as obs
    from prometheus_amd import setupfile
    g = np.load(os.path.join(G, "transit_C1.npz"))
    cfg = json.loads(str(g["config"]))
    cfg["Grids"].update(orbphase_border=0.02, orbphase_steps=3)         # exposure_taps needs a bracket
    gp.register_molecular_table("H2O", O.synthetic_molecular_table(n_nu=2001))
    tr = setupfile.build_transit(cfg)
    orb = tr.spatialGrid.constructOrbphaseAxis()
    n_pix = 60
    px = lc.NA_D2 + 5e-10 * (np.arange(n_pix) - 29.5)
    orders = (np.arange(n_pix) // 3) % 2                                  # interleaved in wavelength: overlapping orders
    ins = obs.Instrument(px[::-1], resolving_power=140000.0, truncate=5.0)
    orders = orders[::-1].copy()
    base = obs.planet_frame_shifts(tr.planet, orb)
    Kp = np.sqrt(const.G * tr.planet.hostStar.M / tr.planet.a)
    n_exp = 6
    mid = np.linspace(orb[0], orb[-1], n_exp + 2)[1:-1]
    width = np.full(n_exp, 0.5 * (orb[1] - orb[0]))
    rows, a, F = obs.exposure_taps(orb, base, mid, width, n_sub=3, Kp=Kp * np.array([0.9, 1.0]), Vsys=[0.0, 2e5])
    rng = np.random.default_rng(3)
    raw = (1.0 + 1e-3 * rng.normal(size=(n_exp, n_pix))) * (1.0 + 0.1 * np.linspace(-1, 1, n_pix))[None, :]
    err = np.full((n_exp, n_pix), 1e-3)
    taps = obs.gaussian_taps(3.0)
    flat = obs.high_pass(raw, taps, orders=orders, mode="divide")        # the data go the model's way
    Ub, clean = obs.sysrem(flat, err, 1, ones=True)
    ex = obs.Exposures(ins, rows, a, F, clean, err)
    hp = obs.HighPass(ex, taps, orders=orders, mode="divide")
    dt = obs.Detrend(ex, Ub)
    plain = tr.expose(ex, return_model=True, devices=[0])
    R = np.array(tr.sumOverChords(devices=[0]))
    wav = np.asarray(tr.wavelength)
    dev = _native.get_device(0)
    for detrend in (None, dt):
        out = tr.expose(ex, return_model=True, devices=[0], highpass=hp, detrend=detrend)
        assert dev.expose_key == ex.key and dev.highpass_key == hp.key
        raw_out = dev.transit_expose_highpass(detrend=detrend is not None, model=True)
        spec = dev.spectrum_expose_highpass(wav, R, detrend=detrend is not None, model=True)
        for got in (raw_out, spec):
            assert np.array_equal(out.moments, got[0]) and np.array_equal(out.n_used, got[1])
            assert np.array_equal(out.model, ins.unsort(got[2]), equal_nan=True)
        assert out.model.shape == (n_exp, 4, n_pix)
        # the library's own numpy filter on the plain model, in the caller's order, gives the same bits
        want = obs.high_pass(plain.model, taps, orders=orders, mode="divide")
        if detrend is not None:
            want = ins.unsort(dref.filter_f64(ins.sort(want), dt.U, dt.W)[0])
        assert np.array_equal(out.model, want, equal_nan=True) and np.isfinite(out.model).any()
        assert not np.array_equal(out.moments, plain.moments)
    # a second call with the same objects: nothing is uploaded, the same bits
    calls = []
    for fn in ("observe_set", "expose_set", "detrend_set", "highpass_set"):
        monkeypatch.setattr(dev, fn, lambda *a, _fn=fn, **k: calls.append(_fn))
    again = tr.expose(ex, devices=[0], highpass=hp, detrend=dt)
    assert calls == [] and again.model is None
    assert np.array_equal(again.moments, out.moments) and np.array_equal(again.n_used, out.n_used)
    monkeypatch.undo()
    # highpass=None: today's calls, bit for bit, the high-pass still resident
    none = tr.expose(ex, return_model=True, devices=[0], highpass=None)
    assert np.array_equal(none.moments, plain.moments, equal_nan=True) and np.array_equal(none.n_used, plain.n_used)
    assert np.array_equal(none.model, plain.model, equal_nan=True) and dev.highpass_key == hp.key
    only_dt = tr.expose(ex, return_model=True, devices=[0], detrend=dt)
    assert np.array_equal(ins.sort(only_dt.model), dref.filter_f64(ins.sort(plain.model), dt.U, dt.W)[0], equal_nan=True)
