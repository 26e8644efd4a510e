"""Detrended exposures on the device (prom_detrend_set / prom_spectrum_expose_detrended /
prom_transit_expose_detrended, Transit.expose(detrend=...)) against the references of tests/helpers/detrend_ref.py.
Marked ``gpu``.

The device's filtered model must be filter_f64 of prom_spectrum_expose's own model_out bit for bit, NaN pattern
included, and n_used exact.  The moments lie within (n_used + 4) u sum |term| of the longdouble sums of the device's own
model, and the model within the derived absolute bound of the longdouble filter of the exposures' longdouble model
(detrend_ref's derivation, from the definition and not from the kernel).  The independence clause, the degenerate case
and the padding rule are tested bitwise.  Every test prints the largest fractions of the bounds it reached
(``DETREND_ERR``; profiles/detrend_errors.txt).
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
from helpers import observe_ref as ref
from helpers import vmap_ref as vref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
E_ARG, E_STATE = "PROM_E_ARG", "PROM_E_STATE"
TILE, T = 32, 8          # pixels of a moments tile, trials of a group (vmap_index.h)


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


def kms(v):
    return vref.doppler(1e5 * np.asarray(v, dtype=np.float64))


def positive_data(shape, seed):
    rng = np.random.default_rng(seed)
    return 0.9 + 0.05 * rng.random(shape), 1e4 * (0.1 + rng.random(shape))


def table(n_exp, n_trial, n_tap, n_orb=3, seed=11):
    """Rows over n_orb, weights that sum to 1, factors a few km/s about 1 that differ per exposure, trial and tap."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_orb, (n_exp, n_tap)).astype(np.int32)
    a = 0.2 + rng.random((n_exp, n_tap))
    a /= a.sum(axis=1, keepdims=True)
    v = np.linspace(-8.0, 8.0, n_trial) if n_trial > 1 else np.array([1.0])
    F = kms(v)[None, :, None] * (1.0 + 1e-5 * np.arange(n_tap))[None, None, :] * (1.0 - 2e-6 * np.arange(n_exp))[:, None, None]
    return rows, a, np.ascontiguousarray(F)


def random_filter(n_exp, n_comp, n_pix, seed=31, holes=True):
    """Any finite U and W are a filter: normal entries, W = 0 at every seventh pixel of exposure 0 and at one
    (component, exposure) everywhere."""
    rng = np.random.default_rng(seed)
    Ub = rng.normal(size=(n_exp, n_comp))
    W = rng.normal(size=(n_comp, n_exp, n_pix)) / n_exp
    if holes:
        W[:, 0, ::7] = 0.0
        W[n_comp - 1, n_exp - 1, :] = 0.0
    return Ub, W


def both(dev, d, Ub, W, model=True):
    """(prom_spectrum_expose's, prom_spectrum_expose_detrended's) (moments, n_used, model) of design d."""
    dev.observe_set(d["lam"], d["sig"], d["k"], d["R"].shape[0])
    dev.expose_set(d["rows"], d["a"], d["F"], d["data"], d["ivar"])
    plain = dev.spectrum_expose(d["wav"], d["R"], model=True)
    dev.detrend_set(Ub, W)
    return plain, dev.spectrum_expose_detrended(d["wav"], d["R"], model=model)


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def used_by_definition(plain_model, ok, data, ivar):
    with np.errstate(invalid="ignore"):
        good = np.isfinite(ivar) & (ivar > 0) & np.isfinite(data)
    return good[:, None, :] & ok[None, :, :] & ~np.isnan(plain_model)


def check(name, d, Ub, W, plain, out, exact=True):
    """The definition on the device's output: the model bitwise against filter_f64 of the unfiltered model, n_used
    exact, no NaN moment, the moments within their summation bounds, the model within the derived bound."""
    mom, nu, model = out
    want, ok = dref.filter_f64(plain[2], Ub, W)
    assert model.shape == want.shape and nu.dtype == np.int64
    assert np.array_equal(np.isnan(model), np.isnan(want)), name
    assert np.array_equal(model, want, equal_nan=True), name
    used = used_by_definition(plain[2], ok, d["data"], d["ivar"])
    assert np.array_equal(nu, used.sum(axis=2)), name
    mld, nld, ald = dref.moments_ld(model, d["data"], d["ivar"])
    assert np.array_equal(nu, nld) and not np.isnan(mom).any(), name
    assert np.all(mom[nu == 0] == 0), name
    frac = dref.moment_fractions(mom, mld, nu, ald)
    mfrac = None
    if exact:
        rmom, rnu, rM, n_max, k_live = eref.expose(d["wav"], d["R"], d["lam"], d["sig"], d["k"], d["rows"], d["a"], d["F"],
                                                   d["data"], d["ivar"])
        eps_e = eref.model_tolerance(d["k"], n_max, k_live)
        rMf, rok = dref.filter_ld(rM, Ub, W)
        assert np.array_equal(rok, ok), name
        mfrac = dref.model_fraction(model, rMf, dref.model_bound(rM, Ub, W, eps_e))
    print("DETREND_ERR %s %s of the bounds (m0 .. m6), model %s" %
          (name, " ".join("%.4f" % f for f in frac), "-" if mfrac is None else "%.4f" % mfrac))
    assert np.all(frac <= 1.0), (name, frac)
    assert mfrac is None or mfrac <= 1.0, (name, mfrac)


def inner_pixels(wav, n_pix, seed=2):
    """Non-decreasing pixel centres over the middle 80 % of the grid, one duplicated: about 0.4 A from either end,
    more than the trials' shifts (0.16 A at 8 km/s) and a support's half width (0.125 A) together, so every pixel has
    a model in every trial."""
    rng = np.random.default_rng(seed)
    span = wav[-1] - wav[0]
    lam = np.sort(wav[0] + span * (0.1 + 0.8 * rng.random(n_pix)))
    if n_pix >= 4:
        lam[n_pix // 2] = lam[n_pix // 2 - 1]
    return lam


def design(n_exp=5, n_pix=TILE + 1, n_trial=T - 1, n_tap=2, outside=True, seed=3):
    wav = ref.grid_nonuniform(1500)
    lam = ref.pixels_over(wav, n_pix) if outside else inner_pixels(wav, n_pix)
    data, ivar = positive_data((n_exp, n_pix), seed)
    rows, a, F = table(n_exp, n_trial, n_tap)
    return dict(wav=wav, R=ref.spectrum(wav, 3), lam=lam, sig=np.full(n_pix, 2.5e-10), k=5.0, rows=rows, a=a, F=F,
                data=data, ivar=ivar)


# ---- smallest shapes: one axis at a time about (n_exp, n_comp, n_pix, n_trial) = (5, 2, 33, 7) ---------------------
def _shape_case(dev, name, n_exp=5, n_comp=2, n_pix=TILE + 1, n_trial=T - 1):
    d = design(n_exp, n_pix, n_trial)
    Ub, W = random_filter(n_exp, n_comp, n_pix)
    plain, out = both(dev, d, Ub, W)
    check(name, d, Ub, W, plain, out)
    return d, plain, out


@pytest.mark.parametrize("n_exp", [1, 2, 5])
def test_smallest_exposure_counts(dev, n_exp):
    _shape_case(dev, "n_exp=%d" % n_exp, n_exp=n_exp)


@pytest.mark.parametrize("n_comp", [1, 2, 16])
def test_smallest_component_counts(dev, n_comp):
    _shape_case(dev, "n_comp=%d" % n_comp, n_comp=n_comp)


@pytest.mark.parametrize("n_pix", [1, TILE + 1, TILE * 16 + 1])
def test_smallest_pixel_counts(dev, n_pix):
    """One pixel, a tile and one more, a chunk of 16 tiles and one more (a second chunk, nine tiles of k_detrend)."""
    d, plain, out = _shape_case(dev, "n_pix=%d" % n_pix, n_pix=n_pix)
    if n_pix > 1:   # (pixels beyond the grid's ends have no model: their columns are not filterable where W != 0)
        assert np.isnan(out[2]).any() and np.isfinite(out[2]).any()


@pytest.mark.parametrize("n_trial", [1, T - 1, T + 1])
def test_smallest_trial_counts(dev, n_trial):
    """One trial, a partial group, a second group."""
    _shape_case(dev, "n_trial=%d" % n_trial, n_trial=n_trial)


# ---- the degenerate case -----------------------------------------------------------------------------------------
def test_zero_basis_is_the_plain_exposures_bitwise(dev):
    """U = 0 with random finite W, R without NaN and every pixel covered: moments, n_used and model are
    prom_spectrum_expose's bit for bit."""
    d = design(5, 2 * TILE + 6, 2 * T + 1, n_tap=3, outside=False)
    Ub, W = random_filter(5, 3, len(d["lam"]))
    plain, out = both(dev, d, np.zeros_like(Ub), W)
    assert not np.isnan(plain[2]).any() and np.all(plain[1] == len(d["lam"]))
    assert same(out, plain)
    mom, nu, model = dev.spectrum_expose_detrended(d["wav"], d["R"], model=False)          # moments alone
    assert model is None and same((mom, nu), plain[:2])
    none, none2, model = dev.spectrum_expose_detrended(d["wav"], d["R"], moments=False, model=True)
    assert none is None and none2 is None and np.array_equal(model, plain[2])
    ms = dev.detrend_kernel_ms(2)
    assert len(ms) == 2 and ms[0] > 0.0 and ms[1] > 0.0
    assert same(dev.spectrum_expose(d["wav"], d["R"], model=True), plain)                  # the plain call stands


# ---- independence ------------------------------------------------------------------------------------------------
def _indep_design():
    d = design(5, 2 * TILE + 6, 2 * T + 1, n_tap=3, outside=True, seed=7)
    Ub, W = random_filter(5, 3, len(d["lam"]), seed=5)
    return d, Ub, W


@pytest.fixture(scope="module")
def indep(dev):
    d, Ub, W = _indep_design()
    plain, out = both(dev, d, Ub, W)
    return d, Ub, W, plain, out


def test_two_calls_trials_permuted_and_alone_bitwise(dev, indep):
    d, Ub, W, plain, base = indep
    check("independence base", d, Ub, W, plain, base)
    assert np.isnan(base[2]).any() and np.all(base[1].max(axis=1) > 0)
    assert same(dev.spectrum_expose_detrended(d["wav"], d["R"], model=True), base)         # two calls in a row
    assert same(both(dev, d, Ub, W)[1], base)
    perm = np.random.default_rng(12).permutation(d["F"].shape[1])
    dp = dict(d, F=np.ascontiguousarray(d["F"][:, perm]))
    assert same(both(dev, dp, Ub, W)[1], tuple(x[:, perm] for x in base))
    for j in (0, T - 1, T, 2 * T):
        dj = dict(d, F=np.ascontiguousarray(d["F"][:, j:j + 1]))
        assert same(both(dev, dj, Ub, W)[1], tuple(x[:, j:j + 1] for x in base)), j


_BATCHED = """
import hashlib, json, sys
sys.path.insert(0, %r)
import numpy as np
from prometheus_amd import _native
from test_gpu_detrend import _indep_design, both
d, Ub, W = _indep_design()
out = both(_native.get_device(0), d, Ub, W)[1]
print(json.dumps([hashlib.sha256(x.tobytes()).hexdigest() for x in out]))
"""


def test_batches_under_a_small_scratch_cap_bitwise(indep):
    """PROM_VMAP_SCRATCH_MB is read at context creation, so the case runs in a process of its own: 0.0001 MB is below
    one trial group's records, so every group of the 17 trials is a batch of its own: three batches."""
    base = indep[4]
    env = dict(os.environ, PROM_VMAP_SCRATCH_MB="0.0001", PROM_DEBUG="1")
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _BATCHED % os.path.join(REPO, "tests")],
                       env=env, cwd=REPO, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = [l for l in p.stderr.splitlines() if "detrended moments:" in l]
    assert lines and "3 groups, 3 batches of up to 1 groups" in lines[-1], p.stderr[-2000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("[")][-1])
    assert out == [hashlib.sha256(x.tobytes()).hexdigest() for x in base]


# ---- the padding rule and the unfilterable column ------------------------------------------------------------------
def _nan_design():
    """4 exposures of one tap each: exposure 1 alone reads row 1 of R, in which a NaN is planted; 62 covered pixels."""
    wav = ref.grid_nonuniform(800)
    R = ref.spectrum(wav, 3)
    lam = inner_pixels(wav, 2 * TILE - 2)
    rows = np.array([[0], [1], [2], [0]], dtype=np.int32)
    F = np.ones((4, 3, 1))
    F[:, 1] = 1.0 + 1e-5
    F[:, 2] = 1.0 - 2e-5
    data, ivar = positive_data((4, len(lam)), 2)
    d = dict(wav=wav, R=R, lam=lam, sig=np.full(len(lam), 2.5e-10), k=5.0, rows=rows, a=np.ones((4, 1)), F=F,
             data=data, ivar=ivar)
    Rn = R.copy()
    Rn[1, 417] = np.nan
    return d, dict(d, R=Rn)


def test_padding_rule_keeps_the_other_exposures_bitwise(dev):
    """Exposure 1 carries W = 0 for all k at the pixels its NaN reaches: the other exposures' numbers are those of a
    run without the NaN bit for bit, and exposure 1's pixels there are unused."""
    d, dn = _nan_design()
    Ub, W = random_filter(4, 2, len(d["lam"]), holes=False)
    plain_n = both(dev, dn, Ub, W)[0]
    hit = np.isnan(plain_n[2][1]).any(axis=0)                     # pixels the NaN reaches in some trial
    assert 0 < hit.sum() < len(hit) and not np.isnan(plain_n[2][[0, 2, 3]]).any()
    W[:, 1, hit] = 0.0
    plain, clean = both(dev, d, Ub, W)
    plain_n, out = both(dev, dn, Ub, W)
    check("padding rule", dn, Ub, W, plain_n, out)
    others = [0, 2, 3]
    assert same(tuple(x[others] for x in out), tuple(x[others] for x in clean))
    gone = np.isnan(plain_n[2][1])                                # [n_trial][n_pix]
    assert np.array_equal(np.isnan(out[2][1]), gone) and gone.any()
    assert np.array_equal(out[1][1], clean[1][1] - gone.sum(axis=1))
    # where the NaN does not reach, exposure 1's own filtered model stands too
    assert np.array_equal(out[2][1][~gone], clean[2][1][~gone])


def test_unfilterable_column_is_unused_in_every_exposure(dev):
    """The same NaN with W != 0: the columns it reaches are NaN down every exposure, n_used drops by exactly their
    count in every exposure, and no moment is NaN."""
    d, dn = _nan_design()
    Ub, W = random_filter(4, 2, len(d["lam"]), holes=False)
    plain, clean = both(dev, d, Ub, W)
    plain_n, out = both(dev, dn, Ub, W)
    check("unfilterable column", dn, Ub, W, plain_n, out)
    gone = np.isnan(plain_n[2][1])                                # [n_trial][n_pix]
    assert gone.any() and not gone.all(axis=1).any()
    assert np.all(clean[1] == len(d["lam"]))
    for e in range(4):
        assert np.array_equal(np.isnan(out[2][e]), gone), e
        assert np.array_equal(out[1][e], clean[1][e] - gone.sum(axis=1)), e
    assert not np.isnan(out[0]).any()
    assert np.array_equal(out[2][:, ~gone], clean[2][:, ~gone])


def test_masked_data_are_excluded_and_the_model_stands(dev):
    """ivar 0, negative, infinite and NaN, NaN and infinite data: the pixel is unused in its exposure, the filtered
    model (which data and ivar play no part in once W is given) is returned all the same."""
    d = design(2, 2 * TILE + 3, 3, n_tap=3, outside=False, seed=4)
    Ub, W = random_filter(2, 2, len(d["lam"]))
    clean = both(dev, d, Ub, W)[1]
    ivar, data = d["ivar"].copy(), d["data"].copy()
    ivar[0, 3], ivar[0, 12], ivar[1, 5], ivar[1, 9] = 0.0, -1.0, np.nan, np.inf
    data[1, 8], data[1, 20] = np.nan, np.inf
    dm = dict(d, ivar=ivar, data=data)
    plain, out = both(dev, dm, Ub, W)
    check("masked data", dm, Ub, W, plain, out)
    assert np.array_equal(out[2], clean[2]) and np.isfinite(out[2]).all()
    assert np.all(clean[1][0] - out[1][0] == 2) and np.all(clean[1][1] - out[1][1] == 4)


def test_planted_signal_is_found(dev):
    """Data := the device's own filtered model of trial j0: m6[:, j0] is exactly 0 and the summed chi-square has its
    minimum there."""
    d = design(5, 2 * TILE + 6, 2 * T + 1, n_tap=3, outside=False, seed=9)
    Ub, W = random_filter(5, 3, len(d["lam"]), seed=8)
    j0 = T + 2
    model = both(dev, d, Ub, W)[1][2]
    dp = dict(d, data=np.ascontiguousarray(model[:, j0]))
    plain, out = both(dev, dp, Ub, W)
    assert np.array_equal(out[2], model) and np.all(out[1] == len(d["lam"]))
    assert np.all(out[0][:, j0, 6] == 0.0)
    chi2 = out[0][..., 6].sum(axis=0)
    assert int(np.argmin(chi2)) == j0 and np.all(np.delete(chi2, j0) > 0)
    check("planted signal", dp, Ub, W, plain, out, exact=False)


# ---- argument and state errors ---------------------------------------------------------------------------------
def test_errors():
    from prometheus_amd import _native
    wav = ref.grid_nonuniform(100)
    R = ref.spectrum(wav, 2)
    lam, sig = wav[[10, 20, 30]], np.full(3, 2e-10)
    data, ivar = positive_data((4, 3), 6)
    rows, a, _ = table(4, 3, 2, n_orb=2)
    F = 1.0 + 1e-6 * np.arange(24.0).reshape(4, 3, 2)
    Ub, W = random_filter(4, 2, 3)
    d = _native.Device(0)
    try:
        for call in (lambda: d.detrend_set(Ub, W), lambda: d.spectrum_expose_detrended(wav, R),
                     d.transit_expose_detrended, d.detrend_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):      # no exposure table on the context
                call()
        d.observe_set(lam, sig, 5.0, 2)
        d.expose_set(rows, a, F, data, ivar)
        for call in (lambda: d.spectrum_expose_detrended(wav, R), d.transit_expose_detrended, d.detrend_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):      # a table, but no filter
                call()
        with pytest.raises(_native.NativeError, match=E_ARG):            # another n_exp
            d.detrend_set(Ub[:3], W[:, :3])
        for n_comp in (0, 17):
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.detrend_set(np.zeros((4, n_comp)), np.zeros((n_comp, 4, 3)))
        for bad in (np.nan, np.inf):
            Ubad = Ub.copy()
            Ubad[2, 1] = bad
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.detrend_set(Ubad, W)
            Wbad = W.copy()
            Wbad[1, 3, 2] = bad
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.detrend_set(Ub, Wbad)
        with pytest.raises(ValueError):                                   # W of another shape
            d.detrend_set(Ub, W[:, :, :2])
        with pytest.raises(_native.NativeError, match=E_STATE):          # a failed set leaves no filter behind
            d.spectrum_expose_detrended(wav, R)
        d.detrend_set(Ub, W, key="f")
        assert d.detrend_key == "f"
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.transit_expose_detrended()                                  # no run yet
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_expose_detrended(wav, ref.spectrum(wav, 3))        # another n_orb
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_expose_detrended(wav[::-1], R)                     # descending grid
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.detrend_kernel_ms()                                         # no detrended call yet
        mom, nu, model = d.spectrum_expose_detrended(wav, R, model=True)
        assert mom.shape == (4, 3, 7) and nu.shape == (4, 3) and model.shape == (4, 3, 3) and np.all(nu == 3)
        assert all(ms > 0.0 for ms in d.detrend_kernel_ms(2))
        d.expose_set(rows, a, F, data, ivar)                              # drops the filter
        assert d.detrend_key is None
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.spectrum_expose_detrended(wav, R)
        d.detrend_set(Ub, W, key="f")
        d.observe_set(lam, sig, 5.0, 2)                                   # drops the table and the filter with it
        assert d.detrend_key is None and d.expose_key is None
        for call in (lambda: d.spectrum_expose_detrended(wav, R), lambda: d.detrend_set(Ub, W)):
            with pytest.raises(_native.NativeError, match=E_STATE):
                call()
        d.observe_set(lam[:0], sig[:0], 5.0, 2)                           # no pixel: zeros
        d.expose_set(rows, a, F, data[:, :0], ivar[:, :0])
        d.detrend_set(Ub, W[:, :, :0])
        mom, nu, model = d.spectrum_expose_detrended(wav, R, model=True)
        assert np.all(mom == 0) and np.all(nu == 0) and model.shape == (4, 3, 0)
    finally:
        d.close()


# ---- end to end ------------------------------------------------------------------------------------------------
def _product_transit(cfg):
    from oracle import prom_oracle as O
    from prometheus_amd import gasProperties as gp
    from prometheus_amd import setupfile
    gp.register_molecular_table("H2O", O.synthetic_molecular_table(n_nu=2001))
    return setupfile.build_transit(cfg)


@pytest.mark.parametrize("name", ["C1", "C3r"])
def test_transit_expose_detrended_end_to_end(name, monkeypatch):
    """Transit.expose(ex, detrend=dt) on the reduced golden problems, 40 pixels about Na D2 in the caller's (descending)
    order, a smeared table of 4 trials: the raw binding's numbers in the caller's pixel order; a second call uploads
    nothing; detrend=None is the plain expose bit for bit."""
    from prometheus_amd import _native
    from prometheus_amd import constants as const
    from prometheus_amd import lightcurve as lc
    from prometheus_amd import observation as obs
    g = np.load(os.path.join(G, "transit_" + name + ".npz"))
    cfg = json.loads(str(g["config"]))
    if cfg["Grids"]["orbphase_steps"] < 2:      # C1 has one phase and exposure_taps needs a bracket: C1 with three
        cfg["Grids"].update(orbphase_border=0.02, orbphase_steps=3)
    tr = _product_transit(cfg)
    orb = tr.spatialGrid.constructOrbphaseAxis()
    n_orb = len(orb)
    px = lc.NA_D2 + 5e-10 * (np.arange(40) - 19.5)
    ins = obs.Instrument(px[::-1], resolving_power=140000.0, truncate=5.0)
    base = obs.planet_frame_shifts(tr.planet, orb)
    Kp = np.sqrt(const.G * tr.planet.hostStar.M / tr.planet.a)
    n_exp = 6
    mid = np.linspace(orb[0], orb[-1], n_exp + 2)[1:-1]
    width = np.full(n_exp, 0.5 * (orb[1] - orb[0]))
    rows, a, F = obs.exposure_taps(orb, base, mid, width, n_sub=3, Kp=Kp * np.array([0.9, 1.0]), Vsys=[0.0, 2e5])
    rng = np.random.default_rng(3)
    data = 1.0 + 1e-3 * rng.normal(size=(n_exp, 40))
    err = np.full((n_exp, 40), 1e-3)
    err[2, 7] = np.nan                                                    # a masked pixel: W = 0 there
    Ub, clean = obs.sysrem(data, err, 1, ones=True)
    ex = obs.Exposures(ins, rows, a, F, clean, err)
    dt = obs.Detrend(ex, Ub)
    assert dt.W.shape == (2, n_exp, 40) and np.all(dt.W[:, 2, ins.sort(np.arange(40.0)) == 7.0] == 0)
    plain = tr.expose(ex, return_model=True, devices=[0])
    out = tr.expose(ex, return_model=True, devices=[0], detrend=dt)
    dev = _native.get_device(0)
    assert dev.expose_key == ex.key and dev.detrend_key == dt.key
    raw = dev.transit_expose_detrended(model=True)
    assert np.array_equal(out.moments, raw[0]) and np.array_equal(out.n_used, raw[1])
    assert np.array_equal(out.model, ins.unsort(raw[2]), equal_nan=True) and out.model.shape == (n_exp, 4, 40)
    # (the reduced grid of C3r leaves some pixels without a model in some exposures: those columns are not filterable)
    want, ok = dref.filter_f64(ins.sort(plain.model), dt.U, dt.W)
    assert ok.any() and np.array_equal(ins.sort(out.model), want, equal_nan=True)
    used = used_by_definition(ins.sort(plain.model), ok, ex.data, ex.ivar)
    assert np.array_equal(out.n_used, used.sum(axis=2)) and np.all(out.n_used >= 1)
    assert not np.array_equal(out.moments, plain.moments) and np.all(out.n_used <= plain.n_used)
    # the filter took the exposures' mean out of every filterable column (uniform weights but for the masked pixel 7)
    left = np.delete(out.model.mean(axis=0), 7, axis=-1)
    assert np.isfinite(left).any() and np.nanmax(np.abs(left)) < 1e-9 * np.nanmax(np.abs(plain.model))
    # a second call with the same objects: nothing is uploaded, the same bits
    calls = []
    for fn in ("observe_set", "expose_set", "detrend_set"):
        monkeypatch.setattr(dev, fn, lambda *a, _fn=fn, **k: calls.append(_fn))
    again = tr.expose(ex, devices=[0], detrend=dt)
    assert calls == [] and again.model is None
    assert np.array_equal(again.moments, out.moments) and np.array_equal(again.n_used, out.n_used)
    monkeypatch.undo()
    # detrend=None: the plain call, bit for bit, the filter still resident
    none = tr.expose(ex, return_model=True, devices=[0], detrend=None)
    assert np.array_equal(none.moments, plain.moments, equal_nan=True) and np.array_equal(none.n_used, plain.n_used)
    assert np.array_equal(none.model, plain.model, equal_nan=True) and dev.detrend_key == dt.key
