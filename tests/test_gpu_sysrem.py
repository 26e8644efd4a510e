"""Injection and SYSREM on the device (include/prom_hip.h, "injection and SYSREM on the device") against the float64
restatement of the definition (tests/helpers/sysrem_ref.py), bit for bit, over the shapes at which the kernels can go
wrong (T = the step kernel's pixel tile): n_pix in {1, T - 1, T, T + 1, 3 T + 5}, n_exp in {1, 2, 7, 70}, n_comp in
{1, 3, 16, 0 with ones}, n_iter in {1, 4}; the masks, the injection's clauses, the accuracy against a longdouble run
with observation.sysrem's own distance as the yardstick, a planted planet end to end, and the refusals."""
import json
import os

import numpy as np
import pytest

from helpers import observe_ref as ref
from helpers import sysrem_ref as sref
from helpers import vmap_ref as vref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
E_ARG, E_STATE = "PROM_E_ARG", "PROM_E_STATE"
T = sref.TILE


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


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


def design(n_exp, n_pix, n_trial=3, seed=3, holes=True):
    """The spectrum entries' inputs on observe_ref.grid_nonuniform(1500): some pixels lie beyond the grid's ends and
    have no model; raw data with a systematic a[e] c[p] on a continuum, with NaN, an infinity and ivar = 0 sprinkled
    in."""
    wav = ref.grid_nonuniform(1500)
    rng = np.random.default_rng(seed)
    lam = ref.pixels_over(wav, n_pix)
    raw = (1.0 + 0.02 * rng.normal(size=(n_exp, n_pix))
           + 0.3 * rng.normal(size=n_exp)[:, None] * rng.normal(size=n_pix)[None, :])
    ivar = 1e4 * (0.1 + rng.random((n_exp, n_pix)))
    if holes and n_pix > 4:
        raw[rng.random(raw.shape) < 0.03] = np.nan
        raw[rng.random(raw.shape) < 0.005] = np.inf
        ivar[rng.random(raw.shape) < 0.03] = 0.0
    rows, a, F = table(n_exp, n_trial, 2)
    return dict(wav=wav, R=ref.spectrum(wav, 3), lam=lam, sig=np.full(n_pix, 2.5e-10), k=5.0, rows=rows, a=a, F=F,
                data=np.ones((n_exp, n_pix)), ivar=ivar, raw=raw)


def two_orders(n_pix, seed=5):
    """(seg_first, perm, labels) of two orders interleaved along the device's pixels (one order when n_pix = 1)."""
    rng = np.random.default_rng(seed)
    labels = (np.arange(n_pix) // 3 + (rng.random(n_pix) < 0.2)) % 2
    if n_pix > 1:
        labels[:2] = [0, 1]
    members = [np.flatnonzero(labels == s) for s in np.unique(labels)]
    seg = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
    return seg, np.concatenate(members).astype(np.int32), labels


def upload(dev, d, hp=None):
    """The observation, the table, the raw exposures and (hp = (taps, mode)) the high-pass over two_orders."""
    dev.observe_set(d["lam"], d["sig"], d["k"], d["R"].shape[0])
    dev.expose_set(d["rows"], d["a"], d["F"], d["data"], d["ivar"])
    dev.sysrem_set(d["raw"])
    if hp is not None:
        seg, perm, _ = two_orders(len(d["lam"]))
        dev.highpass_set(seg, perm, hp[0], hp[1])


def expected(dev, d, trial, scale, n_comp, n_iter, ones, hp=None):
    """(U, cleaned, injected) by the definition in numpy, from prom_spectrum_expose's own model of trial ``trial``
    (None: no injection) and observation.high_pass."""
    from prometheus_amd import observation as obs
    D = d["raw"]
    if trial is not None:
        M = dev.spectrum_expose(d["wav"], d["R"], moments=False, model=True)[2][:, trial]
        D = sref.inject_f64(d["raw"], M, scale)
    if hp is not None:
        D = obs.high_pass(D, hp[0], orders=two_orders(D.shape[1])[2], mode=("subtract", "divide")[hp[1]])
    U, cleaned = sref.sysrem_f64(D, d["ivar"], n_comp, n_iter, ones)
    return U, cleaned, D


def same(got, want, name):
    for g, w, what in zip(got, want, ("U", "cleaned", "injected")):
        assert g.shape == w.shape, (name, what)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (name, what, "NaN pattern")
        assert np.array_equal(g, w, equal_nan=True), (name, what, float(np.nanmax(np.abs(g - w))))


# ---- 1: bit for bit over the shapes -----------------------------------------------------------------------------------
#        n_exp, n_pix, n_comp, n_iter, ones, high-pass mode (None: none)
SHAPES = [(1, 1, 1, 1, False, None),
          (2, T - 1, 3, 4, True, None),
          (7, T, 16, 1, False, 0),
          (7, T + 1, 0, 4, True, 1),
          (70, 3 * T + 5, 3, 4, False, 0),
          (70, 3 * T + 5, 3, 4, True, 1),
          (70, T + 1, 1, 1, False, None),
          (2, 3 * T + 5, 15, 1, True, None),
          (1, T, 3, 4, False, 1)]


@pytest.mark.parametrize("n_exp,n_pix,n_comp,n_iter,ones,mode", SHAPES)
def test_injection_and_sysrem_bitwise_over_the_shapes(dev, n_exp, n_pix, n_comp, n_iter, ones, mode):
    """U, cleaned and injected of prom_spectrum_inject and of prom_sysrem_clean equal sysrem_f64 on the numpy injection
    of prom_spectrum_expose's own model (and observation.high_pass of it), NaN pattern included."""
    d = design(n_exp, n_pix, seed=n_exp + n_pix)
    hp = None if mode is None else (np.exp(-0.5 * (np.arange(6) / 2.0) ** 2), mode)
    upload(dev, d, hp)
    name = "n_exp=%d n_pix=%d n_comp=%d n_iter=%d ones=%d mode=%s" % (n_exp, n_pix, n_comp, n_iter, ones, mode)
    args = dict(n_comp=n_comp, n_iter=n_iter, ones=ones, highpass=hp is not None, injected=True)
    want = expected(dev, d, 1, 0.7, n_comp, n_iter, ones, hp)
    got = dev.spectrum_inject(d["wav"], d["R"], 1, 0.7, **args)
    same(got, want, name + " inject")
    got = dev.sysrem_clean(**args)
    same(got, expected(dev, d, None, 0.0, n_comp, n_iter, ones, hp), name + " clean")
    assert got[0].shape == (n_exp, n_comp + ones) and (not ones or np.all(got[0][:, 0] == 1.0))
    # without asking for it, no injected data; U alone is the same U
    U, cleaned, inj = dev.sysrem_clean(n_comp=n_comp, n_iter=n_iter, ones=ones, highpass=hp is not None)
    assert inj is None and np.array_equal(U, got[0]) and np.array_equal(cleaned, got[1], equal_nan=True)


# ---- 2: masks -----------------------------------------------------------------------------------------------------------
def test_entries_without_weight_come_back_and_influence_nothing(dev):
    d = design(7, 3 * T + 5, seed=8)
    upload(dev, d)
    U, cleaned, _ = dev.sysrem_clean(3, 4)
    w, _ = sref.weights_of(d["raw"], d["ivar"])
    assert (w == 0).sum() > 20 and np.array_equal(cleaned[w == 0], d["raw"][w == 0], equal_nan=True)
    for fill in (np.nan, 1e300):
        d2 = dict(d, raw=np.where(w == 0, fill, d["raw"]), ivar=np.where(w == 0, 0.0, d["ivar"]))
        upload(dev, d2)
        U2, cleaned2, _ = dev.sysrem_clean(3, 4)
        assert np.array_equal(U2, U) and np.array_equal(cleaned2[w > 0], cleaned[w > 0])
        assert np.array_equal(cleaned2[w == 0], d2["raw"][w == 0], equal_nan=True)


def test_a_masked_pixel_a_masked_exposure_and_all_masked_data(dev):
    d = design(7, T + 1, seed=9, holes=False)
    d["ivar"][:, 5] = 0.0
    d["ivar"][2, :] = 0.0
    upload(dev, d)
    U, cleaned, _ = dev.sysrem_clean(3, 4, ones=True)
    same((U, cleaned), sref.sysrem_f64(d["raw"], d["ivar"], 3, 4, True), "masked pixel and exposure")
    assert np.all(U[2, 1:] == 0) and np.isfinite(U).all() and np.isfinite(cleaned).all()
    assert np.array_equal(cleaned[:, 5], d["raw"][:, 5]) and np.array_equal(cleaned[2], d["raw"][2])
    for raw, ivar in ((d["raw"], np.zeros_like(d["ivar"])), (np.full_like(d["raw"], np.nan), d["ivar"])):
        upload(dev, dict(d, raw=raw, ivar=ivar))
        U, cleaned, _ = dev.sysrem_clean(2, 3, ones=True)
        assert np.all(U[:, 0] == 1) and np.all(U[:, 1:] == 0) and not np.signbit(U).any()
        assert np.array_equal(cleaned, raw, equal_nan=True)


# ---- 3: the injection's clauses ---------------------------------------------------------------------------------------
def test_injection_clauses_bitwise(dev):
    d = design(7, 3 * T + 5, n_trial=11, seed=10)
    upload(dev, d)
    args = dict(n_comp=2, n_iter=4, injected=True)
    clean = dev.sysrem_clean(**args)
    zero = dev.spectrum_inject(d["wav"], d["R"], 4, 0.0, **args)
    same(zero, clean, "scale = 0")
    M = dev.spectrum_expose(d["wav"], d["R"], moments=False, model=True)[2]
    j = 7
    out = dev.spectrum_inject(d["wav"], d["R"], j, 1.3, **args)
    gone = np.isnan(M[:, j])
    assert gone.any() and not gone.all()
    assert np.array_equal(out[2][gone], d["raw"][gone], equal_nan=True)           # NaN in M leaves raw
    moved = ~gone & np.isfinite(d["raw"])
    assert np.any(out[2][moved] != d["raw"][moved])
    again = dev.spectrum_inject(d["wav"], d["R"], j, 1.3, **args)                 # two calls agree
    same(again, out, "two calls")
    upload(dev, dict(d, F=np.ascontiguousarray(d["F"][:, j:j + 1])))              # the trial alone, in position 0
    same(dev.spectrum_inject(d["wav"], d["R"], 0, 1.3, **args), out, "trial alone")
    # raw and the table's data are never written: the same call gives the same once more
    same(dev.spectrum_inject(d["wav"], d["R"], 0, 1.3, **args), out, "raw unchanged")


# ---- 4: accuracy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_exp,n_pix,seed", [(7, T + 1, 1), (70, 3 * T + 5, 2), (70, T - 1, 3)])
def test_cleaned_data_within_four_times_the_host_functions_own_distance(dev, n_exp, n_pix, seed):
    """d(x) = max |cleaned_x - cleaned_ld| over the weighted entries; d(device) <= 4 max(d(observation.sysrem),
    n_pix 2^-53 max |D|): the yardstick is the existing float64 host function's own distance from the longdouble run."""
    from prometheus_amd import observation as obs
    D, ivar = sref.planted(n_exp, n_pix, seed)
    d = design(n_exp, n_pix, seed=seed)
    upload(dev, dict(d, raw=D, ivar=ivar))
    U, cleaned, _ = dev.sysrem_clean(3, 30)
    w, _ = sref.weights_of(D, ivar)
    _, cld = sref.sysrem_ld(D, ivar, 3, 30)
    d_dev = sref.distance(cleaned, cld, w)
    d_host = sref.distance(obs.sysrem(D, np.where(ivar > 0, 1e-3, np.nan), 3, 30)[1], cld, w)
    bound = 4.0 * max(d_host, sref.margin(D, n_pix))
    print("SYSREM_ERR n_exp=%d n_pix=%d: device %.3g, observation.sysrem %.3g, bound %.3g, fraction %.4f"
          % (n_exp, n_pix, d_dev, d_host, bound, d_dev / bound))
    assert np.isfinite(U).all() and d_dev <= bound


# ---- 5: a planted planet, end to end, and the Python path -------------------------------------------------------------
@pytest.fixture(scope="module")
def planet():
    from oracle import prom_oracle as O
    from prometheus_amd import gasProperties as gp
    from prometheus_amd import observation as obs
    from prometheus_amd import setupfile
    g = np.load(os.path.join(G, "transit_C1.npz"))
    cfg = json.loads(str(g["config"]))
    cfg["Grids"].update(sref.PLANET_CFG)
    gp.register_molecular_table("H2O", O.synthetic_molecular_table(n_nu=2001))
    tr = setupfile.build_transit(cfg)
    d = sref.planet_design(tr.planet, tr.spatialGrid.constructOrbphaseAxis())
    ex = obs.Exposures(d["ins"], d["rows"], d["a"], d["F"], d["raw"], d["err"])
    return tr, d, ex, obs.Injection(ex, d["raw"]), obs.HighPass(ex, d["taps"], orders=d["orders"], mode=d["mode"])


def test_planted_planet_is_recovered_at_its_trial(planet):
    """Inject trial j* at scale 1 into noisy raw data with planted systematics, clean on the device with the high-pass,
    build Exposures, HighPass and Detrend from the returned data and U, run expose: the summed log-likelihood over the
    trials peaks at j*."""
    from prometheus_amd import observation as obs
    tr, d, ex, inj, hp = planet
    res = tr.inject(inj, sref.PLANET_TRIAL, 1.0, n_comp=d["n_comp"], n_iter=d["n_iter"], ones=d["ones"], highpass=hp,
                    devices=[0])
    assert res.U.shape == (12, 3) and res.data.shape == (12, 400) and res.injected is None
    assert np.isnan(res.data[3, 7]) and np.isfinite(np.delete(res.data.ravel(), 3 * 400 + 7)).all()
    ex2 = obs.Exposures(d["ins"], d["rows"], d["a"], d["F"], res.data, d["err"])
    vm = tr.expose(ex2, devices=[0], highpass=obs.HighPass(ex2, d["taps"], orders=d["orders"], mode=d["mode"]),
                   detrend=obs.Detrend(ex2, res.U))
    ll = vm.loglike.sum(axis=0)
    print("planted planet, device: logL - max per trial", ll - ll.max())
    assert int(np.argmax(ll)) == sref.PLANET_TRIAL


def test_transit_inject_and_clean_are_the_spectrum_entries(planet):
    """Transit.inject equals prom_spectrum_inject on the run's R, and with broaden= on tr.broadened(bk), in the
    caller's pixel order; Transit.clean equals prom_sysrem_clean; a second call uploads nothing."""
    from prometheus_amd import _native
    from prometheus_amd import observation as obs
    tr, d, ex, inj, hp = planet
    ins = d["ins"]
    dev = _native.get_device(0)
    bk = obs.Broadening(*obs.rotation_kernel(3e5, n=33))
    for broaden in (None, bk):
        res = tr.inject(inj, 2, 0.5, n_comp=2, n_iter=4, highpass=hp, broaden=broaden, return_injected=True,
                        devices=[0])
        assert dev.expose_key == ex.key and dev.highpass_key == hp.key and dev.sysrem_key == inj.key
        R = np.array(tr.sumOverChords(devices=[0])) if broaden is None else tr.broadened(bk, devices=[0])
        wav = np.asarray(tr.wavelength)
        U, cleaned, injected = dev.spectrum_inject(wav, R, 2, 0.5, n_comp=2, n_iter=4, highpass=True, injected=True)
        same((res.U, res.data, res.injected), (U, ins.unsort(cleaned), ins.unsort(injected)), "Transit.inject")
        # the definition on Transit.expose's own model, in the caller's order
        M = tr.expose(ex, return_model=True, devices=[0], broaden=broaden).model[:, 2]
        want = obs.high_pass(sref.inject_f64(d["raw"], M, 0.5), d["taps"], orders=d["orders"], mode=d["mode"])
        assert np.array_equal(res.injected, want, equal_nan=True)
    res = tr.clean(inj, n_comp=2, n_iter=4, ones=True, highpass=hp, return_injected=True)
    U, cleaned, injected = dev.sysrem_clean(2, 4, ones=True, highpass=True, injected=True)
    same((res.U, res.data, res.injected), (U, ins.unsort(cleaned), ins.unsort(injected)), "Transit.clean")
    want = obs.high_pass(d["raw"], d["taps"], orders=d["orders"], mode=d["mode"])
    assert np.array_equal(res.injected, want, equal_nan=True)
    same((res.U, ins.sort(res.data)), sref.sysrem_f64(ins.sort(want), ex.ivar, 2, 4, True), "Transit.clean, definition")
    assert tr.clean(inj, n_comp=2).injected is None


# ---- 6: refusals ------------------------------------------------------------------------------------------------------
def test_errors():
    from prometheus_amd import _native
    wav = ref.grid_nonuniform(100)
    R = ref.spectrum(wav, 2)
    lam, sig = wav[[10, 20, 30, 40]], np.full(4, 2e-10)
    rng = np.random.default_rng(6)
    data, ivar = 0.9 + 0.05 * rng.random((4, 4)), 1e4 * (0.1 + rng.random((4, 4)))
    raw = 1.0 + 0.1 * rng.random((4, 4))
    rows, a, _ = table(4, 3, 2, n_orb=2)
    F = 1.0 + 1e-6 * np.arange(24.0).reshape(4, 3, 2)
    seg, perm, g = np.array([0, 1, 4]), np.array([2, 0, 3, 1]), np.array([1.0, 0.5])
    d = _native.Device(0)
    try:
        for call in (lambda: d.sysrem_set(raw), lambda: d.sysrem_clean(2), lambda: d.transit_inject(0, 1.0, 2),
                     lambda: d.spectrum_inject(wav, R, 0, 1.0, 2), d.sysrem_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):      # no exposure table on the context
                call()
        d.observe_set(lam, sig, 5.0, 2)
        d.expose_set(rows, a, F, data, ivar)
        for call in (lambda: d.sysrem_clean(2), lambda: d.spectrum_inject(wav, R, 0, 1.0, 2), d.sysrem_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):      # a table, but no raw exposures
                call()
        for bad in (raw[:3], raw[:, :3], np.ones((5, 4))):
            with pytest.raises(_native.NativeError, match=E_ARG):        # a shape other than the table's
                d.sysrem_set(bad)
        with pytest.raises(_native.NativeError, match=E_STATE):          # a failed set leaves nothing behind
            d.sysrem_clean(2)
        d.sysrem_set(raw, key="r")
        assert d.sysrem_key == "r"
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.sysrem_kernel_ms()                                          # no call yet
        for kw in (dict(n_comp=0), dict(n_comp=-1, ones=True), dict(n_comp=17), dict(n_comp=16, ones=True),
                   dict(n_comp=2, n_iter=0)):
            with pytest.raises(_native.NativeError, match=E_ARG):        # ranges broken
                d.sysrem_clean(**kw)
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.spectrum_inject(wav, R, 0, 1.0, **kw)
        for trial in (-1, 3):
            with pytest.raises(_native.NativeError, match=E_ARG):        # a trial outside [0, n_trial)
                d.spectrum_inject(wav, R, trial, 1.0, 2)
        for scale in (np.nan, np.inf, -np.inf):
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.spectrum_inject(wav, R, 0, scale, 2)
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_inject(wav, ref.spectrum(wav, 3), 0, 1.0, 2)      # another n_orb
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_inject(wav[::-1], R, 0, 1.0, 2)                   # descending grid
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.transit_inject(0, 1.0, 2)                                   # no run yet
        for call in (lambda: d.sysrem_clean(2, highpass=True), lambda: d.spectrum_inject(wav, R, 0, 1.0, 2, highpass=True)):
            with pytest.raises(_native.NativeError, match=E_STATE):      # highpass = 1 without a resident high-pass
                call()
        U, cleaned, inj = d.spectrum_inject(wav, R, 2, -0.5, 2, n_iter=3, ones=True, injected=True)
        assert U.shape == (4, 3) and cleaned.shape == (4, 4) and inj.shape == (4, 4) and np.isfinite(cleaned).all()
        ms = d.sysrem_kernel_ms(2)
        assert ms[0] > 0.0 and ms[1] > 0.0 and np.isnan(ms[2])
        d.highpass_set(seg, perm, g, 1)
        assert d.sysrem_key == "r"                                        # a high-pass leaves the raw exposures alone
        U, cleaned, inj = d.sysrem_clean(1, highpass=True)
        ms = d.sysrem_kernel_ms(2)
        assert ms[0] > 0.0 and np.isnan(ms[1]) and ms[2] > 0.0
        d.expose_set(rows, a, F, data, ivar)                              # drops the raw exposures
        assert d.sysrem_key is None
        for call in (lambda: d.sysrem_clean(2), lambda: d.spectrum_inject(wav, R, 0, 1.0, 2), d.sysrem_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):
                call()
        d.sysrem_set(raw, key="r")
        d.observe_set(lam, sig, 5.0, 2)                                   # drops the table and the raw exposures with it
        assert d.sysrem_key is None and d.expose_key is None
        for call in (lambda: d.sysrem_clean(2), lambda: d.sysrem_set(raw)):
            with pytest.raises(_native.NativeError, match=E_STATE):
                call()
        d.observe_set(lam[:0], sig[:0], 5.0, 2)                           # no pixel: every component ends
        d.expose_set(rows, a, F, data[:, :0], ivar[:, :0])
        d.sysrem_set(raw[:, :0])
        U, cleaned, inj = d.sysrem_clean(2, ones=True)
        assert np.all(U[:, 0] == 1) and np.all(U[:, 1:] == 0) and cleaned.shape == (4, 0)
    finally:
        d.close()
