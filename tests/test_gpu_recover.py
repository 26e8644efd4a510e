"""Recovery on the device (include/prom_hip.h, "recovery on the device"): prom_spectrum_recover against the route of
separate calls on a second table (prom_spectrum_inject, prom_expose_set with data = cleaned, prom_detrend_set with
(U, prom_filter_weights), then the detrended, high-pass or per-order call), bit for bit, over n_pix in {1, 127, 129} x
n_exp in {2, 7}, with and without ones, the high-pass off, subtracting and dividing over two interleaved orders, the
orders on and off; the independence of the trial's position, scale = 0, the resident filter left alone, the refusals,
Transit.recover against the entry, and the planted planet end to end."""
import numpy as np
import pytest

from helpers import observe_ref as ref
from helpers import sysrem_ref as sref
import test_gpu_sysrem as ts

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = "PROM_E_ARG", "PROM_E_STATE"
NAMES = ("moments", "n_used", "order moments", "order n_used", "totals", "model", "U")
TAPS = np.exp(-0.5 * (np.arange(6) / 2.0) ** 2)


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


planet = ts.planet   # (the module's fixture: reduced C1 and the planted-planet design)


def upload(dev, d, mode, orders, data=None):
    """The observation, the table (with ``data`` in the place of the design's), the raw exposures, the high-pass
    (mode 0 or 1, None: none) and the orders over two_orders."""
    ts.upload(dev, d if data is None else dict(d, data=data), None if mode is None else (TAPS, mode))
    if orders:
        seg, perm, _ = ts.two_orders(len(d["lam"]))
        dev.orders_set(seg, perm, np.ones(len(seg) - 1, dtype=np.uint8))


def separate(dev, d, trial, scale, n_comp, n_iter, ones, mode, orders):
    """The recovery by separate calls: inject (clean for trial None), a second table whose data are the cleaned
    exposures, the filter (U, prom_filter_weights(U, ivar)), then the call that fits: recover's seven outputs."""
    upload(dev, d, mode, False)
    kw = dict(n_comp=n_comp, n_iter=n_iter, ones=ones, highpass=mode is not None)
    if trial is None:
        U, cleaned, _ = dev.sysrem_clean(**kw)
    else:
        U, cleaned, _ = dev.spectrum_inject(d["wav"], d["R"], trial, scale, **kw)
    upload(dev, d, mode, orders, data=cleaned)
    dev.detrend_set(U, dev.filter_weights(U, d["ivar"]))
    if orders:
        out = dev.spectrum_expose_orders(d["wav"], d["R"], highpass=mode is not None, detrend=True, model=True)
    elif mode is not None:
        mom, nu, model = dev.spectrum_expose_highpass(d["wav"], d["R"], detrend=True, model=True)
        out = (mom, nu, None, None, None, model)
    else:
        mom, nu, model = dev.spectrum_expose_detrended(d["wav"], d["R"], model=True)
        out = (mom, nu, None, None, None, model)
    return out + (U,)


def same(got, want, name):
    for g, w, what in zip(got, want, NAMES):
        assert (g is None) == (w is None), (name, what)
        if g is not None:
            assert g.shape == w.shape, (name, what)
            assert np.array_equal(g, w, equal_nan=True), (name, what)


# ---- 1: the equivalence clause over the shapes --------------------------------------------------------------------
#          ones, high-pass mode (None: none), orders, n_comp
CONFIGS = [(False, None, False, 2), (True, 0, True, 1), (False, 1, True, 2), (True, 1, False, 0), (True, None, True, 1)]


@pytest.mark.parametrize("n_exp,n_pix", [(2, 1), (2, 127), (2, 129), (7, 1), (7, 127), (7, 129)])
def test_recover_is_the_route_of_separate_calls_bitwise(dev, n_exp, n_pix):
    """NaN, an infinity and ivar = 0 are sprinkled into raw and ivar (test_gpu_sysrem's design); the trial injected is
    1 of 3 at scale 0.7."""
    d = ts.design(n_exp, n_pix, seed=n_exp + n_pix)
    used = 0
    for ones, mode, orders, n_comp in CONFIGS:
        name = "n_exp=%d n_pix=%d ones=%d mode=%s orders=%d" % (n_exp, n_pix, ones, mode, orders)
        want = separate(dev, d, 1, 0.7, n_comp, 4, ones, mode, orders)
        upload(dev, d, mode, orders)
        got = dev.spectrum_recover(d["wav"], d["R"], 1, 0.7, n_comp, n_iter=4, ones=ones, highpass=mode is not None,
                                   orders=orders, model=True)
        same(got, want, name)
        used += int(got[1].sum())
        # every output may be NULL, and what is asked for alone is the same
        lean = dev.spectrum_recover(d["wav"], d["R"], 1, 0.7, n_comp, n_iter=4, ones=ones, highpass=mode is not None,
                                    orders=orders, records=False)
        assert lean[2] is None and lean[3] is None and lean[5] is None
        same((lean[0], lean[1], lean[4], lean[6]), (want[0], want[1], want[4], want[6]), name + " lean")
    assert used > 0 or n_pix == 1


def test_trial_position_scale_zero_and_the_resident_filter(dev):
    """Trial j of an 11-trial table gives the moments the trial alone in position 0 gives; scale = 0 is the recovery
    against prom_sysrem_clean; the filter of prom_detrend_set is neither read nor replaced; two calls agree; raw and
    the table's data are not written."""
    d = ts.design(7, 129, n_trial=11, seed=10)
    j = 7
    kw = dict(n_comp=2, n_iter=4, highpass=True, orders=True, model=True)
    upload(dev, d, 0, True)
    plain = dev.spectrum_expose(d["wav"], d["R"])
    inj0 = dev.spectrum_inject(d["wav"], d["R"], j, 1.3, n_comp=2, n_iter=4, highpass=True, injected=True)
    full = dev.spectrum_recover(d["wav"], d["R"], j, 1.3, **kw)
    same(dev.spectrum_recover(d["wav"], d["R"], j, 1.3, **kw), full, "two calls")
    # the resident filter: a detrended call before and after a recover call gives the same bits
    Ur = np.random.default_rng(3).normal(size=(7, 3))
    dev.detrend_build(Ur, key="mine")
    before = dev.spectrum_expose_detrended(d["wav"], d["R"], model=True)
    same(dev.spectrum_recover(d["wav"], d["R"], j, 1.3, **kw), full, "with a resident filter")
    after = dev.spectrum_expose_detrended(d["wav"], d["R"], model=True)
    assert dev.detrend_key == "mine" and dev.filter_kernel_ms(1) > 0.0
    for a, b in zip(before, after):
        assert np.array_equal(a, b, equal_nan=True)
    # raw and the table's data are never written: the plain exposures and the injection give what they gave
    assert np.array_equal(dev.spectrum_expose(d["wav"], d["R"])[0], plain[0])
    ts.same(dev.spectrum_inject(d["wav"], d["R"], j, 1.3, n_comp=2, n_iter=4, highpass=True, injected=True), inj0,
            "raw unchanged")
    # scale = 0: the recovery against clean
    zero = dev.spectrum_recover(d["wav"], d["R"], 4, 0.0, **kw)
    same(zero, separate(dev, d, None, 0.0, 2, 4, False, 0, True), "scale = 0")
    # the trial alone, in position 0
    d1 = dict(d, F=np.ascontiguousarray(d["F"][:, j:j + 1]))
    upload(dev, d1, 0, True)
    alone = dev.spectrum_recover(d1["wav"], d1["R"], 0, 1.3, **kw)
    assert np.array_equal(alone[6], full[6])
    for k in range(6):
        assert np.array_equal(alone[k][:, 0], full[k][:, j], equal_nan=True), NAMES[k]
    assert full[1][:, j].any()


# ---- 2: refusals ----------------------------------------------------------------------------------------------------
def test_errors():
    from prometheus_amd import _native
    wav = ref.grid_nonuniform(100)
    R = ref.spectrum(wav, 2)
    lam, sig = wav[[10, 20, 30, 40]], np.full(4, 2e-10)
    rng = np.random.default_rng(6)
    data, ivar = 0.9 + 0.05 * rng.random((4, 4)), 1e4 * (0.1 + rng.random((4, 4)))
    raw = 1.0 + 0.1 * rng.random((4, 4))
    rows, a, _ = ts.table(4, 3, 2, n_orb=2)
    F = 1.0 + 1e-6 * np.arange(24.0).reshape(4, 3, 2)
    seg, perm, g = np.array([0, 1, 4]), np.array([2, 0, 3, 1]), np.array([1.0, 0.5])
    d = _native.Device(0)
    try:
        for call in (lambda: d.spectrum_recover(wav, R, 0, 1.0, 2), lambda: d.transit_recover(0, 1.0, 2)):
            with pytest.raises(_native.NativeError, match=E_STATE):      # no exposure table on the context
                call()
        d.observe_set(lam, sig, 5.0, 2)
        d.expose_set(rows, a, F, data, ivar)
        with pytest.raises(_native.NativeError, match=E_STATE):          # a table, but no raw exposures
            d.spectrum_recover(wav, R, 0, 1.0, 2)
        d.sysrem_set(raw, key="r")
        for kw in (dict(n_comp=0), dict(n_comp=-1, ones=True), dict(n_comp=17), dict(n_comp=16, ones=True),
                   dict(n_comp=2, n_iter=0)):
            with pytest.raises(_native.NativeError, match=E_ARG):        # ranges broken
                d.spectrum_recover(wav, R, 0, 1.0, **kw)
        for trial in (-1, 3):
            with pytest.raises(_native.NativeError, match=E_ARG):        # a trial outside [0, n_trial)
                d.spectrum_recover(wav, R, trial, 1.0, 2)
        for scale in (np.nan, np.inf, -np.inf):
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.spectrum_recover(wav, R, 0, scale, 2)
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_recover(wav, ref.spectrum(wav, 3), 0, 1.0, 2)     # another n_orb
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_recover(wav[::-1], R, 0, 1.0, 2)                  # descending grid
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.transit_recover(0, 1.0, 2)                                  # no run yet
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.spectrum_recover(wav, R, 0, 1.0, 2, highpass=True)         # highpass = 1 without a resident high-pass
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.spectrum_recover(wav, R, 0, 1.0, 2, orders=True)           # orders = 1 without resident orders
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.filter_kernel_ms()                                          # no build or recover call yet
        out = d.spectrum_recover(wav, R, 2, -0.5, 2, n_iter=3, ones=True)
        assert out[0].shape == (4, 3, 7) and out[1].shape == (4, 3) and out[6].shape == (4, 3) and out[2] is None
        assert d.filter_kernel_ms(2) > 0.0
        d.highpass_set(seg, perm, g, 1)
        d.orders_set(seg, perm, np.array([1, 1], dtype=np.uint8))
        out = d.spectrum_recover(wav, R, 2, 0.5, 1, highpass=True, orders=True)
        assert out[2].shape == (4, 3, 2, 7) and out[3].shape == (4, 3, 2) and out[4].shape == (4, 3, 4)
        d.spectrum_inject(wav, R, 0, 1.0, 3)                              # another U: nothing to repeat
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.filter_kernel_ms()
        d.expose_set(rows, a, F, data, ivar)                              # drops the raw exposures
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.spectrum_recover(wav, R, 0, 1.0, 2)
        d.observe_set(lam[:0], sig[:0], 5.0, 2)                           # no pixel: zeros, and the inject call's U
        d.expose_set(rows, a, F, data[:, :0], ivar[:, :0])
        d.sysrem_set(raw[:, :0])
        d.orders_set(np.array([0, 0]), np.zeros(0, dtype=np.int32), np.array([1], dtype=np.uint8))
        out = d.spectrum_recover(wav, R, 0, 1.0, 2, ones=True, orders=True)
        assert not out[0].any() and not out[1].any() and not out[2].any() and not out[3].any() and not out[4].any()
        assert np.all(out[6][:, 0] == 1) and np.all(out[6][:, 1:] == 0)
    finally:
        d.close()


# ---- 3: the Python path and the planted planet ----------------------------------------------------------------------
def test_transit_recover_is_the_spectrum_entry(planet):
    """Transit.recover equals prom_spectrum_recover on the run's R, and with broaden= on tr.broadened(bk), the model in
    the caller's pixel order."""
    from prometheus_amd import _native
    from prometheus_amd import observation as obs
    tr, d, ex, inj, hp = planet
    od = obs.Orders(ex, d["orders"])
    dev = _native.get_device(0)
    bk = obs.Broadening(*obs.rotation_kernel(3e5, n=33))
    vms = []
    for broaden in (None, bk):
        vm = tr.recover(inj, 2, 0.5, n_comp=2, n_iter=4, highpass=hp, broaden=broaden, orders=od, return_model=True,
                        devices=[0])
        assert dev.expose_key == ex.key and dev.highpass_key == hp.key and dev.sysrem_key == inj.key
        assert dev.orders_key == od.key
        R = np.array(tr.sumOverChords(devices=[0])) if broaden is None else tr.broadened(bk, devices=[0])
        want = dev.spectrum_recover(np.asarray(tr.wavelength), R, 2, 0.5, 2, n_iter=4, highpass=True, orders=True,
                                    model=True)
        got = (vm.moments, vm.n_used, vm.by_order.moments, vm.by_order.n_used,
               np.stack([vm.order_totals.loglike, vm.order_totals.chi2, vm.order_totals.chi2_scaled], axis=-1),
               d["ins"].sort(vm.model), vm.U)
        same(got, want[:4] + (want[4][..., :3], want[5], want[6]), "Transit.recover")
        assert vm.n_used.any()
        vms.append(vm)
    assert not np.array_equal(vms[0].moments, vms[1].moments)             # (the broadening is seen)
    lean = tr.recover(inj, 2, 0.5, n_comp=2, n_iter=4, highpass=hp, devices=[0])
    assert lean.model is None and not hasattr(lean, "by_order") and np.array_equal(lean.moments, vms[0].moments)


def test_planted_planet_is_recovered_in_one_call(planet):
    """12 exposures, 400 pixels in two orders, 9 trials, the planet injected at trial 6: the summed log-likelihood of
    Transit.recover peaks there, at the trial the host route (Transit.inject, Exposures, Detrend with
    observation.filter_weights' W, Transit.expose) peaks at."""
    from prometheus_amd import observation as obs
    tr, d, ex, inj, hp = planet
    kw = dict(n_comp=d["n_comp"], n_iter=d["n_iter"], ones=d["ones"], highpass=hp, devices=[0])
    vm = tr.recover(inj, sref.PLANET_TRIAL, 1.0, **kw)
    ll = vm.total("loglike")
    print("planted planet, one call: logL - max per trial", ll - ll.max())
    assert vm.U.shape == (12, 3) and int(np.argmax(ll)) == sref.PLANET_TRIAL
    res = tr.inject(inj, sref.PLANET_TRIAL, 1.0, **kw)
    ex2 = obs.Exposures(d["ins"], d["rows"], d["a"], d["F"], res.data, d["err"])
    host = tr.expose(ex2, devices=[0], highpass=obs.HighPass(ex2, d["taps"], orders=d["orders"], mode=d["mode"]),
                     detrend=obs.Detrend(ex2, res.U)).total("loglike")
    print("planted planet, host filter_weights: logL - max per trial", host - host.max())
    assert int(np.argmax(host)) == int(np.argmax(ll)) and np.array_equal(vm.U, res.U)
