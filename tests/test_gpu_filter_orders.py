"""The filter with a basis per echelle order on the device (include/prom_hip.h, "SYSREM per order on the device"):
prom_filter_weights_orders against prom_filter_weights given the pixel's own basis, bit for bit, for K in {1, 6, 14, 16};
prom_detrend_build_orders against prom_detrend_set_orders; the final model of the detrended, high-pass and per-order
calls against the existing calls run with (U_s, W), pixel by pixel; the moments against the existing moment reference
on the returned model; the states (prom_detrend_set puts the single basis back, prom_orders_set drops the filter) and
the refusals; the planted planet cleaned per order and recovered with the per-order Detrend."""
import numpy as np
import pytest

from helpers import detrend_ref as dref
from helpers import sysrem_ref as sref
import test_gpu_detrend as td
import test_gpu_sysrem as ts
from test_gpu_sysrem_orders import interleaved

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = "PROM_E_ARG", "PROM_E_STATE"
LENGTHS = [70, 64, 63]                           # three interleaved orders over 197 pixels: four tiles of 64, a tail


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


planet = ts.planet


def seg_of_orders(seg, perm):
    out = np.zeros(len(perm), dtype=np.int32)
    for s in range(len(seg) - 1):
        out[perm[seg[s]:seg[s + 1]]] = s
    return out


# ---- 1: the weights ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 6, 14, 16])
def test_weights_per_order_are_the_single_basis_weights_of_the_pixels_own_order(dev, K):
    n_exp, n_pix = 20, sum(LENGTHS)
    rng = np.random.default_rng(40 + K)
    seg, perm = interleaved(LENGTHS)
    seg_of = seg_of_orders(seg, perm)
    U = rng.normal(size=(3, n_exp, K))
    U[1, :, 0] = 1.0                                                      # a column of ones in one order
    ivar = 1e4 * (0.1 + rng.random((n_exp, n_pix)))
    ivar[rng.random(ivar.shape) < 0.05] = 0.0
    ivar[3, 5], ivar[4, 6], ivar[5, 7] = np.inf, np.nan, -1.0
    ivar[:, 11] = 0.0                                                     # a pixel without weight: W = +0
    ivar[K - 1:, 12] = 0.0                                                # fewer weighted exposures than components
    W = dev.filter_weights_orders(U, ivar, seg_of)
    assert W.shape == (K, n_exp, n_pix) and np.isfinite(W).all() and not np.signbit(W[W == 0]).any()
    for s in range(3):
        mine = seg_of == s
        Ws = dev.filter_weights(U[s], ivar)
        assert np.ascontiguousarray(W[:, :, mine]).tobytes() == np.ascontiguousarray(Ws[:, :, mine]).tobytes(), s
        assert np.any(W[:, :, mine] != 0)
        assert not np.array_equal(W[:, :, ~mine], Ws[:, :, ~mine])       # ... and of nobody else's
    assert np.all(W[:, :, 11] == 0)
    # one order: the single-basis call, byte for byte
    assert dev.filter_weights_orders(U[:1], ivar, np.zeros(n_pix, dtype=np.int32)).tobytes() == \
        dev.filter_weights(U[0], ivar).tobytes()


# ---- 2: the resident per-order filter ---------------------------------------------------------------------------------
def per_order_filter(n_exp, K, n_pix, seed):
    """Any finite U[3][n_exp][K] and W are a filter (test_gpu_detrend's random_filter, a basis per order)."""
    Us, W = zip(*[td.random_filter(n_exp, K, n_pix, seed=seed + s) for s in range(3)])
    return np.stack(Us), W[0]


def moments_by_the_reference(name, d, out):
    """The existing moment reference on the returned model, as test_gpu_detrend.check applies it."""
    mom, nu, model = out[0], out[1], out[-1]
    mld, nld, ald = dref.moments_ld(model, d["data"], d["ivar"])
    assert np.array_equal(nu, nld) and not np.isnan(mom).any(), name
    assert np.all(mom[nu == 0] == 0), name
    frac = dref.moment_fractions(mom, mld, nu, ald)
    print("FILTER_ORDERS_ERR %s %s of the bounds (m0 .. m6)" % (name, " ".join("%.4f" % f for f in frac)))
    assert np.all(frac <= 1.0), (name, frac)


@pytest.mark.parametrize("K", [2, 16])
def test_final_model_per_order_is_the_single_basis_model_pixel_by_pixel(dev, K):
    """In place (the detrended call) and behind the high-pass (the high-pass and the per-order-moments call with
    detrend = 1): at a pixel of order s the final model equals the existing call's with (U_s, W)."""
    n_exp, n_pix, n_trial = 5, sum(LENGTHS), 9
    d = td.design(n_exp, n_pix, n_trial)
    seg, perm = interleaved(LENGTHS)
    seg_of = seg_of_orders(seg, perm)
    U, W = per_order_filter(n_exp, K, n_pix, 50 + K)
    hp_seg, hp_perm, _ = ts.two_orders(n_pix)
    taps = np.exp(-0.5 * (np.arange(6) / 2.0) ** 2)

    def calls():
        return (dev.spectrum_expose_detrended(d["wav"], d["R"], model=True),
                dev.spectrum_expose_highpass(d["wav"], d["R"], detrend=True, model=True),
                dev.spectrum_expose_orders(d["wav"], d["R"], highpass=True, detrend=True, model=True))

    dev.observe_set(d["lam"], d["sig"], d["k"], d["R"].shape[0])
    dev.expose_set(d["rows"], d["a"], d["F"], d["data"], d["ivar"])
    dev.highpass_set(hp_seg, hp_perm, taps, 1)
    dev.orders_set(seg, perm)
    single = []
    for s in range(3):
        dev.detrend_set(U[s], W)
        single.append(calls())
    dev.detrend_set_orders(U, W)
    many = calls()
    names = ("detrended", "high-pass", "orders")
    for k, name in enumerate(names):
        model = many[k][-1]
        assert model.shape == (n_exp, n_trial, n_pix)
        for s in range(3):
            mine = seg_of == s
            want = single[s][k][-1]
            assert np.array_equal(np.isnan(model[:, :, mine]), np.isnan(want[:, :, mine])), (name, s)
            assert np.ascontiguousarray(model[:, :, mine]).tobytes() == np.ascontiguousarray(want[:, :, mine]).tobytes()
            assert not np.array_equal(model[:, :, ~mine], want[:, :, ~mine], equal_nan=True), (name, s)
        moments_by_the_reference("K=%d %s" % (K, name), d, many[k])
    # the per-order records of the orders call: order s's record is the single-basis call's with U_s
    for s in range(3):
        assert np.array_equal(many[2][2][:, :, s], single[s][2][2][:, :, s]), s
        assert np.array_equal(many[2][3][:, :, s], single[s][2][3][:, :, s]), s
    # two calls agree, and a prom_detrend_set afterwards restores the single-basis bits
    again = calls()
    for a, b in zip(again, many):
        assert td.same(a, b)
    dev.detrend_set(U[0], W)
    for a, b in zip(calls(), single[0]):
        assert td.same(a, b)


def test_build_per_order_is_set_per_order_with_the_devices_weights(dev):
    n_exp, n_pix, K = 20, sum(LENGTHS), 3
    d = td.design(n_exp, n_pix, 5)
    d["ivar"][np.random.default_rng(3).random(d["ivar"].shape) < 0.05] = 0.0
    seg, perm = interleaved(LENGTHS)
    seg_of = seg_of_orders(seg, perm)
    U = np.random.default_rng(9).normal(size=(3, n_exp, K))
    dev.observe_set(d["lam"], d["sig"], d["k"], d["R"].shape[0])
    dev.expose_set(d["rows"], d["a"], d["F"], d["data"], d["ivar"])
    dev.orders_set(seg, perm)
    W = dev.detrend_build_orders(U, weights=True)
    assert W.tobytes() == dev.filter_weights_orders(U, d["ivar"], seg_of).tobytes() and np.any(W != 0)
    built = dev.spectrum_expose_detrended(d["wav"], d["R"], model=True)
    assert dev.filter_kernel_ms(2) > 0.0                                  # repeats the per-order build
    assert td.same(dev.spectrum_expose_detrended(d["wav"], d["R"], model=True), built)
    dev.detrend_set_orders(U, W)
    assert td.same(dev.spectrum_expose_detrended(d["wav"], d["R"], model=True), built)
    assert dev.detrend_build_orders(U) is None                            # W stays on the device unless asked for
    assert td.same(dev.spectrum_expose_detrended(d["wav"], d["R"], model=True), built)
    moments_by_the_reference("build", d, built)


# ---- 3: the states and the refusals ---------------------------------------------------------------------------------
def test_state_and_refusals(dev):
    from prometheus_amd import _native
    n_exp, n_pix, K = 5, sum(LENGTHS), 2
    d = td.design(n_exp, n_pix, 3)
    seg, perm = interleaved(LENGTHS)
    U, W = per_order_filter(n_exp, K, n_pix, 7)
    dev.observe_set(d["lam"], d["sig"], d["k"], d["R"].shape[0])
    dev.expose_set(d["rows"], d["a"], d["F"], d["data"], d["ivar"])      # (a new table: no orders)
    for call in (lambda: dev.detrend_set_orders(U, W), lambda: dev.detrend_build_orders(U)):
        with pytest.raises(_native.NativeError, match=E_STATE):          # no resident orders
            call()
    dev.orders_set(seg, perm)
    for call in (lambda: dev.detrend_set_orders(U[:2], W), lambda: dev.detrend_build_orders(U[:2]),
                 lambda: dev.detrend_set_orders(U[:, :4], W[:, :4]),
                 lambda: dev.detrend_set_orders(np.where(U == U[0, 0, 0], np.nan, U), W)):
        with pytest.raises(_native.NativeError, match=E_ARG):            # another n_seg or n_exp, a NaN in U
            call()
    with pytest.raises(_native.NativeError, match=E_STATE):              # a failed set leaves no filter behind
        dev.spectrum_expose_detrended(d["wav"], d["R"])
    dev.detrend_set_orders(U, W, key="f")
    assert dev.detrend_key == "f"
    out = dev.spectrum_expose_detrended(d["wav"], d["R"], model=True)
    dev.orders_set(seg, perm)                                             # new orders drop a per-order filter ...
    assert dev.detrend_key is None
    with pytest.raises(_native.NativeError, match=E_STATE):
        dev.spectrum_expose_detrended(d["wav"], d["R"])
    dev.detrend_set(U[0], W, key="g")
    dev.orders_set(seg, perm)                                             # ... and leave a single basis alone
    assert dev.detrend_key == "g"
    assert dev.spectrum_expose_detrended(d["wav"], d["R"])[0].shape == out[0].shape
    ivar = d["ivar"]
    bad = np.zeros(n_pix, dtype=np.int32)
    for v in (-1, 3):
        bad[5] = v
        with pytest.raises(_native.NativeError, match=E_ARG):            # seg_of outside [0, n_seg)
            dev.filter_weights_orders(U, ivar, bad)
    with pytest.raises(ValueError):
        dev.filter_weights_orders(U, ivar, bad[:-1])


# ---- 4: the planted planet, cleaned and recovered per order ---------------------------------------------------------
def test_planted_planet_cleaned_and_recovered_per_order(planet):
    """Trial 6 injected at scale 1, cleaned per order on the device (two interleaved orders), recovered with the
    per-order Detrend of the returned bases: the summed log-likelihood peaks at trial 6, as in the all-numpy per-order
    pipeline (tests/test_sysrem_orders_cpu.py)."""
    from prometheus_amd import observation as obs
    tr, d, ex, inj, hp = planet
    od = obs.Orders(ex, d["orders"])
    res = tr.inject(inj, sref.PLANET_TRIAL, 1.0, n_comp=d["n_comp"], n_iter=d["n_iter"], ones=d["ones"], highpass=hp,
                    sysrem_orders=od, devices=[0])
    assert res.U.shape == (2, 12, 3) and res.data.shape == (12, 400)
    ex2 = obs.Exposures(d["ins"], d["rows"], d["a"], d["F"], res.data, d["err"])
    od2 = obs.Orders(ex2, d["orders"])
    hp2 = obs.HighPass(ex2, d["taps"], orders=d["orders"], mode=d["mode"])
    lls = []
    for on_device in (True, False):
        dt = obs.Detrend(ex2, res.U, orders=od2, on_device=on_device)
        vm = tr.expose(ex2, devices=[0], highpass=hp2, detrend=dt)
        ll = vm.loglike.sum(axis=0)
        print("planted planet per order, device (W on device: %s): logL - max per trial" % on_device, ll - ll.max())
        assert int(np.argmax(ll)) == sref.PLANET_TRIAL
        lls.append(ll)
    assert np.allclose(lls[0], lls[1], rtol=1e-6)
    # with the orders of the moments too: the totals over the orders peak there as well
    vm = tr.expose(ex2, devices=[0], highpass=hp2, detrend=obs.Detrend(ex2, res.U, orders=od2), orders=od2)
    assert int(np.argmax(vm.order_totals.loglike.sum(axis=0))) == sref.PLANET_TRIAL
    other = obs.Orders(ex2, np.arange(400) // 200)
    with pytest.raises(ValueError, match="alike"):
        tr.expose(ex2, devices=[0], detrend=obs.Detrend(ex2, res.U, orders=od2), orders=other)
