"""The filter's weights on the device (include/prom_hip.h, "the filter's weights on the device") against the numpy
restatement of the definition (tests/helpers/filter_ref.py), bit for bit and signs of zero included, over the shapes
the host harness walks: n_pix in {1, 63, 64, 65, 130} (one lane, a wave's edge, the tail of the last wave, two
waves), n_exp in {1, 2, 7, 70}, K in {1, 2, 6, 11, 16} (K = 15 and 16 keep part of the triangle in LDS, so 14 and 15
are run too); independence; the accuracy against a longdouble evaluation with observation.filter_weights' own
distance as the yardstick; prom_detrend_build against prom_detrend_set; and the refusals."""
import numpy as np
import pytest

from helpers import filter_ref as fref
from helpers import observe_ref as ref
import test_filter_cpu as tc
import test_gpu_sysrem as ts

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = "PROM_E_ARG", "PROM_E_STATE"


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


def same_bits(got, want, name):
    assert got.shape == want.shape, name
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), (name, float(np.abs(got - want).max()))


# ---- 1: bit for bit over the shapes -------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 6, 11, 14, 15, 16])
def test_weights_bitwise_over_the_shapes(dev, K):
    """prom_filter_weights = weights_f64 for every n_pix and n_exp of the harness; the arrays hold a pixel without
    weight, one with exactly K and one with K - 1 weighted exposures, and NaN, +inf, negative and -0 ivar entries."""
    for n_exp in (1, 2, 7, 70):
        for n_pix in (1, 63, 64, 65, 130):
            U, iv = tc.edge_case(n_exp, K, n_pix)
            want = fref.weights_f64(U, iv)
            same_bits(dev.filter_weights(U, iv), want, "n_exp=%d K=%d n_pix=%d" % (n_exp, K, n_pix))
            if n_exp == 70 and n_pix > 7:
                p = want.any(axis=(0, 1))
                assert p[1] and not p[0] and not p[2] and p[3:].all()
                assert not want[:, n_exp // 2, 3:7].any()              # NaN, +inf, negative and -0 carry no weight
            if n_exp < K:
                assert not want.any()


def test_zero_and_duplicated_columns_and_overflow(dev):
    """A zero column of U makes every pixel singular: W is +0 throughout.  With a duplicated column only the bits
    against weights_f64 are asserted, whichever way the pivot test falls.  A basis whose products overflow gives +0."""
    for name, U, iv in tc._column_cases()[6:]:
        want = fref.weights_f64(U, iv)
        got = dev.filter_weights(U, iv)
        same_bits(got, want, name)
        if name in ("zero_column", "overflow"):
            assert not got.any() and not np.signbit(got).any()


# ---- 2: independence ------------------------------------------------------------------------------------------------
def test_a_pixel_depends_on_its_own_column_alone(dev):
    U, iv = tc.edge_case(7, 6, 130)
    W = dev.filter_weights(U, iv)
    same_bits(dev.filter_weights(U, iv), W, "two calls")
    for p in (0, 1, 63, 64, 129):
        same_bits(dev.filter_weights(U, iv[:, p:p + 1]), W[:, :, p:p + 1], "pixel %d alone" % p)
    perm = np.random.default_rng(2).permutation(130)
    same_bits(dev.filter_weights(U, np.ascontiguousarray(iv[:, perm])), np.ascontiguousarray(W[:, :, perm]), "permuted")


# ---- 3: accuracy ----------------------------------------------------------------------------------------------------
def test_weights_within_four_times_the_host_functions_own_distance(dev):
    """d(x) = max over the regular pixels of |W_x - W_longdouble| / max|W_p|; d(device) <= 4 d(observation.filter_weights)
    on the four prototype designs (seed 5), and the device zeroes the pixels the host function zeroes.  The fractions
    are printed (profiles/filter_weights_errors.txt keeps them)."""
    from prometheus_amd import observation as obs
    u = 2.0 ** -53
    for (n_exp, K, n_pix), (U, iv) in zip(fref.DESIGNS, fref.designs(seed=5)):
        W = dev.filter_weights(U, iv)
        Wh = obs.filter_weights(U, iv)
        Wl = fref.weights_ld(U, iv)
        reg = Wh.any(axis=(0, 1))
        assert np.array_equal(W.any(axis=(0, 1)), reg) and reg.any() and not reg.all()
        scale = np.abs(Wl).max(axis=(0, 1))[reg].astype(np.float64)
        d_dev, d_host = (float((np.abs(X - Wl).max(axis=(0, 1))[reg].astype(np.float64) / scale).max()) for X in (W, Wh))
        print("FILTER_ERR n_exp=%d K=%d n_pix=%d: device %.1f u, observation.filter_weights %.1f u, fraction of the "
              "bound %.4f" % (n_exp, K, n_pix, d_dev / u, d_host / u, d_dev / (4.0 * d_host)))
        assert d_dev <= 4.0 * d_host


# ---- 4: prom_detrend_build = prom_detrend_set with the returned W ---------------------------------------------------
def test_detrend_build_is_detrend_set_with_the_returned_weights(dev):
    """7 exposures x 130 pixels x 5 trials at K = 3: the W that comes back is prom_filter_weights' over the table's
    ivar, and the detrended moments, n_used and model are bit for bit those after prom_detrend_set(U, W)."""
    d = ts.design(7, 130, n_trial=5, seed=21)
    U = np.random.default_rng(4).normal(size=(7, 3))
    ts.upload(dev, d)
    W = dev.detrend_build(U, key="built", weights=True)
    assert dev.detrend_key == "built" and W.any()
    same_bits(W, fref.weights_f64(U, d["ivar"]), "W_out")
    got = dev.spectrum_expose_detrended(d["wav"], d["R"], model=True)
    assert dev.filter_kernel_ms(2) > 0.0
    again = dev.spectrum_expose_detrended(d["wav"], d["R"], model=True)
    assert dev.detrend_build(U) is None                                     # W_out may be NULL
    third = dev.spectrum_expose_detrended(d["wav"], d["R"], model=True)
    dev.detrend_set(U, W)
    want = dev.spectrum_expose_detrended(d["wav"], d["R"], model=True)
    for g in (got, again, third):
        for a, b, what in zip(g, want, ("moments", "n_used", "model")):
            assert np.array_equal(a, b, equal_nan=True), what
    assert want[1].any() and np.isfinite(want[0]).all()


planet = ts.planet   # (the module's fixture: reduced C1 and the planted-planet design)


def test_detrend_on_device_through_transit_expose(planet):
    """Detrend(on_device=True) through Transit.expose on reduced C1 gives what Detrend with Transit.filter_weights' W
    gives, bit for bit; no W is kept on the host and the key does not depend on one."""
    from prometheus_amd import observation as obs
    tr, d, ex, _, _ = planet
    U = np.random.default_rng(8).normal(size=(ex.n_exp, 3))
    dt = obs.Detrend(ex, U, on_device=True)
    assert dt.W is None and dt.on_device and dt.key == obs.Detrend(ex, U.copy(), on_device=True).key
    W = tr.filter_weights(ex, U, devices=[0])
    same_bits(d["ins"].sort(W), fref.weights_f64(U, ex.ivar), "Transit.filter_weights")
    got = tr.expose(ex, return_model=True, devices=[0], detrend=dt)
    want = tr.expose(ex, return_model=True, devices=[0], detrend=obs.Detrend(ex, U, W))
    assert np.array_equal(got.moments, want.moments) and np.array_equal(got.n_used, want.n_used)
    assert np.array_equal(got.model, want.model, equal_nan=True) and want.n_used.any()


# ---- 5: refusals ----------------------------------------------------------------------------------------------------
def test_errors_of_filter_weights_and_detrend_build():
    from prometheus_amd import _native
    rng = np.random.default_rng(6)
    U, iv = rng.normal(size=(4, 2)), 1.0 + rng.random((4, 5))
    d = _native.Device(0)
    try:
        assert d.filter_weights(U, iv).any()                              # no table is needed
        assert d.filter_weights(U, iv[:, :0]).shape == (2, 4, 0)          # n_pix = 0 writes nothing
        for bad in (np.ones((4, 0)), np.ones((4, 17)), np.ones((0, 2)), np.where(U == U[1, 1], np.nan, U),
                    np.where(U == U[2, 0], np.inf, U)):
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.filter_weights(bad, np.ones((bad.shape[0], 5)))
        for call in (lambda: d.detrend_build(U), d.filter_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):      # no exposure table on the context
                call()
        wav = ref.grid_nonuniform(100)
        lam, sig = wav[[10, 20, 30, 40, 50]], np.full(5, 2e-10)
        rows, a, _ = ts.table(4, 3, 2, n_orb=2)
        F = 1.0 + 1e-6 * np.arange(24.0).reshape(4, 3, 2)
        d.observe_set(lam, sig, 5.0, 2)
        d.expose_set(rows, a, F, np.ones((4, 5)), 1e4 * iv)
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.filter_kernel_ms()                                          # no build yet
        for bad in (U[:3], np.ones((4, 17)), np.ones((4, 0)), np.where(U == U[0, 0], np.nan, U)):
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.detrend_build(bad, key="x")
            assert d.detrend_key is None
            with pytest.raises(_native.NativeError, match=E_STATE):      # a failed build leaves no filter behind
                d.spectrum_expose_detrended(wav, ref.spectrum(wav, 2))
        d.detrend_build(U, key="b")
        assert d.detrend_key == "b" and d.filter_kernel_ms(2) > 0.0
        assert d.spectrum_expose_detrended(wav, ref.spectrum(wav, 2))[1].any()
        d.detrend_set(U, np.zeros((2, 4, 5)))
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.filter_kernel_ms()                                          # the built filter was replaced
        d.detrend_build(U, key="b")
        d.expose_set(rows, a, F, np.ones((4, 5)), 1e4 * iv)              # dropping the table drops the built filter
        assert d.detrend_key is None
        for call in (lambda: d.spectrum_expose_detrended(wav, ref.spectrum(wav, 2)), d.filter_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):
                call()
    finally:
        d.close()
