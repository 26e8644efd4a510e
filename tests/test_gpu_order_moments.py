"""Per-order moments on the device (prom_orders_set / prom_spectrum_expose_orders / prom_transit_expose_orders,
Transit.expose(orders=...)) against the references of tests/helpers/order_ref.py.  Marked ``gpu``.

The records of every (exposure, trial, order) must be order_moments_f64 of the call's own model_out bit for bit and
n_used exact, for the four filter combinations; the lumped outputs must be the existing entries' bit for bit; the
totals' chi2, chi2_scaled and count must be totals_f64 of the device's own records bit for bit and loglike within the
helper's derived bound (the device logarithm's ulp bound, from the definition and not from the kernel).  The
independence clause is tested bitwise.  The totals' test prints the largest fraction of the bound it reached
(``ORDER_ERR``; profiles/order_moments_errors.txt).
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import highpass_ref as href
from helpers import observe_ref as ref
from helpers import order_ref as oref
from test_gpu_highpass import design, gauss, same, table, upload

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
E_ARG, E_STATE = "PROM_E_ARG", "PROM_E_STATE"
U = 2.0 ** -53
# one tile less one, one tile, one tile and one, two tiles; k_model_moments' chunk (512) less one, the chunk, the chunk
# and one, two chunks and a bit; 1 and 2 for the orders that cannot or can just enter the totals.  All ten lengths in
# one design make 2,799 pixels
LENGTHS = (1, 2, 31, 32, 33, 64, 511, 512, 513, 1100)
N_PIX = sum(LENGTHS)
FILTERS = {"none": (False, False), "highpass": (True, False), "sysrem": (False, True), "both": (True, True)}


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


def _design(n_trial=17):
    """design() with the orders of LENGTHS dealt over the device's pixel order at random, every second one reversed;
    the length-1 order's ivar is 0 in exposure 0; a high-pass over other segments than the orders and a filter."""
    d = design(3, N_PIX, n_trial, seed=5)
    seg, perm = href.interleaved(LENGTHS, seed=4)
    d["ivar"][0, perm[0]] = 0.0
    keep = np.ones(len(LENGTHS), dtype=np.uint8)
    keep[5] = 0
    rng = np.random.default_rng(31)
    Ub, W = rng.normal(size=(3, 3)), rng.normal(size=(3, 3, N_PIX)) / 3
    W[:, 0, ::7] = 0.0
    hp_seg, hp_perm = href.interleaved((1200, N_PIX - 1200), seed=9)
    return dict(d, seg=seg, perm=perm, keep=keep, filt=(Ub, W), hp=(hp_seg, hp_perm, gauss(40, 12.0), 1))


def setup(dev, d, keep=None):
    upload(dev, d)
    dev.highpass_set(*d["hp"])
    dev.detrend_set(*d["filt"])
    dev.orders_set(d["seg"], d["perm"], d["keep"] if keep is None else keep)


def run(dev, d, which, **kw):
    hp, dt = FILTERS[which]
    kw.setdefault("model", True)
    return dev.spectrum_expose_orders(d["wav"], d["R"], highpass=hp, detrend=dt, **kw)


def check_records(name, d, out):
    """The records against order_moments_f64 of the call's own final model (a column that is not filterable is NaN down
    all exposures, so the flags say nothing the model does not)."""
    mom, nu, rmom, rnu, tot, model = out
    want_mom, want_nu = oref.order_moments_f64(model, d["data"], d["ivar"], None, d["seg"], d["perm"])
    assert rnu.dtype == np.int64 and rmom.shape == want_mom.shape, name
    assert np.array_equal(rnu, want_nu), name
    assert np.array_equal(rmom, want_mom), name
    assert not np.isnan(rmom).any(), name
    return want_mom, want_nu


@pytest.fixture(scope="module")
def base(dev):
    d = _design()
    setup(dev, d)
    return d, {which: run(dev, d, which) for which in FILTERS}


# ---- 1: the records bitwise ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(FILTERS))
def test_records_bitwise_for_the_four_filter_combinations(base, which):
    d, outs = base
    out = outs[which]
    want_mom, want_nu = check_records(which, d, out)
    assert np.isnan(out[5]).any() and np.isfinite(out[5]).any()
    assert (want_nu[0, :, 0] == 0).all() and (want_nu > 0).any()
    assert (want_nu[..., 9] > 512).all()                        # (the long order does hold many used pixels)
    for other in FILTERS:
        if other != which:
            assert not np.array_equal(outs[other][2], out[2]), (which, other)


@pytest.mark.parametrize("n_trial", [1, 5, 9])
def test_records_bitwise_over_trial_counts(dev, n_trial):
    d = _design(n_trial)
    setup(dev, d)
    out = run(dev, d, "both")
    check_records("%d trials" % n_trial, d, out)
    assert out[2].shape == (3, n_trial, len(LENGTHS), 7)


def test_nan_in_R_changes_only_the_orders_that_hold_an_affected_pixel(dev, base):
    d, outs = base
    Rn = d["R"].copy()
    Rn[:, 700] = np.nan
    dn = dict(d, R=Rn)
    setup(dev, dn)
    # the high-pass would carry the NaN's effect along ITS segments, which are not the orders: without it
    for which in ("none", "sysrem"):
        out = run(dev, dn, which)
        check_records("NaN in R, " + which, dn, out)
        clean = outs[which]
        hit = np.isnan(out[5]) & ~np.isnan(clean[5])
        assert hit.any()
        # (with the filter a column with a NaN is NaN down the exposures whose W is not 0: `hit` holds those too)
        in_order = np.stack([hit[..., d["perm"][d["seg"][s]:d["seg"][s + 1]]].any(axis=-1)
                             for s in range(len(LENGTHS))], axis=-1)
        assert in_order.any() and (~in_order).any()
        assert np.array_equal(out[2][~in_order], clean[2][~in_order])
        assert np.array_equal(out[3][~in_order], clean[3][~in_order])
        assert np.all(out[3][in_order] <= clean[3][in_order]) and np.any(out[3][in_order] < clean[3][in_order])
    setup(dev, d)


# ---- 2: one order is the lumped record ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pix", [1, 33, 512, 513, 1100])
def test_one_order_with_the_identity_perm_against_the_lumped_output(dev, n_pix):
    """Up to 512 pixels k_model_moments has one chunk, so its sum is the order's tile sum: bit for bit.  Beyond, the
    lumped sum adds chunks: the two differ by rounding, within (n + 4) u sum |term|."""
    d = design(3, n_pix, 5, outside=n_pix >= 512, seed=6)
    seg, perm = href.one_segment(n_pix)
    upload(dev, d)
    dev.orders_set(seg, perm)
    mom, nu, rmom, rnu, tot, model = dev.spectrum_expose_orders(d["wav"], d["R"], model=True)
    assert np.array_equal(rnu[:, :, 0], nu) and nu.max() > 0
    if n_pix <= 512:
        assert np.array_equal(rmom[:, :, 0], mom)
    else:
        _, _, mag = oref.order_moments_ld(model, d["data"], d["ivar"], None, seg, perm)
        bound = (n_pix + 4) * U * mag[:, :, 0].astype(np.float64)
        assert np.all(np.abs(rmom[:, :, 0] - mom) <= bound)


# ---- 3: the orders partition the exposure --------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(FILTERS))
def test_orders_partition_the_lumped_moments(base, which):
    d, outs = base
    mom, nu, rmom, rnu, tot, model = outs[which]
    assert np.array_equal(rnu.sum(axis=2), nu)
    _, _, mag = oref.order_moments_ld(model, d["data"], d["ivar"], None, d["seg"], d["perm"])
    bound = (N_PIX + 4) * U * mag.sum(axis=2)
    diff = np.abs(rmom.astype(np.longdouble).sum(axis=2) - mom)
    assert np.all(diff <= bound)


# ---- 4: the lumped outputs are the existing entries' ----------------------------------------------------------------------
def test_lumped_outputs_equal_the_existing_entries_bitwise(dev, base):
    """R holds no NaN here, so the unfiltered case is covered by k_model_moments' promise too: a pixel without a model
    (beyond the grid's ends) is unused on both sides."""
    d, outs = base
    setup(dev, d)                                              # (other tests have set other tables since)
    old = {"none": dev.spectrum_expose(d["wav"], d["R"], model=True),
           "sysrem": dev.spectrum_expose_detrended(d["wav"], d["R"], model=True),
           "highpass": dev.spectrum_expose_highpass(d["wav"], d["R"], detrend=False, model=True),
           "both": dev.spectrum_expose_highpass(d["wav"], d["R"], detrend=True, model=True)}
    for which, out in outs.items():
        assert same((out[0], out[1], out[5]), old[which]), which
        assert np.isnan(out[5]).any()
    # only what is asked for comes back
    mom, nu, rmom, rnu, tot, model = run(dev, d, "both", moments=False, records=False, model=False)
    assert mom is None and nu is None and rmom is None and rnu is None and model is None
    assert np.array_equal(tot, outs["both"][4], equal_nan=True)
    out = run(dev, d, "both", totals=False, model=False)
    assert out[4] is None and same(out[:4], outs["both"][:4])
    ms = dev.orders_kernel_ms(2)
    assert ms[0] > 0.0 and ms[1] > 0.0


# ---- 5: independence ---------------------------------------------------------------------------------------------------
def test_independence_bitwise(dev, base):
    d, outs = base
    ref_out = outs["both"]
    setup(dev, d)
    assert same(run(dev, d, "both"), ref_out)                                  # a second call
    other_keep = 1 - d["keep"]
    setup(dev, d, keep=other_keep)
    out = run(dev, d, "both")
    assert same(out[:4], ref_out[:4]) and not np.array_equal(out[4], ref_out[4], equal_nan=True)
    for j in (0, 7, 8, 16):                                                  # a trial alone
        dj = dict(d, F=np.ascontiguousarray(d["F"][:, j:j + 1]))
        setup(dev, dj)
        assert same(run(dev, dj, "both"), tuple(x[:, j:j + 1] for x in ref_out)), j
    pj = np.random.default_rng(12).permutation(d["F"].shape[1])                # permuted trials
    dp = dict(d, F=np.ascontiguousarray(d["F"][:, pj]))
    setup(dev, dp)
    assert same(run(dev, dp, "both"), tuple(x[:, pj] for x in ref_out))
    setup(dev, d)


_BATCHED = """
import hashlib, json, sys
sys.path.insert(0, %r)
import numpy as np
from prometheus_amd import _native
from test_gpu_order_moments import _design, setup, run
d = _design()
dev = _native.get_device(0)
setup(dev, d)
out = run(dev, d, "both")
print(json.dumps([hashlib.sha256(x.tobytes()).hexdigest() for x in out]))
"""


def test_batches_under_a_small_scratch_cap_bitwise(base):
    """PROM_VMAP_SCRATCH_MB is read at context creation, so the case runs in a process of its own: 0.0001 MB is below
    one trial group's records (3 x 8 x 10 x 64 bytes), so every group of the 17 trials is a batch of its own."""
    ref_out = base[1]["both"]
    env = dict(os.environ, PROM_VMAP_SCRATCH_MB="0.0001", PROM_DEBUG="1")
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _BATCHED % os.path.join(REPO, "tests")],
                       env=env, cwd=REPO, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = [l for l in p.stderr.splitlines() if "per-order moments:" in l]
    assert lines and "3 groups, 3 batches of up to 1 groups" in lines[-1], p.stderr[-2000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("[")][-1])
    assert out == [hashlib.sha256(x.tobytes()).hexdigest() for x in ref_out]


# ---- 6: the totals -------------------------------------------------------------------------------------------------------
def check_totals(name, keep, out):
    """chi2, chi2_scaled and the count bitwise, loglike within the helper's bound of totals_f64 of the device's own
    records; where the reference is not finite the device must say the same.  Returns the fraction of the bound."""
    rmom, rnu, tot = out[2], out[3], out[4]
    want = oref.totals_f64(rmom, rnu, keep)
    assert np.array_equal(tot[..., 1:], want[..., 1:], equal_nan=True), name
    fin = np.isfinite(want[..., 0])
    assert np.array_equal(tot[..., 0][~fin], want[..., 0][~fin], equal_nan=True), name
    bound = oref.loglike_bound(rmom, rnu, keep)
    diff = np.abs(tot[..., 0][fin] - want[..., 0][fin])
    b = bound[fin]
    frac = float(np.max(np.where(b > 0, diff / np.where(b > 0, b, 1), np.where(diff == 0, 0.0, np.inf)))) if fin.any() else 0.0
    print("ORDER_ERR %s: loglike total reaches %.4f of its bound; chi2, chi2_scaled and the count are bitwise" %
          (name, frac))
    assert frac <= 1.0, (name, frac)
    return want, frac


@pytest.mark.parametrize("which", sorted(FILTERS))
def test_totals_against_the_reference_of_the_devices_own_records(base, which):
    d, outs = base
    out = outs[which]
    want, _ = check_totals(which, d["keep"], out)
    en = oref.enters(out[3], d["keep"])
    assert not en[..., 0].any() and not en[..., 5].any() and en[..., 9].all()    # length 1 never, keep = 0 never
    assert np.isfinite(out[4]).all() and np.all(out[4][..., 0] != 0)
    assert np.array_equal(out[4][..., 3], np.where(en, out[3], 0).sum(axis=2))
    # the order that is not kept and the orders with n_used < 2 do not enter: dropping their records changes nothing
    gone = out[2].copy()
    gone[~en] = np.nan
    assert np.array_equal(oref.totals_f64(gone, out[3], d["keep"]), want)


def test_totals_keep_nothing_and_a_nan_statistic(dev, base):
    d, outs = base
    setup(dev, d, keep=np.zeros(len(LENGTHS), dtype=np.uint8))
    assert np.all(run(dev, d, "both")[4] == 0)                                    # no entering order: zeros
    # two huge weights in the 33-pixel order of exposure 1: m2 m2 overflows, s_f^2 and C are -inf and loglike is NaN;
    # m4 m4 overflows and chi2_scaled is -inf.  Nothing is hidden, and exposure 0 stays finite
    dn = dict(d, ivar=d["ivar"].copy())
    px = d["perm"][d["seg"][4]:d["seg"][5]]
    dn["ivar"][1, px[(px > 300) & (px < 2000)][:2]] = 1e300         # (two pixels well inside the grid)
    setup(dev, dn)
    out = run(dev, dn, "none")
    check_records("huge weights", dn, out)
    check_totals("huge weights", d["keep"], out)
    assert oref.enters(out[3], d["keep"])[1, :, 4].all()
    assert np.isnan(out[4][1, :, 0]).all() and np.all(out[4][1, :, 2] == -np.inf)
    assert np.isfinite(out[4][0]).all() and np.isfinite(out[4][1, :, 1]).all()
    setup(dev, d)


# ---- 7: a planted signal ---------------------------------------------------------------------------------------------------
def planted(model_of):
    """Two orders of 150 pixels; the data are a_s M of trial column 4 plus seeded noise, a_s = 0.5 and 2, the noise
    levels a factor 3 apart.  ``model_of(d)`` gives the exposures' model [n_exp][n_trial][n_pix].

    The seeds were picked with the float64 references on the CPU (the exposures' longdouble model, order_moments_f64,
    totals_f64).  chi2_scaled fits a scale per order and found the column for every seed tried.  The likelihood does not
    fit a scale: with a_s far from 1 its argument is sg^2 (1 + a_s^2 - 2 a_s rho) + noise, which also falls with the
    model's own variance sg^2 over the order, and for about a quarter of the designs tried a neighbouring column won by
    5 to 8 in ln L.  With these seeds the reference's ln L at the planted column leads the runner-up by 27.5."""
    d = design(3, 300, 9, outside=False, seed=21)
    seg, perm = href.interleaved((150, 150), seed=3)
    M = np.asarray(model_of(d), dtype=np.float64)
    rng = np.random.default_rng(8)
    data, ivar = np.empty((3, 300)), np.empty((3, 300))
    for s, (a_s, sigma) in enumerate(((0.5, 2e-3), (2.0, 6e-3))):
        px = perm[seg[s]:seg[s + 1]]
        data[:, px] = a_s * M[:, 4, px] + sigma * rng.normal(size=(3, 150))
        ivar[:, px] = 1.0 / sigma ** 2
    return dict(d, data=data, ivar=ivar, seg=seg, perm=perm)


def test_planted_signal_is_found_per_order(dev):
    from prometheus_amd import observation as obs

    def model_of(d):
        upload(dev, d)
        return dev.spectrum_expose(d["wav"], d["R"], model=True)[2]
    d = planted(model_of)
    upload(dev, d)
    dev.orders_set(d["seg"], d["perm"])
    mom, nu, rmom, rnu, tot, _ = dev.spectrum_expose_orders(d["wav"], d["R"])
    assert np.all(rnu == 150)
    om = obs.OrderMap(rmom, rnu, [0, 1], [True, True])
    scaled = om.total("chi2_scaled")
    ll = obs.OrderTotals(tot).loglike.sum(axis=0)
    print("planted: chi2_scaled", scaled, "loglike", ll)
    assert int(np.argmin(scaled)) == 4 and int(np.argmax(ll)) == 4
    # the per-order scales are the planted ones, which one scale over both orders cannot be
    assert np.allclose(om.scale[:, 4, 0], 0.5, rtol=0.02) and np.allclose(om.scale[:, 4, 1], 2.0, rtol=0.02)


# ---- 8: state and argument errors ------------------------------------------------------------------------------------------
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
        for call in (lambda: d.orders_set(seg, perm), lambda: d.spectrum_expose_orders(wav, R),
                     d.transit_expose_orders, d.orders_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):      # no exposure table on the context
                call()
        d.observe_set(lam, sig, 5.0, 2)
        d.expose_set(rows, a, F, data, ivar)
        for call in (lambda: d.spectrum_expose_orders(wav, R), d.transit_expose_orders, d.orders_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):      # a table, but no orders
                call()
        bad_sets = [
            (seg, perm[:3]),                                              # n_pix other than the observation's
            ([0, 1, 3], [2, 0, 1]),
            ([1, 2, 4], perm),                                            # seg_first does not start at 0
            ([0, 1, 3], perm),                                            # ... or end at n_pix
            ([0, 2, 2, 4], perm),                                         # an empty order
            ([0, 3, 2, 4], perm),                                         # descending
            (seg, [2, 0, 3, 3]),                                          # a repeated perm entry
            (seg, [2, 0, 4, 1]),                                          # out of range
            (seg, [2, 0, -1, 1]),
            (seg, perm, [1, 2]),                                          # keep is 0 or 1
        ]
        for args in bad_sets:
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.orders_set(*args)
        with pytest.raises(_native.NativeError, match=E_STATE):          # a failed set leaves no orders behind
            d.spectrum_expose_orders(wav, R)
        d.orders_set(seg, perm, [1, 0], key="o")
        assert d.orders_key == "o"
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.transit_expose_orders()                                     # no run yet
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.spectrum_expose_orders(wav, R, highpass=True)               # highpass = 1 without a high-pass
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.spectrum_expose_orders(wav, R, detrend=True)                # detrend = 1 without a filter
        for flags in (dict(highpass=2), dict(detrend=2), dict(highpass=-1), dict(detrend=-1)):
            with pytest.raises(_native.NativeError, match=E_ARG):        # the flags are 0 or 1
                d.spectrum_expose_orders(wav, R, **flags)
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_expose_orders(wav, ref.spectrum(wav, 3))           # another n_orb
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_expose_orders(wav[::-1], R)                        # descending grid
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.orders_kernel_ms()                                          # no per-order call yet
        mom, nu, rmom, rnu, tot, model = d.spectrum_expose_orders(wav, R, model=True)
        assert mom.shape == (4, 3, 7) and rmom.shape == (4, 3, 2, 7) and rnu.shape == (4, 3, 2) and tot.shape == (4, 3, 4)
        assert np.all(nu == 4) and np.all(rnu == [1, 3]) and model.shape == (4, 3, 4)
        assert np.all(tot == 0)                                           # order 0 has one pixel, order 1 is not kept
        d.orders_set(seg, perm, key="o")
        assert np.all(d.spectrum_expose_orders(wav, R)[4][..., 3] == 3)
        d.highpass_set(seg, perm, g, 1, key="h")
        d.detrend_set(Ub, W)
        assert d.orders_key == "o" and d.highpass_key == "h"              # neither touches the orders
        assert np.all(d.spectrum_expose_orders(wav, R, highpass=True, detrend=True)[3] == [1, 3])
        assert d.orders_kernel_ms(2)[0] > 0.0
        d.spectrum_expose(wav, R)                                         # another entry ran since
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.orders_kernel_ms()
        d.expose_set(rows, a, F, data, ivar)                              # drops the orders
        assert d.orders_key is None
        for call in (lambda: d.spectrum_expose_orders(wav, R), d.orders_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):
                call()
        d.orders_set(seg, perm, key="o")
        d.observe_set(lam, sig, 5.0, 2)                                   # drops the table and the orders with it
        assert d.orders_key is None and d.expose_key is None
        for call in (lambda: d.spectrum_expose_orders(wav, R), lambda: d.orders_set(seg, perm)):
            with pytest.raises(_native.NativeError, match=E_STATE):
                call()
        d.observe_set(lam[:0], sig[:0], 5.0, 2)                           # no pixel: zeros
        d.expose_set(rows, a, F, data[:, :0], ivar[:, :0])
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.orders_set([0, 1], [])
        d.orders_set([0, 0], [])
        mom, nu, rmom, rnu, tot, model = d.spectrum_expose_orders(wav, R, model=True)
        assert np.all(mom == 0) and np.all(nu == 0) and np.all(rmom == 0) and np.all(rnu == 0) and np.all(tot == 0)
        assert rmom.shape == (4, 3, 1, 7) and model.shape == (4, 3, 0)
    finally:
        d.close()


# ---- 9: the Python path ------------------------------------------------------------------------------------------------------
def test_transit_expose_orders_end_to_end(monkeypatch):
    """Transit.expose(ex, orders=od, highpass=hp, detrend=dt) on the reduced C1 problem of
    test_transit_expose_highpass_end_to_end (60 pixels about Na D2 in two overlapping orders given in descending
    wavelength): the spectrum entry's numbers on that transit's R; order_records=False brings the totals alone;
    a second call uploads nothing; orders=None is the old call bit for bit, without by_order."""
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
    orders = ((np.arange(n_pix) // 3) % 2)[::-1].copy() + 40            # overlapping orders, labels 40 and 41
    ins = obs.Instrument(px[::-1], resolving_power=140000.0, truncate=5.0)
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
    flat = obs.high_pass(raw, taps, orders=orders, mode="divide")
    Ub, clean = obs.sysrem(flat, err, 1, ones=True)
    ex = obs.Exposures(ins, rows, a, F, clean, err)
    hp = obs.HighPass(ex, taps, orders=orders, mode="divide")
    dt = obs.Detrend(ex, Ub)
    od = obs.Orders(ex, orders, keep=[True, True])
    old = tr.expose(ex, return_model=True, devices=[0], highpass=hp, detrend=dt)
    assert not hasattr(old, "by_order") and not hasattr(old, "order_totals")
    R = np.array(tr.sumOverChords(devices=[0]))
    wav = np.asarray(tr.wavelength)
    dev = _native.get_device(0)
    out = tr.expose(ex, return_model=True, devices=[0], highpass=hp, detrend=dt, orders=od)
    assert dev.expose_key == ex.key and dev.highpass_key == hp.key and dev.orders_key == od.key
    for got in (dev.transit_expose_orders(highpass=True, detrend=True, model=True),
                dev.spectrum_expose_orders(wav, R, highpass=True, detrend=True, model=True)):
        assert np.array_equal(out.moments, got[0]) and np.array_equal(out.n_used, got[1])
        assert np.array_equal(out.by_order.moments, got[2]) and np.array_equal(out.by_order.n_used, got[3])
        assert np.array_equal(out.order_totals.loglike, got[4][..., 0], equal_nan=True)
        assert np.array_equal(out.order_totals.chi2, got[4][..., 1])
        assert np.array_equal(out.order_totals.chi2_scaled, got[4][..., 2], equal_nan=True)
        assert np.array_equal(out.order_totals.n_used, got[4][..., 3].astype(np.int64))
        assert np.array_equal(out.model, ins.unsort(got[5]), equal_nan=True)
    # the lumped numbers are the old call's; the records are the reference's of the final model in the device's order
    assert np.array_equal(out.moments, old.moments) and np.array_equal(out.n_used, old.n_used)
    assert np.array_equal(out.model, old.model, equal_nan=True)
    want_mom, want_nu = oref.order_moments_f64(ins.sort(out.model), ex.data, ex.ivar, None, od.seg_first, od.perm)
    assert np.array_equal(out.by_order.moments, want_mom) and np.array_equal(out.by_order.n_used, want_nu)
    assert list(out.by_order.labels) == [40, 41] and out.by_order.moments.shape == (n_exp, 4, 2, 7)
    assert np.array_equal(out.by_order.n_used.sum(axis=2), out.n_used) and np.all(out.by_order.n_used >= 2)
    assert np.array_equal(out.order_totals.n_used, out.n_used)
    assert np.array_equal(out.order_totals.chi2, out.by_order.moments[..., 6].sum(axis=2))
    assert np.allclose(out.by_order.total("loglike"), out.order_totals.loglike.sum(axis=0), rtol=1e-12, atol=0)
    # the totals alone; a second call with the same objects uploads nothing
    calls = []
    for fn in ("observe_set", "expose_set", "detrend_set", "highpass_set", "orders_set"):
        monkeypatch.setattr(dev, fn, lambda *a, _fn=fn, **k: calls.append(_fn))
    lean = tr.expose(ex, devices=[0], highpass=hp, detrend=dt, orders=od, order_records=False)
    assert calls == [] and lean.model is None and lean.by_order is None
    assert np.array_equal(lean.order_totals.loglike, out.order_totals.loglike, equal_nan=True)
    assert np.array_equal(lean.order_totals.chi2_scaled, out.order_totals.chi2_scaled, equal_nan=True)
    assert np.array_equal(lean.moments, out.moments)
    monkeypatch.undo()
    # without filters, and orders=None: the old bits, the orders still resident
    bare = tr.expose(ex, return_model=True, devices=[0], orders=od)
    plain = tr.expose(ex, return_model=True, devices=[0], orders=None)
    assert not hasattr(plain, "by_order") and dev.orders_key == od.key
    assert np.array_equal(bare.moments, plain.moments) and np.array_equal(bare.model, plain.model, equal_nan=True)
    again = tr.expose(ex, return_model=True, devices=[0], highpass=hp, detrend=dt)
    assert np.array_equal(again.moments, old.moments) and np.array_equal(again.model, old.model, equal_nan=True)
