"""Injection grids on the device (include/prom_hip.h, "injection grids on the device"): prom_spectrum_inject_grid and
prom_spectrum_recover_grid against loops of the single calls, bit for bit, over n_exp in {2, 7} x n_pix in {1, 127, 129}
and the five configurations of test_gpu_recover; the independence of n_inj, the position and the sub-batches (the
byte cap forced down); an entry whose components end beside neighbours whose components do not; the state a grid call
leaves; the refusals; Transit.inject_grid / Transit.recover_grid against the entries and the planted planet as a grid."""
import numpy as np
import pytest

from helpers import grid_design as gd
from helpers import observe_ref as ref
from helpers import sysrem_ref as sref
import test_gpu_recover as tr_
import test_gpu_sysrem as ts

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = "PROM_E_ARG", "PROM_E_STATE"
LIST = gd.LIST                                   # a duplicate and a scale of 0
TRIALS, SCALES = [t for t, _ in LIST], [s for _, s in LIST]
CAP = "PROM_GRID_SCRATCH_MB"                     # read at every grid call


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


planet = ts.planet


def eq(got, want, name):
    assert len(got) == len(want), name
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), (name, i)
        if g is not None:
            assert g.shape == w.shape and g.dtype == w.dtype, (name, i, g.shape, w.shape)
            assert np.array_equal(g, w, equal_nan=True), (name, i)


def inject_loop(dev, d, points, **kw):
    """(U, cleaned, injected) of a loop of prom_spectrum_inject, stacked."""
    outs = [dev.spectrum_inject(d["wav"], d["R"], t, s, injected=True, **kw) for t, s in points]
    return tuple(np.stack(x) for x in zip(*outs))


def recover_loop(dev, d, points, orders, **kw):
    """(moments, n_used, totals, U) of a loop of prom_spectrum_recover, stacked."""
    outs = [dev.spectrum_recover(d["wav"], d["R"], t, s, orders=orders, records=False, **kw) for t, s in points]
    return (np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]),
            np.stack([o[4] for o in outs]) if orders else None, np.stack([o[6] for o in outs]))


def cap_for(dev, d, n_cols, recover, nb):
    """Megabytes under which a sub-batch holds exactly nb injections of the design (grid_index.h's count)."""
    n_exp, n_pix = d["raw"].shape
    per = gd.injection_bytes(n_exp, n_pix, n_cols, d["F"].shape[2], recover)
    return repr((nb * per + per // 2) / 1048576.0)


# ---- 1: the equivalence clause over the shapes --------------------------------------------------------------------
@pytest.mark.parametrize("n_exp,n_pix", [(2, 1), (2, 127), (2, 129), (7, 1), (7, 127), (7, 129)])
def test_grid_calls_are_loops_of_the_single_calls_bitwise(dev, n_exp, n_pix):
    d = ts.design(n_exp, n_pix, seed=n_exp + n_pix)
    for ones, mode, orders, n_comp in tr_.CONFIGS:
        name = "n_exp=%d n_pix=%d ones=%d mode=%s orders=%d" % (n_exp, n_pix, ones, mode, orders)
        kw = dict(n_comp=n_comp, n_iter=4, ones=ones, highpass=mode is not None)
        tr_.upload(dev, d, mode, orders)
        want_i = inject_loop(dev, d, LIST, **kw)
        want_r = recover_loop(dev, d, LIST, orders, **kw)
        eq(dev.spectrum_inject_grid(d["wav"], d["R"], TRIALS, SCALES, injected=True, **kw), want_i, name + " inject")
        eq(dev.spectrum_recover_grid(d["wav"], d["R"], TRIALS, SCALES, orders=orders, **kw), want_r, name + " recover")
        # every output may be NULL, and what is asked for alone is the same
        lean = dev.spectrum_inject_grid(d["wav"], d["R"], TRIALS, SCALES, data=False, **kw)
        assert lean[1] is None and lean[2] is None and np.array_equal(lean[0], want_i[0])
        lean = dev.spectrum_recover_grid(d["wav"], d["R"], TRIALS, SCALES, orders=orders, moments=False, **kw)
        assert lean[0] is None and lean[1] is None
        eq(lean[2:], want_r[2:], name + " lean recover")
    assert want_r[1].any() or n_pix == 1


# ---- 2: the independence clause --------------------------------------------------------------------------------------
def test_entries_do_not_depend_on_the_list_or_on_the_sub_batches(dev, monkeypatch):
    d = ts.design(7, 129, seed=21)
    kw = dict(n_comp=2, n_iter=4, ones=True, highpass=True)
    tr_.upload(dev, d, 1, True)
    monkeypatch.delenv(CAP, raising=False)
    full_i = dev.spectrum_inject_grid(d["wav"], d["R"], TRIALS, SCALES, injected=True, **kw)
    full_r = dev.spectrum_recover_grid(d["wav"], d["R"], TRIALS, SCALES, orders=True, **kw)
    assert full_r[1].any()
    for b, (t, s) in enumerate(LIST):                                     # every entry alone
        eq(dev.spectrum_inject_grid(d["wav"], d["R"], [t], [s], injected=True, **kw), [x[b:b + 1] for x in full_i],
           "alone %d" % b)
        eq(dev.spectrum_recover_grid(d["wav"], d["R"], [t], [s], orders=True, **kw), [x[b:b + 1] for x in full_r],
           "alone %d" % b)
    eq(dev.spectrum_inject_grid(d["wav"], d["R"], TRIALS[::-1], SCALES[::-1], injected=True, **kw),
       [x[::-1] for x in full_i], "reversed")
    eq(dev.spectrum_recover_grid(d["wav"], d["R"], TRIALS[::-1], SCALES[::-1], orders=True, **kw),
       [x[::-1] for x in full_r], "reversed")
    for nb in (2, 1):                                                     # sub-batches of 2, 2, 1 and of 1
        for recover, call, want in ((False, lambda: dev.spectrum_inject_grid(d["wav"], d["R"], TRIALS, SCALES,
                                                                             injected=True, **kw), full_i),
                                    (True, lambda: dev.spectrum_recover_grid(d["wav"], d["R"], TRIALS, SCALES,
                                                                             orders=True, **kw), full_r)):
            monkeypatch.setenv(CAP, cap_for(dev, d, 3, recover, nb))
            eq(call(), want, "sub-batches of %d, recover=%d" % (nb, recover))
    monkeypatch.setenv(CAP, "1e-9")                                       # below one injection: one at a time
    eq(dev.spectrum_recover_grid(d["wav"], d["R"], TRIALS, SCALES, orders=True, **kw), full_r, "tiny cap")


# ---- 3: a component that ends stops its own injection alone -----------------------------------------------------
@pytest.mark.parametrize("nb", [None, 2])
def test_an_entry_whose_components_end_leaves_its_neighbours_alone(dev, monkeypatch, nb):
    """grid_design.overflow_design: the middle entry's scale makes D infinite at every pixel, so it has no weight and
    each of its components ends at once (test_inject_grid_cpu.py checks that on the numpy model); its neighbours in
    the same launches, on either side, fit theirs."""
    d, points = gd.overflow_design()
    kw = dict(n_comp=2, n_iter=4)
    ts.upload(dev, d)
    if nb is None:
        monkeypatch.delenv(CAP, raising=False)
    else:
        monkeypatch.setenv(CAP, cap_for(dev, d, 2, True, nb))
    want_i = inject_loop(dev, d, points, **kw)
    want_r = recover_loop(dev, d, points, False, **kw)
    t, s = [p[0] for p in points], [p[1] for p in points]
    got = dev.spectrum_inject_grid(d["wav"], d["R"], t, s, injected=True, **kw)
    eq(got, want_i, "inject")
    eq(dev.spectrum_recover_grid(d["wav"], d["R"], t, s, **kw), want_r, "recover")
    U = got[0]
    assert not U[1].any() and np.isinf(got[2][1]).any()                   # the design exercises the flags
    for b in (0, 2):
        assert all(U[b][:, k].any() for k in range(2)) and want_r[1][b].any()


# ---- 4: the state a grid call leaves, and the refusals ------------------------------------------------------------
def test_state_after_a_grid_call(dev, monkeypatch):
    monkeypatch.delenv(CAP, raising=False)
    d = ts.design(7, 129, n_trial=5, seed=10)
    kw = dict(n_comp=2, n_iter=4, highpass=True)
    tr_.upload(dev, d, 0, True)
    plain = dev.spectrum_expose(d["wav"], d["R"], model=True)
    inj0 = dev.spectrum_inject(d["wav"], d["R"], 3, 1.3, injected=True, **kw)
    rec0 = dev.spectrum_recover(d["wav"], d["R"], 3, 1.3, orders=True, model=True, **kw)
    dev.detrend_build(np.random.default_rng(3).normal(size=(7, 3)), key="mine")
    before = dev.spectrum_expose_detrended(d["wav"], d["R"], model=True)
    t, s = [3, 0, 4], [1.3, 0.2, -1.0]
    g1 = dev.spectrum_inject_grid(d["wav"], d["R"], t, s, injected=True, **kw)
    r1 = dev.spectrum_recover_grid(d["wav"], d["R"], t, s, orders=True, **kw)
    with pytest.raises(Exception, match=E_STATE):                         # nothing of a grid call to repeat
        dev.sysrem_kernel_ms(1)
    eq(dev.spectrum_inject_grid(d["wav"], d["R"], t, s, injected=True, **kw), g1, "two inject grid calls")
    eq(dev.spectrum_recover_grid(d["wav"], d["R"], t, s, orders=True, **kw), r1, "two recover grid calls")
    eq([x[0] for x in g1], inj0, "entry 0 is the single call")
    eq([r1[0][0], r1[1][0], r1[2][0], r1[3][0]], [rec0[0], rec0[1], rec0[4], rec0[6]], "entry 0 is the single call")
    # the resident filter, raw and the table's data are as they were
    assert dev.detrend_key == "mine"
    eq(dev.spectrum_expose_detrended(d["wav"], d["R"], model=True), before, "the resident filter")
    eq(dev.spectrum_expose(d["wav"], d["R"], model=True), plain, "the table's data")
    eq(dev.spectrum_inject(d["wav"], d["R"], 3, 1.3, injected=True, **kw), inj0, "raw")
    eq(dev.spectrum_recover(d["wav"], d["R"], 3, 1.3, orders=True, model=True, **kw), rec0, "recover afterwards")
    # n_inj = 0 succeeds and writes nothing
    e = dev.spectrum_inject_grid(d["wav"], d["R"], [], [], **kw)
    assert e[0].shape == (0, 7, 2) and e[1].shape == (0, 7, 129)
    e = dev.spectrum_recover_grid(d["wav"], d["R"], [], [], orders=True, **kw)
    assert e[0].shape == (0, 7, 5, 7) and e[2].shape == (0, 7, 5, 4)


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
    calls = (lambda t, s, **kw: d.spectrum_inject_grid(wav, R, t, s, **kw),
             lambda t, s, **kw: d.spectrum_recover_grid(wav, R, t, s, **kw))
    try:
        for call in calls + (lambda t, s, **kw: d.transit_inject_grid(t, s, **kw),
                             lambda t, s, **kw: d.transit_recover_grid(t, s, **kw)):
            with pytest.raises(_native.NativeError, match=E_STATE):      # no exposure table on the context
                call([0], [1.0], n_comp=2)
        d.observe_set(lam, sig, 5.0, 2)
        d.expose_set(rows, a, F, data, ivar)
        for call in calls:
            with pytest.raises(_native.NativeError, match=E_STATE):      # a table, but no raw exposures
                call([0], [1.0], n_comp=2)
        d.sysrem_set(raw, key="r")
        for call in calls:
            for kw in (dict(n_comp=0), dict(n_comp=-1, ones=True), dict(n_comp=17), dict(n_comp=16, ones=True),
                       dict(n_comp=2, n_iter=0)):
                with pytest.raises(_native.NativeError, match=E_ARG):    # ranges broken
                    call([0], [1.0], **kw)
            for trial in (-1, 3):
                with pytest.raises(_native.NativeError, match="entry 1"):  # a trial outside [0, n_trial)
                    call([0, trial], [1.0, 1.0], n_comp=2)
            for scale in (np.nan, np.inf, -np.inf):
                with pytest.raises(_native.NativeError, match="entry 2"):
                    call([0, 1, 2], [1.0, 0.0, scale], n_comp=2)
            with pytest.raises(_native.NativeError, match=E_STATE):
                call([0], [1.0], n_comp=2, highpass=True)                # highpass = 1 without a resident high-pass
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.spectrum_recover_grid(wav, R, [0], [1.0], n_comp=2, orders=True)   # orders = 1 without resident orders
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_inject_grid(wav, ref.spectrum(wav, 3), [0], [1.0], n_comp=2)   # another n_orb
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.transit_recover_grid([0], [1.0], n_comp=2)                  # no run yet
        for n_inj in (-1, 2):                                             # n_inj < 0; arrays missing with n_inj > 0
            rc = d.lib.prom_spectrum_inject_grid(d.h, 2, len(wav), wav.ctypes.data_as(_native._dp),
                                                 R.ctypes.data_as(_native._dp), n_inj, None, None, 0, 2, 3, 0, None,
                                                 None, None)
            assert _native.STATUS[rc] == E_ARG
        # a valid call after every refusal
        U, cleaned, _ = d.spectrum_inject_grid(wav, R, [2, 0], [-0.5, 1.0], n_comp=2, n_iter=3, ones=True)
        one = d.spectrum_inject(wav, R, 2, -0.5, n_comp=2, n_iter=3, ones=True)
        assert np.array_equal(U[0], one[0]) and np.array_equal(cleaned[0], one[1], equal_nan=True)
        d.highpass_set(seg, perm, g, 1)
        d.orders_set(seg, perm, np.array([1, 1], dtype=np.uint8))
        out = d.spectrum_recover_grid(wav, R, [2, 0], [0.5, 1.0], n_comp=1, highpass=True, orders=True)
        one = d.spectrum_recover(wav, R, 0, 1.0, 1, highpass=True, orders=True)
        assert out[0].shape == (2, 4, 3, 7) and out[2].shape == (2, 4, 3, 4) and out[3].shape == (2, 4, 1)
        assert np.array_equal(out[0][1], one[0]) and np.array_equal(out[2][1], one[4])
        d.observe_set(lam[:0], sig[:0], 5.0, 2)                           # no pixel: zeros, and the inject call's U
        d.expose_set(rows, a, F, data[:, :0], ivar[:, :0])
        d.sysrem_set(raw[:, :0])
        d.orders_set(np.array([0, 0]), np.zeros(0, dtype=np.int32), np.array([1], dtype=np.uint8))
        out = d.spectrum_recover_grid(wav, R, [0, 1], [1.0, 2.0], n_comp=2, ones=True, orders=True)
        assert not out[0].any() and not out[1].any() and not out[2].any()
        assert np.all(out[3][:, :, 0] == 1) and np.all(out[3][:, :, 1:] == 0)
        U = d.spectrum_inject_grid(wav, R, [0, 1], [1.0, 2.0], n_comp=2, ones=True)[0]
        assert np.array_equal(U, out[3])
    finally:
        d.close()


# ---- 5: the Python path and the planted planet as a grid -------------------------------------------------------------
def test_transit_grid_calls_are_the_entries(planet):
    """Transit.inject_grid / recover_grid equal the prom_transit_*_grid entries on the run's R and, with broaden=, on
    tr.broadened(bk); grid[b] is Transit.inject / Transit.recover for that point."""
    from prometheus_amd import _native
    from prometheus_amd import observation as obs
    tr, d, ex, inj, hp = planet
    ins = d["ins"]
    od = obs.Orders(ex, d["orders"])
    dev = _native.get_device(0)
    bk = obs.Broadening(*obs.rotation_kernel(3e5, n=33))
    t, s = obs.injection_grid([2, 5], [0.5, 1.0])
    kw = dict(n_comp=2, n_iter=4, highpass=hp, devices=[0])
    grids = []
    for broaden in (None, bk):
        cg = tr.inject_grid(inj, t, s, broaden=broaden, **kw)
        rg = tr.recover_grid(inj, t, s, orders=od, broaden=broaden, **kw)
        assert dev.expose_key == ex.key and dev.highpass_key == hp.key and dev.sysrem_key == inj.key
        assert len(cg) == len(rg) == 4 and rg.total("loglike").shape == (4, 9)
        # the entries on the same run (the last run's R, its R_b while that is current)
        U, cleaned, _ = dev.transit_inject_grid(t, s, n_comp=2, n_iter=4, highpass=True)
        eq((cg.U, cg.data), (U, ins.unsort(cleaned)), "Transit.inject_grid")
        mom, nu, tot, U = dev.transit_recover_grid(t, s, n_comp=2, n_iter=4, highpass=True, orders=True)
        eq((rg.moments, rg.n_used, rg.U), (mom, nu, U), "Transit.recover_grid")
        R = np.array(tr.sumOverChords(devices=[0])) if broaden is None else tr.broadened(bk, devices=[0])
        eq(dev.spectrum_recover_grid(np.asarray(tr.wavelength), R, t, s, n_comp=2, n_iter=4, highpass=True,
                                     orders=True), (mom, nu, tot, U), "the spectrum entry")
        for b in (0, 3):
            one = tr.inject(inj, int(t[b]), float(s[b]), broaden=broaden, **kw)
            eq((cg[b].U, cg[b].data), (one.U, one.data), "grid[b] of inject_grid")
            vm = tr.recover(inj, int(t[b]), float(s[b]), orders=od, broaden=broaden, order_records=False, **kw)
            eq((rg[b].moments, rg[b].n_used, rg[b].U, rg[b].order_totals.loglike, rg[b].order_totals.n_used),
               (vm.moments, vm.n_used, vm.U, vm.order_totals.loglike, vm.order_totals.n_used), "grid[b] of recover_grid")
            assert np.array_equal(rg.total("loglike")[b], vm.total("loglike"), equal_nan=True)
        grids.append(rg)
    assert not np.array_equal(grids[0].moments, grids[1].moments)         # (the broadening is seen)
    assert tr.inject_grid(inj, 2, [0.5, 1.0], data=False, **kw).data is None


def test_planted_planet_grid_peaks_where_the_loop_peaks(planet):
    """12 exposures, 400 pixels, 9 trials; a 3 x 2 grid of (trial, scale): for every point recover_grid peaks where
    Transit.recover peaks, and at the injected trial for the planet's own strength."""
    from prometheus_amd import observation as obs
    tr, d, ex, inj, hp = planet
    kw = dict(n_comp=d["n_comp"], n_iter=d["n_iter"], ones=d["ones"], highpass=hp, devices=[0])
    t, s = obs.injection_grid([2, sref.PLANET_TRIAL, 7], [1.0, 2.0])
    rg = tr.recover_grid(inj, t, s, **kw)
    ll = rg.total("loglike")
    for b in range(6):
        vm = tr.recover(inj, int(t[b]), float(s[b]), **kw)
        assert int(np.argmax(ll[b])) == int(np.argmax(vm.total("loglike")))
        assert np.array_equal(rg[b].moments, vm.moments) and np.array_equal(rg.U[b], vm.U)
    assert int(np.argmax(ll[2])) == sref.PLANET_TRIAL
