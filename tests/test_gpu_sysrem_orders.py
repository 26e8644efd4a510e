"""SYSREM per echelle order on the device (include/prom_hip.h, "SYSREM per order on the device") against the float64
restatement of the single call's definition (tests/helpers/sysrem_ref.py, unchanged) applied order by order, bit for
bit: orders of 1, T - 1, T, T + 1 and 3 T + 5 pixels (T = the step kernel's tile) mixed and interleaved in one table,
n_exp in {1, 2, 7, 70}, with and without ones and the high-pass of both modes, NaN, an infinity and ivar = 0 sprinkled
in; the equality with the existing single calls; the independence of the orders and components that end in one order
alone; the grids, also in two sub-batches; the state and the refusals; Transit.clean / inject / inject_grid with
``sysrem_orders``."""
import numpy as np
import pytest

from helpers import sysrem_ref as sref
import test_gpu_sysrem as ts

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = "PROM_E_ARG", "PROM_E_STATE"
T = sref.TILE
MIXED = [1, T - 1, T, T + 1, 3 * T + 5]
CAP = "PROM_GRID_SCRATCH_MB"                     # read at every grid call


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


planet = ts.planet


def interleaved(lengths):
    """(seg_first, perm) of orders of the given lengths dealt over the device's pixels in turn, every second order
    reversed: perm is monotonic neither across the orders nor inside them."""
    n_seg, n_pix = len(lengths), int(sum(lengths))
    members = [[] for _ in lengths]
    s = 0
    for p in range(n_pix):
        while len(members[s]) >= lengths[s]:
            s = (s + 1) % n_seg
        members[s].append(p)
        s = (s + 1) % n_seg
    members = [m[::-1] if k % 2 else m for k, m in enumerate(members)]
    seg = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return seg, np.concatenate(members).astype(np.int32)


def per_order(D, ivar, seg, perm, n_comp, n_iter, ones):
    """(U [n_seg][n_exp][cols], cleaned) of sysrem_f64 applied to every order's columns of D."""
    cleaned = np.array(D)
    Us = []
    for s in range(len(seg) - 1):
        idx = perm[seg[s]:seg[s + 1]]
        U, cl = sref.sysrem_f64(D[:, idx], ivar[:, idx], n_comp, n_iter, ones)
        Us.append(U)
        cleaned[:, idx] = cl
    return np.stack(Us), cleaned


def expected(dev, d, seg, perm, trial, scale, n_comp, n_iter, ones, hp=None):
    """The reference: test_gpu_sysrem's numpy injection and host high-pass, then sysrem_f64 order by order."""
    D = ts.expected(dev, d, trial, scale, 1, 1, False, hp)[2]
    U, cleaned = per_order(D, d["ivar"], seg, perm, n_comp, n_iter, ones)
    return U, cleaned, D


# ---- 1: bit for bit against the reference over the shapes ---------------------------------------------------------
#        n_exp, order lengths, n_comp, n_iter, ones, high-pass mode (None: none)
SHAPES = [(7, MIXED, 3, 4, True, None),
          (70, MIXED, 2, 2, False, 0),
          (2, [3 * T + 5, 1, T + 1], 16, 1, False, 1),
          (1, [T, T, T], 0, 4, True, None),
          (7, [1, 2, 1], 3, 4, False, 1),
          (2, [T - 1, T + 1], 15, 1, True, 0)]


@pytest.mark.parametrize("n_exp,lengths,n_comp,n_iter,ones,mode", SHAPES)
def test_per_order_sysrem_bitwise_over_the_shapes(dev, n_exp, lengths, n_comp, n_iter, ones, mode):
    """U, cleaned and injected of prom_spectrum_inject_orders and prom_sysrem_clean_orders equal sysrem_f64 applied to
    the columns perm[...] of every order of the numpy-injected, host-high-passed D, NaN pattern included."""
    n_pix = sum(lengths)
    d = ts.design(n_exp, n_pix, seed=n_exp + n_pix)
    hp = None if mode is None else (np.exp(-0.5 * (np.arange(6) / 2.0) ** 2), mode)
    ts.upload(dev, d, hp)
    seg, perm = interleaved(lengths)
    dev.orders_set(seg, perm)
    name = "n_exp=%d lengths=%s n_comp=%d n_iter=%d ones=%d mode=%s" % (n_exp, lengths, n_comp, n_iter, ones, mode)
    args = dict(n_comp=n_comp, n_iter=n_iter, ones=ones, highpass=hp is not None, injected=True)
    got = dev.spectrum_inject_orders(d["wav"], d["R"], 1, 0.7, **args)
    ts.same(got, expected(dev, d, seg, perm, 1, 0.7, n_comp, n_iter, ones, hp), name + " inject")
    got = dev.sysrem_clean_orders(**args)
    ts.same(got, expected(dev, d, seg, perm, None, 0.0, n_comp, n_iter, ones, hp), name + " clean")
    assert got[0].shape == (len(lengths), n_exp, n_comp + ones) and (not ones or np.all(got[0][:, :, 0] == 1.0))
    assert not np.signbit(got[0][got[0] == 0]).any()
    # the injected data are the single call's: the injection and the high-pass are not per order
    single = dev.sysrem_clean(**args)
    assert np.array_equal(got[2], single[2], equal_nan=True)
    if len(lengths) > 1 and n_pix > 8 and n_exp > 1:
        assert not np.array_equal(got[1], single[1], equal_nan=True)     # ... and the cleaning is


# ---- 2: equality with the existing single calls -------------------------------------------------------------------
def test_one_order_with_the_identity_perm_is_the_single_call(dev):
    for n_exp, n_pix in ((7, 3 * T + 5), (2, T), (7, 1)):
        d = ts.design(n_exp, n_pix, seed=31 + n_pix)
        hp = (np.exp(-0.5 * (np.arange(6) / 2.0) ** 2), 1)
        ts.upload(dev, d, hp)
        dev.orders_set([0, n_pix], np.arange(n_pix))
        for args in (dict(n_comp=3, n_iter=4, ones=True, highpass=True, injected=True),
                     dict(n_comp=2, n_iter=3, injected=True)):
            for one, many in ((dev.sysrem_clean(**args), dev.sysrem_clean_orders(**args)),
                              (dev.spectrum_inject(d["wav"], d["R"], 2, 0.4, **args),
                               dev.spectrum_inject_orders(d["wav"], d["R"], 2, 0.4, **args))):
                assert many[0].shape == (1,) + one[0].shape
                assert many[0][0].tobytes() == one[0].tobytes()
                assert many[1].tobytes() == one[1].tobytes() and many[2].tobytes() == one[2].tobytes()


def sub_table(d, idx):
    """The design cut down to the pixels idx (ascending)."""
    out = dict(d)
    for k in ("lam", "sig"):
        out[k] = d[k][idx]
    for k in ("data", "ivar", "raw"):
        out[k] = np.ascontiguousarray(d[k][:, idx])
    return out


def test_each_order_equals_the_single_call_on_its_own_table(dev):
    """Three interleaved orders (ascending pixels inside each): order s of the per-order calls equals the existing
    single call on a table made of that order's columns alone, byte for byte."""
    n_exp, lengths = 7, [T + 1, 3 * T + 5, T - 1]
    n_pix = sum(lengths)
    d = ts.design(n_exp, n_pix, seed=77)
    labels = np.random.default_rng(1).permutation(np.repeat(np.arange(3), lengths))
    members = [np.flatnonzero(labels == s) for s in range(3)]
    seg = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    perm = np.concatenate(members).astype(np.int32)
    args = dict(n_comp=3, n_iter=4, ones=True, injected=True)
    ts.upload(dev, d)
    dev.orders_set(seg, perm)
    clean = dev.sysrem_clean_orders(**args)
    inject = dev.spectrum_inject_orders(d["wav"], d["R"], 1, 0.7, **args)
    for s, idx in enumerate(members):
        ts.upload(dev, sub_table(d, idx))
        for many, one in ((clean, dev.sysrem_clean(**args)),
                          (inject, dev.spectrum_inject(d["wav"], d["R"], 1, 0.7, **args))):
            assert many[0][s].tobytes() == one[0].tobytes(), s
            assert np.ascontiguousarray(many[1][:, idx]).tobytes() == one[1].tobytes(), s
            assert np.ascontiguousarray(many[2][:, idx]).tobytes() == one[2].tobytes(), s


# ---- 3: independence and ended components ------------------------------------------------------------------------
def test_a_masked_order_and_an_order_of_one_pixel_end_their_own_components_only(dev):
    n_exp, lengths = 7, [T + 1, 1, T - 1, 40]
    n_pix = sum(lengths)
    d = ts.design(n_exp, n_pix, seed=13, holes=False)
    seg, perm = interleaved(lengths)
    d["raw"][:, perm[seg[1]]] = 1.0                                       # the lone pixel: the column of ones takes all
    d["ivar"][:, perm[seg[1]]] = 1024.0                                   # of it, exactly
    args = dict(n_comp=3, n_iter=4, ones=True)
    ts.upload(dev, d)
    dev.orders_set(seg, perm)
    U0, c0, _ = dev.sysrem_clean_orders(**args)
    ts.same((U0, c0), per_order(d["raw"], d["ivar"], seg, perm, 3, 4, True), "four orders")
    # the order of one pixel: the column of ones takes the pixel's mean and leaves exact zeros, so its later components
    # end: zeros, never -0, and cleaned data of zero
    assert np.all(U0[1, :, 0] == 1) and np.all(U0[1, :, 1:] == 0) and not np.signbit(U0[1]).any()
    assert np.all(c0[:, perm[seg[1]]] == 0.0)
    assert np.all(np.abs(U0[[0, 2, 3], :, 1:]).max(axis=1) > 0)          # nobody else's components ended
    # order 3 all masked: its U is zeros behind the ones, its data come back as they came, the others' bits stay
    masked = perm[seg[3]:seg[4]]
    d2 = dict(d, ivar=np.array(d["ivar"]))
    d2["ivar"][:, masked] = 0.0
    ts.upload(dev, d2)
    dev.orders_set(seg, perm)
    U1, c1, _ = dev.sysrem_clean_orders(**args)
    assert np.all(U1[3, :, 0] == 1) and np.all(U1[3, :, 1:] == 0) and not np.signbit(U1[3]).any()
    assert np.array_equal(c1[:, masked], d["raw"][:, masked])
    assert U1[:3].tobytes() == U0[:3].tobytes()
    rest = np.setdiff1d(np.arange(n_pix), masked)
    assert np.array_equal(c1[:, rest], c0[:, rest])
    ts.same((U1, c1), per_order(d2["raw"], d2["ivar"], seg, perm, 3, 4, True), "a masked order")


def test_an_orders_bits_do_not_depend_on_the_other_orders(dev):
    """Reordering the orders permutes U's rows and leaves every cleaned pixel; merging the other orders into one
    leaves order s's U and pixels."""
    n_exp, lengths = 7, [T + 1, 30, 3 * T + 5, T]
    n_pix = sum(lengths)
    d = ts.design(n_exp, n_pix, seed=17)
    seg, perm = interleaved(lengths)
    members = [perm[seg[s]:seg[s + 1]] for s in range(4)]
    args = dict(n_comp=2, n_iter=4)
    ts.upload(dev, d)
    dev.orders_set(seg, perm)
    U0, c0, _ = dev.sysrem_clean_orders(**args)
    turn = [2, 0, 3, 1]
    seg2 = np.concatenate([[0], np.cumsum([lengths[s] for s in turn])]).astype(np.int32)
    dev.orders_set(seg2, np.concatenate([members[s] for s in turn]))
    U1, c1, _ = dev.sysrem_clean_orders(**args)
    assert U1.tobytes() == U0[turn].tobytes() and c1.tobytes() == c0.tobytes()
    for s in range(4):                                                    # order s first, everybody else in one order
        others = np.concatenate([members[k] for k in range(4) if k != s])
        dev.orders_set([0, lengths[s], n_pix], np.concatenate([members[s], others]))
        U2, c2, _ = dev.sysrem_clean_orders(**args)
        assert U2.shape[0] == 2 and U2[0].tobytes() == U0[s].tobytes(), s
        assert np.array_equal(c2[:, members[s]], c0[:, members[s]], equal_nan=True), s
    # keep plays no part: every order is cleaned
    dev.orders_set(seg, perm, keep=[1, 0, 0, 1])
    U3, c3, _ = dev.sysrem_clean_orders(**args)
    assert U3.tobytes() == U0.tobytes() and c3.tobytes() == c0.tobytes()


# ---- 4: the grids ---------------------------------------------------------------------------------------------------
def order_bytes(n_exp, n_pix, n_seg, n_max, n_cols, n_tap):
    """os_injection_bytes of order_sysrem_index.h, restated."""
    tiles = (n_max + T - 1) // T
    per_order = 2 * n_exp * tiles * T + n_exp + 2 * n_exp * tiles + n_exp * n_cols
    return 8 * (3 * n_exp * n_pix + n_exp * n_tap + n_seg * per_order) + 4 * 17 * n_seg


def test_grid_per_order_is_the_loop_of_the_single_per_order_calls(dev, monkeypatch):
    n_exp, lengths = 7, [T + 1, 5, T - 1]
    n_pix = sum(lengths)
    d = ts.design(n_exp, n_pix, n_trial=5, seed=23)
    hp = (np.exp(-0.5 * (np.arange(6) / 2.0) ** 2), 0)
    ts.upload(dev, d, hp)
    seg, perm = interleaved(lengths)
    dev.orders_set(seg, perm)
    points = [(3, 1.0), (0, 0.0), (3, 1.0), (4, -0.5), (1, 2.0)]         # a duplicate and a scale of 0
    trials, scales = [t for t, _ in points], [s for _, s in points]
    kw = dict(n_comp=2, n_iter=4, ones=True, highpass=True)
    monkeypatch.delenv(CAP, raising=False)
    outs = [dev.spectrum_inject_orders(d["wav"], d["R"], t, s, injected=True, **kw) for t, s in points]
    want = tuple(np.stack(x) for x in zip(*outs))
    got = dev.spectrum_inject_grid_orders(d["wav"], d["R"], trials, scales, injected=True, **kw)
    assert got[0].shape == (5, 3, n_exp, 3)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.tobytes() == w.tobytes()
    assert not np.array_equal(got[1][0], got[1][3], equal_nan=True)
    # two sub-batches (3 + 2) under the forced cap, then one injection at a time
    per = order_bytes(n_exp, n_pix, 3, max(lengths), 3, d["F"].shape[2])
    for cap in (repr((3 * per + per // 2) / 1048576.0), "1e-9"):
        monkeypatch.setenv(CAP, cap)
        again = dev.spectrum_inject_grid_orders(d["wav"], d["R"], trials, scales, injected=True, **kw)
        for g, w in zip(again, want):
            assert g.tobytes() == w.tobytes(), cap
    monkeypatch.delenv(CAP, raising=False)
    lean = dev.spectrum_inject_grid_orders(d["wav"], d["R"], trials, scales, data=False, **kw)
    assert lean[1] is None and lean[2] is None and lean[0].tobytes() == want[0].tobytes()
    # the existing grid on the same state is untouched by the orders
    one = dev.spectrum_inject_grid(d["wav"], d["R"], trials, scales, **kw)
    assert one[0].shape == (5, n_exp, 3)
    loop = np.stack([dev.spectrum_inject(d["wav"], d["R"], t, s, **kw)[0] for t, s in points])
    assert one[0].tobytes() == loop.tobytes()
    empty = dev.spectrum_inject_grid_orders(d["wav"], d["R"], [], [], **kw)
    assert empty[0].shape == (0, 3, n_exp, 3)


# ---- 5: the state and the refusals ----------------------------------------------------------------------------------
def test_state_and_refusals(dev):
    from prometheus_amd import _native
    d = ts.design(4, 40, seed=5)
    ts.upload(dev, d)                                                     # (a new table drops the orders)
    calls = (lambda: dev.sysrem_clean_orders(2), lambda: dev.spectrum_inject_orders(d["wav"], d["R"], 0, 1.0, 2),
             lambda: dev.spectrum_inject_grid_orders(d["wav"], d["R"], [0], [1.0], 2))
    for call in calls:
        with pytest.raises(_native.NativeError, match=E_STATE):          # no resident orders
            call()
    assert dev.sysrem_clean(2)[0].shape == (4, 2)                         # the single call needs none
    seg, perm = interleaved([13, 27])
    dev.orders_set(seg, perm)
    for kw in (dict(n_comp=0), dict(n_comp=17), dict(n_comp=16, ones=True), dict(n_comp=2, n_iter=0)):
        with pytest.raises(_native.NativeError, match=E_ARG):
            dev.sysrem_clean_orders(**kw)
    with pytest.raises(_native.NativeError, match=E_STATE):              # highpass = 1 without a resident high-pass
        dev.sysrem_clean_orders(2, highpass=True)
    with pytest.raises(_native.NativeError, match=E_ARG):
        dev.spectrum_inject_orders(d["wav"], d["R"], 3, 1.0, 2)          # a trial outside [0, n_trial)
    U, cleaned, _ = dev.sysrem_clean_orders(2, 3)
    assert U.shape == (2, 4, 2)
    ms = dev.sysrem_kernel_ms(2)                                          # repeats the per-order call ...
    assert ms[0] > 0.0 and np.isnan(ms[1]) and np.isnan(ms[2])
    again = dev.sysrem_clean_orders(2, 3)
    assert again[0].tobytes() == U.tobytes() and again[1].tobytes() == cleaned.tobytes()
    one = dev.sysrem_clean(2, 3)                                          # ... and a single call after it is itself
    ts.same(one[:2], sref.sysrem_f64(d["raw"], d["ivar"], 2, 3), "single call after a per-order one")
    dev.expose_set(d["rows"], d["a"], d["F"], d["data"], d["ivar"])      # drops the orders and the raw exposures
    dev.sysrem_set(d["raw"])
    with pytest.raises(_native.NativeError, match=E_STATE):
        dev.sysrem_clean_orders(2)


# ---- 6: the Python path ---------------------------------------------------------------------------------------------
def test_transit_clean_inject_and_inject_grid_take_sysrem_orders(planet):
    """Transit.clean / inject / inject_grid with sysrem_orders equal the per-order entries on the run's R, in the
    caller's pixel order, and sysrem_f64 order by order; grid[b] is the Cleaned of inject."""
    from prometheus_amd import _native
    from prometheus_amd import observation as obs
    tr, d, ex, inj, hp = planet
    ins = d["ins"]
    dev = _native.get_device(0)
    od = obs.Orders(ex, d["orders"])
    kw = dict(n_comp=2, n_iter=4, ones=True, highpass=hp)
    res = tr.clean(inj, sysrem_orders=od, return_injected=True, **kw)
    assert dev.orders_key == od.key and res.U.shape == (2, 12, 3) and res.data.shape == (12, 400)
    U, cleaned, injected = dev.sysrem_clean_orders(2, 4, ones=True, highpass=True, injected=True)
    ts.same((res.U, res.data, res.injected), (U, ins.unsort(cleaned), ins.unsort(injected)), "Transit.clean")
    flat = obs.high_pass(d["raw"], d["taps"], orders=d["orders"], mode=d["mode"])
    want = per_order(ins.sort(flat), ex.ivar, od.seg_first, od.perm, 2, 4, True)
    ts.same((res.U, ins.sort(res.data)), want, "Transit.clean, definition")
    for s, label in enumerate(od.labels):                                 # U[s] belongs to the Orders' label s
        mine = ins.order[od.perm[od.seg_first[s]:od.seg_first[s + 1]]]    # (the caller's pixels of order s)
        assert np.all(d["orders"][mine] == label)
    single = tr.clean(inj, **kw)
    assert single.U.shape == (12, 3) and not np.array_equal(single.data, res.data, equal_nan=True)
    one = tr.inject(inj, 2, 0.5, sysrem_orders=od, devices=[0], **kw)
    R, wav = np.array(tr.sumOverChords(devices=[0])), np.asarray(tr.wavelength)
    U, cleaned, _ = dev.spectrum_inject_orders(wav, R, 2, 0.5, n_comp=2, n_iter=4, ones=True, highpass=True)
    ts.same((one.U, one.data), (U, ins.unsort(cleaned)), "Transit.inject")
    grid = tr.inject_grid(inj, [2, 6], [0.5, 1.0], sysrem_orders=od, devices=[0], **kw)
    assert grid.U.shape == (2, 2, 12, 3) and grid.data.shape == (2, 12, 400)
    ts.same((grid[0].U, grid[0].data), (one.U, one.data), "grid[0] of inject_grid")
