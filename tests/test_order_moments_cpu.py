"""Per-order moments without a device: the host harness of k_order_moments' and k_order_totals' index arithmetic and
formulas (tests/helpers/order_host.cpp, a stand-alone program, plain, sanitized and with small compile-time constants),
the float64 references (tests/helpers/order_ref.py) and their bounds, observation.Orders / OrderMap, and the refusals of
Orders and Transit.expose(orders=...) that come before a device is needed."""
import os
import subprocess

import numpy as np
import pytest

from helpers import highpass_ref as href
from helpers import order_ref as oref
from test_highpass_cpu import _bare_transit

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "prometheus_amd", "csrc")
HOST = os.path.join(REPO, "tests", "helpers", "order_host.cpp")
U = 2.0 ** -53
LENGTHS = (1, 2, 31, 32, 33, 64, 200)


def _case(n_exp=2, n_trial=11, lengths=LENGTHS, seed=17):
    """Model, data, ivar, flags and interleaved orders with every way a position can be unused: NaN model, ivar 0,
    negative and infinite, data NaN and infinite, a cleared flag; the length-1 order unused in exposure 0."""
    rng = np.random.default_rng(seed)
    n_pix = int(sum(lengths))
    seg, perm = href.interleaved(lengths, seed=seed)
    model = 1.0 - 0.05 * rng.random((n_exp, n_trial, n_pix))
    data = 0.9 + 0.05 * rng.random((n_exp, n_pix))
    ivar = 1e4 * (0.1 + rng.random((n_exp, n_pix)))
    flag = np.ones((n_trial, n_pix), dtype=np.uint8)
    model[0, :, ::13] = np.nan
    model[1, n_trial - 1, 40:60] = np.nan
    ivar[0, 5], ivar[1, 6], ivar[0, 7] = 0.0, -1.0, np.inf
    data[1, 8], data[0, 9] = np.nan, np.inf
    flag[2, ::5] = 0
    ivar[0, perm[0]] = 0.0
    keep = np.ones(len(lengths), dtype=np.uint8)
    keep[3:4] = 0
    return model, data, ivar, flag, seg, perm, keep


def _write_case(path, model, data, ivar, flag, seg, perm, keep, cap_bytes):
    ints = lambda a: " ".join(str(int(v)) for v in np.asarray(a).ravel())
    vals = lambda a: " ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel())
    n_exp, n_trial, n_pix = model.shape
    with open(path, "w") as f:
        f.write("%d %d %d %d %d\n" % (n_exp, n_trial, n_pix, len(seg) - 1, cap_bytes))
        f.write("\n".join([ints(seg), ints(perm), ints(keep), ints(flag), vals(model), vals(data), vals(ivar)]) + "\n")


def _read_out(path, shape, n_seg):
    n_rec = shape[0] * shape[1] * n_seg
    rows = [l.split() for l in open(path).read().splitlines()]
    rec = rows[:n_rec]
    mom = np.array([[float.fromhex(v) for v in r[:7]] for r in rec]).reshape(shape + (n_seg, 7))
    nu = np.array([int(r[7]) for r in rec], dtype=np.int64).reshape(shape + (n_seg,))
    arg = np.array([float.fromhex(r[8]) for r in rec]).reshape(shape + (n_seg,))
    tot = np.array([[float.fromhex(v) for v in r] for r in rows[n_rec:]]).reshape(shape + (4,))
    return mom, nu, arg, tot


BUILDS = {"plain": ("-O2",),
          "sanitized": ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"),
          "small": ("-O2", "-DPROM_OD_TILE=4", "-DPROM_OD_TRIALS=2")}


# ---- the harness -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(BUILDS))
def test_harness_walks_every_index_and_matches_the_reference_bitwise(tmp_path, which):
    """Every (batch, exposure, trial group, order, tile, thread) of order_index.h with the kernel's text: every perm,
    model, data, flag and record index inside its array, every record and total written exactly once, in one batch and
    in batches of one trial group; the walked sums equal order_moments_f64 bit for bit, n_used exactly; the logarithm's
    argument, chi2, chi2_scaled and the count equal the numpy formulas bit for bit.  Also with a tile of 4 positions
    and 2 trials per workgroup."""
    exe = tmp_path / "order_host"
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *BUILDS[which], "-I" + CSRC, HOST, "-o", str(exe)],
                   check=True)
    tile, trials = (4, 2) if which == "small" else (32, 8)
    model, data, ivar, flag, seg, perm, keep = _case()
    n_seg = len(seg) - 1
    want_mom, want_nu = oref.order_moments_f64(model, data, ivar, flag, seg, perm, tile=tile)
    assert (want_nu[0, :, 0] == 0).all() and (want_nu[1, :, 0] == 1).all() and (want_nu < np.diff(seg)).any()
    want_tot = oref.totals_f64(want_mom, want_nu, keep)
    m0, m1, m2, m3, m4, m5 = (want_mom[..., i] for i in range(6))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = oref._ratio
        want_arg = (r(m5 - r(m2 * m2, m0), m0) - 2.0 * r(m4 - r(m1 * m2, m0), m0)) + r(m3 - r(m1 * m1, m0), m0)
    n_groups = -(-model.shape[1] // trials)
    for cap, batches in ((1 << 40, 1), (1, n_groups)):
        case, out = tmp_path / ("case_%d.txt" % batches), tmp_path / ("out_%d.txt" % batches)
        _write_case(case, model, data, ivar, flag, seg, perm, keep, cap)
        p = subprocess.run([str(exe), str(case), str(out)], capture_output=True, text=True)
        print(p.stdout, p.stderr)
        assert p.returncode == 0
        line = p.stdout.splitlines()[-1]
        assert line.startswith("tile=%d trials=%d " % (tile, trials))
        for name in ("perm_oor", "model_oor", "data_oor", "flag_oor", "rec_oor", "tot_oor", "visit_err"):
            assert " %s=0" % name in line, line
        assert " batches=%d " % batches in line
        assert " workgroups=%d " % (model.shape[0] * n_groups * n_seg) in line
        mom, nu, arg, tot = _read_out(out, model.shape[:2], n_seg)
        assert np.array_equal(nu, want_nu)
        assert np.array_equal(mom, want_mom)
        assert np.array_equal(arg, want_arg, equal_nan=True)
        assert np.array_equal(tot[..., 1:], want_tot[..., 1:], equal_nan=True)
        # (the host's logarithm is not numpy's: the helper's bound with the C library's ulp on both sides holds)
        assert np.all(np.abs(tot[..., 0] - want_tot[..., 0]) <= oref.loglike_bound(want_mom, want_nu, keep))


# ---- the references and their bounds -------------------------------------------------------------------------------
def test_float64_orders_of_addition_stay_inside_the_bound():
    """order_moments_f64 forwards and with every order's positions reversed against order_moments_ld: within
    (n + 4) u sum |term|, n the order's length; the print shows how far."""
    model, data, ivar, flag, seg, perm, _ = _case(lengths=(1, 2, 33, 513, 1100), n_trial=3)
    mld, nld, mag = oref.order_moments_ld(model, data, ivar, flag, seg, perm)
    n = np.diff(seg)[None, None, :]
    for reverse in (False, True):
        mom, nu = oref.order_moments_f64(model, data, ivar, flag, seg, perm, reverse=reverse)
        assert np.array_equal(nu, nld)
        frac = oref.moment_fraction(mom, mld, n, mag)
        print("float64 order moments, reverse=%s: %s of the bound" % (reverse, " ".join("%.4f" % f for f in frac)))
        assert np.all(frac <= 1.0)
    fwd = oref.order_moments_f64(model, data, ivar, flag, seg, perm)[0]
    assert not np.array_equal(fwd, mom)                  # (the reversal does change the roundings)


def test_one_tile_is_the_plain_butterfly_and_unused_positions_add_zero():
    rng = np.random.default_rng(2)
    model = rng.random((1, 1, 32))
    data, ivar = rng.random((1, 32)), 1.0 + rng.random((1, 32))
    seg, perm = href.one_segment(32)
    mom, nu = oref.order_moments_f64(model, data, ivar, None, seg, perm)
    t = ivar[0].copy()
    for m in (1, 2, 4, 8, 16):
        t = t + t[np.arange(32) ^ m]
    assert mom[0, 0, 0, 0] == t[0] and nu[0, 0, 0] == 32
    ivar[0, 3] = 0.0
    model[0, 0, 9] = np.nan
    mom2, nu2 = oref.order_moments_f64(model, data, ivar, None, seg, perm)
    assert nu2[0, 0, 0] == 30 and not np.isnan(mom2).any()
    empty = oref.order_moments_f64(np.full((1, 1, 32), np.nan), data, ivar, None, seg, perm)
    assert np.all(empty[0] == 0) and not np.signbit(empty[0]).any() and np.all(empty[1] == 0)


def test_totals_f64_gives_velocity_maps_numbers_for_one_order():
    """One order: the totals are VelocityMap's loglike, chi2 and chi2_scaled of the same moments bit for bit; keep = 0
    and n_used < 2 give zeros; a NaN statistic of an entering order reaches the total; several orders add in order."""
    from prometheus_amd import observation as obs
    model, data, ivar, flag, seg, perm, _ = _case(lengths=(300,), n_trial=4)
    mom, nu = oref.order_moments_f64(model, data, ivar, flag, seg, perm)
    vm = obs.VelocityMap(mom[:, :, 0], nu[:, :, 0], np.ones((2, 4, 1)))
    tot = oref.totals_f64(mom, nu, [1])
    assert np.array_equal(tot[..., 0], vm.loglike) and np.array_equal(tot[..., 1], vm.chi2)
    assert np.array_equal(tot[..., 2], vm.chi2_scaled) and np.array_equal(tot[..., 3], nu[:, :, 0])
    assert np.isfinite(tot).all() and np.all(tot[..., 0] != 0)
    assert np.all(oref.totals_f64(mom, nu, [0]) == 0)
    assert np.all(oref.totals_f64(mom, np.minimum(nu, 1), [1]) == 0)
    bad = mom.copy()
    bad[0, 0, 0, 0] = 0.0                                # m0 = 0: every ratio over it is NaN
    tb = oref.totals_f64(bad, nu, [1])
    assert np.isnan(tb[0, 0, 0]) and np.isfinite(tb[0, 0, 1:]).all() and np.isfinite(tb[1]).all()
    # the OrderMap shares VelocityMap's formulas, and its total runs over exposures and entering orders
    model, data, ivar, flag, seg, perm, keep = _case()
    mom, nu = oref.order_moments_f64(model, data, ivar, flag, seg, perm)
    om = obs.OrderMap(mom, nu, np.arange(len(keep)), keep.astype(bool))
    ll, scaled = oref.order_stats_f64(mom, nu)
    assert np.array_equal(om.loglike, ll, equal_nan=True) and np.array_equal(om.chi2_scaled, scaled, equal_nan=True)
    tot = oref.totals_f64(mom, nu, keep)
    en = oref.enters(nu, keep)
    assert not en[..., 3].any() and not en[0, :, 0].any() and en[..., 4].all()
    for i, stat in enumerate(("loglike", "chi2", "chi2_scaled")):
        assert np.allclose(om.total(stat), tot[..., i].sum(axis=0), rtol=1e-13, atol=0)
    every = om.total("chi2", keep=np.ones(len(keep), dtype=bool))
    assert np.all(every > om.total("chi2"))
    assert om.grid("chi2", 1, 11).shape == (2, 1, 11, len(keep)) and om.grid(every, 11, 1).shape == (11, 1)
    assert np.array_equal(om.grid("chi2", 1, 11)[:, 0], om.chi2)
    with pytest.raises(ValueError, match="OrderMap.grid"):
        om.grid("chi2", 2, 5)
    with pytest.raises(ValueError, match="OrderMap"):
        om.total("nope")
    with pytest.raises(ValueError):
        obs.OrderMap(mom, nu[..., :2], np.arange(len(keep)), keep)
    assert np.all(oref.loglike_bound(mom, nu, keep) >= 0)


# ---- Orders and Transit.expose(orders=...) without a device ----------------------------------------------------------
def test_orders_and_expose_refuse_before_touching_a_device(monkeypatch):
    from prometheus_amd import _native
    from prometheus_amd import observation as obs

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_native, "get_device", no_device)
    monkeypatch.setattr(_native, "device_count", no_device)
    tr = _bare_transit(20000, 3)
    ins = obs.Instrument(tr.wavelength[[300, 100, 200, 150]], resolving_power=140000.0)
    rows, a, F = np.array([[0, 1], [1, 2], [0, 2]]), np.full((3, 2), 0.5), np.ones((3, 4, 2))
    data, err = np.ones((3, 4)), np.full((3, 4), 1e-3)
    ex = obs.Exposures(ins, rows, a, F, data, err)
    od = obs.Orders(ex, [7, 3, 7, 3], keep=[True, False])
    hp = obs.HighPass(ex, obs.box_taps(1), orders=[7, 3, 7, 3])
    # the segments are HighPass' for the same labels
    assert od.n_seg == 2 and list(od.labels) == [3, 7] and list(od.keep) == [True, False]
    assert np.array_equal(od.seg_first, hp.seg_first) and np.array_equal(od.perm, hp.perm)
    assert od.perm.dtype == np.int32 and od.seg_first.dtype == np.int32 and od.exposures_key == ex.key
    assert obs.Orders(ex, [7, 3, 7, 3], keep=[1, 0]).key == od.key
    assert obs.Orders(ex, [7, 3, 7, 3]).key != od.key
    assert obs.Orders(ex, [7, 3, 3, 7], keep=[True, False]).key != od.key
    one = obs.Orders(ex, None)
    assert one.n_seg == 1 and list(one.keep) == [True] and np.array_equal(ins.order[one.perm], np.arange(4))
    for bad in (dict(orders=[0, 1, 0]), dict(orders=np.zeros((2, 2), dtype=int)), dict(keep=[True]),
                dict(keep=[True, False, True])):
        args = dict(orders=[7, 3, 7, 3], keep=None)
        args.update(bad)
        with pytest.raises(ValueError):
            obs.Orders(ex, **args)
    with pytest.raises(TypeError):
        obs.Orders(ex, [0.5, 1.0, 0.0, 1.0])
    with pytest.raises(TypeError):
        obs.Orders(ex, [7, 3, 7, 3], keep=[0.5, 1.0])
    with pytest.raises(TypeError):
        obs.Orders(ex, [7, 3, 7, 3], keep=[2, 0])
    with pytest.raises(TypeError):
        obs.Orders(ins, [7, 3, 7, 3])
    with pytest.raises(TypeError, match="observation.Orders"):
        tr.expose(ex, orders=[7, 3, 7, 3])
    with pytest.raises(TypeError, match="observation.Orders"):
        tr.expose(ex, orders=hp)
    other = obs.Exposures(ins, rows, a, F, data * 1.5, err)
    with pytest.raises(ValueError, match="Orders were made for other exposures"):
        tr.expose(other, orders=od)
    with pytest.raises(ValueError, match="HighPass was made for other exposures"):
        tr.expose(other, orders=obs.Orders(other, [7, 3, 7, 3]), highpass=hp)
    with pytest.raises(ValueError, match="not additive over wavelength partials"):    # the plain refusals stand
        tr.expose(ex, orders=od, highpass=hp, devices=[0, 1])
