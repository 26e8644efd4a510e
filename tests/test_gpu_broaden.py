"""Broadened spectra on the device (prom_broaden_set / prom_spectrum_broaden / prom_transit_broaden /
prom_transit_broadened, observation.Broadening and the ``broaden`` keyword of Transit.observe / velocity_map / expose)
against the references of tests/helpers/broaden_ref.py.  Marked ``gpu``.

Every comparison with broaden_f64 is bit for bit, the NaN pattern included: the definition names every rounding and
the order of the sums.  The comparison with the longdouble reference uses broaden_ref.bound, derived there from the
definition; the largest fraction of it reached is printed as ``BROADEN_ERR`` (profiles/broaden_errors.txt).
"""
import json
import os
import re

import numpy as np
import pytest

from helpers import broaden_ref as bref
from helpers import observe_ref as oref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
_hdr = open(os.path.join(REPO, "prometheus_amd", "csrc", "broaden_index.h")).read()
TILE = int(re.search(r"kBrBlock = (\d+)", _hdr).group(1))
GROUP = int(re.search(r"kBrPhases = (\d+)", _hdr).group(1))
E_ARG, E_STATE = "PROM_E_ARG", "PROM_E_STATE"
KMS = 1e5


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


def same(a, b):
    """Bit for bit, NaN for NaN (the sign of a zero included)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(np.where(np.isnan(a), 0.0, a).view(np.uint64), np.where(np.isnan(b), 0.0, b).view(np.uint64))


def broaden(dev, wav, R, K, b0, s):
    dev.broaden_set(K, b0, s)
    return dev.spectrum_broaden(wav, np.atleast_2d(R))


# ---- shapes ----------------------------------------------------------------------------------------------------------
def test_tile_and_group_constants():
    assert TILE == 256 and GROUP == 8          # the sizes below sit about these


@pytest.mark.parametrize("n_orb", [1, 3, 8, 9])
@pytest.mark.parametrize("n_wav", [1, 2, 255, 256, 257, 3 * 256 + 45])
def test_grid_sizes_and_row_counts(dev, n_wav, n_orb):
    """About a tile of outputs and about a group of rows (a full group, and a group plus one), on the non-uniform grid
    with 10x spacing jumps and duplicated points."""
    wav = oref.grid_nonuniform(n_wav)
    R = oref.spectrum(wav, n_orb, seed=n_wav + n_orb)
    K, b0, s = bref.kernel(33, -3 * KMS, 3 * KMS)
    assert same(broaden(dev, wav, R, K, b0, s), bref.broaden_f64(wav, R, K, b0, s))


@pytest.mark.parametrize("name", sorted(bref.designs()))
def test_kernels_and_grids(dev, name):
    """Kernels of 2, 33, 65 (with zero nodes) and 1025 nodes on grid_nonuniform(1500), supports of one point to more
    than a hundred; grid_coarse_fine with one-point supports and a tile across the spacing jump; grid_dyadic."""
    wav, K, b0, s = bref.designs()[name]
    R = oref.spectrum(wav, 3, seed=21)
    assert same(broaden(dev, wav, R, K, b0, s), bref.broaden_f64(wav, R, K, b0, s))


def test_unions_beyond_the_stage_take_the_global_path(dev):
    """+-160 km/s on grid_nonuniform(3000): no tile's union fits the stage (tests/test_broaden_cpu.py walks the same
    design on the host and finds no staged tile), so every output comes from global memory."""
    wav, K, b0, s = bref.wide_design()
    R = oref.spectrum(wav, 2, seed=22)
    assert same(broaden(dev, wav, R, K, b0, s), bref.broaden_f64(wav, R, K, b0, s))


def test_neighbouring_tiles_on_different_paths_agree_with_the_definition(dev):
    """+-10 km/s on a coarse/fine grid: the fine core's tiles fall back to global memory, the coarse wings' tiles are
    staged (the host harness counts both kinds on this design), nine rows make two groups; a narrow kernel on the same
    grid stages every tile.  Both equal the definition bit for bit, and the definition knows no paths: that is the same
    statement as comparing one output across two path assignments, so a staged output does not depend on what its
    neighbours do."""
    wav, K, b0, s = bref.mixed_design()
    R = oref.spectrum(wav, 9, seed=23)
    assert same(broaden(dev, wav, R, K, b0, s), bref.broaden_f64(wav, R, K, b0, s))
    K, b0, s = bref.kernel(33, -1 * KMS, 1 * KMS)
    assert same(broaden(dev, wav, R, K, b0, s), bref.broaden_f64(wav, R, K, b0, s))


def test_a_pure_shift_leaves_nan_at_one_end(dev):
    """A kernel over +2 .. +4 km/s does not cover beta = 0: the outputs whose whole support lies beyond the end of the
    grid are NaN (den = 0 over an empty support), the rest are the definition's bits."""
    wav, K, b0, s = bref.shift_design()
    R = oref.spectrum(wav, 2, seed=24)
    got, want = broaden(dev, wav, R, K, b0, s), bref.broaden_f64(wav, R, K, b0, s)
    n_nan = int(np.isnan(want[0]).sum())
    print("BROADEN_SHIFT outputs without a support: %d of %d" % (n_nan, len(wav)))
    assert 10 <= n_nan <= 100 and np.array_equal(np.isnan(want[0]), np.isnan(want[1]))
    # gas moving away reads R bluewards of the output: the blue end of the grid has nothing to read
    assert np.isnan(want[0][:n_nan // 2]).all() and not np.isnan(want[0][-200:]).any()
    assert same(got, want)


def test_nan_reaches_exactly_the_outputs_whose_support_holds_it(dev):
    """A NaN planted in one row, at a point that some outputs see through a node of weight zero: exactly the outputs
    whose support holds it are NaN, in that row only."""
    wav, K, b0, s = bref.designs()["nonuniform n_k=65 random"]
    assert (K == 0.0).sum() > 10
    R = oref.spectrum(wav, 3, seed=25)
    R[1, 640] = np.nan
    R[2, 5] = np.inf                                  # (what IEEE gives: inf, or NaN under a zero weight)
    got = broaden(dev, wav, R, K, b0, s)
    holds = np.array([a <= 640 < b for a, b, _ in (bref.support(wav, w, len(K), b0, s) for w in range(len(wav)))])
    assert holds.sum() > 10
    assert np.array_equal(np.isnan(got[1]), holds) and not np.isnan(got[0]).any()
    assert same(got, bref.broaden_f64(wav, R, K, b0, s))


def test_a_row_does_not_depend_on_its_neighbours_or_on_the_call(dev):
    """A row alone, rows permuted, n_orb changed (within a group, across groups) and a second call: the same bits."""
    wav, K, b0, s = bref.designs()["nonuniform n_k=33"]
    R = oref.spectrum(wav, 11, seed=26)
    full = broaden(dev, wav, R, K, b0, s)
    assert same(dev.spectrum_broaden(wav, R), full)
    for o in (0, 7, 8, 10):
        assert same(dev.spectrum_broaden(wav, R[o:o + 1])[0], full[o])
    perm = np.random.default_rng(3).permutation(11)
    assert same(dev.spectrum_broaden(wav, R[perm]), full[perm])
    assert same(dev.spectrum_broaden(wav, R[3:10]), full[3:10])
    assert dev.broaden_kernel_ms(2) > 0.0
    assert same(dev.spectrum_broaden(wav, R), full)


def test_device_stays_inside_the_bound_of_the_longdouble_reference(dev):
    """Every shared design against broaden_ld: inside the bound derived from the definition."""
    worst = 0.0
    for name, (wav, K, b0, s) in sorted(bref.designs().items()):
        R = oref.spectrum(wav, 2, seed=27)
        got = broaden(dev, wav, R, K, b0, s)
        ref, cnt, rmax, gsum, qsum = bref.broaden_ld(wav, R, K, b0, s)
        tol = bref.bound(K, b0, s, cnt, rmax, gsum, qsum)
        assert np.array_equal(np.isnan(got), np.isnan(ref.astype(np.float64))), name
        ok = ~np.isnan(got)
        err = np.abs(got.astype(np.longdouble) - ref)[ok].astype(np.float64)
        frac = float((err / tol[ok]).max())
        print("BROADEN_ERR %-28s supports %d..%d  %.4f of the bound" % (name, cnt.min(), cnt.max(), frac))
        assert np.all(err <= tol[ok]), (name, frac)
        worst = max(worst, frac)
    print("BROADEN_ERR largest fraction %.4f" % worst)


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors():
    from prometheus_amd import _native
    wav = oref.grid_nonuniform(100)
    R = oref.spectrum(wav, 2)
    K, b0, s = bref.kernel(9, -3 * KMS, 3 * KMS)
    d = _native.Device(0)
    try:
        for call in (lambda: d.spectrum_broaden(wav, R), d.transit_broaden, d.transit_broadened, d.broaden_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):      # no kernel on the context
                call()
        bad_K = [K[:1], np.ones(1026), np.where(np.arange(9) == 4, -1e-9, K), np.where(np.arange(9) == 4, np.nan, K),
                 np.where(np.arange(9) == 4, np.inf, K), np.zeros(9)]
        for Kb in bad_K:
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.broaden_set(Kb, b0, s)
        for b0b, sb in ((np.nan, s), (np.inf, s), (b0, 0.0), (b0, -s), (b0, np.nan), (b0, np.inf)):
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.broaden_set(K, b0b, sb)
        with pytest.raises(_native.NativeError, match=E_STATE):          # a failed set leaves no kernel behind
            d.spectrum_broaden(wav, R)
        d.broaden_set(K, b0, s, key="k")
        assert d.broaden_key == "k"
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.transit_broaden()                                           # no run yet
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.transit_broadened()
        for wb in (wav[::-1], np.where(np.arange(100) == 50, np.nan, wav), wav - wav[0], -wav[::-1],
                   np.where(np.arange(100) == 99, np.inf, wav)):
            with pytest.raises(_native.NativeError, match=E_ARG):        # descending, NaN, a zero, negative, infinite
                d.spectrum_broaden(wb, R)
        with pytest.raises(ValueError):
            d.spectrum_broaden(wav, R[:, :50])
        out = d.spectrum_broaden(wav, R)
        assert out.shape == R.shape and same(out, bref.broaden_f64(wav, R, K, b0, s))
        assert d.broaden_kernel_ms(2) > 0.0
        d.broaden_drop()                                                  # n_k = 0 drops the kernel
        assert d.broaden_key is None
        for call in (lambda: d.spectrum_broaden(wav, R), d.broaden_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):
                call()
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
def test_transit_broaden_end_to_end(name, monkeypatch):
    """The reduced golden problems (C1 with three phases), 40 pixels about Na D2 in two orders, a 33-node ring at
    3 km/s with a wind.  Transit.broadened is prom_spectrum_broaden of sumOverChords' R; expose, expose with high-pass,
    filter and orders, velocity_map and observe with ``broaden`` are their spectrum entries on R_b; all bit for bit.
    A run without ``broaden`` gives the plain results again and leaves no R_b; shards raise ValueError; a second call
    uploads nothing."""
    from prometheus_amd import _native
    from prometheus_amd import constants as const
    from prometheus_amd import lightcurve as lc
    from prometheus_amd import observation as obs
    d = np.load(os.path.join(G, "transit_" + name + ".npz"))
    cfg = json.loads(str(d["config"]))
    if cfg["Grids"]["orbphase_steps"] < 2:      # C1 has one phase and exposure_taps needs a bracket: C1 with three
        cfg["Grids"].update(orbphase_border=0.02, orbphase_steps=3)
    tr = _product_transit(cfg)
    R = np.array(tr.sumOverChords(devices=[0]))
    wav = np.asarray(tr.wavelength)
    n_orb = R.shape[0]
    orb = tr.spatialGrid.constructOrbphaseAxis()
    dev = _native.get_device(0)
    bk = obs.Broadening(*obs.rotation_kernel(3e5, n=33, wind=-1e5))
    # R_b itself
    Rb = tr.broadened(bk, devices=[0])
    assert dev.broaden_key == bk.key
    want_Rb = dev.spectrum_broaden(wav, R)
    assert same(Rb, want_Rb) and same(Rb, bref.broaden_f64(wav, R, bk.K, bk.b0, bk.s))
    assert not same(Rb, R) and same(dev.transit_result(), R)             # (the result stays the unbroadened R)
    assert dev.broaden_kernel_ms(2) > 0.0                                 # (the launch on the run's own buffers)
    # exposures
    px = lc.NA_D2 + 5e-10 * (np.arange(40) - 19.5)
    ins = obs.Instrument(px[::-1], resolving_power=140000.0, truncate=5.0)
    base = obs.planet_frame_shifts(tr.planet, orb)
    Kp = np.sqrt(const.G * tr.planet.hostStar.M / tr.planet.a)
    planted = tr.observe(ins, devices=[0])
    err = np.full(planted.model.shape, 1e-4)
    data = np.where(np.isfinite(planted.model), planted.model, np.nan) * (1.0 + 1e-3)
    step = orb[1] - orb[0]
    mid = np.concatenate([0.5 * (orb[:-1] + orb[1:]), [orb[1]]])
    width = np.concatenate([np.full(n_orb - 1, 0.9 * step), [1.9 * step]])
    rows, a, F = obs.exposure_taps(orb, base, mid, width, n_sub=3, Kp=Kp * np.array([0.9, 1.0]), Vsys=[0.0, 2e5])
    ex = obs.Exposures(ins, rows, a, F, np.resize(data, (len(mid), 40)), np.resize(err, (len(mid), 40)))
    plain = tr.expose(ex, return_model=True, devices=[0])
    with pytest.raises(_native.NativeError, match=E_STATE):              # that run left no R_b
        dev.transit_broadened()
    with pytest.raises(_native.NativeError, match=E_STATE):              # ... and the new set nothing to repeat: the
        dev.broaden_kernel_ms(2)                                          # buffers the last launch read may have moved
    out = tr.expose(ex, return_model=True, devices=[0], broaden=bk)
    mom, nu, model = dev.spectrum_expose(wav, Rb, model=True)
    assert same(out.moments, mom) and np.array_equal(out.n_used, nu) and same(ins.sort(out.model), model)
    assert not same(out.moments, plain.moments)
    # a second call: nothing is uploaded, the same bits
    calls = []
    for fn in ("observe_set", "expose_set", "broaden_set"):
        monkeypatch.setattr(dev, fn, lambda *a, _fn=fn, **k: calls.append(_fn))
    again = tr.expose(ex, return_model=True, devices=[0], broaden=bk)
    assert calls == [] and same(again.moments, out.moments) and same(again.model, out.model)
    monkeypatch.undo()
    # with the high-pass, the filter and the orders
    labels = np.arange(40) // 20
    hp = obs.HighPass(ex, obs.box_taps(3), orders=labels)
    dt = obs.Detrend(ex, 1.0 + 0.1 * np.arange(len(mid), dtype=np.float64)[:, None])
    od = obs.Orders(ex, labels)
    full = tr.expose(ex, return_model=True, devices=[0], highpass=hp, detrend=dt, orders=od, broaden=bk)
    mom, nu, rm, rn, tot, model = dev.spectrum_expose_orders(wav, Rb, highpass=True, detrend=True, model=True)
    assert same(full.moments, mom) and np.array_equal(full.n_used, nu) and same(ins.sort(full.model), model)
    assert same(full.by_order.moments, rm) and np.array_equal(full.by_order.n_used, rn)
    assert same(full.order_totals.loglike, tot[..., 0]) and same(full.order_totals.chi2, tot[..., 1])
    unbroadened = tr.expose(ex, devices=[0], highpass=hp, detrend=dt, orders=od)
    assert not same(unbroadened.moments, full.moments)
    # velocity_map and observe
    ob = obs.Observation(ins, n_orb, None, data, err)
    Fv = obs.trial_factors(base, [-2e5, 0.0, 2e5])
    vm = tr.velocity_map(ob, Fv, devices=[0], broaden=bk)
    mom, nu = dev.spectrum_vmap(wav, Rb)
    assert same(vm.moments, mom) and np.array_equal(vm.n_used, nu)
    assert not same(vm.moments, tr.velocity_map(ob, Fv, devices=[0]).moments)
    seen = tr.observe(ob, devices=[0], broaden=bk, return_spectrum=True)
    num, den, chi2, n_used = dev.spectrum_observe(wav, Rb, partials=True, chi2=True)
    assert same(ins.sort(seen.model), obs.model_spectrum(num, den)) and same(seen.chi2, chi2)
    assert np.array_equal(seen.n_used, n_used) and same(seen.spectrum, R)
    # R_b is current after that call: the observation may only ask for the whole grid
    for edges in ((0.5 * wav[0], np.nan), (np.nan, 2.0 * wav[-1])):
        with pytest.raises(_native.NativeError, match=E_ARG):
            dev.transit_observe(*edges)
    # the next run without broaden: the plain results again, and no R_b
    back = tr.expose(ex, return_model=True, devices=[0])
    assert same(back.moments, plain.moments) and same(back.model, plain.model)
    with pytest.raises(_native.NativeError, match=E_STATE):
        dev.transit_broadened()
    # shards and chunks
    for call in (lambda **k: tr.expose(ex, broaden=bk, **k), lambda **k: tr.velocity_map(ob, Fv, broaden=bk, **k),
                 lambda **k: tr.observe(ob, broaden=bk, **k), lambda **k: tr.broadened(bk, **k)):
        with pytest.raises(ValueError, match="wavelength shard"):
            call(devices=[0, 1])
        if len(wav) > 4096:
            with pytest.raises(ValueError, match="wavelength shard"):
                call(devices=[0], max_memory_gb=1e-9)


# ---- a planted rotation ------------------------------------------------------------------------------------------------
def test_a_planted_rotation_is_found(dev):
    """A narrow line on a uniform 0.3 km/s grid of 600 points, 120 pixels at a resolving power of 140,000.  The data
    are the device's own model with rotation_kernel(4 km/s); trials of 1, 2.5, 4, 5.5 and 7 km/s give chi2 exactly 0
    at 4 and > 0 elsewhere, and loglike peaks at 4."""
    from prometheus_amd import constants as const
    from prometheus_amd import observation as obs
    lam0 = 5890e-8
    wav = lam0 * (1.0 + (np.arange(600) - 300) * (0.3e5 / const.c))
    R = (1.0 - 0.3 * np.exp(-0.5 * ((wav / lam0 - 1.0) * const.c / 0.8e5) ** 2))[None, :]
    px = lam0 * (1.0 + np.linspace(-60e5, 60e5, 120) / const.c)
    ins = obs.Instrument(px, resolving_power=140000.0, truncate=5.0)
    trials = [1e5, 2.5e5, 4e5, 5.5e5, 7e5]

    def model_of(v_eq):
        b = obs.Broadening(*obs.rotation_kernel(v_eq))
        dev.broaden_set(b.K, b.b0, b.s)
        return dev.spectrum_broaden(wav, R)

    dev.observe_set(ins.lam, ins.sig, ins.truncate, 1)
    num, den, _, _ = dev.spectrum_observe(wav, model_of(4e5))
    data = obs.model_spectrum(num, den)
    assert np.isfinite(data).all() and data.min() < 0.95
    ivar = np.full(data.shape, 1e8)
    dev.observe_set(ins.lam, ins.sig, ins.truncate, 1, None, data, ivar)
    dev.vmap_set(np.ones((1, 1)))
    chi2, loglike = [], []
    for v in trials:
        Rb = model_of(v)
        _, _, c2, nu = dev.spectrum_observe(wav, Rb, partials=False, chi2=True)
        assert nu[0] == 120
        chi2.append(float(c2[0]))
        mom, n_used = dev.spectrum_vmap(wav, Rb)
        loglike.append(float(obs.VelocityMap(mom, n_used, np.ones((1, 1))).loglike[0, 0]))
    print("BROADEN_PLANTED chi2 %s loglike %s" % (chi2, loglike))
    assert chi2[2] == 0.0 and all(c > 0.0 for i, c in enumerate(chi2) if i != 2)
    assert chi2[0] > chi2[1] and chi2[4] > chi2[3]
    assert int(np.argmax(loglike)) == 2 and not np.isnan(loglike).any()
