"""Velocity maps on the device (prom_vmap_set / prom_spectrum_vmap / prom_transit_vmap, Transit.velocity_map) against
the longdouble reference of tests/helpers/vmap_ref.py.  Marked ``gpu``.

Tolerances (vmap_ref.bounds; derived from the definition, not from the kernel), with u = 2^-53, eps =
observe_ref.m_tolerance(k, n_max) the bound on M and n = n_used; data and model are positive, so the sums of m0 .. m5
have non-negative terms: m0, m2, m5 within (n + 4) u relative; m1, m4 within eps + (n + 4) u; m3 within
2 eps + (n + 4) u; m6 within 2 eps sqrt(m6 m3) + eps^2 m3 + (n + 4) u m6 absolute (a term (M - d)^2 moves by at most
2 |M - d| eps |M| + eps^2 M^2; Cauchy-Schwarz over the used pixels).  n_used is exact.

The independence clause of the definition (a trial's numbers depend on the spectrum, the observation and its factor
only) is tested bitwise.  Every test prints its largest error per moment as a fraction of its bound (``VMAP_ERR``;
profiles/vmap_errors.txt).
"""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import observe_ref as ref
from helpers import vmap_plan as plan
from helpers import vmap_ref as vref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
LD = np.longdouble
_csrc = os.path.join(REPO, "prometheus_amd", "csrc")
TILE = int(re.search(r"kObsTile = (\d+)", open(os.path.join(_csrc, "obs_index.h")).read()).group(1))
_hdr = open(os.path.join(_csrc, "vmap_index.h")).read()
STAGE = int(re.search(r"#define PROM_VM_STAGE (\d+)", _hdr).group(1))
C = int(re.search(r"#define PROM_VM_CHUNK (\d+)", _hdr).group(1))
T = int(re.search(r"#define PROM_VM_TRIALS (\d+)", _hdr).group(1))
E_ARG, E_STATE = "PROM_E_ARG", "PROM_E_STATE"


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


def kms(v):
    return vref.doppler(1e5 * np.asarray(v, dtype=np.float64))


def positive_data(shape, seed):
    rng = np.random.default_rng(seed)
    return 0.9 + 0.05 * rng.random(shape), 1e4 * (0.1 + rng.random(shape))


def vmap(dev, wav, R, lam, sig, k, F, data, ivar):
    R = np.atleast_2d(R)
    dev.observe_set(lam, sig, k, R.shape[0], None, data, ivar)
    dev.vmap_set(F)
    return dev.spectrum_vmap(wav, R)


def report(name, frac):
    print("VMAP_ERR %s %s of the bounds (m0 .. m6)" % (name, " ".join("%.4f" % f for f in frac)))


def check(name, out, want, k):
    """Device (moments, n_used) against the reference's: n_used exact, equal NaN masks, every moment within its
    bound.  Returns the largest error per moment as a fraction of its bound."""
    mom, nu = out
    rmom, rnu, _, n_max = want
    assert mom.shape == rmom.shape and nu.dtype == np.int64
    assert np.array_equal(nu, rnu), name
    assert np.array_equal(np.isnan(mom), np.isnan(rmom.astype(np.float64))), name
    assert np.all(mom[rnu == 0] == 0), name
    frac = vref.fractions(mom, rmom, rnu, k, n_max)
    report(name, frac)
    assert np.all(frac <= 1.0), (name, frac)
    return frac


def case(dev, name, wav, n_orb, lam, sig, F, k=5.0, seed=3):
    R = ref.spectrum(wav, n_orb)
    data, ivar = positive_data((n_orb, len(lam)), seed)
    F = np.ascontiguousarray(np.broadcast_to(F, (n_orb, np.shape(F)[-1])) * (1.0 + 1e-5 * np.arange(n_orb))[:, None])
    out = vmap(dev, wav, R, lam, sig, k, F, data, ivar)
    return check(name, out, vref.vmap(wav, R, lam, sig, k, F, data, ivar), k)


# ---- smallest shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_orb", [1, 3])
@pytest.mark.parametrize("n_wav", [1, 2, 63, 64, 65, STAGE - 1, STAGE, STAGE + 1])
def test_smallest_grids(dev, n_wav, n_orb):
    """A non-uniform grid with 10x spacing jumps inside the supports and duplicated points, 5 pixels (one duplicated,
    some beyond the ends), 3 trials."""
    wav = ref.grid_nonuniform(n_wav)
    lam = ref.pixels_over(wav, 5)
    case(dev, "grids n_wav=%d n_orb=%d" % (n_wav, n_orb), wav, n_orb, lam, np.full(5, 2.5e-10), kms([-3.0, 0.0, 4.0]))


@pytest.mark.parametrize("n_orb", [1, 3])
@pytest.mark.parametrize("n_pix", [1, TILE - 1, TILE, TILE + 1, TILE * C - 1, TILE * C, TILE * C + 1])
def test_smallest_pixel_counts(dev, n_pix, n_orb):
    """About a tile and about a chunk (the second workgroup along the pixels starts at 32 C), 2 trials; widths too
    small to reach a node among them."""
    wav = ref.grid_nonuniform(1500)
    lam = ref.pixels_over(wav, n_pix)
    sig = np.full(n_pix, 2.5e-10)
    sig[::7] = 1e-13
    case(dev, "pixels n_pix=%d n_orb=%d" % (n_pix, n_orb), wav, n_orb, lam, sig, kms([-2.0, 2.0]))


@pytest.mark.parametrize("n_orb", [1, 3])
@pytest.mark.parametrize("n_trial", [1, T - 1, T, T + 1, 2 * T + 1])
def test_smallest_trial_counts(dev, n_trial, n_orb):
    wav = ref.grid_nonuniform(1500)
    lam = ref.pixels_over(wav, TILE + 1)
    case(dev, "trials n_trial=%d n_orb=%d" % (n_trial, n_orb), wav, n_orb, lam, np.full(TILE + 1, 2.5e-10),
         kms(np.linspace(-8.0, 8.0, 2 * T + 1)[:n_trial]))


# ---- independence ----------------------------------------------------------------------------------------------
def _independence_design():
    """A long fine core, 70 pixels in its upper part at R = 140,000 (supports of about 180 points), 2 phases,
    2 T + 1 trials 2 km/s apart."""
    wav = ref.grid_coarse_fine(3000, 200)
    R = ref.spectrum(wav, 2)
    lam = wav[200 + 2500] + 1e-10 * (np.arange(2 * TILE + 6) - 20.0)
    sig = lam / (140000.0 * 2.3548)
    F = np.stack([kms(np.linspace(-16.0, 16.0, 2 * T + 1)), kms(np.linspace(-16.0, 16.0, 2 * T + 1) + 3.0)])
    data, ivar = positive_data((2, len(lam)), 7)
    return wav, R, lam, sig, 5.0, F, data, ivar


@pytest.fixture(scope="module")
def independent(dev):
    d = _independence_design()
    return d, vmap(dev, *d)


def same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


def test_base_table_is_right_and_repeats_bitwise(dev, independent):
    (wav, R, lam, sig, k, F, data, ivar), base = independent
    check("independence base", base, vref.vmap(wav, R, lam, sig, k, F, data, ivar), k)
    assert same(vmap(dev, wav, R, lam, sig, k, F, data, ivar), base)
    assert same(dev.spectrum_vmap(wav, R), base)


def test_columns_permuted_and_alone_bitwise(dev, independent):
    (wav, R, lam, sig, k, F, data, ivar), base = independent
    dev.observe_set(lam, sig, k, 2, None, data, ivar)
    perm = np.random.default_rng(12).permutation(F.shape[1])
    dev.vmap_set(np.ascontiguousarray(F[:, perm]))
    out = dev.spectrum_vmap(wav, R)
    assert same(out, (base[0][:, perm], base[1][:, perm]))
    for j in range(F.shape[1]):
        dev.vmap_set(np.ascontiguousarray(F[:, j:j + 1]))
        out = dev.spectrum_vmap(wav, R)
        assert same(out, (base[0][:, j:j + 1], base[1][:, j:j + 1])), j


def test_wide_columns_force_global_reads_bitwise(dev, independent, tmp_path):
    """A -300 or +300 km/s column at the head of every group of T: with -300 the stage starts 2,500 points below the
    other trials' supports, which are then read from global memory (counted by the host harness); the other columns'
    numbers do not move."""
    (wav, R, lam, sig, k, F, data, ivar), base = independent
    cols, keep = [], []
    for j in range(F.shape[1]):
        if len(cols) % T == 0:
            cols.append(np.full(2, kms(-300.0 if (len(cols) // T) % 2 == 0 else 300.0)))
        keep.append(len(cols))
        cols.append(F[:, j])
    Fw = np.ascontiguousarray(np.stack(cols, axis=1))
    plan.compile_harness(tmp_path / "libvmap_host.so")
    L = plan.bind(tmp_path / "libvmap_host.so")
    before, _ = plan.audit(L, wav, lam, sig, k, F, supports=False)
    after, _ = plan.audit(L, wav, lam, sig, k, Fw, supports=False)
    assert before["fallback"] == 0 and after["fallback"] >= 2 * len(lam) * (T - 1) and after["staged"] > 0
    dev.observe_set(lam, sig, k, 2, None, data, ivar)
    dev.vmap_set(Fw)
    out = dev.spectrum_vmap(wav, R)
    assert same((out[0][:, keep], out[1][:, keep]), base)
    wide = [j for j in range(Fw.shape[1]) if j not in keep]
    check("independence wide columns", (out[0][:, wide], out[1][:, wide]),
          vref.vmap(wav, R, lam, sig, k, Fw[:, wide], data, ivar), k)


_BATCHED = """
import hashlib, json, sys
sys.path.insert(0, %r)
import numpy as np
from prometheus_amd import _native
from test_gpu_vmap import _independence_design, vmap
mom, nu = vmap(_native.get_device(0), *_independence_design())
print(json.dumps({"mom": hashlib.sha256(mom.tobytes()).hexdigest(), "nu": hashlib.sha256(nu.tobytes()).hexdigest()}))
"""


def test_batches_under_a_small_scratch_cap_bitwise(independent):
    """PROM_VMAP_SCRATCH_MB is read at context creation, so the case runs in a process of its own: 0.0001 MB (104
    bytes) is below one trial group's records, so every group is a batch of its own: three batches."""
    _, base = independent
    env = dict(os.environ, PROM_VMAP_SCRATCH_MB="0.0001", PROM_DEBUG="1")
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _BATCHED % os.path.join(REPO, "tests")],
                       env=env, cwd=REPO, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = [l for l in p.stderr.splitlines() if "velocity map" in l]
    assert lines and "3 groups, 3 batches of up to 1 groups" in lines[-1], p.stderr[-2000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert out["mom"] == hashlib.sha256(base[0].tobytes()).hexdigest()
    assert out["nu"] == hashlib.sha256(base[1].tobytes()).hexdigest()


# ---- consistency with the observation --------------------------------------------------------------------------
def test_chi2_is_the_observation_chi2(dev, independent):
    """Three columns against prom_spectrum_observe with f = F[:, j]: n_used equal, chi2 within the bound of m6 (the two
    kernels add a support's points in different orders)."""
    (wav, R, lam, sig, k, F, data, ivar), base = independent
    rmom, rnu, _, n_max = vref.vmap(wav, R, lam, sig, k, F[:, [0, T, 2 * T]], data, ivar)
    bound = vref.bounds(rmom, rnu, k, n_max)[..., 6]
    worst = 0.0
    for i, j in enumerate((0, T, 2 * T)):
        dev.observe_set(lam, sig, k, 2, F[:, j], data, ivar)
        _, _, c2, nu = dev.spectrum_observe(wav, R, partials=False, chi2=True)
        assert np.array_equal(nu, base[1][:, j])
        worst = max(worst, float(np.max(np.abs(c2 - base[0][:, j, 6]) / bound[:, i])))
    print("VMAP_ERR chi2 against prom_spectrum_observe %.4f of the m6 bound" % worst)
    assert worst <= 1.0


# ---- edge cases ------------------------------------------------------------------------------------------------
def test_trials_off_the_grid_give_zeros(dev):
    wav = ref.grid_nonuniform(600)
    R = ref.spectrum(wav, 2)
    lam = ref.pixels_over(wav, TILE + 3)
    data, ivar = positive_data((2, len(lam)), 1)
    F = np.array([[2.0, 0.5, 1.0], [0.5, 1.0, 3.0]])
    mom, nu = vmap(dev, wav, R, lam, np.full(len(lam), 2.5e-10), 5.0, F, data, ivar)
    off = np.array([[True, True, False], [True, False, True]])
    assert np.all(nu[off] == 0) and np.all(mom[off] == 0) and np.all(nu[~off] > 0)
    assert not np.isnan(mom).any()


def test_nan_in_r_reaches_exactly_its_trials(dev):
    wav = ref.grid_nonuniform(800)
    R = ref.spectrum(wav, 3)
    R[1, 417] = np.nan
    lam = np.sort(np.concatenate([ref.pixels_over(wav, 2 * TILE - 2), [wav[417] * 1.01, wav[417] * 1.01 + 1e-10]]))
    sig = np.full(len(lam), 2.5e-10)
    data, ivar = positive_data((3, len(lam)), 2)
    # a factor of 1 / 1.01 brings the two far pixels onto the NaN; 0.97 moves every pixel away from it and off the grid
    F = np.tile(np.array([1.0, 1.0 + 1e-5, 1.0 / 1.01, 0.97, 1.0 - 2e-5]), (3, 1))
    want = vref.vmap(wav, R, lam, sig, 5.0, F, data, ivar)
    hit = np.isnan(want[0][..., 1].astype(np.float64))
    assert hit[1, :3].all() and not hit[1, 3] and not hit[0].any() and not hit[2].any()
    mom, nu = vmap(dev, wav, R, lam, sig, 5.0, F, data, ivar)
    for i in (1, 3, 4, 6):
        assert np.array_equal(np.isnan(mom[..., i]), hit), i
    assert np.isfinite(mom[..., [0, 2, 5]]).all()
    check("test_nan_in_r_reaches_exactly_its_trials", (mom, nu), want, 5.0)
    # with the pixels on the NaN masked, the trials whose other pixels stay clear of it are finite again
    ivar2 = ivar.copy()
    ivar2[1] = np.where(np.abs(lam - wav[417]) < 5e-9, 0.0, ivar[1])
    want2 = vref.vmap(wav, R, lam, sig, 5.0, F, data, ivar2)
    out2 = vmap(dev, wav, R, lam, sig, 5.0, F, data, ivar2)
    assert not np.isnan(out2[0][1, [0, 1, 4]]).any() and np.isnan(out2[0][1, 2, 6])
    check("test_nan_in_r_reaches_exactly_its_trials masked", out2, want2, 5.0)


def test_masked_pixels_are_excluded(dev):
    """ivar 0, negative, infinite and NaN, ivar from an infinite err (1 / inf^2 = 0), NaN and infinite data."""
    wav = ref.grid_nonuniform(900)
    n_orb = 2
    R = ref.spectrum(wav, n_orb)
    lam = ref.pixels_over(wav, 2 * TILE + 3, outside=False)
    sig = np.full(len(lam), 2.5e-10)
    data, ivar = positive_data((n_orb, len(lam)), 4)
    err = np.full(ivar.shape, 1e-2)
    err[0, 6] = np.inf
    with np.errstate(divide="ignore"):
        ivar = np.where(np.isinf(err), 1.0 / (err * err), ivar)
    assert ivar[0, 6] == 0.0
    ivar[0, 3], ivar[0, 12], ivar[1, 5], ivar[1, 9] = 0.0, -1.0, np.nan, np.inf
    data[1, 8], data[1, 20] = np.nan, np.inf
    F = np.tile(kms([-2.0, 0.0, 2.0]), (n_orb, 1))
    want = vref.vmap(wav, R, lam, sig, 5.0, F, data, ivar)
    assert np.all(want[1][0] == len(lam) - 3) and np.all(want[1][1] == len(lam) - 4)
    check("test_masked_pixels_are_excluded", vmap(dev, wav, R, lam, sig, 5.0, F, data, ivar), want, 5.0)


def test_truncation_boundary_is_inclusive(dev):
    """Dyadic grid, pixels on nodes, a trial factor of exactly 1, k = 4 and sig = 2 spacings: c is exactly 8 spacings,
    the points at +-8 spacings are in (17 points); with sig one ulp smaller they are out (15).  The two references
    differ by far more than the bounds, so the check tells 17 from 15."""
    wav = ref.grid_dyadic(400)
    R = ref.spectrum(wav, 2)
    lam = wav[[8, 9, 100, 101, 250, 390, 391]]
    data, ivar = positive_data((2, len(lam)), 5)
    F = np.array([[1.0, 1.0 + 2.0 ** -20], [1.0, 1.0]])
    wants = []
    for sig0, n in ((2 * ref.DYADIC_STEP, 17), (np.nextafter(2 * ref.DYADIC_STEP, 0.0), 15)):
        sig = np.full(len(lam), sig0)
        assert np.all(ref.observe(wav, R, lam, sig, 4.0, F[:, 0])[2] == n)
        wants.append(vref.vmap(wav, R, lam, sig, 4.0, F, data, ivar))
        check("test_truncation_boundary_is_inclusive[%d]" % n, vmap(dev, wav, R, lam, sig, 4.0, F, data, ivar),
              wants[-1], 4.0)
    b = vref.bounds(wants[0][0], wants[0][1], 4.0, 17)
    assert np.all(np.abs(wants[0][0][:, 0, 1] - wants[1][0][:, 0, 1]).astype(np.float64) > 1e3 * b[:, 0, 1])


# ---- argument and state errors ---------------------------------------------------------------------------------
def test_errors():
    from prometheus_amd import _native
    wav = ref.grid_nonuniform(100)
    R = ref.spectrum(wav, 2)
    lam, sig = wav[[10, 20, 30]], np.full(3, 2e-10)
    data, ivar = positive_data((2, 3), 6)
    F = np.tile(kms([-2.0, 0.0, 2.0]), (2, 1))
    d = _native.Device(0)
    try:
        for call in (lambda: d.spectrum_vmap(wav, R), d.transit_vmap, lambda: d.vmap_set(F), d.vmap_kernel_ms):
            with pytest.raises(_native.NativeError, match=E_STATE):      # no observation on the context
                call()
        d.observe_set(lam, sig, 5.0, 2)
        with pytest.raises(_native.NativeError, match=E_STATE):          # an observation without data
            d.vmap_set(F)
        d.observe_set(lam, sig, 5.0, 2, None, data, ivar)
        with pytest.raises(_native.NativeError, match=E_STATE):          # another n_orb than the observation's
            d.vmap_set(np.tile(F[:1], (3, 1)))
        for bad in (0.0, -1.0, np.nan, np.inf):
            Fb = F.copy()
            Fb[1, 2] = bad
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.vmap_set(Fb)
        with pytest.raises(_native.NativeError, match=E_ARG):            # n_trial = 0
            d.vmap_set(np.zeros((2, 0)))
        with pytest.raises(_native.NativeError, match=E_STATE):          # a failed set leaves no table behind
            d.spectrum_vmap(wav, R)
        d.vmap_set(F, key="k")
        assert d.vmap_key == "k"
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.transit_vmap()                                             # no run yet
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_vmap(wav, ref.spectrum(wav, 3))                   # another n_orb
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_vmap(wav[::-1], R)                                # descending grid
        mom, nu = d.spectrum_vmap(wav, R)
        assert mom.shape == (2, 3, 7) and nu.shape == (2, 3) and np.all(nu == 3)
        assert d.vmap_kernel_ms(2) > 0.0
        d.observe_set(lam, sig, 5.0, 2, None, data, ivar)                # drops the table
        assert d.vmap_key is None
        for call in (lambda: d.spectrum_vmap(wav, R), d.vmap_kernel_ms):
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
def test_transit_velocity_map_end_to_end(name, monkeypatch):
    """Transit.velocity_map on the reduced golden problems: 40 pixels about Na D2, 9 trials about the planet's frame,
    data planted through Transit.observe(frame_shifts=F[:, j*]) on the same transit.  chi2 at j* is within the
    chi-square bound of 0 (data and map come from two kernels that add in different orders: |M - d| <= 2 eps |M|, so
    m6 <= 4 eps^2 m3), the summed chi2 has its minimum there, the moments match the reference formed from R, and a
    second call uploads neither the observation nor the table."""
    from prometheus_amd import _native
    from prometheus_amd import lightcurve as lc
    from prometheus_amd import observation as obs
    d = np.load(os.path.join(G, "transit_" + name + ".npz"))
    tr = _product_transit(json.loads(str(d["config"])))
    R = np.array(tr.sumOverChords(devices=[0]))
    wav = np.asarray(tr.wavelength)
    n_orb = R.shape[0]
    assert wav[0] < lc.NA_D2 - 2e-8 and lc.NA_D2 + 2e-8 < wav[-1]
    px = lc.NA_D2 + 5e-10 * (np.arange(40) - 19.5)
    ins = obs.Instrument(px, resolving_power=140000.0, truncate=5.0)
    shifts = obs.planet_frame_shifts(tr.planet, tr.spatialGrid.constructOrbphaseAxis())
    F = obs.trial_factors(shifts, 1e5 * np.linspace(-16.0, 16.0, 9))
    j_star = 6
    planted = tr.observe(ins, frame_shifts=F[:, j_star], devices=[0])
    # (on C3r's coarse stretches a pixel's support can be empty: no model there, the pixel is masked through its data)
    assert np.all(np.isfinite(planted.model).sum(axis=1) >= 20)
    err = np.full(planted.model.shape, 1e-4)
    observation = obs.Observation(ins, n_orb, None, planted.model, err)
    vm = tr.velocity_map(observation, F, devices=[0])
    assert len(tr.last_stats) == 1 and vm.moments.shape == (n_orb, 9, 7)
    dev = _native.get_device(0)
    assert dev.observe_key == observation.key and dev.vmap_key is not None
    want = vref.vmap(wav, R, ins.lam, ins.sig, ins.truncate, F, observation.data, observation.ivar)
    frac = check("test_transit_velocity_map_end_to_end[%s]" % name, (vm.moments, vm.n_used), want, ins.truncate)
    eps = ref.m_tolerance(ins.truncate, want[3])
    zero_bound = 4.0 * eps * eps * want[0][:, j_star, 3].astype(np.float64)
    print("VMAP_ERR end to end %s chi2 at the planted column %s, bound %s; total chi2 %s" %
          (name, vm.chi2[:, j_star], zero_bound, vm.total("chi2")))
    assert np.all(vm.chi2[:, j_star] <= zero_bound)
    assert int(np.argmin(vm.total("chi2"))) == j_star
    assert np.all(frac <= 1.0)
    # a second call with the same Observation and table: nothing is uploaded, the same bits
    calls = []
    key = dev.vmap_key
    monkeypatch.setattr(dev, "observe_set", lambda *a, **k: calls.append("observe_set"))
    monkeypatch.setattr(dev, "vmap_set", lambda *a, **k: calls.append("vmap_set"))
    again = tr.velocity_map(observation, F.copy(), devices=[0])
    assert calls == [] and dev.observe_key == observation.key and dev.vmap_key == key
    assert np.array_equal(again.moments, vm.moments) and np.array_equal(again.n_used, vm.n_used)
