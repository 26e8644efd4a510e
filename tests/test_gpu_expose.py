"""Exposures on the device (prom_expose_set / prom_spectrum_expose / prom_transit_expose, Transit.expose) against the
longdouble reference of tests/helpers/expose_ref.py.  Marked ``gpu``.

Tolerances (expose_ref.bounds; derived there from the definition, not from the kernel): with u = 2^-53, eps the
documented bound on a tap's model and K the live taps, the exposure's model is within eps_e = eps + (K + 1) u relative
and the moments within vmap_ref's bounds with eps_e for eps.  n_used and the NaN pattern are exact.

The independence clause of the definition is tested bitwise, the degenerate table against prom_spectrum_vmap.  Every
test prints its largest error per moment and for the model as a fraction of its bound (``EXPOSE_ERR``;
profiles/expose_errors.txt).
"""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import expose_ref as eref
from helpers import observe_ref as ref
from helpers import vmap_ref as vref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
_csrc = os.path.join(REPO, "prometheus_amd", "csrc")
TILE = int(re.search(r"kObsTile = (\d+)", open(os.path.join(_csrc, "obs_index.h")).read()).group(1))
_hdr = open(os.path.join(_csrc, "vmap_index.h")).read()
STAGE = int(re.search(r"#define PROM_VM_STAGE (\d+)", _hdr).group(1))
C = int(re.search(r"#define PROM_VM_CHUNK (\d+)", _hdr).group(1))
T = int(re.search(r"#define PROM_VM_TRIALS (\d+)", _hdr).group(1))
LANES = int(re.search(r"kVmLanes = (\d+)", _hdr).group(1))
E_ARG, E_STATE = "PROM_E_ARG", "PROM_E_STATE"
U = 2.0 ** -53


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


def kms(v):
    return vref.doppler(1e5 * np.asarray(v, dtype=np.float64))


def positive_data(shape, seed):
    rng = np.random.default_rng(seed)
    return 0.9 + 0.05 * rng.random(shape), 1e4 * (0.1 + rng.random(shape))


def expose(dev, wav, R, lam, sig, k, rows, a, F, data, ivar, model=True):
    R = np.atleast_2d(R)
    dev.observe_set(lam, sig, k, R.shape[0])
    dev.expose_set(rows, a, F, data, ivar)
    return dev.spectrum_expose(wav, R, model=model)


def table(n_exp, n_trial, n_tap, n_orb=3, seed=11, dead=True):
    """Rows over n_orb, weights that sum to 1 (a dead tap in every second exposure when there are three taps or
    more), factors a few km/s about 1 that differ per exposure, trial and tap."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_orb, (n_exp, n_tap)).astype(np.int32)
    a = 0.2 + rng.random((n_exp, n_tap))
    if dead and n_tap >= 3:
        a[::2, 1] = 0.0
    a /= a.sum(axis=1, keepdims=True)
    v = np.linspace(-8.0, 8.0, n_trial) if n_trial > 1 else np.array([1.0])
    F = kms(v)[None, :, None] * (1.0 + 1e-5 * np.arange(n_tap))[None, None, :] * (1.0 - 2e-6 * np.arange(n_exp))[:, None, None]
    return rows, a, np.ascontiguousarray(F)


def report(name, frac, mfrac):
    print("EXPOSE_ERR %s %s of the bounds (m0 .. m6), model %s" %
          (name, " ".join("%.4f" % f for f in frac), "-" if mfrac is None else "%.4f" % mfrac))


def check(name, out, want, k):
    """Device (moments, n_used, model) against the reference's: n_used exact, equal NaN masks, every moment and the
    model within their bounds."""
    mom, nu, model = out
    rmom, rnu, rM, n_max, k_live = want
    assert mom.shape == rmom.shape and nu.dtype == np.int64
    assert np.array_equal(nu, rnu), name
    assert np.array_equal(np.isnan(mom), np.isnan(rmom.astype(np.float64))), name
    assert np.all(mom[rnu == 0] == 0), name
    frac = eref.fractions(mom, rmom, rnu, k, n_max, k_live)
    mfrac = None
    if model is not None:
        assert model.shape == rM.shape
        assert np.array_equal(np.isnan(model), np.isnan(rM.astype(np.float64))), name
        mfrac = eref.model_fraction(model, rM, k, n_max, k_live)
    report(name, frac, mfrac)
    assert np.all(frac <= 1.0), (name, frac)
    assert mfrac is None or mfrac <= 1.0, (name, mfrac)
    return frac


def case(dev, name, wav, lam, sig, n_exp, n_trial, n_tap, k=5.0, seed=3):
    R = ref.spectrum(wav, 3)
    data, ivar = positive_data((n_exp, len(lam)), seed)
    rows, a, F = table(n_exp, n_trial, n_tap)
    out = expose(dev, wav, R, lam, sig, k, rows, a, F, data, ivar)
    return check(name, out, eref.expose(wav, R, lam, sig, k, rows, a, F, data, ivar), k)


# ---- smallest shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_exp", [1, 5])
@pytest.mark.parametrize("n_wav", [1, 2, 65, STAGE + 1])
def test_smallest_grids(dev, n_wav, n_exp):
    """A non-uniform grid with 10x spacing jumps inside the supports and duplicated points, 5 pixels (one duplicated,
    some beyond the ends), 3 trials, 2 taps."""
    wav = ref.grid_nonuniform(n_wav)
    case(dev, "grids n_wav=%d n_exp=%d" % (n_wav, n_exp), wav, ref.pixels_over(wav, 5), np.full(5, 2.5e-10), n_exp, 3, 2)


@pytest.mark.parametrize("n_exp", [1, 5])
@pytest.mark.parametrize("n_pix", [1, TILE + 1, TILE * C + 1])
def test_smallest_pixel_counts(dev, n_pix, n_exp):
    """About a tile and about a chunk (the second workgroup along the pixels starts at 32 C), 2 trials, 2 taps; widths
    too small to reach a node among them."""
    wav = ref.grid_nonuniform(1500)
    sig = np.full(n_pix, 2.5e-10)
    sig[::7] = 1e-13
    case(dev, "pixels n_pix=%d n_exp=%d" % (n_pix, n_exp), wav, ref.pixels_over(wav, n_pix), sig, n_exp, 2, 2)


@pytest.mark.parametrize("n_exp", [1, 5])
@pytest.mark.parametrize("n_trial", [1, T - 1, T + 1])
def test_smallest_trial_counts(dev, n_trial, n_exp):
    wav = ref.grid_nonuniform(1500)
    case(dev, "trials n_trial=%d n_exp=%d" % (n_trial, n_exp), wav, ref.pixels_over(wav, TILE + 1),
         np.full(TILE + 1, 2.5e-10), n_exp, n_trial, 2)


@pytest.mark.parametrize("n_exp", [1, 5])
@pytest.mark.parametrize("n_tap", [1, 2, 3, 6])
def test_smallest_tap_counts(dev, n_tap, n_exp):
    wav = ref.grid_nonuniform(1500)
    case(dev, "taps n_tap=%d n_exp=%d" % (n_tap, n_exp), wav, ref.pixels_over(wav, TILE + 1),
         np.full(TILE + 1, 2.5e-10), n_exp, 3, n_tap)


# ---- bitwise identities ----------------------------------------------------------------------------------------
def _design():
    """A long fine core, 70 pixels in its upper part at R = 140,000 (supports of about 180 points), 3 rows of R, a
    map table of 2 T + 1 trials 2 km/s apart per row, and a smeared table of 5 exposures with 4 taps on them."""
    wav = ref.grid_coarse_fine(3000, 200)
    R = ref.spectrum(wav, 3)
    lam = wav[200 + 2500] + 1e-10 * (np.arange(2 * TILE + 6) - 20.0)
    sig = lam / (140000.0 * 2.3548)
    v = np.linspace(-16.0, 16.0, 2 * T + 1)
    Fm = np.stack([kms(v), kms(v + 3.0), kms(v - 2.0)])
    data, ivar = positive_data((5, len(lam)), 7)
    rows, a, F = table(5, 2 * T + 1, 4, seed=21)
    return dict(wav=wav, R=R, lam=lam, sig=sig, k=5.0, Fm=Fm, data=data, ivar=ivar, rows=rows, a=a, F=F)


def _smeared(dev, d, model=True):
    return expose(dev, d["wav"], d["R"], d["lam"], d["sig"], d["k"], d["rows"], d["a"], d["F"], d["data"], d["ivar"],
                  model=model)


@pytest.fixture(scope="module")
def smeared(dev):
    d = _design()
    return d, _smeared(dev, d)


def same(a, b):
    ok = np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])
    if len(a) > 2 and len(b) > 2 and a[2] is not None and b[2] is not None:
        ok = ok and np.array_equal(a[2], b[2], equal_nan=True)
    return ok


def test_smeared_table_is_right_and_repeats_bitwise(dev, smeared):
    d, base = smeared
    check("smeared base", base, eref.expose(d["wav"], d["R"], d["lam"], d["sig"], d["k"], d["rows"], d["a"], d["F"],
                                            d["data"], d["ivar"]), d["k"])
    # (the reddest trials move the upper pixels off the fine core, where the coarse grid leaves some supports empty)
    assert np.all(base[1] >= 60) and np.all(base[1][:, -1] == len(d["lam"])) and np.isnan(base[2]).any()
    assert same(_smeared(dev, d), base)
    assert same(dev.spectrum_expose(d["wav"], d["R"], model=True), base)      # two calls in a row
    mom, nu, model = dev.spectrum_expose(d["wav"], d["R"], model=False)        # moments alone
    assert model is None and same((mom, nu), base[:2])
    none, none2, model = dev.spectrum_expose(d["wav"], d["R"], moments=False, model=True)   # the model alone
    assert none is None and none2 is None and np.array_equal(model, base[2], equal_nan=True)


def test_degenerate_table_is_the_velocity_map_bitwise(dev, smeared):
    """One tap of weight 1 on row e: prom_spectrum_vmap's eight numbers; two taps of 1/2 on the same row and factor
    too; exposure e on row pi(e): the map over R with its rows permuted."""
    d, _ = smeared
    wav, R, lam, sig, k, Fm = (d[n] for n in ("wav", "R", "lam", "sig", "k", "Fm"))
    data, ivar = d["data"][:3], d["ivar"][:3]
    dev.observe_set(lam, sig, k, 3, None, data, ivar)
    dev.vmap_set(Fm)
    vm = dev.spectrum_vmap(wav, R)
    assert np.all(vm[1] >= 56)
    rows, a, F = eref.degenerate(Fm)
    out = expose(dev, wav, R, lam, sig, k, rows, a, F, data, ivar)
    assert same(out[:2], vm)
    half = expose(dev, wav, R, lam, sig, k, np.repeat(rows, 2, axis=1), np.full((3, 2), 0.5), np.repeat(F, 2, axis=2),
                  data, ivar)
    assert same(half, out)
    perm = np.array([2, 0, 1])
    dev.observe_set(lam, sig, k, 3, None, data, ivar)
    dev.vmap_set(Fm)
    vmp = dev.spectrum_vmap(wav, np.ascontiguousarray(R[perm]))
    assert not same(vmp, vm)
    outp = expose(dev, wav, R, lam, sig, k, perm[:, None].astype(np.int32), a, F, data, ivar)
    assert same(outp[:2], vmp)


def test_trials_and_exposures_permuted_and_alone_bitwise(dev, smeared):
    d, base = smeared
    wav, R, lam, sig, k = (d[n] for n in ("wav", "R", "lam", "sig", "k"))
    rows, a, F, data, ivar = (d[n] for n in ("rows", "a", "F", "data", "ivar"))
    dev.observe_set(lam, sig, k, 3)
    perm = np.random.default_rng(12).permutation(F.shape[1])
    dev.expose_set(rows, a, np.ascontiguousarray(F[:, perm]), data, ivar)
    out = dev.spectrum_expose(wav, R, model=True)
    assert same(out, tuple(x[:, perm] for x in base))
    for j in (0, T - 1, T, 2 * T):
        dev.expose_set(rows, a, np.ascontiguousarray(F[:, j:j + 1]), data, ivar)
        assert same(dev.spectrum_expose(wav, R, model=True), tuple(x[:, j:j + 1] for x in base)), j
    for e in range(len(rows)):
        dev.expose_set(rows[e:e + 1], a[e:e + 1], F[e:e + 1], data[e:e + 1], ivar[e:e + 1])
        assert same(dev.spectrum_expose(wav, R, model=True), tuple(x[e:e + 1] for x in base)), e
    pe = np.array([3, 0, 4, 2, 1])
    dev.expose_set(rows[pe], a[pe], F[pe], data[pe], ivar[pe])
    assert same(dev.spectrum_expose(wav, R, model=True), tuple(x[pe] for x in base))


def test_dead_taps_anywhere_bitwise(dev, smeared):
    """Dead taps appended, prepended and interleaved (their factors far off the grid, their rows any); a dead tap
    whose row of R is all NaN."""
    d, base = smeared
    wav, lam, sig, k = (d[n] for n in ("wav", "lam", "sig", "k"))
    rows, a, F, data, ivar = (d[n] for n in ("rows", "a", "F", "data", "ivar"))
    R4 = np.concatenate([d["R"], np.full((1, len(wav)), np.nan)])
    n_exp, n_trial, n_tap = F.shape
    for name, at in (("appended", [n_tap, n_tap]), ("prepended", [0, 0]), ("interleaved", [1, 2, 3])):
        r2 = np.insert(rows, at, 3, axis=1)
        a2 = np.insert(a, at, 0.0, axis=1)
        F2 = np.insert(F, at, 1.7, axis=2)
        assert r2.shape[1] == n_tap + len(at) and np.all(a2[:, at[0]] == 0)
        out = expose(dev, wav, R4, lam, sig, k, r2, a2, F2, data, ivar)
        assert same(out, base), name
    # ... while the same tap alive makes every number of its exposure NaN or unused
    a3 = np.insert(a, [0], 0.25, axis=1)
    out = expose(dev, wav, R4, lam, sig, k, np.insert(rows, [0], 3, axis=1), a3, np.insert(F, [0], 1.0, axis=2), data,
                 ivar)
    assert np.isnan(out[2]).all() and np.isnan(out[0][..., 6]).all() and np.all(out[1] >= 56)


def test_wide_columns_force_global_reads_bitwise(dev, smeared):
    """A -300 or +300 km/s trial at the head of every group of T: with -300 the stage starts 2,500 points below the
    other trials' supports, which are then read from global memory (tests/test_gpu_vmap.py counts them for the same
    pixels and factors with the host walk); the other trials' numbers do not move."""
    d, base = smeared
    wav, R, lam, sig, k = (d[n] for n in ("wav", "R", "lam", "sig", "k"))
    rows, a, F, data, ivar = (d[n] for n in ("rows", "a", "F", "data", "ivar"))
    cols, keep = [], []
    for j in range(F.shape[1]):
        if len(cols) % T == 0:
            cols.append(np.full(F[:, 0].shape, kms(-300.0 if (len(cols) // T) % 2 == 0 else 300.0)))
        keep.append(len(cols))
        cols.append(F[:, j])
    Fw = np.ascontiguousarray(np.stack(cols, axis=1))
    out = expose(dev, wav, R, lam, sig, k, rows, a, Fw, data, ivar)
    assert same(tuple(x[:, keep] for x in out), base)
    wide = [j for j in range(Fw.shape[1]) if j not in keep]
    check("wide columns", tuple(x[:, wide] for x in out),
          eref.expose(wav, R, lam, sig, k, rows, a, np.ascontiguousarray(Fw[:, wide]), data, ivar), k)


_BATCHED = """
import hashlib, json, sys
sys.path.insert(0, %r)
import numpy as np
from prometheus_amd import _native
from test_gpu_expose import _design, _smeared
out = _smeared(_native.get_device(0), _design())
print(json.dumps([hashlib.sha256(x.tobytes()).hexdigest() for x in out]))
"""


def test_batches_under_a_small_scratch_cap_bitwise(smeared):
    """PROM_VMAP_SCRATCH_MB is read at context creation, so the case runs in a process of its own: 0.0001 MB (104
    bytes) is below one trial group's records, so every group is a batch of its own: three batches."""
    _, base = smeared
    env = dict(os.environ, PROM_VMAP_SCRATCH_MB="0.0001", PROM_DEBUG="1")
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _BATCHED % os.path.join(REPO, "tests")],
                       env=env, cwd=REPO, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = [l for l in p.stderr.splitlines() if "exposures:" in l]
    assert lines and "3 groups, 3 batches of up to 1 groups" in lines[-1], p.stderr[-2000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("[")][-1])
    assert out == [hashlib.sha256(x.tobytes()).hexdigest() for x in base]


# ---- semantics -------------------------------------------------------------------------------------------------
def test_nan_in_r_reaches_exactly_its_exposures(dev):
    """A NaN in row 1 reaches the (exposure, trial, pixel) whose live taps on row 1 hold it in their support: not the
    exposures that read row 1 through a dead tap only, nor the trial whose factor moves every pixel away."""
    wav = ref.grid_nonuniform(800)
    R = ref.spectrum(wav, 3)
    R[1, 417] = np.nan
    lam = ref.pixels_over(wav, 2 * TILE - 2, outside=False)
    sig = np.full(len(lam), 2.5e-10)
    rows = np.array([[0, 1], [1, 2], [0, 1], [2, 0]], dtype=np.int32)
    a = np.array([[0.5, 0.5], [0.25, 0.75], [1.0, 0.0], [0.5, 0.5]])
    F = np.ones((4, 3, 2))
    F[:, 1, :] = 1.0 + 1e-5
    F[:, 2, 1] = 1.0 + 4e-4          # trial 2: the second tap looks 2.4 A away
    data, ivar = positive_data((4, len(lam)), 2)
    want = eref.expose(wav, R, lam, sig, 5.0, rows, a, F, data, ivar)
    hit = np.isnan(want[0][..., 1].astype(np.float64))
    assert hit[0].any() and hit[1].all() and not hit[2].any() and not hit[3].any()
    out = expose(dev, wav, R, lam, sig, 5.0, rows, a, F, data, ivar)
    for i in (1, 3, 4, 6):
        assert np.array_equal(np.isnan(out[0][..., i]), hit), i
    assert np.isfinite(out[0][..., [0, 2, 5]]).all()
    check("nan in R", out, want, 5.0)
    near = np.abs(lam - wav[417]) < 5e-9
    assert np.isnan(out[2][1, 0, near]).any() and np.isfinite(out[2][1, 0, ~near]).all()


def test_live_tap_off_the_grid_unuses_the_pixel(dev):
    """The second tap of exposure 1 looks beyond the grid's end for the upper pixels at trial 1: den = 0 there, the
    pixel is unused and its model NaN, the other pixels, trials and exposures stand."""
    wav = ref.grid_nonuniform(900)
    R = ref.spectrum(wav, 3)
    lam = ref.pixels_over(wav, TILE + 5, outside=False)
    sig = np.full(len(lam), 2.5e-10)
    rows, a, F = table(3, 2, 2, seed=5)
    data, ivar = positive_data((3, len(lam)), 8)
    base = expose(dev, wav, R, lam, sig, 5.0, rows, a, F, data, ivar)
    assert np.all(base[1] == len(lam))
    F2 = F.copy()
    F2[1, 1, 1] = 1.0 + 0.5 * (wav[-1] - wav[0]) / wav[0]
    want = eref.expose(wav, R, lam, sig, 5.0, rows, a, F2, data, ivar)
    gone = np.isnan(want[2][1, 1].astype(np.float64))
    assert 0 < gone.sum() < len(lam) and want[1][1, 1] == len(lam) - gone.sum()
    out = expose(dev, wav, R, lam, sig, 5.0, rows, a, F2, data, ivar)
    check("live tap off the grid", out, want, 5.0)
    assert np.array_equal(np.isnan(out[2][1, 1]), gone) and not np.isnan(out[0]).any()
    keep = np.ones((3, 2), dtype=bool)
    keep[1, 1] = False
    assert same(tuple(x[keep] for x in out), tuple(x[keep] for x in base))
    # every tap of an exposure dead: no model, nothing used
    a0 = a.copy()
    a0[2] = 0.0
    out = expose(dev, wav, R, lam, sig, 5.0, rows, a0, F, data, ivar)
    assert np.isnan(out[2][2]).all() and np.all(out[1][2] == 0) and np.all(out[0][2] == 0)
    assert same(tuple(x[:2] for x in out), tuple(x[:2] for x in base))


def test_masked_pixels_are_excluded(dev):
    """ivar 0, negative, infinite and NaN, NaN and infinite data: unused, while the model ignores data and ivar."""
    wav = ref.grid_nonuniform(900)
    R = ref.spectrum(wav, 3)
    lam = ref.pixels_over(wav, 2 * TILE + 3, outside=False)
    sig = np.full(len(lam), 2.5e-10)
    rows, a, F = table(2, 3, 3, seed=6)
    data, ivar = positive_data((2, len(lam)), 4)
    clean = expose(dev, wav, R, lam, sig, 5.0, rows, a, F, data, ivar)
    ivar[0, 3], ivar[0, 12], ivar[1, 5], ivar[1, 9] = 0.0, -1.0, np.nan, np.inf
    data[1, 8], data[1, 20] = np.nan, np.inf
    want = eref.expose(wav, R, lam, sig, 5.0, rows, a, F, data, ivar)
    assert np.isfinite(clean[2][0][:, [3, 12]]).all() and np.isfinite(clean[2][1][:, [5, 9, 8, 20]]).all()
    assert np.all(clean[1][0] - want[1][0] == 2) and np.all(clean[1][1] - want[1][1] == 4)
    out = expose(dev, wav, R, lam, sig, 5.0, rows, a, F, data, ivar)
    assert np.array_equal(out[2], clean[2], equal_nan=True)
    mom, nu, model = out
    assert np.array_equal(nu, want[1]) and np.isfinite(mom).all()
    frac = eref.fractions(mom, want[0], nu, 5.0, want[3], want[4])
    report("masked pixels", frac, None)
    assert np.all(frac <= 1.0)


def test_model_is_the_weighted_sum_of_the_observation_models(dev):
    """model_out against sum a_i M_i formed on the host from prom_spectrum_observe's num / den per tap, within
    (K + 2) u relative.  The supports hold at most kVmLanes points (asserted through the reference's counts): there
    k_observe's 64-lane and k_expose's 16-lane butterflies add the same values in the same shape (the idle lanes add
    +0), so M_i is the same number and only the K products and K - 1 additions remain.  (Over wider supports the two
    kernels' orders differ and M_i agree within eps only: tests/test_gpu_vmap.py, the chi-square test.)"""
    wav = ref.grid_coarse_fine(1200, 20)
    R = ref.spectrum(wav, 3)
    lam = wav[20 + 600] + 1e-10 * (np.arange(TILE + 3) - 15.0)
    sig = np.full(len(lam), 1.4e-11)
    k = 5.0
    rows, a, F = table(2, 2, 3, seed=9, dead=False)
    K = 3
    data, ivar = positive_data((2, len(lam)), 10)
    out = expose(dev, wav, R, lam, sig, k, rows, a, F, data, ivar)
    host = np.zeros(out[2].shape)
    for e in range(2):
        for j in range(2):
            for i in range(K):
                dev.observe_set(lam, sig, k, 3, np.full(3, F[e, j, i]))
                num, den, _, _ = dev.spectrum_observe(wav, R)
                assert np.all(den[rows[e, i]] > 0)
                assert ref.observe(wav, R[:1], lam, sig, k, [F[e, j, i]])[2].max() <= LANES
                term = a[e, i] * (num[rows[e, i]] / den[rows[e, i]])
                host[e, j] = term if i == 0 else host[e, j] + term
    worst = float(np.max(np.abs(out[2] - host) / np.abs(host))) / ((K + 2) * U)
    print("EXPOSE_ERR model against the observation's models: %.4f of (K + 2) u" % worst)
    assert worst <= 1.0


# ---- argument and state errors ---------------------------------------------------------------------------------
def test_errors():
    from prometheus_amd import _native
    wav = ref.grid_nonuniform(100)
    R = ref.spectrum(wav, 2)
    lam, sig = wav[[10, 20, 30]], np.full(3, 2e-10)
    data, ivar = positive_data((4, 3), 6)
    rows, a, _ = table(4, 3, 2, n_orb=2)
    F = 1.0 + 1e-6 * np.arange(24.0).reshape(4, 3, 2)       # (the grid is 0.2 A long: the pixels stay on it)
    d = _native.Device(0)
    try:
        with pytest.raises(ValueError):                                   # (no observation: no pixels to match)
            d.expose_set(rows, a, F, data, ivar)
        for call in (lambda: d.spectrum_expose(wav, R), d.transit_expose, d.expose_kernel_ms,
                     lambda: d.expose_set(rows, a, F, data[:, :0], ivar[:, :0])):
            with pytest.raises(_native.NativeError, match=E_STATE):      # no observation on the context
                call()
        d.observe_set(lam, sig, 5.0, 2)                                   # (an observation without data is enough)
        for r_bad in (-1, 2):
            rb = rows.copy()
            rb[3, 1] = r_bad
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.expose_set(rb, a, F, data, ivar)
        for bad in (-1.0, np.nan, np.inf):
            ab = a.copy()
            ab[1, 0] = bad
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.expose_set(rows, ab, F, data, ivar)
        for bad in (0.0, -1.0, np.nan, np.inf):
            Fb = F.copy()
            Fb[3, 2, 1] = bad
            with pytest.raises(_native.NativeError, match=E_ARG):
                d.expose_set(rows, a, Fb, data, ivar)
        with pytest.raises(_native.NativeError, match=E_ARG):            # n_trial = 0
            d.expose_set(rows, a, np.zeros((4, 0, 2)), data, ivar)
        with pytest.raises(_native.NativeError, match=E_ARG):            # n_tap = 0
            d.expose_set(rows[:, :0], a[:, :0], np.zeros((4, 3, 0)), data, ivar)
        with pytest.raises(_native.NativeError, match=E_STATE):          # a failed set leaves no table behind
            d.spectrum_expose(wav, R)
        d.expose_set(rows, a, F, data, ivar, key="k")
        assert d.expose_key == "k"
        with pytest.raises(_native.NativeError, match=E_STATE):
            d.transit_expose()                                            # no run yet
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_expose(wav, ref.spectrum(wav, 3))                  # another n_orb
        with pytest.raises(_native.NativeError, match=E_ARG):
            d.spectrum_expose(wav[::-1], R)                               # descending grid
        mom, nu, model = d.spectrum_expose(wav, R, model=True)
        assert mom.shape == (4, 3, 7) and nu.shape == (4, 3) and model.shape == (4, 3, 3) and np.all(nu == 3)
        assert d.expose_kernel_ms(2) > 0.0
        d.observe_set(lam, sig, 5.0, 2)                                   # drops the table
        assert d.expose_key is None
        for call in (lambda: d.spectrum_expose(wav, R), d.expose_kernel_ms):
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
def test_transit_expose_end_to_end(name, monkeypatch):
    """Transit.expose on the reduced golden problems, 40 pixels about Na D2, exposure_taps with the planet's own Kp and
    Vsys = 0.  Exposures at the model's own phases with no width are Transit.velocity_map's moments for a table of
    ones, bit for bit; a smeared table (three sub-samples, exposures between the phases) is within the bounds of the
    reference evaluated on sumOverChords' R; a second call uploads nothing; the run refuses shards; a transit with
    another number of phases drops the table."""
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
    assert n_orb == len(orb) >= 3
    px = lc.NA_D2 + 5e-10 * (np.arange(40) - 19.5)
    ins = obs.Instrument(px[::-1], resolving_power=140000.0, truncate=5.0)      # (the caller's order: descending)
    base = obs.planet_frame_shifts(tr.planet, orb)
    Kp = np.sqrt(const.G * tr.planet.hostStar.M / tr.planet.a)
    planted = tr.observe(ins, devices=[0])
    err = np.full(planted.model.shape, 1e-4)
    data = np.where(np.isfinite(planted.model), planted.model, np.nan) * (1.0 + 1e-3)
    # at the model's own phases
    rows, a, F = obs.exposure_taps(orb, base, orb, np.zeros(n_orb), Kp=[Kp], Vsys=[0.0])
    assert F.shape == (n_orb, 1, 2) and np.all(F[:, 0][a > 0] == 1.0)
    ex = obs.Exposures(ins, rows, a, F, data, err)
    out = tr.expose(ex, return_model=True, devices=[0])
    dev = _native.get_device(0)
    assert dev.expose_key == ex.key and len(tr.last_stats) == 1
    vm = tr.velocity_map(obs.Observation(ins, n_orb, None, data, err), np.ones((n_orb, 1)), devices=[0])
    assert np.array_equal(out.moments, vm.moments, equal_nan=True) and np.array_equal(out.n_used, vm.n_used)
    assert np.all(out.n_used >= 1) and out.model.shape == (n_orb, 1, 40)
    assert np.array_equal(np.isfinite(out.model[:, 0]), np.isfinite(planted.model))
    assert np.array_equal(out.chi2, vm.chi2) and out.total("chi2").shape == (1,)
    # smeared, between the phases
    # (the last exposure is two phase steps long and centred between two phases: its sub-samples lie in three brackets)
    step = orb[1] - orb[0]
    mid = np.concatenate([0.5 * (orb[:-1] + orb[1:]), [orb[1]]])
    width = np.concatenate([np.full(n_orb - 1, 0.9 * step), [1.9 * step]])
    rows, a, F = obs.exposure_taps(orb, base, mid, width, n_sub=3, Kp=Kp * np.array([0.9, 1.0]), Vsys=[0.0, 2e5])
    assert len(np.unique(rows[-1])) >= 3
    data, err = np.resize(data, (len(mid), 40)), np.resize(err, (len(mid), 40))
    ex = obs.Exposures(ins, rows, a, F, data[:len(mid)], err[:len(mid)])
    out = tr.expose(ex, return_model=True, devices=[0])
    assert out.moments.shape == (len(mid), 4, 7) and out.grid("chi2", 2, 2).shape == (len(mid), 2, 2)
    want = eref.expose(wav, R, ins.lam, ins.sig, ins.truncate, rows, a, F, ex.data, ex.ivar)
    check("end to end %s" % name, (out.moments, out.n_used, ins.sort(out.model)), want, ins.truncate)
    # a second call with the same Exposures: nothing is uploaded, the same bits
    calls = []
    monkeypatch.setattr(dev, "observe_set", lambda *a, **k: calls.append("observe_set"))
    monkeypatch.setattr(dev, "expose_set", lambda *a, **k: calls.append("expose_set"))
    again = tr.expose(ex, devices=[0])
    assert calls == [] and again.model is None
    assert np.array_equal(again.moments, out.moments, equal_nan=True) and np.array_equal(again.n_used, out.n_used)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="not additive over wavelength partials"):
        tr.expose(ex, devices=[0, 1])
    if len(wav) > 4096:
        with pytest.raises(ValueError, match="not additive over wavelength partials"):
            tr.expose(ex, devices=[0], max_memory_gb=1e-9)
    # a table set for another number of phases is dropped by the next transit
    dev.observe_set(ins.lam, ins.sig, ins.truncate, n_orb + 1)
    dev.expose_set(rows, a, F, ex.data, ex.ivar, key="other")
    tr.sumOverChords(devices=[0])
    assert dev.expose_key is None and dev.observe_key is None
    with pytest.raises(_native.NativeError, match=E_STATE):
        dev.transit_expose()
