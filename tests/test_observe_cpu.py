"""The observation's definition and host side without a GPU: the longdouble reference (tests/helpers/observe_ref.py)
against closed forms, the Instrument's bookkeeping, and the host harness of k_observe's index arithmetic
(prometheus_amd/csrc/obs_index.h through tests/helpers/observe_host.cpp)."""
import math
import subprocess

import numpy as np
import pytest

from helpers import observe_plan as plan
from helpers import observe_ref as ref

LD = np.longdouble
COUNTERS = plan.COUNTERS


def relerr(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b) / np.abs(b)))


# ---- the reference against closed forms ------------------------------------------------------------------------
def test_constant_spectrum_gives_the_constant():
    wav = ref.grid_nonuniform(700)
    lam = ref.pixels_over(wav, 40, outside=False)
    sig = np.full(40, 3e-10)
    num, den, cnt = ref.observe(wav, np.full((2, 700), 0.75), lam, sig, 5.0)
    assert cnt.min() > 0
    assert relerr(ref.model(num, den), 0.75) < 1e-17


def test_linear_spectrum_symmetric_support_gives_the_value_at_the_pixel():
    """Uniform (dyadic) grid, pixels on nodes well inside: the weights are symmetric about the pixel, so a spectrum
    linear in lambda comes out as its value at the pixel (up to longdouble rounding of ~200 terms)."""
    wav = ref.grid_dyadic(600)
    lam = wav[[100, 250, 333, 480]]
    R = (0.2 + 3.0e3 * wav)[None, :]
    num, den, cnt = ref.observe(wav, R, lam, np.full(4, 6.5 * ref.DYADIC_STEP), 5.0)
    assert np.all(cnt == 65)
    assert relerr(ref.model(num, den), (0.2 + 3.0e3 * lam)[None, :]) < 1e-17


def test_gaussian_line_under_gaussian_lsf():
    """A line 1 - d exp(-(x - x0)^2 / 2a^2) under an LSF of width b is 1 - d a / s exp(-(x - x0)^2 / 2 s^2) with
    s = sqrt(a^2 + b^2): width and depth.  Bound on a uniform grid of spacing h with a = b = 20 h and k = 8: the
    truncation drops a tail weight erfc(k / sqrt 2) = 1.2e-15 from either sum, and the trapezoid rule on a Gaussian
    of width w errs by about 2 exp(-2 pi^2 (w / h)^2) relatively -- the narrowest integrand, LSF times line, has
    w = a b / s = 14.1 h, far below rounding -- so |M - analytic| <= 4 erfc(k / sqrt 2) + 4 exp(-2 pi^2 (w / h)^2)
    + 64 * 2^-53 = 1.2e-14."""
    h = 1e-11
    wav = 5890e-8 + h * np.arange(2001)
    x0, a, b, d, k = wav[1000], 20 * h, 20 * h, 0.3, 8.0
    R = 1.0 - d * np.exp(-0.5 * ((wav - x0) / a) ** 2)
    lam = wav[600:1401:8] + 0.3 * h
    num, den, cnt = ref.observe(wav, R[None, :], lam, np.full(len(lam), b), k)
    s = math.hypot(a, b)
    want = 1.0 - d * a / s * np.exp(-0.5 * ((lam - x0) / s) ** 2)
    w = a * b / s
    bound = 4 * math.erfc(k / math.sqrt(2)) + 4 * math.exp(-2 * math.pi ** 2 * (w / h) ** 2) + 64 * ref.U
    err = float(np.max(np.abs(ref.model(num, den)[0] - want.astype(LD))))
    print("gaussian line: max |M - analytic| %.3e, bound %.3e" % (err, bound))
    assert err <= bound


@pytest.mark.parametrize("n_shards", [1, 2, 3, 7])
def test_shard_partials_with_edges_combine_to_the_whole(n_shards):
    wav = ref.grid_nonuniform(900)
    R = ref.spectrum(wav, 3)
    lam = ref.pixels_over(wav, 70)
    sig = np.full(70, 2.5e-10)
    f = np.array([1.0 - 1e-5, 1.0, 1.0 + 2e-5])
    num1, den1, _ = ref.observe(wav, R, lam, sig, 5.0, f)
    cuts = np.linspace(0, len(wav), n_shards + 1).astype(int)
    num, den = np.zeros_like(num1), np.zeros_like(den1)
    for a, b in zip(cuts[:-1], cuts[1:]):
        n, d, _ = ref.observe(wav[a:b], R[:, a:b], lam, sig, 5.0, f, wav[a - 1] if a else np.nan,
                              wav[b] if b < len(wav) else np.nan)
        num += n
        den += d
    ok = den1 > 0
    assert np.array_equal(den > 0, ok)
    assert relerr(num[ok], num1[ok]) < 1e-16 and relerr(den[ok], den1[ok]) < 1e-16


def test_float64_orders_stay_far_below_the_tolerance():
    """The tolerance of the GPU tests, (3 k^2 + 2 n_max + 16) u, against what float64 evaluation does in forward and
    reverse order on a coarse / fine grid: far below it (< 0.1 of the bound), so the bound is not tight."""
    wav = ref.grid_coarse_fine()
    R = ref.spectrum(wav, 1)[0]
    rng = np.random.default_rng(5)
    lam = np.sort(wav[0] + (wav[-1] - wav[0]) * rng.random(300))
    q = ref.q_weights(wav)
    for k in (3.0, 5.0, 8.0):
        sig = lam / (140000.0 * 2.3548) * (0.5 + rng.random(300))
        num, den, cnt = ref.observe(wav, R[None, :], lam, sig, k)
        M = ref.model(num, den)[0]
        worst = 0.0
        for p in range(300):
            a, b = ref.support(wav, lam[p], k * sig[p])
            if a == b:
                continue
            z = (wav[a:b] - lam[p]) / sig[p]
            gq = np.exp(-0.5 * z * z) * q[a:b]
            for order in (slice(None), slice(None, None, -1)):
                n = d = 0.0
                for t, r in zip(gq[order], R[a:b][order]):
                    d += t
                    n += t * r
                worst = max(worst, float(abs(LD(n / d) - M[p]) / abs(M[p])) / ref.m_tolerance(k, b - a))
        assert worst < 0.1, (k, worst)


# ---- the host side of the package ------------------------------------------------------------------------------
def test_instrument_sorts_and_unsorts():
    from prometheus_amd import observation as obs
    px = np.array([5.0, 1.0, 3.0, 3.0, 2.0, 9.0]) * 1e-5
    ins = obs.Instrument(px, resolving_power=1e5)
    assert np.all(np.diff(ins.lam) >= 0) and ins.n_pix == 6
    assert np.array_equal(ins.sig, ins.lam / (1e5 * 2 * math.sqrt(2 * math.log(2))))
    a = np.arange(12.0).reshape(2, 6)
    assert np.array_equal(ins.unsort(ins.sort(a)), a)
    assert np.array_equal(ins.sort(px), ins.lam)
    assert np.array_equal(obs.Instrument(px, sigma=2e-10).sig, np.full(6, 2e-10))
    with pytest.raises(ValueError):
        obs.Instrument(px)
    with pytest.raises(ValueError):
        obs.Instrument(px, sigma=-1.0)


def test_observation_prepares_once():
    """An Observation sorts data and err into the device's pixel order, masks bad errors, and carries a content key:
    equal content gives an equal key, any changed array another."""
    from prometheus_amd import observation as obs
    ins = obs.Instrument(np.array([3.0, 1.0, 2.0]) * 1e-5, sigma=1e-10)
    data = np.array([[3.0, 1.0, 2.0], [30.0, 10.0, 20.0]])
    err = np.array([[0.5, np.nan, 2.0], [0.0, -1.0, np.inf]])
    o = obs.Observation(ins, 2, [1.0, 1.0001], data, err)
    assert np.array_equal(o.data, [[1.0, 2.0, 3.0], [10.0, 20.0, 30.0]])
    assert np.array_equal(o.ivar, [[0.0, 0.25, 4.0], [0.0, 0.0, 0.0]])
    assert o.key == obs.Observation(ins, 2, [1.0, 1.0001], data.copy(), err.copy()).key
    data2 = data.copy()
    data2[1, 1] += 1.0
    keys = {o.key, obs.Observation(ins, 2, [1.0, 1.0001], data2, err).key, obs.Observation(ins, 2, None, data, err).key,
            obs.Observation(ins, 2, [1.0, 1.0002], data, err).key, obs.Observation(ins, 2).key,
            obs.Observation(obs.Instrument(ins.pixels, sigma=2e-10), 2, [1.0, 1.0001], data, err).key}
    assert len(keys) == 6
    with pytest.raises(ValueError):
        obs.Observation(ins, 3, [1.0, 1.0])
    with pytest.raises(ValueError):
        obs.Observation(ins, 2, None, data)


def test_coverage_is_one_inside_and_less_at_the_ends():
    """Inside, den is the trapezoid sum of the truncated Gaussian: it differs from the integral by at most one grid
    step of the integrand at the cut, h exp(-k^2 / 2), that is (h / sigma) exp(-k^2 / 2) of the full weight."""
    from prometheus_amd import observation as obs
    h = 1e-11
    wav = 5890e-8 + h * np.arange(1500)
    ins = obs.Instrument([wav[0], wav[3], wav[700] + 0.4 * h, wav[-1], wav[-1] + 1e-8], sigma=12 * h, truncate=5.0)
    _, den, _ = ref.observe(wav, np.ones((1, 1500)), ins.lam, ins.sig, ins.truncate)
    cov = ins.unsort(den.astype(np.float64)) / ins.full_weight()
    assert abs(cov[0, 2] - 1.0) < (1.0 / 12.0) * math.exp(-12.5)
    assert abs(cov[0, 0] - 0.5) < 1e-3 and abs(cov[0, 3] - 0.5) < 1e-3 and 0.5 < cov[0, 1] < 1.0
    assert cov[0, 4] == 0.0


def test_host_model_chi_square_and_coadd():
    from prometheus_amd import observation as obs
    rng = np.random.default_rng(3)
    num, den = rng.random((3, 50)), 0.5 + rng.random((3, 50))
    den[0, 4] = num[0, 4] = 0.0
    M = obs.model_spectrum(num, den)
    assert np.isnan(M[0, 4]) and np.array_equal(M[1], num[1] / den[1])
    data, ivar = M + 0.01 * rng.standard_normal(M.shape), 1e4 * rng.random(M.shape)
    data[1, 3], ivar[1, 5], ivar[2, 6] = np.nan, 0.0, np.inf
    c2, nu = obs.chi_square(M, den, data, ivar)
    c2r, nur = ref.chi2(M, den, data, ivar)
    assert np.array_equal(nu, nur) and list(nu) == [49, 48, 49]
    assert relerr(c2, c2r) < 60 * ref.U
    M2 = M.copy()
    M2[2, 10] = np.nan
    assert np.isnan(obs.chi_square(M2, den, data, ivar)[0][2])
    co = obs.coadd(M, weights=[1.0, 2.0, 1.0])
    assert co[4] == pytest.approx((2 * M[1, 4] + M[2, 4]) / 3) and co[0] == pytest.approx((M[0, 0] + 2 * M[1, 0] + M[2, 0]) / 4)
    assert np.isnan(obs.coadd(np.full((2, 3), np.nan))).all()


# ---- the host harness of obs_index.h ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("observe_host") / "libobserve_host.so"
    plan.compile_harness(out)
    return plan.bind(out)


audit = plan.audit


def designs(tile, stage):
    """(name, wav, lam, sig, k, f, n_orb): the shapes of tests/test_gpu_observe.py and the wide-support cases."""
    out = []
    for n_wav in (1, 2, 63, 64, 65, stage - 1, stage, stage + 1, 1500):
        wav = ref.grid_nonuniform(n_wav)
        for n_pix in (1, tile - 1, tile, tile + 1, 3 * tile + 5):
            lam = ref.pixels_over(wav, n_pix)
            sig = np.full(n_pix, 2.5e-10)
            sig[::7] = 1e-13            # between the nodes: empty supports
            out.append(("nonuniform %d x %d" % (n_wav, n_pix), wav, lam, sig, 5.0, None, 3))
    wav = ref.grid_coarse_fine()
    lam = ref.pixels_over(wav, 5 * tile + 3)
    sig = lam / (140000.0 * 2.3548)
    sig[tile + 3] = 1.0                 # the whole grid: fallback beside staged pixels
    out.append(("coarse/fine", wav, lam, sig, 5.0, None, 17))
    out.append(("coarse/fine frames", wav, lam, sig, 5.0, 1.0 + 1e-4 * np.linspace(-1, 1, 5), 5))
    out.append(("coarse/fine wide", wav, lam, sig * 40, 8.0, None, 9))
    # half-widths comparable with the wavelength itself: wav - L is no longer exact, the rounded targets of the
    # searches may leave a member out, and the membership test alone decides
    rng = np.random.default_rng(8)
    wav = np.sort(1e-6 + 2e-4 * rng.random(3000))
    lam = np.sort(2e-5 + 8e-5 * rng.random(2 * tile))
    out.append(("c ~ L", wav, lam, lam * (0.05 + 0.3 * rng.random(len(lam))), 5.0, None, 2))
    return out


def test_index_walk_finds_every_index_inside(harness):
    """Every workgroup, pixel, pass and lane of every design: no index outside the stage or the arrays, every support
    point read once, every output written once; staged, fallback and empty pixels are all reached; the supports are
    the reference's."""
    tile, stage = harness.obs_const(0), harness.obs_const(1)
    total = dict.fromkeys(COUNTERS, 0)
    for name, wav, lam, sig, k, f, n_orb in designs(tile, stage):
        cnt, supp = audit(harness, wav, lam, sig, k, f, n_orb)
        for key in ("staged_oor", "global_oor", "stage_load_oor", "out_oor"):
            assert cnt[key] == 0, (name, cnt)
        assert cnt["stage_max"] <= stage
        for g in range(supp.shape[0]):
            fo = 1.0 if f is None else f[g]
            for p in range(len(lam)):
                a, b = ref.support(wav, lam[p] * fo, k * (sig[p] * fo))
                assert (b - a == 0 and supp[g, p, 1] == supp[g, p, 0]) or (a, b) == tuple(supp[g, p]), (name, g, p)
        for key in COUNTERS:
            total[key] = max(total[key], cnt[key]) if key == "stage_max" else total[key] + cnt[key]
    print("index walk:", total)
    assert total["staged_pix"] > 0 and total["fallback_pix"] > 0 and total["empty_pix"] > 0
    assert total["stage_max"] == stage


def test_index_walk_stand_alone_under_sanitizers(tmp_path):
    """The harness' own main (a coarse / fine grid, both frame modes) built with -fsanitize=address,undefined."""
    exe = tmp_path / "observe_host"
    plan.compile_harness(exe, ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                "-DOBSERVE_HOST_MAIN"))
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
