"""Velocity maps without a GPU: the longdouble reference (tests/helpers/vmap_ref.py) and the host statistics of
observation.VelocityMap against closed forms, the factor helpers, the error bounds against plain float64, a planted
signal, the host harness of k_vmap's index arithmetic (prometheus_amd/csrc/vmap_index.h through
tests/helpers/vmap_host.cpp) and the refusals of Transit.velocity_map that need no device."""
import subprocess
import types

import numpy as np
import pytest

from helpers import observe_ref as ref
from helpers import vmap_plan as plan
from helpers import vmap_ref as vref

LD = np.longdouble


@pytest.fixture(scope="module")
def planted():
    d = vref.planted_design()
    d["mom"], d["n_used"], d["M"], d["n_max"] = vref.vmap(d["wav"], d["R"], d["lam"], d["sig"], d["k"], d["F"], d["data"],
                                                         d["ivar"])
    return d


# ---- the reference ---------------------------------------------------------------------------------------------
def test_reference_is_the_observation_per_column():
    """A trial's moments are those of the observation with f = F[:, j] (observe_ref.chi2 for m6), the observation's
    own frame plays no part, masked pixels and pixels off the grid are left out, no used pixel gives zeros."""
    wav = ref.grid_nonuniform(700)
    R = ref.spectrum(wav, 2)
    lam = ref.pixels_over(wav, 40)
    sig = np.full(40, 2.5e-10)
    rng = np.random.default_rng(1)
    data, ivar = 0.9 + 0.05 * rng.standard_normal((2, 40)), 1e4 * (0.1 + rng.random((2, 40)))
    ivar[0, 3], ivar[1, 5], data[1, 7], data[0, 9] = 0.0, np.inf, np.nan, np.inf
    F = np.array([[1.0 - 1e-5, 1.0, 1.0 + 3e-5, 2.0], [1.0 + 1e-5, 1.0 - 2e-5, 1.0, 0.5]])
    mom, nu, M, n_max = vref.vmap(wav, R, lam, sig, 5.0, F, data, ivar)
    assert mom.dtype == LD and nu.dtype == np.int64 and n_max > 0
    for j in range(4):
        num, den, _ = ref.observe(wav, R, lam, sig, 5.0, F[:, j])
        c2, n = ref.chi2(ref.model(num, den), den, data, ivar)
        assert np.array_equal(n, nu[:, j])
        assert np.all(np.abs(c2 - mom[:, j, 6]) <= 1e-17 * np.abs(c2))
    assert np.all(nu[:, 3] == 0) and np.all(mom[:, 3] == 0)          # factors 2 and 0.5: every pixel off the grid
    assert 0 < nu[0, 1] <= 40 - 2 and 0 < nu[1, 1] <= 40 - 2     # two masked pixels per phase at least
    # the identities between the moments: m6 = m3 - 2 m4 + m5
    live = nu > 0
    m = mom[live]
    assert np.all(np.abs(m[:, 3] - 2 * m[:, 4] + m[:, 5] - m[:, 6]) <= 1e-15 * m[:, 5])


# ---- the statistics --------------------------------------------------------------------------------------------
def test_statistics_closed_forms():
    from prometheus_amd import observation as obs
    rng = np.random.default_rng(2)
    n_orb, n_trial, n_pix = 3, 6, 50
    M = 0.9 + 0.05 * rng.standard_normal((n_orb, n_trial, n_pix))
    d = 0.9 + 0.05 * rng.standard_normal((n_orb, 1, n_pix))
    iv = 1e4 * (0.1 + rng.random((n_orb, 1, n_pix)))
    s = lambda x: np.sum(x, axis=-1)                                                  # noqa: E731
    mom = np.stack([s(iv + 0 * M), s(iv * M), s(iv * d + 0 * M), s(iv * M * M), s(iv * M * d), s(iv * d * d + 0 * M),
                    s(iv * (M - d) ** 2)], axis=-1)
    nu = np.full((n_orb, n_trial), n_pix, dtype=np.int64)
    vm = obs.VelocityMap(mom, nu, np.ones((n_orb, n_trial)))
    assert np.array_equal(vm.chi2, mom[..., 6])
    # chi2_scaled is the minimum over a of sum iv (a M - d)^2: at a = scale, and larger on either side
    for a_off in (0.0, 1e-3, -1e-3):
        a = vm.scale + a_off
        direct = s(iv * (a[..., None] * M - d) ** 2)
        if a_off == 0.0:
            assert np.allclose(direct, vm.chi2_scaled, rtol=1e-9)
        else:
            assert np.all(direct > vm.chi2_scaled)
    w = s(iv + 0 * M)
    Mb, db = s(iv * M) / w, s(iv * d + 0 * M) / w
    ccf = s(iv * (M - Mb[..., None]) * (d - db[..., None]))
    assert np.allclose(vm.ccf, ccf, rtol=1e-7, atol=1e-9 * np.abs(ccf).max())
    sf = s(iv * (d - db[..., None]) ** 2 + 0 * M) / w
    sg = s(iv * (M - Mb[..., None]) ** 2) / w
    want = -0.5 * n_pix * np.log(sf - 2 * ccf / w + sg)
    assert np.allclose(vm.loglike, want, rtol=1e-6)
    # total and grid
    assert np.array_equal(vm.total("chi2"), vm.chi2.sum(axis=0)) and vm.total("loglike").shape == (n_trial,)
    assert np.array_equal(vm.total(vm.ccf), vm.ccf.sum(axis=0))
    g = vm.grid("chi2", 2, 3)
    assert g.shape == (n_orb, 2, 3) and g[1, 1, 2] == vm.chi2[1, 1 * 3 + 2]
    assert vm.grid(vm.total("chi2"), 3, 2).shape == (3, 2) and vm.grid(vm.total("chi2"), 3, 2)[2, 1] == vm.total("chi2")[5]
    with pytest.raises(ValueError):
        vm.grid("chi2", 4, 2)
    with pytest.raises(ValueError):
        vm.total("nope")
    with pytest.raises(ValueError):
        obs.VelocityMap(mom[..., :6], nu, np.ones((n_orb, n_trial)))


def test_statistics_zero_denominators_give_nan():
    from prometheus_amd import observation as obs
    mom = np.zeros((1, 3, 7))
    nu = np.zeros((1, 3), dtype=np.int64)
    mom[0, 1] = [2.0, 0.0, 3.0, 0.0, 0.0, 5.0, 5.0]      # a model of zeros: m3 = 0
    mom[0, 2] = [2.0, 2.0, 3.0, 2.5, 3.0, 5.0, 1.5]
    nu[0, 1:] = 2
    vm = obs.VelocityMap(mom, nu, np.ones((1, 3)))
    assert vm.chi2[0, 0] == 0.0
    for name in ("chi2_scaled", "scale", "ccf", "loglike"):
        v = getattr(vm, name)
        assert np.isnan(v[0, 0]), name
        assert np.isfinite(v[0, 2]), name
    assert np.isnan(vm.chi2_scaled[0, 1]) and np.isnan(vm.scale[0, 1]) and np.isfinite(vm.ccf[0, 1])
    assert vm.chi2_scaled[0, 2] == 5.0 - 9.0 / 2.5 and vm.scale[0, 2] == 3.0 / 2.5 and vm.ccf[0, 2] == 3.0 - 2.0 * 3.0 / 2.0


# ---- the factor helpers ----------------------------------------------------------------------------------------
def test_factor_helpers():
    from prometheus_amd import constants as const
    from prometheus_amd import observation as obs
    base = np.array([0.9999, 1.0, 1.0002])
    vel = np.array([-4e6, 0.0, 2e5, 4e6])
    F = obs.trial_factors(base, vel)
    assert F.shape == (3, 4) and F.flags.c_contiguous
    assert np.array_equal(F, base[:, None] * const.calculateDopplerShift(vel)[None, :])
    assert np.array_equal(F[:, 1], base)
    assert np.array_equal(obs.trial_factors(None, vel), const.calculateDopplerShift(vel)[None, :])
    orb = np.linspace(-0.05, 0.05, 5)
    Kp, Vs = np.array([1.0e7, 1.5e7, 2.0e7]), np.array([-2e6, 0.0])
    K = obs.kp_vsys_factors(orb, Kp, Vs)
    assert K.shape == (5, 6)
    for o in range(5):
        for i in range(3):
            for l in range(2):
                assert K[o, i * 2 + l] == const.calculateDopplerShift(-Kp[i] * np.sin(orb[o]) + Vs[l])
    assert np.all(np.diff(K[0, ::2]) < 0) and np.all(np.diff(K[-1, ::2]) > 0)     # ingress: approaching... receding


def test_kp_vsys_reproduces_the_planet_frame_bitwise():
    from prometheus_amd import constants as const
    from prometheus_amd import observation as obs
    from prometheus_amd.celestialBodies import AvailablePlanets
    planet = AvailablePlanets().findPlanet("WASP-49b")
    orb = np.linspace(-0.04, 0.04, 17)
    Kp = np.sqrt(const.G * planet.hostStar.M / planet.a)
    assert np.array_equal(obs.kp_vsys_factors(orb, [Kp], [0.0])[:, 0], obs.planet_frame_shifts(planet, orb))


# ---- the error bounds ------------------------------------------------------------------------------------------
def test_float64_orders_stay_far_below_the_bounds(planted):
    """The bounds of the GPU tests (vmap_ref.bounds) against what float64 evaluation does in forward and in reverse
    order on the planted design (every 5th trial): below 0.1 of them, so they are not tight."""
    d = planted
    cols = slice(0, None, 5)
    F = np.ascontiguousarray(d["F"][:, cols])
    worst = np.zeros(7)
    for reverse in (False, True):
        mom, nu = vref.float64_moments(d["wav"], d["R"], d["lam"], d["sig"], d["k"], F, d["data"], d["ivar"], reverse)
        assert np.array_equal(nu, d["n_used"][:, cols])
        worst = np.maximum(worst, vref.fractions(mom, d["mom"][:, cols], nu, d["k"], d["n_max"]))
    print("float64 orders, fraction of the bound per moment:", worst)
    assert np.all(worst < 0.1), worst


# ---- a planted signal ------------------------------------------------------------------------------------------
def test_planted_signal_is_found_by_chi2(planted):
    from prometheus_amd import observation as obs
    d = planted
    vm = obs.VelocityMap(d["mom"].astype(np.float64), d["n_used"], d["F"])
    assert d["F"].shape == (3, 41) and d["vel"][d["j_star"]] == 6.0e5 and np.all(d["n_used"] == 64)
    for stat in (vm.chi2, vm.chi2_scaled):
        assert np.all(np.argmin(stat, axis=1) == d["j_star"])
    second = np.sort(vm.chi2, axis=1)[:, 1]
    print("planted signal: chi2 at the column", vm.chi2[:, d["j_star"]], "second smallest", second)
    assert np.all(vm.chi2[:, d["j_star"]] < 1e-20) and np.all(second >= 141.0)
    assert int(np.argmin(vm.total("chi2"))) == d["j_star"] and int(np.argmax(vm.total("loglike"))) == d["j_star"]
    assert np.all(np.abs(vm.scale[:, d["j_star"]] - 1.0) < 1e-12)


# ---- the host harness of vmap_index.h --------------------------------------------------------------------------
SMALL = dict(tile=4, stage=40, chunk=2, trials=3)


@pytest.fixture(scope="module")
def harnesses(tmp_path_factory):
    d = tmp_path_factory.mktemp("vmap_host")
    plan.compile_harness(d / "libvmap_host.so")
    plan.compile_harness(d / "libvmap_host_small.so", defines=plan.small_constants(**SMALL))
    return plan.bind(d / "libvmap_host.so"), plan.bind(d / "libvmap_host_small.so")


def kms(v):
    return vref.doppler(1e5 * np.asarray(v, dtype=np.float64))


def designs(c):
    """(name, wav, lam, sig, k, F, cap_bytes) for constants c: the shapes of tests/test_gpu_vmap.py, trial groups
    +-300 km/s wide, pixels off both ends, duplicated grid points and pixels, one grid point, c ~ L, batches."""
    tile, stage, chunk, T = c["tile"], c["stage"], c["chunk"], c["trials"]
    out = []
    near = kms(np.linspace(-6.0, 6.0, 2 * T + 1))
    for n_wav in (1, 2, 63, 64, 65, stage - 1, stage, stage + 1):
        wav = ref.grid_nonuniform(n_wav)
        lam = ref.pixels_over(wav, 5)
        out.append(("n_wav %d" % n_wav, wav, lam, np.full(5, 2.5e-10), 5.0, np.tile(near[:3], (2, 1)), plan.DEFAULT_CAP))
    wav = ref.grid_nonuniform(min(1500, 12 * stage))
    for n_pix in (1, tile - 1, tile, tile + 1, tile * chunk - 1, tile * chunk, tile * chunk + 1):
        lam = ref.pixels_over(wav, n_pix)
        sig = np.full(n_pix, 2.5e-10)
        sig[::7] = 1e-13                # between the nodes: empty supports
        out.append(("n_pix %d" % n_pix, wav, lam, sig, 5.0, np.tile(near[:2], (3, 1)), plan.DEFAULT_CAP))
    lam = ref.pixels_over(wav, tile + 1)
    for n_trial in (1, T - 1, T, T + 1, 2 * T + 1):
        F = np.tile(near[:n_trial], (2, 1)) * np.array([[1.0], [1.0 + 2e-5]])
        out.append(("n_trial %d" % n_trial, wav, lam, np.full(len(lam), 2.5e-10), 5.0, F, plan.DEFAULT_CAP))
        out.append(("n_trial %d in batches" % n_trial, wav, lam, np.full(len(lam), 2.5e-10), 5.0, F, 1))
    # a +-300 km/s column in every group: the union exceeds the stage, some supports are read from global memory
    wav = ref.grid_coarse_fine(1200, 150)
    lam = ref.pixels_over(wav, 2 * tile + 3)
    sig = lam / (140000.0 * 2.3548)
    sig[tile + 1] = 1.0                 # the whole grid
    wide = near.copy()
    wide[1::T] = kms(300.0)
    wide[0] = kms(-300.0)
    out.append(("+-300 km/s", wav, lam, sig, 5.0, np.tile(wide, (2, 1)), plan.DEFAULT_CAP))
    out.append(("descending factors", wav, lam, sig, 5.0, np.tile(wide[::-1], (1, 1)), plan.DEFAULT_CAP))
    # half-widths comparable with the wavelength itself: the targets are not monotone enough to trust, obs_trim decides
    rng = np.random.default_rng(8)
    wav = np.sort(1e-6 + 2e-4 * rng.random(3000))
    lam = np.sort(2e-5 + 8e-5 * rng.random(2 * tile))
    out.append(("c ~ L", wav, lam, lam * (0.05 + 0.3 * rng.random(len(lam))), 5.0,
                np.tile(1.0 + 0.3 * rng.random(T + 2), (2, 1)), plan.DEFAULT_CAP))
    out.append(("k sig > lam", wav, lam, lam * 0.4, 5.0, np.tile(1.0 + 0.3 * rng.random(T + 2), (1, 1)), plan.DEFAULT_CAP))
    return out


@pytest.mark.parametrize("which", ["real", "small"])
def test_index_walk_finds_every_index_inside(harnesses, which):
    """Every batch, phase, chunk, tile, trial group, pixel, trial, pass and lane of every design, with the real
    constants and with small ones: no index outside the stage, the arrays or the scratch, every support point read
    once, every (phase, trial, pixel) visited once, every partial record written once and read, a bracketed search
    gives the full search's answer; staged, fallback and empty supports are all reached; the supports are the
    reference's."""
    L = harnesses[0 if which == "real" else 1]
    c = plan.constants(L)
    if which == "small":
        assert {k: c[k] for k in SMALL} == SMALL
    total = dict.fromkeys(plan.COUNTERS, 0)
    for name, wav, lam, sig, k, F, cap in designs(c):
        cnt, supp = plan.audit(L, wav, lam, sig, k, F, cap)
        for key in plan.ERRORS:
            assert cnt[key] == 0, (name, cnt)
        assert cnt["stage_max"] <= c["stage"]
        if cap == 1:
            assert cnt["batches"] == -(-F.shape[1] // c["trials"]), (name, cnt)
        for o in range(F.shape[0]):
            for j in range(F.shape[1]):
                for p in range(len(lam)):
                    a, b = ref.support(wav, lam[p] * F[o, j], k * (sig[p] * F[o, j]))
                    s = supp[o, j, p]
                    assert (b - a == 0 and s[1] == s[0]) or (a, b) == tuple(s), (name, o, j, p)
        for key in plan.COUNTERS:
            total[key] = max(total[key], cnt[key]) if key == "stage_max" else total[key] + cnt[key]
    print("index walk (%s):" % which, total)
    assert total["staged"] > 0 and total["fallback"] > 0 and total["empty"] > 0
    assert total["stage_max"] == c["stage"]
    assert total["bracket_searches"] > 0 and total["full_searches"] > 0


def test_index_walk_stand_alone_under_sanitizers(tmp_path):
    """The harness' own main (a coarse / fine grid, groups a few km/s and +-300 km/s wide, one batch and three) built
    with -fsanitize=address,undefined and run as a program."""
    exe = tmp_path / "vmap_host"
    plan.compile_harness(exe, ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                "-DVMAP_HOST_MAIN"))
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0


# ---- Transit.velocity_map without a device ---------------------------------------------------------------------
def _bare_transit(n_wav, n_orb):
    """A Transit with a grid and phases and nothing a device could run: velocity_map must refuse before it needs one."""
    from prometheus_amd import gasProperties as gp
    tr = gp.Transit.__new__(gp.Transit)
    tr.wavelength = 5880e-8 + 1e-11 * np.arange(n_wav)
    tr.spatialGrid = types.SimpleNamespace(constructOrbphaseAxis=lambda: np.linspace(-0.03, 0.03, n_orb))
    tr.atmosphere = types.SimpleNamespace(densityDistributionList=[])
    tr.last_stats, tr.collect_stats = [], False
    return tr


def test_velocity_map_refuses_before_touching_a_device():
    from prometheus_amd import observation as obs
    n_orb = 3
    tr = _bare_transit(20000, n_orb)
    ins = obs.Instrument(tr.wavelength[[100, 200, 300]], resolving_power=140000.0)
    F = obs.trial_factors(np.ones(n_orb), [-2e5, 0.0, 2e5])
    with pytest.raises(ValueError, match="no data"):
        tr.velocity_map(obs.Observation(ins, n_orb), F)
    with pytest.raises(TypeError):
        tr.velocity_map(ins, F)
    data = obs.Observation(ins, n_orb, None, np.ones((n_orb, 3)), np.full((n_orb, 3), 1e-3))
    with pytest.raises(ValueError, match="not additive over wavelength partials.*one device.*max_memory_gb"):
        tr.velocity_map(data, F, devices=[0, 1])
    with pytest.raises(ValueError, match="not additive over wavelength partials.*one device.*max_memory_gb"):
        tr.velocity_map(data, F, devices=[0], max_memory_gb=1e-9)     # chunks of 4,096 wavelengths: five of them
    with pytest.raises(ValueError, match="phases"):
        tr.velocity_map(obs.Observation(ins, 2, None, np.ones((2, 3)), np.full((2, 3), 1e-3)), F)
    with pytest.raises(ValueError, match=r"\[n_orb\]\[n_trial\]"):
        tr.velocity_map(data, F[:2])
    with pytest.raises(ValueError, match="finite and positive"):
        tr.velocity_map(data, np.where(F == F[0, 0], 0.0, F))
