"""Broadened spectra without a device: the host harness of k_broaden's index arithmetic and evaluation text
(tests/helpers/broaden_host.cpp, a stand-alone program, plain and sanitized), the float64 reference of the definition
(tests/helpers/broaden_ref.py) against its longdouble reference and bound, observation.rotation_kernel /
gaussian_velocity_kernel / tidally_locked_speed, the refusals of observation.Broadening and of the Transit methods
that come before a device is needed, and the sign convention."""
import os
import subprocess
import types

import numpy as np
import pytest

from helpers import broaden_ref as bref
from helpers import observe_ref as oref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "prometheus_amd", "csrc")
HOST = os.path.join(REPO, "tests", "helpers", "broaden_host.cpp")
U = 2.0 ** -53
STAGE = 576   # kBrStage


# ---- the harness -------------------------------------------------------------------------------------------------
def _design_file(path, wav, R, K, b0, s, want):
    vals = lambda a: " ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel())
    with open(path, "w") as f:
        f.write("%d %d %d %s %s\n%s\n%s\n%s\n%s\n" % (len(wav), R.shape[0], len(K), float(b0).hex(), float(s).hex(),
                                                     vals(wav), vals(R), vals(K), vals(want)))


def _fields(line):
    return {k: v for k, v in (p.split("=") for p in line.split())}


def _harness_cases():
    """name -> (wav, R, K, b0, s, expectation on the paths)."""
    cases = {}
    for name, (wav, K, b0, s) in bref.designs().items():
        cases[name] = (wav, oref.spectrum(wav, 3, seed=4), K, b0, s, "staged")
    wav, K, b0, s = bref.wide_design()
    cases["wide"] = (wav, oref.spectrum(wav, 2, seed=5), K, b0, s, "global")
    wav, K, b0, s = bref.mixed_design()
    cases["mixed"] = (wav, oref.spectrum(wav, 9, seed=6), K, b0, s, "both")
    wav, K, b0, s = bref.shift_design()
    R = oref.spectrum(wav, 2, seed=7)
    R[1, 700] = np.nan
    cases["shift with NaN"] = (wav, R, K, b0, s, "staged")
    for n in (1, 2, 255, 256, 257):
        wav = oref.grid_nonuniform(n)
        cases["n_wav=%d" % n] = (wav, oref.spectrum(wav, 9, seed=n), *bref.kernel(33, -3e5, 3e5)[0:3], "staged")
    return cases


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_harness_walks_every_tile_and_lane_and_matches_the_reference_bitwise(tmp_path, which):
    """Over the shared designs, the wide and the mixed design, a pure shift with a NaN and the tile-edge sizes: every
    output is owned once, each lane's ends are the membership's, a tile is staged only when its union fits (and then
    no lane reads outside it), the record index stays in range, the staged walk equals the global one and the shared
    evaluation text equals broaden_f64 bit for bit.  The wide design stages nothing, the mixed one takes both paths."""
    flags = {"plain": ("-O2",), "sanitized": ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")}
    exe = tmp_path / "broaden_host"
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags[which], "-I" + CSRC, HOST, "-o", str(exe)],
                   check=True)
    for name, (wav, R, K, b0, s, paths) in _harness_cases().items():
        want = bref.broaden_f64(wav, R, K, b0, s)
        path = tmp_path / "design.txt"
        _design_file(path, wav, R, K, b0, s, want)
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        print(name, r.stdout, r.stderr)
        assert r.returncode == 0, name
        f = _fields(r.stdout.strip())
        for key in ("owner_err", "end_err", "stage_err", "rec_err", "mismatch", "path_err"):
            assert f[key] == "0", (name, key)
        assert int(f["tiles"]) == (len(wav) + 255) // 256 and int(f["groups"]) == (R.shape[0] + 7) // 8
        assert int(f["lds"]) <= 65536
        assert int(f["window"]) + int(f["searched"]) == int(f["tiles"])
        if paths == "staged":
            assert f["global"] == "0" and f["searched"] == "0", name      # every tile keeps its window
        if paths == "global":
            assert f["staged"] == "0" and f["window"] == "0" and int(f["support_min"]) > 0, name
        if paths == "both":
            assert int(f["staged"]) > 0 and int(f["global"]) > 0, name
        if name == "coarse_fine n_k=33":
            assert f["support_min"] == "1"                       # one-point supports in the coarse wings
        if name == "nonuniform n_k=2":
            assert 1 <= int(f["support_min"]) <= 3                  # a few points ...
        if name == "nonuniform n_k=1025":
            assert 100 <= int(f["support_max"]) <= STAGE - 256      # ... to more than a hundred, inside a stage
        if name == "shift with NaN":
            assert f["support_min"] == "0"
            assert np.isnan(want[0]).sum() > 0 and np.isnan(want[1]).sum() > np.isnan(want[0]).sum()


# ---- the reference and its bound -----------------------------------------------------------------------------------
def test_float64_definition_stays_inside_the_bound_of_the_longdouble_reference():
    """broaden_f64 against broaden_ld on every shared design (2, 33, 65 and 1025 nodes among them): inside the bound
    derived from the definition; the print shows how far."""
    worst = 0.0
    for name, (wav, K, b0, s) in bref.designs().items():
        R = oref.spectrum(wav, 2, seed=11)
        got = bref.broaden_f64(wav, R, K, b0, s)
        ref, cnt, rmax, gsum, qsum = bref.broaden_ld(wav, R, K, b0, s)
        tol = bref.bound(K, b0, s, cnt, rmax, gsum, qsum)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), name
        ok = ~np.isnan(got)
        err = np.abs(got.astype(np.longdouble) - ref)[ok].astype(np.float64)
        frac = float((err / tol[ok]).max())
        rel = float((err / np.abs(ref[ok]).astype(np.float64)).max() / U)
        print("%-28s supports %d..%d  max err / bound %.4f  max relative error %.1f u" % (name, cnt.min(), cnt.max(),
                                                                                      frac, rel))
        assert np.all(err <= tol[ok]), name
        worst = max(worst, frac)
    assert worst > 1e-4       # the bound is not vacuous: the error reaches a visible fraction of it


def test_a_wrong_evaluation_leaves_the_bound():
    """The bound tells the definition from near misses: a kernel whose every second node's value is held for two nodes
    and a first node moved by 1 % of b0 both leave it by far."""
    wav, K, b0, s = bref.designs()["nonuniform n_k=33"]
    R = oref.spectrum(wav, 1, seed=12)
    ref, cnt, rmax, gsum, qsum = bref.broaden_ld(wav, R, K, b0, s)
    tol = bref.bound(K, b0, s, cnt, rmax, gsum, qsum)
    stepped = np.repeat(K[::2], 2)[:len(K)]                          # every second node's value held for two nodes
    for wrong in (bref.broaden_f64(wav, R, stepped, b0, s), bref.broaden_f64(wav, R, K, b0 * 1.01, s)):
        ok = ~np.isnan(wrong) & ~np.isnan(ref)
        err = np.abs(wrong.astype(np.longdouble) - ref)[ok].astype(np.float64)
        assert (err / tol[ok]).max() > 100.0


def test_support_is_contiguous_and_nan_reaches_exactly_its_outputs():
    """support() asserts contiguity on every output; a NaN planted in one row reaches exactly the outputs whose
    support holds it, also where its weight is zero, and no other row."""
    wav, K, b0, s = bref.designs()["nonuniform n_k=65 random"]
    R = oref.spectrum(wav, 2, seed=13)
    R[1, 640] = np.nan
    got = bref.broaden_f64(wav, R, K, b0, s)
    holds = np.array([a <= 640 < b for a, b, _ in (bref.support(wav, w, len(K), b0, s) for w in range(len(wav)))])
    assert holds.sum() > 10
    assert np.array_equal(np.isnan(got[1]), holds) and not np.isnan(got[0]).any()
    # an output that sees the NaN through a weight of exactly zero: between two zero nodes kern = 0 + a 0 = 0, and
    # 0 NaN is still NaN
    wav = oref.grid_dyadic(64)
    K, b0, s = np.array([0.0, 0.0, 1.0, 0.0, 0.0]), -2.0 ** -15, 2.0 ** 16      # nodes at -2 .. +2 grid steps
    R = np.ones((1, 64))
    R[0, 32] = np.nan
    a, b, t = bref.support(wav, 30, 5, b0, s)
    assert a <= 32 < b and 3.0 < t[32 - a] <= 4.0                      # output 30 holds point 32 between zero nodes
    got = bref.broaden_f64(wav, R, K, b0, s)
    holds = [w for w in range(64) if (lambda ab: ab[0] <= 32 < ab[1])(bref.support(wav, w, 5, b0, s))]
    assert 30 in holds and len(holds) >= 4 and np.array_equal(np.flatnonzero(np.isnan(got[0])), holds)
    assert not np.isnan(bref.broaden_f64(wav, np.ones((1, 64)), K, b0, s)).any()


# ---- the kernels of observation.py -----------------------------------------------------------------------------------
def test_rotation_kernel_sums_to_one_is_symmetric_and_follows_wind_and_limbs():
    from prometheus_amd import observation as obs
    for n in (2, 33, 64, 65, 1025):
        v, w = obs.rotation_kernel(4e5, n=n)
        assert len(v) == len(w) == n and abs(w.sum() - 1.0) <= 4 * U * n
        assert np.allclose(w, w[::-1], rtol=0, atol=1e-15) and np.allclose(v, -v[::-1], rtol=0, atol=1e-6)
        assert v[0] == -4e5 and v[-1] == 4e5 and np.all(w > 0)
        assert abs((v * w).sum()) <= 1e-9 * 4e5
    v, w = obs.rotation_kernel(4e5, n=65)
    assert w[0] > w[1] > w[32] and w[-1] > w[32]                        # the horns
    # the exact cell integrals: the first cell holds arcsin's share of the ring however narrow it is
    assert abs(w[0] - (np.arcsin(-1.0 + 1.0 / 64) + np.pi / 2) / np.pi) <= 1e-15
    v2, w2 = obs.rotation_kernel(4e5, n=65, wind=-1.5e5)
    assert np.array_equal(w2, w) and abs((v2 * w2).sum() - (v * w).sum() + 1.5e5) <= 1e-9 * 4e5
    v3, w3 = obs.rotation_kernel(4e5, n=65, east_west=(3.0, 1.0))
    assert abs(w3.sum() - 1.0) <= 1e-14
    # (the centre node's cell lies half on either side: the receding half holds 3/4 of the ring)
    assert abs(w3[33:].sum() / w3[:32].sum() - 3.0) <= 1e-12
    v4, w4 = obs.rotation_kernel(4e5, n=64, east_west=(0.0, 1.0))       # no centre node: the halves are the nodes'
    assert np.all(w4[32:] <= 1e-16) and abs(w4[:32].sum() - 1.0) <= 1e-14   # (a cell's end rounds past 0)
    for bad in (dict(v_eq=0.0), dict(v_eq=np.nan), dict(v_eq=1e5, n=1), dict(v_eq=1e5, n=1026),
                dict(v_eq=1e5, east_west=(0.0, 0.0)), dict(v_eq=1e5, east_west=(1.0, -1.0)), dict(v_eq=1e5, wind=np.inf)):
        with pytest.raises(ValueError):
            obs.rotation_kernel(**bad)


def test_gaussian_velocity_kernel_and_tidally_locked_speed():
    from prometheus_amd import observation as obs, constants as const
    v, w = obs.gaussian_velocity_kernel(2e5, truncate=4.0, n=65)
    assert v[0] == -8e5 and v[-1] == 8e5 and abs(w.sum() - 1.0) <= 1e-14 and np.allclose(w, w[::-1], rtol=0, atol=1e-16)
    assert abs(np.sqrt((v * v * w).sum()) / 2e5 - 1.0) < 2e-3            # its standard deviation
    with pytest.raises(ValueError):
        obs.gaussian_velocity_kernel(0.0)
    star = types.SimpleNamespace(M=1.989e33)
    planet = types.SimpleNamespace(R=1.3 * 7.1492e9, a=0.05 * 1.496e13, hostStar=star)
    want = planet.R * np.sqrt(const.G * star.M / planet.a ** 3)
    assert obs.tidally_locked_speed(planet) == pytest.approx(want, rel=1e-15)
    assert 1e5 < want < 1e6                                             # a hot Jupiter: a few km/s


def test_broadening_forms_the_device_kernel_and_rejects_bad_input():
    from prometheus_amd import observation as obs, constants as const
    v, w = obs.rotation_kernel(4e5, n=33, wind=-1e5, east_west=(2.0, 1.0))
    b = obs.Broadening(v, w)
    assert np.array_equal(b.K, w[::-1]) and b.b0 == -v[-1] / const.c and b.s == pytest.approx(const.c / 0.25e5, rel=1e-12)
    # node i of K sits at beta = b0 + i / s = -v[n - 1 - i] / c
    assert np.allclose(b.b0 + np.arange(33) / b.s, -v[::-1] / const.c, rtol=0, atol=1e-18)
    assert b.key == obs.Broadening(list(v), list(w)).key and b.key != obs.Broadening(v, w[::-1]).key
    lin = np.linspace(-1e5, 1e5, 9)
    one = np.ones(9)
    bad = {
        "non-uniform": (lin * np.abs(lin) / 1e5, one),
        "descending": (lin[::-1], one),
        "negative": (lin, np.where(np.arange(9) == 3, -1e-3, 1.0)),
        "NaN weight": (lin, np.where(np.arange(9) == 3, np.nan, 1.0)),
        "NaN velocity": (np.where(np.arange(9) == 3, np.nan, lin), one),
        "all zero": (lin, 0.0 * one),
        "one node": (lin[:1], one[:1]),
        "1026 nodes": (np.linspace(-1e5, 1e5, 1026), np.ones(1026)),
        "two lengths": (lin, one[:8]),
        "2-D": (lin.reshape(3, 3), one.reshape(3, 3)),
        "repeated": (np.zeros(9), one),
    }
    for name, (vv, ww) in bad.items():
        with pytest.raises(ValueError):
            print("case:", name)
            obs.Broadening(vv, ww)
    with pytest.raises(TypeError):
        obs.Broadening("fast", [1.0, 1.0])
    obs.Broadening(np.linspace(-1e5, 1e5, 1025), np.ones(1025))
    obs.Broadening([0.0, 1e5], [0.0, 1.0])


def test_transit_methods_refuse_a_bad_broaden_before_a_device_is_needed():
    """TypeError for anything but a Broadening and ValueError for a run that would be split, from every method, with
    no library loaded: the Transit is a stub whose device path would fail."""
    from prometheus_amd import gasProperties as gp, observation as obs
    tr = gp.Transit.__new__(gp.Transit)
    tr.spatialGrid = types.SimpleNamespace(constructOrbphaseAxis=lambda: np.zeros(3))
    tr.wavelength = np.linspace(5e-5, 6e-5, 10000)
    tr._wavelength_chunk = lambda max_memory_gb, n_orb: 4096
    tr._integrate = lambda *a, **k: (_ for _ in ()).throw(AssertionError("a device was asked for"))
    ins = obs.Instrument(np.linspace(5.2e-5, 5.8e-5, 50), resolving_power=1e5)
    bk = obs.Broadening(*obs.rotation_kernel(4e5, n=9))
    with pytest.raises(TypeError, match="observe: broaden must be an observation.Broadening"):
        tr.observe(ins, broaden=(1.0, 2.0))
    with pytest.raises(ValueError, match="observe: the run would be split into 1 wavelength shard"):
        tr.observe(ins, broaden=bk)
    with pytest.raises(ValueError, match="observe: the run would be split into 2 wavelength shard"):
        tr.observe(ins, broaden=bk, devices=[0, 1])
    with pytest.raises(TypeError, match="broadened: broaden"):
        tr.broadened(None)
    with pytest.raises(ValueError, match="broadened: the run would be split"):
        tr.broadened(bk)
    ob = obs.Observation(ins, 3, data=np.ones((3, 50)), err=np.ones((3, 50)))
    with pytest.raises(TypeError, match="velocity_map: broaden"):
        tr.velocity_map(ob, np.ones((3, 2)), broaden="ring")
    with pytest.raises(ValueError, match="velocity_map: the run would be split"):
        tr.velocity_map(ob, np.ones((3, 2)), broaden=bk)
    ex = obs.Exposures(ins, [[0]], [[1.0]], [[1.0]], np.ones((1, 50)), np.ones((1, 50)))
    with pytest.raises(TypeError, match="expose: broaden"):
        tr.expose(ex, broaden=4e5)
    with pytest.raises(ValueError, match="expose: the run would be split"):
        tr.expose(ex, broaden=bk)


# ---- the sign convention -----------------------------------------------------------------------------------------------
def test_gas_moving_away_moves_the_line_to_the_red():
    """A narrow line broadened with all weight at +v has its centroid at lambda_0 (1 + v / c): the definition
    (broaden_f64) with observation.Broadening's kernel."""
    from prometheus_amd import observation as obs, constants as const
    lam0, v = 5890e-8, 6e5
    wav = lam0 * (1.0 + np.arange(-400, 401) * (0.3e5 / const.c))       # 0.3 km/s per point
    depth = np.exp(-0.5 * ((wav / lam0 - 1.0) * const.c / 0.6e5) ** 2)  # a line 0.6 km/s wide at lambda_0
    R = 1.0 - 0.4 * depth
    b = obs.Broadening([v - 0.3e5, v, v + 0.3e5], [0.0, 1.0, 0.0])
    Rb = bref.broaden_f64(wav, R[None, :], b.K, b.b0, b.s)[0]
    ok = ~np.isnan(Rb)
    assert ok.sum() > 700
    centroid = ((1.0 - Rb[ok]) * wav[ok]).sum() / (1.0 - Rb[ok]).sum()
    assert abs(centroid / lam0 - (1.0 + v / const.c)) < 0.01e5 / const.c        # to 0.01 km/s
    assert abs(((1.0 - R) * wav).sum() / (1.0 - R).sum() / lam0 - 1.0) < 1e-9
