"""Exposures without a device: the longdouble reference (tests/helpers/expose_ref.py) and its bounds, the tap tables of
observation.exposure_taps, the refusals of observation.Exposures and Transit.expose, and the host walk of k_expose's
index arithmetic (tests/helpers/expose_host.cpp, a stand-alone program)."""
import os
import subprocess
import types

import numpy as np
import pytest

from helpers import expose_ref as eref
from helpers import observe_ref as ref
from helpers import vmap_ref as vref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "prometheus_amd", "csrc")
HOST = os.path.join(REPO, "tests", "helpers", "expose_host.cpp")
U = 2.0 ** -53


# ---- the reference -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def design():
    """A fine core, 24 pixels at R = 140,000 (supports of about 180 points), 3 rows of R, 3 trials."""
    wav = ref.grid_coarse_fine(1200, 40)
    R = ref.spectrum(wav, 3)
    lam = wav[40 + 600] + 1e-10 * (np.arange(24) - 11.5)
    sig = lam / (140000.0 * 2.3548)
    F = np.stack([vref.doppler(1e5 * (np.array([-4.0, 0.0, 4.0]) + 2.0 * o)) for o in range(3)])
    rng = np.random.default_rng(5)
    data = 0.9 + 0.05 * rng.random((3, len(lam)))
    ivar = 1e4 * (0.1 + rng.random((3, len(lam))))
    return dict(wav=wav, R=R, lam=lam, sig=sig, k=5.0, F=F, data=data, ivar=ivar)


def test_reference_reduces_to_the_velocity_map(design):
    d = design
    rows, a, F = eref.degenerate(d["F"])
    mom, nu, M, n_max, k_live = eref.expose(d["wav"], d["R"], d["lam"], d["sig"], d["k"], rows, a, F, d["data"], d["ivar"])
    vmom, vnu, vM, vmax = vref.vmap(d["wav"], d["R"], d["lam"], d["sig"], d["k"], d["F"], d["data"], d["ivar"])
    assert k_live == 1 and n_max == vmax and n_max > 100
    assert np.array_equal(nu, vnu) and np.array_equal(mom, vmom) and np.array_equal(M, vM, equal_nan=True)
    # ... and its bounds to the map's with (K_live + 1) u = 2 u more on the model
    b, vb = eref.bounds(mom, nu, d["k"], n_max, 1), vref.bounds(vmom, vnu, d["k"], vmax)
    assert np.all(b >= vb) and np.all(b <= vb * (1.0 + 1e-2))


def _smeared(d):
    """3 exposures of 4 taps over the 3 rows: a dead tap among them, weights that sum to 1."""
    rows = np.array([[0, 1, 0, 1], [1, 2, 1, 2], [2, 0, 1, 0]], dtype=np.int32)
    a = np.array([[0.3, 0.2, 0.1, 0.4], [0.5, 0.0, 0.25, 0.25], [0.125, 0.125, 0.25, 0.5]])
    F = d["F"][rows][:, :, :].transpose(0, 2, 1) * (1.0 + 3e-6 * np.arange(4))[None, None, :]
    return rows, a, np.ascontiguousarray(F)


def test_float64_orders_stay_far_below_the_bounds(design):
    """The bounds of the GPU tests (expose_ref.bounds) against what float64 evaluation does with the support's points,
    the taps and the pixels in forward and in reverse order: measured here at 0.083 of them at most (the print; the
    largest are the data's own sums m0, m2 and m5), and
    asserted below 0.1 as for the map, so they are not tight."""
    d = design
    rows, a, F = _smeared(d)
    want = eref.expose(d["wav"], d["R"], d["lam"], d["sig"], d["k"], rows, a, F, d["data"], d["ivar"])
    assert want[4] == 4 and np.all(want[1] == len(d["lam"]))
    worst = np.zeros(7)
    for reverse in (False, True):
        mom, nu = eref.float64_moments(d["wav"], d["R"], d["lam"], d["sig"], d["k"], rows, a, F, d["data"], d["ivar"],
                                       reverse)
        assert np.array_equal(nu, want[1])
        worst = np.maximum(worst, eref.fractions(mom, want[0], nu, d["k"], want[3], want[4]))
    print("float64 orders, fraction of the bound per moment:", worst)
    assert np.all(worst < 0.1), worst


def test_reference_padding_and_coverage(design):
    """Dead taps change nothing wherever they stand; a live tap off the grid takes the model away."""
    d = design
    rows, a, F = _smeared(d)
    base = eref.expose(d["wav"], d["R"], d["lam"], d["sig"], d["k"], rows, a, F, d["data"], d["ivar"])
    pad_r = np.concatenate([np.full((3, 1), 2), rows, np.full((3, 1), 0)], axis=1)
    pad_a = np.concatenate([np.zeros((3, 1)), a, np.zeros((3, 1))], axis=1)
    pad_F = np.concatenate([np.full((3, 3, 1), 7.0), F, np.full((3, 3, 1), 0.1)], axis=2)
    Rn = d["R"].copy()
    out = eref.expose(d["wav"], Rn, d["lam"], d["sig"], d["k"], pad_r, pad_a, pad_F, d["data"], d["ivar"])
    assert np.array_equal(out[0], base[0]) and np.array_equal(out[1], base[1])
    off = F.copy()
    off[1, 2, 0] = 1.5
    out = eref.expose(d["wav"], d["R"], d["lam"], d["sig"], d["k"], rows, a, off, d["data"], d["ivar"])
    assert out[1][1, 2] == 0 and np.all(out[0][1, 2] == 0) and np.isnan(out[2][1, 2]).all()
    assert np.array_equal(np.delete(out[1].ravel(), 5), np.delete(base[1].ravel(), 5))


# ---- exposure_taps -----------------------------------------------------------------------------------------------
def _planet():
    from prometheus_amd import constants as const
    from prometheus_amd.celestialBodies import AvailablePlanets
    planet = AvailablePlanets().findPlanet("WASP-49b")
    return planet, float(np.sqrt(const.G * planet.hostStar.M / planet.a))


def test_exposure_taps_weights_rows_and_nodes():
    from prometheus_amd import observation as obs
    planet, Kp = _planet()
    orb = np.linspace(-0.04, 0.04, 9)
    base = obs.planet_frame_shifts(planet, orb)
    rng = np.random.default_rng(3)
    mid = np.sort(-0.035 + 0.07 * rng.random(11))
    width = 0.004 * rng.random(11)
    for n_sub in (1, 3, 4):
        rows, a, F = obs.exposure_taps(orb, base, mid, width, n_sub=n_sub)
        n_tap = 2 * n_sub
        assert rows.shape == a.shape == (11, n_tap) and F.shape == (11, 1, n_tap) and rows.dtype == np.int32
        assert np.all(np.abs(a.sum(axis=1) - 1.0) <= n_tap * U)
        assert np.all(a >= 0) and np.all(F > 0)
        phi = mid[:, None] + width[:, None] * ((np.arange(n_sub) + 0.5) / n_sub - 0.5)[None, :]
        lo, hi = rows[:, 0::2], rows[:, 1::2]
        assert np.array_equal(hi, lo + 1) and np.all(orb[lo] <= phi) and np.all(phi <= orb[hi])
        # the one trial's denominator is base interpolated to phi: the factors of a pair bracket 1
        t = (phi - orb[lo]) / (orb[hi] - orb[lo])
        assert np.array_equal(F[:, 0, 0::2], base[lo] / ((1 - t) * base[lo] + t * base[hi]))
    # an exposure on a node with no width: one live tap of weight 1, and with the planet's own Kp a factor of exactly 1
    for node in range(len(orb)):
        rows, a, F = obs.exposure_taps(orb, base, [orb[node]], [0.0], Kp=[Kp], Vsys=[0.0])
        live = np.nonzero(a[0] > 0)[0]
        assert len(live) == 1 and a[0, live[0]] == 1.0 and rows[0, live[0]] == node
        assert F[0, 0, live[0]] == 1.0
        rows1, a1, F1 = obs.exposure_taps(orb, base, [orb[node]], [0.0])
        assert np.array_equal(rows1, rows) and np.array_equal(a1, a) and F1[0, 0, live[0]] == 1.0
    # the last node: the bracket is the last interval and t = 1
    rows, a, F = obs.exposure_taps(orb, base, [orb[-1]], [0.0], n_sub=2)
    assert np.array_equal(rows[0], [7, 8, 7, 8]) and np.array_equal(a[0], [0.0, 0.5, 0.0, 0.5])


def test_exposure_taps_refuses_and_orders_trials():
    from prometheus_amd import observation as obs
    planet, Kp = _planet()
    orb = np.linspace(-0.04, 0.04, 9)
    base = obs.planet_frame_shifts(planet, orb)
    for mid, width in (([-0.041], [0.0]), ([0.0401], [0.0]), ([0.039], [0.006]), ([-0.039], [0.006])):
        with pytest.raises(ValueError, match="outside"):
            obs.exposure_taps(orb, base, mid, width, n_sub=2)
    obs.exposure_taps(orb, base, [0.039], [0.006], n_sub=1)            # the one sub-sample is the middle
    for bad in (dict(orbphase=orb[::-1]), dict(orbphase=orb[:1], base=base[:1]), dict(base=base[:-1]),
                dict(width=[-1e-3]), dict(n_sub=0), dict(Kp=[Kp]), dict(mid=[np.nan])):
        args = dict(orbphase=orb, base=base, mid=[0.0], width=[1e-3])
        args.update(bad)
        with pytest.raises(ValueError):
            obs.exposure_taps(**args)
    # Kp-major trials, as kp_vsys_factors: on nodes the denominators are that table's entries
    kp, vs = Kp * np.array([0.9, 1.0, 1.1]), np.array([-3e5, 2e5])
    K = obs.kp_vsys_factors(orb, kp, vs)
    rows, a, F = obs.exposure_taps(orb, base, orb[:-1], np.zeros(8), Kp=kp, Vsys=vs)
    assert F.shape == (8, 6, 2) and np.all(a[:, 0] == 1.0) and np.array_equal(rows[:, 0], np.arange(8))
    assert np.array_equal(F[:, :, 0], base[:8, None] / K[:8])
    assert np.array_equal(F[:, :, 1], base[1:, None] / K[:8])          # the dead partner: the same sub-sample's frame


# ---- Exposures and Transit.expose without a device -----------------------------------------------------------------
def _bare_transit(n_wav, n_orb):
    """A Transit with a grid and phases and nothing a device could run: expose must refuse before it needs one."""
    from prometheus_amd import gasProperties as gp
    tr = gp.Transit.__new__(gp.Transit)
    tr.wavelength = 5880e-8 + 1e-11 * np.arange(n_wav)
    tr.spatialGrid = types.SimpleNamespace(constructOrbphaseAxis=lambda: np.linspace(-0.03, 0.03, n_orb))
    tr.atmosphere = types.SimpleNamespace(densityDistributionList=[])
    tr.last_stats, tr.collect_stats = [], False
    return tr


def test_exposures_and_expose_refuse_before_touching_a_device(monkeypatch):
    from prometheus_amd import _native
    from prometheus_amd import observation as obs

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_native, "get_device", no_device)
    monkeypatch.setattr(_native, "device_count", no_device)
    n_orb = 3
    tr = _bare_transit(20000, n_orb)
    ins = obs.Instrument(tr.wavelength[[300, 100, 200]], resolving_power=140000.0)
    rows = np.array([[0, 1], [1, 2]])
    a = np.array([[0.5, 0.5], [1.0, 0.0]])
    F = np.ones((2, 4, 2))
    data, err = np.ones((2, 3)), np.full((2, 3), 1e-3)
    ex = obs.Exposures(ins, rows, a, F, data, err)
    assert (ex.n_exp, ex.n_trial, ex.n_tap) == (2, 4, 2) and ex.data.shape == (2, 3)
    assert obs.Exposures(ins, rows, a, F[:, 0], data, err).factors.shape == (2, 1, 2)      # [n_exp][n_tap]: one trial
    assert obs.Exposures(ins, rows, a, F, data, err).key == ex.key
    assert obs.Exposures(ins, rows, a, F * (1 + 1e-15), data, err).key != ex.key
    bad = [dict(rows=rows[0]), dict(rows=rows[:, :1]), dict(rows=[[0, -1], [1, 2]]), dict(rows=[[0.5, 1], [1, 2]]),
           dict(weights=a[:1]), dict(weights=[[0.5, -0.5], [1, 0]]), dict(weights=[[0.5, np.nan], [1, 0]]),
           dict(weights=[[0.5, np.inf], [1, 0]]), dict(factors=F[:1]), dict(factors=F[:, :, :1]),
           dict(factors=np.ones((2, 0, 2))), dict(factors=np.where(np.arange(2) == 1, 0.0, F)),
           dict(factors=-F), dict(factors=F * np.nan), dict(data=np.ones((3, 3))), dict(err=np.ones((2, 4))),
           dict(data=None)]
    for b in bad:
        args = dict(rows=rows, weights=a, factors=F, data=data, err=err)
        args.update(b)
        with pytest.raises(ValueError):
            obs.Exposures(ins, **args)
    with pytest.raises(TypeError):
        tr.expose(ins)
    with pytest.raises(ValueError, match="row 3.*3 phases"):
        tr.expose(obs.Exposures(ins, [[0, 3]], [[0.5, 0.5]], np.ones((1, 1, 2)), data[:1], err[:1]))
    with pytest.raises(ValueError, match="row 3"):                                         # ... a dead tap's too
        tr.expose(obs.Exposures(ins, [[0, 3]], [[1.0, 0.0]], np.ones((1, 1, 2)), data[:1], err[:1]))
    with pytest.raises(ValueError, match="not additive over wavelength partials.*one device.*max_memory_gb"):
        tr.expose(ex, devices=[0, 1])
    with pytest.raises(ValueError, match="not additive over wavelength partials.*one device.*max_memory_gb"):
        tr.expose(ex, devices=[0], max_memory_gb=1e-9)                 # chunks of 4,096 wavelengths: five of them


# ---- the index walk ------------------------------------------------------------------------------------------------
def _build(out, *extra):
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *extra, "-I" + CSRC, HOST, "-o", str(out)], check=True)


@pytest.mark.parametrize("which", ["real", "small", "sanitized"])
def test_index_walk_finds_every_index_inside(tmp_path, which):
    """tests/helpers/expose_host.cpp's own main (5 exposures of 6 taps over 3 rows, dead taps at the head, inside and
    at the tail, one exposure all dead, a dead tap with a row far out of range, wide taps that force global reads; one
    batch and three) with the kernel's constants, with small ones, and under -fsanitize=address,undefined."""
    flags = {"real": ("-O2",),
             "small": ("-O2", "-DPROM_VM_TILE=4", "-DPROM_VM_STAGE=40", "-DPROM_VM_CHUNK=2", "-DPROM_VM_TRIALS=3"),
             "sanitized": ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")}[which]
    exe = tmp_path / "expose_host"
    _build(exe, *flags)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert r.stdout.count("_oor=0") == 12 and r.stdout.count("visit_err=0") == 2
