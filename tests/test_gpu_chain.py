"""k_columns8's instances for one term of one analytic density kind (the transmission-curve path's column kernel).

The instance changes which code is compiled, never a floating-point operation: R and the columns are compared
bitwise between PROM_COL_SPEC=1 and 0 (read at every prom_transit_set), and prom_transit_set's PROM_DEBUG line
shows which instance each run took and whether the run wrote phase partials.

The golden reduced configs have 12 x 20 = 240 chords, not a multiple of 32, and never write phase partials; the
chord grids here do: 8 x 4 = 32 (one partial per phase), 8 x 8, 12 x 8 (three partials), 16 x 130 (65 partials) and
60 x 40 (the workload's 2,400 chords, 75 partials), with 1, 2, 3 and 16 phases.  The two large grids run every
config at every phase count.  The three small ones run a deliberate Latin-square subset, case (config i, grid j)
with phases[(i + j) % 4]: every config meets every grid and every phase count.  A few hundred wavelengths about
the Na D lines keep a case well under a second.
"""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ["1", "0"]   # PROM_COL_SPEC
GRIDS = [(8, 4), (8, 8), (12, 8), (16, 130), (60, 40)]
PHASES = [1, 2, 3, 16]
KIND = {"C2": 1, "hydrostatic": 2, "C3": 3, "C3q": 3, "C4": 4, "exomoon": 3}   # prom_density_kind


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


def config(name, phi, rho, n_orb):
    from prometheus_amd import configs
    if name == "hydrostatic":
        cfg = configs.get("C2")
        cfg["Scenarios"] = {"hydrostatic": {"T": 1500., "P_0": 1e5, "mu": 2.3 * 1.661e-24}}
        cfg["Species"] = {"hydrostatic": {"NaI": {"chi": 1e-6}, "KI": {"chi": 1e-6}}}
    elif name == "C3q":
        cfg = configs.get("C3")
        cfg["Scenarios"]["powerLaw"]["q_esc"] = 6.5   # a non-integral exponent: pow, not repeated squaring
    else:
        cfg = configs.get(name)
    return configs.reduced(cfg, phi_steps=phi, rho_steps=rho, orbphase_steps=n_orb, lower_w=5886e-8, upper_w=5900e-8,
                           res_low=1e-8, res_high=5e-10)


def transit(cfg):
    from prometheus_amd import setupfile
    tr = setupfile.build_transit(cfg)
    return tr, tr._host_inputs()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))   # bitwise, NaN patterns included


def chain_line(err):
    """{'curves', 'partials', 'kind'} of the last 'column chain' line of prom_transit_set's debug output."""
    lines = [l for l in err.splitlines() if "column chain:" in l]
    assert lines, err[-2000:]
    t = lines[-1].split("column chain:")[1].replace("(0: generic)", "").split(",")
    v = [int(x.split()[-1]) for x in t]
    return dict(curves=v[0], partials=v[1], kind=v[2])


def run(dev, tr, host, monkeypatch, capfd, spec, cull=0.0):
    """One set and one stats run under PROM_COL_SPEC=spec: (R, columns, stats, the debug line's fields)."""
    monkeypatch.setenv("PROM_DEBUG", "1")
    monkeypatch.setenv("PROM_COL_SPEC", spec)
    capfd.readouterr()
    with dev.lock:
        dev.transit_set(tr._problem(dev, host, 0, len(tr.wavelength), cull))
        monkeypatch.delenv("PROM_DEBUG")   # (the set's line is all that is read: no per-run debug output)
        st = dev.transit_run(stats=True)
        R, cols = dev.transit_result(), dev.transit_columns()
    return R, cols, st, chain_line(capfd.readouterr().err)


def check_knobs(dev, tr, host, monkeypatch, capfd, kind, cull=0.0, partials=True):
    """Bitwise R and columns between the two instances; each taken as the debug line says."""
    ref = None
    for kn in KNOBS:
        R, cols, st, ln = run(dev, tr, host, monkeypatch, capfd, kn, cull)
        assert st["tau_kernel_variant"] // 10 in (8, 9), st
        assert ln["curves"] == 1 and ln["partials"] == int(partials)
        assert ln["kind"] == (kind if kn == "1" else 0), (kn, ln)
        if ref is None:
            ref = (R, cols)
        assert same(R, ref[0]), "R differs under PROM_COL_SPEC=%s" % kn
        assert same(cols, ref[1]), "columns differ under PROM_COL_SPEC=%s" % kn
    return ref


NAMES = ["C2", "C3", "C4", "exomoon"]
CASES = [(n, g, PHASES[(i + j) % 4]) for i, n in enumerate(NAMES) for j, g in enumerate(GRIDS[:3])]
CASES += [(n, g, p) for n in NAMES for g in GRIDS[3:] for p in PHASES]


@pytest.mark.parametrize("name,grid,n_orb", CASES, ids=["%s-%dx%d-p%d" % (n, g[0], g[1], p) for n, g, p in CASES])
def test_bitwise_on_off(dev, monkeypatch, capfd, name, grid, n_orb):
    tr, host = transit(config(name, grid[0], grid[1], n_orb))
    R, cols = check_knobs(dev, tr, host, monkeypatch, capfd, KIND[name])
    assert R.shape[0] == n_orb and cols.shape[-1] == grid[0] * grid[1]
    assert np.all(np.isfinite(R)) and np.any(cols > 0.0)


def test_fallback_without_partials(dev, monkeypatch, capfd):
    """11 x 3 = 33 chords, not a multiple of 32: no partials, k_tc_build sweeps the chords; the instance still applies."""
    tr, host = transit(config("C3", 11, 3, 3))
    check_knobs(dev, tr, host, monkeypatch, capfd, KIND["C3"], partials=False)


def test_all_transparent_by_density(dev, monkeypatch, capfd):
    """The density scaled to zero (n_0 = 0): every unblocked chord has a zero column and is transparent, N_max = 0,
    no phase has a table."""
    tr, host = transit(config("C3", 8, 8, 3))
    host = copy.copy(host)
    host["scenarios"] = [dict(e) for e in host["scenarios"]]
    for e in host["scenarios"]:
        prm = np.array(e["params"], dtype=np.float64)
        prm[0] = 0.0
        e["params"] = prm
    R, cols = check_knobs(dev, tr, host, monkeypatch, capfd, KIND["C3"])
    assert np.all(cols[0] == 0.0)
    check_transparent(R, host)


def check_transparent(R, host):
    blocked = np.sqrt((host["y"][None, :] - host["planet_y"][:, None]) ** 2 + host["z"][None, :] ** 2) < host["planet_R"]
    fo = host["fout"]
    expect = np.array([1.0 if not b.any() else fo[~b].sum() / fo.sum() for b in blocked])
    assert np.allclose(R, expect[:, None], rtol=1e-14, atol=0)


def test_all_transparent_by_culling(dev, monkeypatch, capfd):
    """A culling bound above every chord's optical depth: every unblocked chord is transparent, the columns stay."""
    tr, host = transit(config("C3", 8, 8, 3))
    R, cols = check_knobs(dev, tr, host, monkeypatch, capfd, KIND["C3"], cull=1e300)
    check_transparent(R, host)


def test_phase_fully_blocked(dev, monkeypatch, capfd):
    """Every chord of the middle phase behind the planet.  A setup file cannot say that (the chords span the stellar
    disk, the planet is smaller), so the host inputs are edited: a planet of twice the chord grid's radius, on the
    disk's centre at the middle phase and far off it at the others."""
    tr, host = transit(config("C2", 8, 8, 3))
    host = copy.copy(host)
    rmax = float(np.sqrt(host["y"] ** 2 + host["z"] ** 2).max())
    host["planet_R"] = 2.0 * rmax
    host["planet_y"] = np.array([10.0 * rmax, 0.0, -10.0 * rmax])
    R, cols = check_knobs(dev, tr, host, monkeypatch, capfd, KIND["C2"])
    assert np.all(cols[0, 1, :] == 0.0) and np.all(R[1] == 0.0)   # (the merged absorber's columns; nothing unblocked: no flux)
    assert np.all(R[0] > 0.0) and np.all(R[2] > 0.0)


def test_nonfinite_column(dev, monkeypatch, capfd):
    """The setup of test_nonfinite_columns_exact_path (a density plugin tabulated on the host, one infinite sample) on
    a 64-chord grid: the phase with the infinite column has no table and takes the exact path; the tabulated density
    keeps the generic column kernel under either setting."""
    from oracle import prom_oracle as O
    cfg = config("C2", 8, 8, 3)
    tr, _ = transit(cfg)
    scen, dop, grids = O.from_setup(cfg)
    base = scen[0]
    cg = O.chord_grid(grids)
    orbs = O.orbphase_axis(grids)
    pl = base.planet
    y, z = cg[:, 1] * np.sin(cg[:, 0]), cg[:, 1] * np.cos(cg[:, 0])
    blocked = np.sqrt((y - pl.a * np.sin(cg[:, 2])) ** 2 + z ** 2) < pl.R
    k0 = np.where((cg[:, 2] == orbs[1]) & ~blocked)[0][5]
    tphi, trho, torb = cg[k0]

    def fn(x_, phi_, rho_, orb_):
        n = np.array(O.number_density(base, x_, phi_, rho_, orb_), dtype=np.float64)
        m = (np.isclose(phi_, tphi, rtol=1e-12, atol=0) & np.isclose(rho_, trho, rtol=1e-12, atol=0) &
             np.isclose(orb_, torb, rtol=1e-12, atol=1e-15))
        n[m, 3] = np.inf
        return n

    d0 = tr.atmosphere.densityDistributionList[0]

    class Plug(type(d0)):
        def densityModel(self):
            raise NotImplementedError

        def calculateNumberDensity(self, x_, phi_, rho_, orb_):
            return fn(x_, phi_, rho_, orb_)

    p = copy.copy(d0)
    p.__class__ = Plug
    tr.atmosphere.densityDistributionList[0] = p
    host = tr._host_inputs()
    ref = None
    for kn in KNOBS:
        R, cols, st, ln = run(dev, tr, host, monkeypatch, capfd, kn)
        assert st["tau_kernel_variant"] // 10 in (8, 9) and st["exact_phases"] == 1, st
        assert ln == dict(curves=1, partials=1, kind=0), (kn, ln)
        ref = ref or (R, cols)
        assert same(R, ref[0]) and same(cols, ref[1]), kn
    assert np.isinf(ref[1]).sum() == 1


def test_repeated_runs(dev, monkeypatch, capfd):
    """13 consecutive runs (more than three rotations of the four slots), a run after a stats run and a run after
    serialized kernel timing reproduce the first R bitwise with the one-kind instance."""
    tr, host = transit(config("C3", 12, 8, 16))
    R0, _, _, ln = run(dev, tr, host, monkeypatch, capfd, "1")
    assert ln["kind"] == KIND["C3"]

    def again():
        dev.transit_run()
        dev.synchronize()
        assert same(dev.transit_result(), R0)

    with dev.lock:
        for _ in range(13):
            again()
        dev.transit_run(stats=True)
        again()
        dev.transit_kernel_ms(2)
        again()


@pytest.mark.parametrize("name", ["C2", "C3", "C3q", "C4", "hydrostatic"])
def test_each_analytic_kind(dev, monkeypatch, capfd, name):
    """Barometric, power law with an integral (6) and a non-integral (6.5) exponent, torus, hydrostatic: the columns of
    the instance compiled for the kind are bitwise the generic instance's.  30 and 11 samples per chord (4 and 2
    per lane: two of the instances per kind)."""
    for x_steps in (30, 11):
        cfg = config(name, 12, 8, 3)
        cfg["Grids"]["x_steps"] = x_steps
        tr, host = transit(cfg)
        R1, c1, _, l1 = run(dev, tr, host, monkeypatch, capfd, "1")
        R0, c0, _, l0 = run(dev, tr, host, monkeypatch, capfd, "0")
        assert l1["kind"] == KIND[name] and l0["kind"] == 0
        assert same(c1, c0) and same(R1, R0)
        assert np.any(c1 > 0.0)
