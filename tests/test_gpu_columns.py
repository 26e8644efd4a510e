"""The column stage against numpy: N[s][o][ip] = (0.0 + pairwise_x(n chi)) delta_x and the transparent / active /
blocked flags, on every path that computes them -- k_columns8's generic and one-kind instances and the k_ntot +
k_columns pair -- through the raw C-ABI (prom_transit_set / run / columns, prom_number_density).

Bitwise parts.  The reference is np.sum(n * chi, axis=1) * delta_x itself (helpers/columns_ref.columns_numpy); columns
are compared as uint64.  tests/test_columns_ref_cpu.py shows that the designs used here change their bits under every
wrong order listed there, at every sample count.  Problems are tiny: a two-node lookup table, 64 wavelengths, 33 or 64
chords, one or three phases.  Every run asserts its route from tau_kernel_variant and prom_transit_set's PROM_DEBUG
"column chain" line:
  default    curve path, variant 81, curves 1, partials iff n_pr % 32 == 0, kind as expected   k_columns8
  tcurve0    PROM_TCURVE=0: windowed kernels, variant 2x / 3x, curves 0                        k_columns8
  ocml       PROM_OPT_OCML_EXP: k_tau with the ocml exp, variant 0x                            k_columns8
  pad5       four more scenarios, tabulated zeros without constituents (n_sc > 4)              k_ntot + k_columns
  nine       nine atomic terms of one scenario, variant 10                                     k_ntot + k_columns
  n_x > 64                                                                                     k_ntot + k_columns
(The stats do not name the column kernel: tcurve0 and pad5 differ by the launcher's n_sc <= 4 rule alone.)

Density samples (d) against helpers/columns_ref.density_ld, whose docstring derives the bound eps(x) u per sample from
the arithmetic; results that are or pass through a denormal (an exp below 2^-1022, scaled by n0) get the absolute
bound eps u 2^-1022 max(1, |n0|).  The ocml terms (2 ulp each for exp and pow) are supposed: the installed ROCm
states no bound.  Measured worst error over bound per kind: profiles/columns_errors.txt (written from this module's
output when PROM_COLUMNS_RECORD names a file).
"""
import os

import numpy as np
import pytest

from helpers import columns_ref as CR

pytestmark = pytest.mark.gpu

OFFSET = 1e-50
SIGMA = 1e-20
WAV = np.linspace(5.0e-5, 6.0e-5, 64)
CHI9 = [1.0, 0.3, 1e-6, 0.5, 0.25, 0.7, 0.9, 0.11, 0.013]


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


@pytest.fixture(scope="module")
def tid(dev):
    """One two-node lookup table, sigma = 1e-20 over the wavelengths."""
    with dev.lock:
        t = dev.table_upload(np.array([4.0e-5, 7.0e-5]), np.full(2, np.log10(SIGMA + OFFSET)), OFFSET)
    yield t
    with dev.lock:
        dev.table_free(t)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def chain_line(err):
    lines = [l for l in err.splitlines() if "column chain:" in l]
    assert lines, err[-2000:]
    t = lines[-1].split("column chain:")[1].replace("(0: generic)", "").split(",")
    v = [int(x.split()[-1]) for x in t]
    return dict(curves=v[0], partials=v[1], kind=v[2])


def tab_scenario(rows, n_orb, cons):
    from prometheus_amd import _native
    return {"kind": _native.DENSITY_TABULATED, "params": [], "shift": np.ones(n_orb),
            "n_tabulated": np.ascontiguousarray(rows, dtype=np.float64).ravel(), "constituents": cons}


def padded(scenarios, n_pr, n_orb, n_x):
    """Five scenarios: the given one and tabulated all-zero ones without constituents."""
    zero = np.zeros((n_pr, n_orb, n_x))
    return list(scenarios) + [tab_scenario(zero, n_orb, []) for _ in range(5 - len(scenarios))]


def run(dev, monkeypatch, capfd, g, x, delta_x, scenarios, env=(), options=0, cull_tau=0.0, moon_y=None, moon_R=(),
        wav=WAV):
    """One set and one stats run: (stats, columns [n_atoms, n_orb, n_pr], the debug line's fields)."""
    from prometheus_amd import _native
    n_orb = len(g["planet_y"])
    for k in ("PROM_TCURVE", "PROM_SPECIES_MERGE", "PROM_COL_SPEC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PROM_DEBUG", "1")
    capfd.readouterr()
    prob = _native.TransitInputs(
        wavelength=wav, chord_y=g["y"], chord_z=g["z"], chord_fout=np.ones(len(g["y"])), n_orb=n_orb, x=x,
        delta_x=delta_x, planet_y=g["planet_y"], planet_R=g["planet_R"],
        moon_y=np.zeros((0, n_orb)) if moon_y is None else moon_y, moon_R=np.asarray(moon_R, dtype=np.float64),
        scenarios=scenarios, cull_tau=cull_tau, options=options)
    with dev.lock:
        dev.transit_set(prob)
        monkeypatch.delenv("PROM_DEBUG")
        st = dev.transit_run(stats=True)
        cols = dev.transit_columns()
    return st, cols, chain_line(capfd.readouterr().err)


def check_route(route, st, ln, n_pr, kind=0, na=1):
    v = st["tau_kernel_variant"]
    what = (route, v, ln)
    if route == "default":
        assert v in (80 + na, 90 + na) and ln == dict(curves=1, partials=int(n_pr % 32 == 0), kind=kind), what
    elif route in ("tcurve0", "pad5", "large", "windowed"):
        assert v in (20 + na, 30 + na) and ln["curves"] == 0, what
    elif route == "ocml":
        assert v == na and ln["curves"] == 0, what
    elif route == "generic":   # more than four species: k_tau, the units digit 0
        assert v == 10 and ln["curves"] == 0, what
    elif route == "molecular":
        assert v == 10 + na and ln["curves"] == 0, what
    else:
        raise ValueError(route)


def assert_columns(case, got, want, blocked):
    """got, want [n_orb, n_pr]: 0.0 exactly on blocked chords; NaN where numpy has NaN; numpy's bits elsewhere (an
    infinity's sign included)."""
    assert got.shape == want.shape == blocked.shape, case
    assert np.all(bits(got)[blocked] == 0), "%s: a blocked chord's column is not +0.0" % (case,)
    nan = np.isnan(want) & ~blocked
    assert np.all(np.isnan(got[nan])), "%s: numpy has NaN, the device %s" % (case, got[nan])
    cmp = ~blocked & ~nan
    bad = np.argwhere(cmp & (bits(got) != bits(want)))
    assert len(bad) == 0, "%s: %d of %d columns differ from numpy's bits, first (o, ip) = %s: %r against %r" % (
        case, len(bad), int(cmp.sum()), tuple(bad[0]), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))


def numpy_columns(rows, chi, delta_x):
    """[n_orb, n_pr] from rows [n_pr, n_orb, n_x]."""
    n_pr, n_orb, n_x = rows.shape
    with np.errstate(invalid="ignore"):
        return CR.columns_numpy(rows.reshape(-1, n_x), chi, delta_x).reshape(n_pr, n_orb).T


# ---- a. tabulated densities, bitwise ---------------------------------------------------------------------------------
ROUTES = ["default", "tcurve0", "ocml", "pad5", "nine"]
ROUTE_ENV = {"tcurve0": (("PROM_TCURVE", "0"),)}
A_CASES = [(n, r) for n in CR.NX_SMALL for r in ROUTES] + [(n, "large") for n in CR.NX_LARGE]


@pytest.mark.parametrize("n_x,route", A_CASES, ids=["nx%d-%s" % c for c in A_CASES])
def test_tabulated_bitwise(dev, tid, monkeypatch, capfd, n_x, route):
    from prometheus_amd import _native
    for n_pr, n_orb in CR.GRIDS:
        d = CR.table_design(n_pr, n_orb, n_x)
        chis = CHI9 if route == "nine" else [1.0]
        sc = [tab_scenario(d["rows"], n_orb, [{"table_id": tid, "chi": c} for c in chis])]
        if route == "pad5":
            sc = padded(sc, n_pr, n_orb, n_x)
        st, cols, ln = run(dev, monkeypatch, capfd, d, np.arange(float(n_x)), CR.DELTA_X, sc,
                           env=ROUTE_ENV.get(route, ()), options=_native.OPT_OCML_EXP if route == "ocml" else 0)
        check_route("generic" if route == "nine" else route, st, ln, n_pr)
        assert cols.shape == (len(chis), n_orb, n_pr)
        for s, chi in enumerate(chis):
            want = numpy_columns(d["rows"], chi, CR.DELTA_X)
            (ia, oa), (ib, ob) = d["special"]
            assert want[oa, ia] == np.inf and np.isnan(want[ob, ib])
            assert_columns("n_x %d %s grid %dx%d slot %d" % (n_x, route, n_pr, n_orb, s), cols[s], want, d["blocked"])
        assert st["blocked_chords"] == int(d["blocked"].sum())


# ---- b. terms and scenarios --------------------------------------------------------------------------------------------
def finite_design(n_pr, n_orb, n_x, seed):
    g = CR.grid(n_pr, n_orb)
    g["rows"] = CR.design_rows(n_pr * n_orb, n_x, seed).reshape(n_pr, n_orb, n_x)
    return g


@pytest.mark.parametrize("n_x", [7, 13, 30, 64])
@pytest.mark.parametrize("merge", ["0", None])
def test_three_species_one_scenario(dev, tid, monkeypatch, capfd, n_x, merge):
    """chi = {1.0, 0.3, 1e-6}: with PROM_SPECIES_MERGE=0 every slot holds its own chi's column; with species merged
    into one effective absorber (the default) the launcher passes k_columns8 one term of chi = 1 and slot 0, and only
    that slot is written."""
    chis = [1.0, 0.3, 1e-6]
    for n_pr, n_orb in CR.GRIDS:
        g = finite_design(n_pr, n_orb, n_x, 7)
        sc = [tab_scenario(g["rows"], n_orb, [{"table_id": tid, "chi": c} for c in chis])]
        st, cols, ln = run(dev, monkeypatch, capfd, g, np.arange(float(n_x)), CR.DELTA_X, sc,
                           env=(("PROM_SPECIES_MERGE", "0"),) if merge else ())
        if merge:
            check_route("windowed", st, ln, n_pr, na=3)
            for s, chi in enumerate(chis):
                assert_columns("unmerged n_x %d slot %d" % (n_x, s), cols[s], numpy_columns(g["rows"], chi, CR.DELTA_X),
                               g["blocked"])
        else:
            check_route("default", st, ln, n_pr, na=1)
            assert_columns("merged n_x %d" % n_x, cols[0], numpy_columns(g["rows"], 1.0, CR.DELTA_X), g["blocked"])


@pytest.mark.parametrize("n_x", [5, 11, 30, 57])
@pytest.mark.parametrize("n_sc,per", [(2, 1), (4, 1), (4, 2)], ids=["2sc", "4sc", "8terms"])
def test_scenarios_in_order(dev, tid, monkeypatch, capfd, n_x, n_sc, per):
    """Two and four scenarios, each with its own table of densities and its own chi; and four scenarios of two species:
    eight terms, k_columns8's limit.  Slots in scenario order, then constituent order."""
    for n_pr, n_orb in CR.GRIDS:
        gs = [finite_design(n_pr, n_orb, n_x, 20 + k) for k in range(n_sc)]
        chis = [[CHI9[(2 * k + j) % 9] for j in range(per)] for k in range(n_sc)]
        sc = [tab_scenario(gs[k]["rows"], n_orb, [{"table_id": tid, "chi": c} for c in chis[k]]) for k in range(n_sc)]
        st, cols, ln = run(dev, monkeypatch, capfd, gs[0], np.arange(float(n_x)), CR.DELTA_X, sc)
        check_route("generic" if n_sc * per > 4 else "windowed", st, ln, n_pr, na=n_sc * per)
        s = 0
        for k in range(n_sc):
            for chi in chis[k]:
                assert_columns("%d scenarios x %d, n_x %d, slot %d" % (n_sc, per, n_x, s), cols[s],
                               numpy_columns(gs[k]["rows"], chi, CR.DELTA_X), gs[0]["blocked"])
                s += 1


def test_atoms_beside_a_molecule(dev, tid, monkeypatch, capfd):
    """A molecular constituent sends the atoms' columns (n_x = 30) through k_ntot + k_columns."""
    from oracle import prom_oracle as O
    t = O.synthetic_molecular_table(n_p=4, n_t=3, n_nu=65, nu_lo=16000., nu_hi=21000.)
    P, W = t["p"] * 10., np.ascontiguousarray(1. / t["bin_edges"][::-1])
    V = np.ascontiguousarray(np.log10(t["xsecarr"][:, :, ::-1] + OFFSET))
    with dev.lock:
        mid = dev.molecular_upload(P, t["t"], W, V, OFFSET)
    try:
        for n_pr, n_orb in CR.GRIDS:
            g = finite_design(n_pr, n_orb, 30, 31)
            cons = [{"table_id": tid, "chi": 0.3}, {"table_id": mid, "chi": 1e-3, "is_molecule": True},
                    {"table_id": tid, "chi": 1.0}]
            sc = tab_scenario(g["rows"], n_orb, cons)
            sc["T"] = 1000.0
            st, cols, ln = run(dev, monkeypatch, capfd, g, np.arange(30.0), CR.DELTA_X, [sc])
            check_route("molecular", st, ln, n_pr, na=2)
            for s, chi in enumerate([0.3, 1.0]):
                assert_columns("molecular slot %d" % s, cols[s], numpy_columns(g["rows"], chi, CR.DELTA_X), g["blocked"])
    finally:
        with dev.lock:
            dev.table_free(mid, molecular=True)


# ---- c. analytic densities, bitwise through the device's own samples ---------------------------------------------------
R_P = 7.0e9
GMUM, KT = 6.67e-8 * 2.3 * 1.661e-24 * 1.9e30, 1.381e-16 * 1500.0
KINDS = {
    "barometric": (CR.BAROMETRIC, (1e10, R_P, 4.0e8)),
    "hydrostatic": (CR.HYDROSTATIC, (1e8, R_P, GMUM, KT, GMUM / (KT * R_P))),
    "powerlaw-q0": (CR.POWERLAW, (1e5, R_P, 0.0)),
    "powerlaw-q1": (CR.POWERLAW, (1e5, R_P, 1.0)),
    "powerlaw-q5": (CR.POWERLAW, (1e5, R_P, 5.0)),
    "powerlaw-q8": (CR.POWERLAW, (1e5, R_P, 8.0)),
    "powerlaw-q9": (CR.POWERLAW, (1e5, R_P, 9.0)),
    "powerlaw-q6.5": (CR.POWERLAW, (1e5, R_P, 6.5)),
    "torus": (CR.TORUS, (1e4, 4.2e10, 4 * 2.0e9, 2.0e9)),
    "moon-powerlaw": (CR.POWERLAW, (1e7, 1.8e8, 3.0)),
}


def analytic_grid(name, n_pr, n_orb):
    i = np.arange(n_pr)
    py = np.array([-6.0e9, 1.0e8, 5.0e9])[:n_orb]
    g = {"y": np.linspace(-1.5e10, 1.5e10, n_pr) + 3.0e7 * (i % 3), "z": 2.0e9 * ((i % 5) - 2.0) + 1.0e8,
         "planet_y": py, "planet_R": R_P}
    if name == "moon-powerlaw":   # the density's centre moves with the moon, off the planet, every phase another
        g["bx"] = np.array([3.0e10, 1.0e10, -2.0e10])[:n_orb]
        g["by"] = py + np.array([2.0e9, -9.0e9, 4.0e9])[:n_orb]
    else:
        g["bx"] = np.array([1.0e8, 0.0, -2.0e8])[:n_orb]
        g["by"] = py
    g["blocked"] = CR.blocked_mask(g["y"], g["z"], py, R_P, np.zeros((0, n_orb)), [])
    return g


C_CASES = [(k, n) for k in KINDS for n in (7, 8, 11, 30, 33, 64, 80)]


@pytest.mark.parametrize("name,n_x", C_CASES, ids=["%s-nx%d" % c for c in C_CASES])
def test_analytic_bitwise(dev, tid, monkeypatch, capfd, name, n_x):
    """prom_number_density and the column kernels call the same density_at: the columns are numpy's sum over the
    device's own samples, bit for bit, in the one-kind instance, the generic one (PROM_COL_SPEC=0) and k_ntot +
    k_columns (n_x = 80; five scenarios at n_x = 30)."""
    kind, p = KINDS[name]
    chi = 0.3
    x = np.linspace(-5.0e10, 5.0e10, n_x)
    delta_x = float(x[1] - x[0])
    routes = [("large", ())] if n_x > 64 else [("default", ()), ("default", (("PROM_COL_SPEC", "0"),))]
    if n_x == 30:
        routes.append(("pad5", ()))
    for n_pr, n_orb in CR.GRIDS:
        g = analytic_grid(name, n_pr, n_orb)
        with dev.lock:
            smp = [dev.number_density(kind, p, x, g["y"], g["z"], np.full(n_pr, g["bx"][o]), np.full(n_pr, g["by"][o]))
                   for o in range(n_orb)]
        want = np.stack([CR.columns_numpy(s, chi, delta_x) for s in smp])
        assert np.count_nonzero(want[~g["blocked"]] > 0) >= n_pr // 4, "the case has hardly a column"
        for route, env in routes:
            sc = [{"kind": kind, "params": list(p), "shift": np.ones(n_orb), "body_x": g["bx"], "body_y": g["by"],
                   "constituents": [{"table_id": tid, "chi": chi}]}]
            if route == "pad5":
                sc = padded(sc, n_pr, n_orb, n_x)
            st, cols, ln = run(dev, monkeypatch, capfd, g, x, delta_x, sc, env=env)
            check_route(route, st, ln, n_pr, kind=0 if env else kind)
            assert_columns("%s n_x %d %s%s grid %dx%d" % (name, n_x, route, " generic" if env else "", n_pr, n_orb),
                           cols[0], want, g["blocked"])


# ---- d. density samples at their edges ---------------------------------------------------------------------------------
def record(line):
    print(line)
    path = os.environ.get("PROM_COLUMNS_RECORD")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def check_samples(dev, case, kind, p, x, y, z, bx, by):
    """Every (chord, x) sample of prom_number_density against density_ld: the class where the reference is 0, inf or
    NaN, within eps u elsewhere.  Returns the worst error over its bound."""
    x, y, z = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(z, dtype=np.float64)
    with dev.lock:
        got = dev.number_density(kind, p, x, y, z, np.full(len(y), bx), np.full(len(y), by))
    ref, eps = CR.density_ld(kind, p, x[None, :], y[:, None], z[:, None], bx, by)
    nan, inf, zero = np.isnan(ref), np.isinf(ref), ref == 0
    assert np.all(np.isnan(got[nan])), "%s: NaN expected, got %s" % (case, got[nan])
    assert np.all(got[inf] == ref[inf].astype(np.float64)), "%s: inf expected, got %s" % (case, got[inf])
    assert np.all(bits(got)[zero] == 0), "%s: +0.0 expected, got %s" % (case, got[zero])
    m = ~(nan | inf | zero)
    floor = CR.LD(2.0 ** -1022) * max(1.0, abs(float(p[0])))
    tol = eps[m] * CR.U * np.maximum(np.abs(ref[m]), floor)
    ratio = (np.abs(got[m].astype(CR.LD) - ref[m]) / tol).astype(np.float64)
    worst = float(ratio.max()) if ratio.size else 0.0
    k = int(np.argmax(ratio)) if ratio.size else 0
    record("%s: %d samples (%d NaN, %d inf, %d zero), worst error / bound %.3f (eps %.1f, value %.3e)" % (
        case, ref.size, nan.sum(), inf.sum(), zero.sum(), worst, eps[m][k] if ratio.size else 0.0,
        float(ref[m][k]) if ratio.size else 0.0))
    assert worst <= 1.0, "%s: sample %.17g against %.17g, %.3f of the bound" % (
        case, got[m][k], float(ref[m][k]), worst)
    return got, ref


# Integer geometry: dx^2 + dy^2 + z^2 is exact, so r is the correctly rounded root of an integer and r = R exactly at
# (3, 4, 0), (0, 3, 4), (5, 0, 0).  x holds the body centre (0), points inside, on and outside the edge, and far ones.
EDGE_X = [0.0, 1.0, 3.0, 4.0, 5.0, 6.0, 12.0, 84.0, 1000.0]
EDGE_Y = [0.0, 3.0, 4.0, 0.0, 5.0, 13.0]
EDGE_Z = [0.0, 0.0, 0.0, 4.0, 12.0, 0.0]
UP = float(np.nextafter(5.0, 6.0))
H_DEN = 8.0 / 740.0   # r = 13: exp(-740), a denormal; r = 12: e^-647; r >= 15: 0
EDGE_CASES = {
    "barometric": [(CR.BAROMETRIC, (1.0, 5.0, H_DEN)), (CR.BAROMETRIC, (1.0, UP, H_DEN)), (CR.BAROMETRIC, (1e10, 5.0, 0.75)),
                   (CR.BAROMETRIC, (1e10, UP, 0.75))],
    "hydrostatic": [(CR.HYDROSTATIC, (1e8, 5.0, 60.0, 0.75, 16.0)), (CR.HYDROSTATIC, (1e8, UP, 60.0, 0.75, 16.0)),
                    (CR.HYDROSTATIC, (1.0, 5.0, 3000.0, 0.75, 790.0))],   # r = 85: exp(-742.9), a denormal
    "powerlaw": [(CR.POWERLAW, (1e5, R, q)) for q in (0.0, 1.0, 5.0, 8.0, 9.0, 6.5) for R in (5.0, UP)] +
                [(CR.POWERLAW, (1.0, 5.0, 150.0))],
    "torus": [(CR.TORUS, (1e4, 5.0, 2.0, 0.5)), (CR.TORUS, (1.0, 5.0, 0.125, 0.5)), (CR.TORUS, (1e4, 13.0, 2.0, 0.03125))],
}


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_density_edges(dev, name):
    for kind, p in EDGE_CASES[name]:
        got, ref = check_samples(dev, "%s p = %s edges" % (name, p), kind, p, EDGE_X, EDGE_Y, EDGE_Z, 0.0, 0.0)
        if kind == CR.TORUS:
            continue
        # chord 1 = (y, z) = (3, 0): x = 4 lies on r = 5 exactly -- outside for R = 5 (heaviside(0) = 1), inside for
        # R one ulp larger
        on = got[1, EDGE_X.index(4.0)]
        if kind == CR.HYDROSTATIC:
            assert on == got[1, EDGE_X.index(0.0)] if p[1] == UP else on != got[1, EDGE_X.index(0.0)]
        else:
            assert (on == 0.0) == (p[1] == UP), (name, p, on)
    if name == "torus":
        kind, p = EDGE_CASES["torus"][0]
        with dev.lock:
            ring = dev.number_density(kind, p, [3.0], [4.0], [0.0], [0.0], [0.0])
        assert ring[0, 0] == p[0]   # on the ring and in its plane: exp(-0) exp(-0)


@pytest.mark.parametrize("name", sorted(KINDS))
def test_density_samples(dev, name):
    """The (c) cases' own samples (physical magnitudes, a body off the origin) within the same bound."""
    kind, p = KINDS[name]
    g = analytic_grid(name, 64, 3)
    x = np.linspace(-5.0e10, 5.0e10, 33)
    for o in range(3):
        r = np.sqrt((x[None, :] - g["bx"][o]) ** 2 + (g["y"][:, None] - g["by"][o]) ** 2 + g["z"][:, None] ** 2)
        if kind != CR.TORUS:   # no sample so close to the edge that float64 and the reference may disagree on its side
            assert np.all(np.abs(r - p[1]) > 1e-12 * r)
        check_samples(dev, "%s phase %d" % (name, o), kind, p, x, g["y"], g["z"], g["bx"][o], g["by"][o])


# ---- e. flags ------------------------------------------------------------------------------------------------------------
def flag_grid(n_pr, n_orb, planet_R, moon_R):
    """Integer chords.  Phase 0: chord 0 lies at (3, 4) from the planet's centre and chord 1 at (3, 4) from the moon's;
    chord 2 is covered by the moon alone (at 2 from its centre, 38 from the planet's)."""
    i = np.arange(n_pr)
    y = np.concatenate([[3.0, 43.0, 38.0], (i[3:] * 3 - 40.0)])
    z = np.concatenate([[4.0, 4.0, 0.0], (i[3:] % 7) - 3.0])
    g = {"y": y, "z": z, "planet_y": np.array([0.0, 6.0, -11.0])[:n_orb], "planet_R": planet_R}
    g["moon_y"] = np.array([[40.0, -20.0, 15.0]])[:, :n_orb]
    g["moon_R"] = np.array([moon_R])
    g["blocked"] = CR.blocked_mask(y, z, g["planet_y"], planet_R, g["moon_y"], g["moon_R"])
    return g


@pytest.mark.parametrize("route", ["default", "pad5"])
@pytest.mark.parametrize("edge", ["on", "planet-up", "moon-up"])
def test_flags(dev, tid, monkeypatch, capfd, route, edge):
    """blocked / transparent / active counts of the stats against blocked_mask and numpy, with chords exactly on the
    planet's limb (sqrt form) and the moon's (squared form); a radius one ulp larger blocks them.  cull_tau lies a
    factor of a hundred or more from every chord's bound N sigma_max on either side."""
    n_x, cull = 12, 1e-13
    for n_pr, n_orb in CR.GRIDS:
        g = flag_grid(n_pr, n_orb, UP if edge == "planet-up" else 5.0, UP if edge == "moon-up" else 5.0)
        assert bool(g["blocked"][0, 0]) == (edge == "planet-up") and bool(g["blocked"][0, 1]) == (edge == "moon-up")
        assert g["blocked"][0, 2] and np.hypot(g["y"][2] - g["planet_y"][0], g["z"][2]) > 5.0
        rng = np.random.default_rng(n_pr * n_orb)
        cls = rng.integers(0, 3, size=(n_pr, n_orb))   # zero column, far below the cull, far above
        mag = np.where(cls == 1, 10.0 ** rng.uniform(1, 3, cls.shape), 10.0 ** rng.uniform(10, 12, cls.shape))
        rows = CR.design_rows(n_pr * n_orb, n_x, 5).reshape(n_pr, n_orb, n_x)
        rows = rows / rows.max(axis=2, keepdims=True) * mag[:, :, None] * (cls[:, :, None] > 0)
        N = numpy_columns(rows, 1.0, CR.DELTA_X)
        bound = N * SIGMA
        assert not np.any((bound > cull / 1e2) & (bound < cull * 1e2))
        sc = [tab_scenario(rows, n_orb, [{"table_id": tid, "chi": 1.0}])]
        if route == "pad5":
            sc = padded(sc, n_pr, n_orb, n_x)
        st, cols, ln = run(dev, monkeypatch, capfd, g, np.arange(float(n_x)), CR.DELTA_X, sc, cull_tau=cull,
                           moon_y=g["moon_y"], moon_R=g["moon_R"])
        check_route(route, st, ln, n_pr)
        assert_columns("flags %s %s" % (route, edge), cols[0], N, g["blocked"])
        nb = int(g["blocked"].sum())
        ntr = int((~g["blocked"] & (bound <= cull)).sum())
        assert (st["blocked_chords"], st["transparent_chords"], st["active_chords"]) == (nb, ntr, n_pr * n_orb - nb - ntr), (
            route, edge, n_pr, n_orb, st)
        assert nb > 2 and ntr > 2 and n_pr * n_orb - nb - ntr > 2
