"""The transmission curves (k_tc_build; tc_eval in k_sigma_tc and k_sigma_tw) swept over q = Y N_max, chord counts
and column spreads, against the closed-form disk sum in longdouble (tests/helpers/tc_sweep.py: the designs, whose
coverage tests/test_tc_sweep_cpu.py asserts, and the reference).

Every case drives the raw C-ABI: a lookup table with one node per wavelength, a tabulated density with the column in
sample 0 of 8 (n(chord, phase, x) chosen so that N is the stored value, which transit_columns() confirms bit for bit),
chords on a ring.  Every case asserts that the curve path took the run (tau_kernel_variant 81 or 91).

Tolerance, absolute in R, per unit weight of the active chords (their share of the disk flux, <= 1), u = 2^-53.
By the branch tc_eval takes at the reference's q (a point within 2^-40 of a power of two takes the larger of its two
neighbours' bounds, since the device's rounded q may fall on the other side):
  tail, q < 2^-7     the degree-5 Taylor sum's truncation q^6 / 720 <= 2^-42 / 720 = 3.2e-16 and six fma roundings
                     (five of Horner's, tf + p): 9.8e-16;
  octave j           T at the 16 Chebyshev nodes is good to 31 u after three squarings (prom_tcurve.hip's header);
                     interpolation multiplies a node error by at most the Lebesgue constant of 16 Chebyshev nodes,
                     2/pi ln 16 + 0.9625 = 2.73; the 16 x 16 product to coefficients and Clenshaw add about 48 u:
                     (31 * 2.73 + 48) u = 1.47e-14;
  above the table    "every chord opaque": what is dropped is <= e^-40 = 4.2e-18, and tf carries no more rounding
                     than in the tail (6 u): 6.7e-16.  Truncated at the 64-octave cap (the `two` columns): nact terms
                     added in chord order, (nact + 4) u (tc_sweep.tol_exact_sum) -- 2.7e-13 at 2,400 chords, still
                     1,500 times below one dropped chord;
plus the lookup's error e_Y in Y through |dT / dln Y| <= max x e^-x = 1/e:
  static             a node: 10^y_k rounded and the offset subtracted, 2 u: 8.2e-17 (PROM_SIG_POLY=0 the same: ocml
                     exp10's ulp);
  Doppler shift      E_k e^a - offset with the degree-D polynomial of e^a, D <= 14: the documented truncation 2^-53 and
                     D + 4 roundings: 7.8e-16.
A phase without an active chord must give exactly 1.  None of this is borrowed from test_gpu_tcurve.py's TC_TOL.
The errors this sweep is after are far above any of these figures: one chord of 16,400 dropped, counted twice or read
from a stale part is 6e-5; a wrong octave or table extent is 1e-3 or more.

Measured maxima per case and branch: profiles/tc_sweep_errors.txt (written from this module's output when
PROM_TC_SWEEP_RECORD names a file).
"""
import functools
import os

import numpy as np
import pytest

from helpers import tc_sweep as S

pytestmark = pytest.mark.gpu
LD = np.longdouble


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


def run(dev, sw, N, y, z, fout, planet_y, factors):
    """One problem through the C-ABI: (R [n_orb, n_wav], stats, columns [n_orb, n_pr])."""
    from prometheus_amd import _native
    n_orb, n_pr = N.shape
    dens = np.zeros((n_pr, n_orb, 8))
    dens[:, :, 0] = N.T
    with dev.lock:
        tid = dev.table_upload(sw["tx"], sw["ty"], S.OFFSET)
        try:
            prob = _native.TransitInputs(
                wavelength=sw["wav"], chord_y=y, chord_z=z, chord_fout=fout, n_orb=n_orb, x=np.arange(8.0), delta_x=1.0,
                planet_y=planet_y, planet_R=S.PLANET_R, moon_y=np.zeros((0, n_orb)), moon_R=np.zeros(0),
                scenarios=[{"kind": _native.DENSITY_TABULATED, "params": [], "shift": np.asarray(factors, dtype=np.float64),
                            "n_tabulated": dens.ravel(), "constituents": [{"table_id": tid, "chi": 1.0}]}])
            dev.transit_set(prob)
            st = dev.transit_run(stats=True)
            R = dev.transit_result()
            cols = dev.transit_columns()[0]
        finally:
            dev.table_free(tid)
    return R, st, cols


def record(line):
    print(line)
    path = os.environ.get("PROM_TC_SWEEP_RECORD")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def check(case, R, st, cols, N, blocked, fout, Y, mode):
    """Every row of R against reference_R within the module docstring's bound, every phase measured before any fails."""
    assert st["tau_kernel_variant"] in (81, 91), st
    assert st["exact_phases"] == 0
    design = np.where(blocked, 0.0, N)
    same = np.array_equal(cols, design)
    if not same:
        print("%s: transit_columns() differs from the design at %d chords; the reference takes the device's columns"
              % (case, np.count_nonzero(cols != design)))
    Rref = S.reference_R(fout, blocked, cols, Y)
    err = np.abs(R.astype(LD) - Rref).astype(np.float64)
    n_orb = R.shape[0]
    Y = np.broadcast_to(Y, R.shape)
    fails = []
    for o in range(n_orb):
        act = cols[o][cols[o] > 0]
        if len(act) == 0:
            ok = bool(np.all(R[o] == 1.0))
            record("%s phase %d: no active chord, max |R - 1| = %.3e" % (case, o, float(np.max(np.abs(R[o] - 1.0)))))
            if not ok:
                fails.append("phase %d has no active chord but R != 1 at %d points (max |R - 1| = %.3e)"
                             % (o, np.count_nonzero(R[o] != 1.0), float(np.max(np.abs(R[o] - 1.0)))))
            continue
        n_max, n_min = float(act.max()), float(act.min())
        L = S.table_octaves(n_max, n_min)
        truncated = S.K_SAT * (n_max / n_min) >= 2.0 ** (L + S.K_EPS_EXP)
        q = Y[o] * LD(n_max)
        above = S.tol_exact_sum(len(act)) if truncated else S.TOL_OPAQUE + 6 * S.U
        by_region = np.concatenate([[S.TOL_TAIL], np.full(L, S.TOL_OCTAVE), [above]])   # index r + 1
        r = S.regions(q, L)
        bound = by_region[r + 1]
        for side in (1 - 2.0 ** -40, 1 + 2.0 ** -40):
            bound = np.maximum(bound, by_region[S.regions(q * LD(side), L) + 1])
        bound = bound + S.TOL_LOOKUP[mode]
        e = err[o]
        octs = [float(e[r == j].max()) if np.any(r == j) else 0.0 for j in range(L)]
        jw = int(np.argmax(octs))
        record("%s phase %d: nact %d L %d%s tail %.2e octaves %.2e (j = %d) above %.2e | per octave %s"
               % (case, o, len(act), L, " truncated" if truncated else "", e[r == -1].max() if np.any(r == -1) else 0.0,
                  octs[jw], jw, e[r == L].max() if np.any(r == L) else 0.0, " ".join("%.1e" % v for v in octs)))
        bad = np.where(e > bound)[0]
        if len(bad):
            w = bad[np.argmax(e[bad] / bound[bad])]
            fails.append("phase %d: %d points over the bound; worst at q = %.17g (branch %d of L = %d): %.3e > %.3e"
                         % (o, len(bad), float(q[w]), int(r[w]), L, float(e[w]), float(bound[w])))
    assert not fails, case + ": " + "; ".join(fails)
    assert same, "%s: transit_columns() is not the design bit for bit" % case


# ---- chord counts --------------------------------------------------------------------------------------------------
MATRIX = [(n, None) for n in (1, 15, 32, 33, 64, 240, 320, 352, 960, 1216, 3100, 4801, 16384 + 32, 16390)] + \
         [(n, p) for n in (2400, 1056) for p in ("1", "3", "16")]


@pytest.mark.parametrize("n_pr,parts", MATRIX, ids=["%d-parts_%s" % (n, p or "default") for n, p in MATRIX])
def test_chord_count_matrix(dev, n_pr, parts, monkeypatch):
    """Static lookups, log-uniform columns over twelve decades, four phases (all active; none active; the planet over
    about 45 % of the ring; one active chord) at the chord counts where k_tc_build changes its front end (k_columns8's
    partials for n_pr % 32 == 0, sweeps of 3,072 chords otherwise), its number of parts ((n_pr + 299) / 300 up to 16,
    or PROM_TC_PARTS) and its chord source (a part of more than 1,024 chords reads global memory): see
    tc_sweep.build_config and test_tc_sweep_cpu.py::test_build_configurations."""
    if parts:
        monkeypatch.setenv("PROM_TC_PARTS", parts)
    p = S.matrix_problem(n_pr)
    sw = S.sweep_for("loguniform", p["N"][0])
    R, st, cols = run(dev, sw, p["N"], p["y"], p["z"], p["fout"], p["planet_y"], np.ones(4))
    front, n_parts, src, _ = S.build_config(n_pr, parts)
    case = "matrix n_pr %d (%s, %d parts, %s)" % (n_pr, front, n_parts, src)
    assert st["tau_kernel_variant"] == 81
    assert st["blocked_chords"] == int(p["blocked"].sum())
    assert st["active_chords"] == int(((p["N"] > 0) & ~p["blocked"]).sum())
    assert st["transparent_chords"] == 4 * n_pr - st["blocked_chords"] - st["active_chords"]
    check(case, R, st, cols, p["N"], p["blocked"], p["fout"], sw["Y"], "static")


# ---- column kinds x lookup kernels -----------------------------------------------------------------------------------
FACTORS = 1.0 + 3e-5 * np.array([-1.0, -0.5, 0.0, 0.5, 1.0])
KINDS = [(k, n) for k in S.KINDS for n in (240, 2400)]
kinds = pytest.mark.parametrize("kind,n_pr", KINDS, ids=["%s-%d" % kn for kn in KINDS])


@functools.lru_cache(maxsize=None)
def kind_problem(kind, n_pr):
    N = S.design_columns(kind, n_pr, 1)
    y, z = S.ring(n_pr)
    return {"N": N, "y": y, "z": z, "fout": S.chord_fout(n_pr), "sw": S.sweep_for(kind, N[0])}


def run_kind(dev, kind, n_pr, factors):
    p = kind_problem(kind, n_pr)
    n_orb = len(factors)
    N = np.repeat(p["N"], n_orb, axis=0)
    R, st, cols = run(dev, p["sw"], N, p["y"], p["z"], p["fout"], np.full(n_orb, S.PLANET_FAR), factors)
    return p, N, R, st, cols


def exact_sum_evals(st, p, q, n_pr, n_orb, dead):
    """`two`: the table is truncated at the 64-octave cap (curve header flag 4), so every point with q >= 2^57 takes
    the exact sum, which the kernels count as nact exp evaluations; the table itself is 16 nodes x 64 octaves x nact
    per phase.  Points within 2^-40 of the cap may fall on either side.  The lanes past the end of a row evaluate the
    row's last wavelength (the largest q, above the cap) and are counted with the rest: at most `dead` per phase."""
    sw = p["sw"]
    assert sw["L"] == 64 and sw["cap"] < sw["top"]
    table = n_orb * n_pr * 16 * 64
    sure = int(np.count_nonzero(q >= LD(sw["cap"]) * LD(1 + 2.0 ** -40)))
    maybe = int(np.count_nonzero(q >= LD(sw["cap"]) * LD(1 - 2.0 ** -40)))
    extra = st["exp_evals"] - table
    assert extra % n_pr == 0 and sure <= extra // n_pr <= maybe + n_orb * dead, (st["exp_evals"], table, sure, maybe)
    assert sure >= 16 * n_orb and maybe + n_orb * dead < 0.6 * q.size


def dead_lanes_tc(n_wav):
    return -n_wav % 256   # k_sigma_tc: 256 wavelengths per workgroup


DEAD_LANES_TW = 4 * 63    # k_sigma_tw: 64-wavelength chunks per (window, row); the planner makes 3 windows here


@kinds
@pytest.mark.parametrize("lookup", ["poly", "exp10"])
def test_column_kinds_static(dev, kind, n_pr, lookup, monkeypatch):
    """Two phases without Doppler shift: k_sigma_tc's shared-target instantiation, with the polynomial node lookups
    and with numpy.interp + exp10 (PROM_SIG_POLY=0)."""
    if lookup == "exp10":
        monkeypatch.setenv("PROM_SIG_POLY", "0")
    p, N, R, st, cols = run_kind(dev, kind, n_pr, np.ones(2))
    assert st["tau_kernel_variant"] == 81
    Y = p["sw"]["Y"]
    check("%s n_pr %d static %s" % (kind, n_pr, lookup), R, st, cols, N, np.zeros(N.shape, dtype=bool), p["fout"], Y, "static")
    if kind == "two":
        exact_sum_evals(st, p, np.stack([Y, Y]) * LD(p["sw"]["n_max"]), n_pr, 2, dead_lanes_tc(len(Y)))
    else:
        assert st["exp_evals"] == 2 * n_pr * 16 * p["sw"]["L"]


@kinds
def test_column_kinds_doppler(dev, kind, n_pr, monkeypatch):
    """Five phases with Doppler factors 1 +- 3e-5 (the middle one exactly 1): the target-window lookups (PROM_TW=1,
    k_sigma_tw, variant 91; the planner takes these tables under its default caps,
    test_tc_sweep_cpu.py::test_window_planner_takes_the_sweeps) and k_sigma_tc's per-phase lookups (PROM_TW=0,
    variant 81), bitwise equal."""
    monkeypatch.setenv("PROM_TW", "1")
    p, N, R, st, cols = run_kind(dev, kind, n_pr, FACTORS)
    assert st["tau_kernel_variant"] == 91, st
    sw = p["sw"]
    Y = S.reference_Y(sw["tx"], sw["ty"], S.OFFSET, FACTORS, sw["wav"])
    check("%s n_pr %d doppler tw" % (kind, n_pr), R, st, cols, N, np.zeros(N.shape, dtype=bool), p["fout"], Y, "doppler")
    if kind == "two":
        exact_sum_evals(st, p, Y * LD(sw["n_max"]), n_pr, 5, DEAD_LANES_TW)
    monkeypatch.setenv("PROM_TW", "0")
    _, _, R0, st0, _ = run_kind(dev, kind, n_pr, FACTORS)
    assert st0["tau_kernel_variant"] == 81, st0
    assert np.array_equal(R, R0), "k_sigma_tw and k_sigma_tc differ at %d points, max %.3e" % (
        np.count_nonzero(R != R0), float(np.max(np.abs(R - R0))))
    if kind == "two":
        exact_sum_evals(st0, p, Y * LD(sw["n_max"]), n_pr, 5, dead_lanes_tc(Y.shape[1]))
