"""The conditions the transmission-curve sweep's designs must meet (tests/helpers/tc_sweep.py), so that
tests/test_gpu_tc_sweep.py cannot pass by leaving cases out, and the longdouble reference against 40-digit sums.
No GPU and none of the product's code.

One condition is weaker than first asked for.  The sweep was to put a point within 4 ulp of every octave boundary
q = 2^j on each side.  The design asks for those targets (asserted below), but a cross-section reaches the device as a
float64 node y = log10(Y + offset) with |y| = 18 .. 29, and neighbouring y's are ln10 ulp(y) = 37 ulp of Y apart: the
nearest cross-sections the table can express are asserted instead, within BOUNDARY_ULPS = 40 ulp on each side.
"""
import numpy as np
import pytest

from helpers import tc_sweep as S

LD = np.longdouble


def sweep(kind, n_pr=240):
    return S.sweep_for(kind, S.design_columns(kind, n_pr, 1)[0])


@pytest.mark.parametrize("kind", S.KINDS)
def test_design_covers_every_branch(kind):
    sw = sweep(kind)
    L, q = sw["L"], sw["q"]
    assert np.all(np.diff(sw["y"]) > 0) and np.all(np.diff(sw["Y"]) > 0) and np.all(np.diff(sw["wav"]) > 0)
    assert np.array_equal(sw["tx"][S.PAD:S.PAD + len(q)], sw["wav"]) and len(sw["tx"]) == len(sw["ty"])
    assert L == {"equal": 13, "loguniform": S.table_octaves(S.N_EQUAL, S.design_columns(kind, 240, 1).min()),
                 "two": 64}[kind]
    r = S.regions(q, L)
    for j in range(L):
        assert np.count_nonzero(r == j) >= 16, j
    assert np.count_nonzero(r == -1) >= 8 and np.count_nonzero(r == L) >= 8
    assert float(q[0]) < 2.0 ** -11 and float(q[-1]) > 3.9 * sw["top"]
    # three points straddling top = 40 N_max / N_min
    rel = np.asarray(q / LD(sw["top"]) - 1, dtype=np.float64)
    assert np.any((rel < 0) & (rel > -1e-8)) and np.any((rel > 0) & (rel < 1e-8)) and np.any(np.abs(rel) < 1e-13)
    for j in range(S.K_EPS_EXP, L + S.K_EPS_EXP + 1):
        b = 2.0 ** j
        # the targets: within 4 ulp on each side, and the boundary itself
        t = (sw["targets"] - b) / (b * 2.0 ** -52)
        assert np.any((t < 0) & (t >= -4)) and np.any((t > 0) & (t <= 4)) and np.any(t == 0), j
        # what the table expresses: a point on each side within BOUNDARY_ULPS
        d = np.asarray((q - LD(b)) / LD(b * 2.0 ** -52), dtype=np.float64)
        assert np.any((d < 0) & (d >= -S.BOUNDARY_ULPS)) and np.any((d >= 0) & (d <= S.BOUNDARY_ULPS)), (j, d[np.abs(d) < 200])
    if kind == "two":
        # truncated at the 64-octave cap: the exact sum runs between the cap and the top
        assert sw["cap"] == 2.0 ** 57 and np.count_nonzero((q > sw["cap"]) & (q < sw["top"])) >= 16
    # the polynomial lookups' range: ln10 |dy| <= 0.0866 keeps degree <= 14 (prom_segments.hip sigma_poly_degree)
    assert np.log(10.0) * np.max(np.diff(sw["ty"])) < 0.0866


def test_matrix_phases():
    for n_pr in (1, 15, 33, 320, 4801):
        p = S.matrix_problem(n_pr)
        N, bl = p["N"], p["blocked"]
        act = (N > 0) & ~bl
        assert act[0].all() and not act[1].any() and act[3].sum() == 1
        assert not bl[[0, 1, 3]].any()
        if n_pr >= 15:
            assert 0.3 * n_pr < bl[2].sum() < 0.6 * n_pr
        assert N[0].max() == S.N_EQUAL == N[3].max() and np.all((p["fout"] >= 0.5) & (p["fout"] < 1.5))
        assert N[2][act[2]].max() == S.N_EQUAL


def test_build_configurations():
    """The chord counts of the GPU matrix reach every k_tc_build configuration the sweep is after."""
    got = {n: S.build_config(n)[:3] for n in (1, 15, 32, 33, 64, 240, 320, 352, 960, 1216, 3100, 4801, 16416, 16390)}
    assert got[32] == ("partials", 1, "LDS") and got[240] == ("sweep x1", 1, "LDS")
    assert [got[n][:2] for n in (320, 352, 960, 1216)] == [("partials", p) for p in (2, 2, 4, 5)]
    assert all(l % 64 for n in (320, 352, 960, 1216) for l in S.build_config(n)[3])
    assert got[3100] == ("sweep x2", 11, "LDS") and got[4801] == ("sweep x2", 16, "LDS")
    assert got[16416] == ("partials", 16, "global") and got[16390] == ("sweep x6", 16, "mixed")
    assert S.build_config(2400, 1)[1:3] == (1, "global") and S.build_config(1056, 1)[1:3] == (1, "global")
    assert S.build_config(2400, 3)[1:3] == (3, "LDS") and S.build_config(1056, 16)[1:3] == (16, "LDS")


def _mp_R(mpmath, fout, blocked, N, Y):
    mp = mpmath.mp
    F = [mp.mpf(float(f)) for f in fout]
    out = []
    for yv in Y:
        yv = _mp_of(mpmath, yv)
        s = mp.mpf(0)
        for f, b, n in zip(F, blocked, N):
            if not b:
                s += f * mp.exp(-mp.mpf(float(n)) * yv)
        out.append(s / sum(F))
    return out


def _mp_of(mpmath, v):
    """A longdouble as an mpf, exactly (two float64 pieces)."""
    hi = np.float64(v)
    lo = np.float64(v - LD(hi))
    return mpmath.mpf(float(hi)) + mpmath.mpf(float(lo))


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("n_pr", [1, 33, 320])
def test_reference_against_mpmath(kind, n_pr):
    """reference_R against a 40-digit sum at every 25th point: 1e-17 absolute."""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 40
    N = S.design_columns(kind, n_pr, 1)
    sw = S.sweep_for(kind, N[0])
    y, z = S.ring(n_pr)
    blocked = S.blocked_by(y, z, 1.0)[None, :] if n_pr > 1 else np.zeros((1, 1), dtype=bool)
    fout = S.chord_fout(n_pr)
    Y = sw["Y"][::25]
    R = S.reference_R(fout, blocked, N, Y)[0]
    Rm = _mp_R(mpmath, fout, blocked[0], N[0], Y)
    err = max(abs(_mp_of(mpmath, r) - m) for r, m in zip(R, Rm))
    assert err < 1e-17, err


def test_reference_one_chord_closed_form():
    sw = sweep("equal", 1)
    R = S.reference_R(np.array([0.75]), np.zeros((1, 1), dtype=bool), np.array([[S.N_EQUAL]]), sw["Y"])[0]
    assert np.all(np.abs(R - np.exp(-sw["q"])) <= 2 * np.finfo(LD).eps)
    # a blocked chord gives 0, a zero column gives its whole weight
    R2 = S.reference_R(np.array([1.0, 3.0]), np.array([[True, False]]), np.array([[S.N_EQUAL, 0.0]]), sw["Y"])[0]
    assert np.all(R2 == LD(0.75))


def test_reference_Y_on_and_between_nodes():
    """Static targets land on nodes (Y is what the node expresses); shifted targets follow numpy.interp's bracket and
    its end rules."""
    sw = sweep("loguniform")
    Y = S.reference_Y(sw["tx"], sw["ty"], S.OFFSET, np.array([1.0]), sw["wav"])[0]
    assert np.array_equal(Y, sw["Y"])
    f = np.array([1 - 3e-5, 1 + 3e-5])
    Ys = S.reference_Y(sw["tx"], sw["ty"], S.OFFSET, f, sw["wav"])
    t = f[:, None] * sw["wav"][None, :]
    assert t.min() > sw["tx"][0] and t.max() < sw["tx"][-1]          # the padding covers the Doppler spread
    v = np.stack([np.interp(t[i], sw["tx"], sw["ty"]) for i in range(2)])
    assert np.max(np.abs(np.asarray(np.log10(Ys + LD(S.OFFSET)), dtype=np.float64) - v)) < 1e-13
    out = S.reference_Y(sw["tx"], sw["ty"], S.OFFSET, np.array([0.5, 2.0]), sw["wav"][:3])
    assert np.all(out[0] == sw["Y"][0]) and np.all(out[1] == sw["Y"][-1])


def test_window_planner_takes_the_sweeps(tmp_path):
    """The target-window planner (prom_window.hip, built for the host) accepts the sweeps' tables with the Doppler
    factors of test_gpu_tc_sweep.py under prom_transit_set's default caps: PROM_TW=1 there needs no cap knobs."""
    from helpers import window_plan as W
    libs = W.Libs(tmp_path)
    f = 1.0 + 3e-5 * np.array([-1.0, -0.5, 0.0, 0.5, 1.0])
    for kind in S.KINDS:
        sw = sweep(kind)
        plan = W.make_plan(libs, W.Inputs(sw["wav"], f, [sw["tx"]]), W.Caps(len(f)))
        assert 1 <= plan.n_win <= 8 and np.all(plan.kind == 1), (kind, W.debug_counts(plan))


def test_tolerances():
    assert abs(S.TOL_OCTAVE - 1.47e-14) < 1e-16 and abs(S.TOL_TAIL - 9.82e-16) < 1e-18
    assert S.TOL_LOOKUP["static"] < S.TOL_LOOKUP["doppler"] < 1e-15
