"""The target-window planner (build_target_windows, prometheus_amd/csrc/prom_window.hip) and the index arithmetic
of k_sigma_tw's first pass (prometheus_amd/csrc/tw_index.h), on the host.

The planner is pure host code: tests/helpers/window_host.cpp links it, compiled as C++ with g++, and returns the
raw plan (row starts, SigSeg per species, staged wavelength range per window).  Inputs come from the oracle with
no device: the wavelength grid, the tables' node x's and the per-phase Doppler factors of reduced C3, of fine
low-end grids of C4 and C3 (a Doppler spread many 64-wavelength chunks wide, row counts 2 .. 8 where the kernel's
row dispatch changes) and of a synthetic problem that reaches the slice kinds a setup file cannot (a table
narrower than the targets: kind 0; a table whose node spacing changes inside a window: kind 3).

Every plan is checked against plain numpy over every (row, wavelength): the partition, the slices and their
guesses (the header's own tw_guess, called through the harness), the LDS budget, and an audit that walks every
window, wave, dispatched row or pair, chunk and lane as the kernel does, with the header's functions, and counts
every index that would leave its array.  The audit run with the pair dispatch as it was before empty rows counted
as absent (a test-only argument of the harness) reports the reads that rule made outside the wavelength array and
outside the staged wavelengths; with the header's rule it reports none.
"""
import ctypes as C
import os

import numpy as np
import pytest

from helpers.window_plan import (CAP_TUPLES, COUNTERS, CSRC, K_TW_LAMCAP, K_TW_LDS, Caps, Libs, _dp, _ip, debug_counts,
                                 inputs, make_plan)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    return Libs(tmp_path_factory.mktemp("tw"))


def window_of(inp, p):
    """The window of every (row, wavelength), [n_rows, n_wav]: the last window whose start is <= w."""
    w = np.arange(inp.n_wav)
    return np.stack([np.searchsorted(p.row[:-1, o], w, "right") - 1 for o in range(inp.n_rows)])


def check_plan(inp, p, caps, lamfit_all=False):
    nw, NS = p.n_win, inp.ns
    row = p.row.astype(np.int64)
    # 1. partition
    assert np.all(np.diff(row, axis=0) >= 0)
    assert np.all(row[0] == 0) and np.all(row[-1] == inp.n_wav)
    cnt = row[1:] - row[:-1]
    assert np.all(cnt.sum(axis=1) > 0), "an empty window is stored"
    wid = window_of(inp, p)
    assert wid.min() == 0 and wid.max() == nw - 1
    for o in range(inp.n_rows):   # (wid is the partition the plan states)
        assert np.array_equal(np.bincount(wid[o], minlength=nw), cnt[:, o])
    tmin, tmax = np.full(nw, np.inf), np.full(nw, -np.inf)
    np.minimum.at(tmin, wid.ravel(), inp.t.ravel())
    np.maximum.at(tmax, wid.ravel(), inp.t.ravel())
    assert np.all(tmax[:-1] < tmin[1:]), "targets of neighbouring windows overlap"
    # 2. slices
    lam_n = (p.lam[:, 1] - p.lam[:, 0]).astype(np.int64)
    pool = (caps.lds - NS - lam_n) // 3
    off = np.zeros(nw, dtype=np.int64)   # staged nodes of the earlier species
    for s in range(NS):
        X, k = inp.X[s], inp.k[s]
        sg, kind = p.seg[:, s], p.kind[:, s]
        kd = kind[wid]
        sel = kd != 0
        rel = (k - sg["lo"][wid])[sel]
        assert np.all(rel >= 0) and np.all(rel <= (sg["m"][wid] - 2)[sel]), "a bracket outside its slice"
        sel = (kd == 1) | (kd == 2)
        tt = np.ascontiguousarray(inp.t[sel])
        g = np.empty(len(tt), dtype=np.int32)
        b = wid[sel]
        p.L.tw_guess_n(len(tt), _dp(tt), _dp(np.ascontiguousarray(sg["inv"][b])), _dp(np.ascontiguousarray(sg["xs"][b])),
                       _ip(np.ascontiguousarray(sg["m"][b])), _ip(g))
        assert np.all(g >= 0) and np.all(np.abs(g - (k - sg["lo"][wid])[sel]) <= 1), "a guess more than one node off"
        fits = off + sg["m"] <= pool
        outside = (tmin < X[0]) | ~(tmax < X[-1])
        k0 = kind == 0
        assert np.all(outside[k0 & (sg["m"] == 0)])
        assert np.all(~outside[k0 & (sg["m"] > 0)] & (sg["inv"] == 0.0)[k0 & (sg["m"] > 0)] & ~fits[k0 & (sg["m"] > 0)])
        assert not np.any(outside[~k0])
        assert np.all(~fits[kind == 2]) and np.all(fits[(kind == 1) | (kind == 3)])
        # 3. pool ranges, species order
        st = (kind == 1) | (kind == 3)
        assert np.all(sg["pad"][st] == off[st])
        off = off + np.where(st, sg["m"], 0)
    # 3. LDS
    assert np.all(3 * off + NS + lam_n <= caps.lds)
    assert np.all(lam_n >= 0) and np.all(lam_n <= caps.lamcap)
    live = cnt > 0
    stg = lam_n > 0
    assert np.all((row[:-1] >= p.lam[:, :1])[live & stg[:, None]])
    assert np.all((row[1:] <= p.lam[:, 1:])[live & stg[:, None]])
    if caps.lamcap == 0:
        assert not np.any(stg)
    la = np.where(live, row[:-1], inp.n_wav).min(axis=1)
    lz = np.where(live, row[1:], 0).max(axis=1)
    need = np.sum(np.where(p.seg["m"] > 0, p.seg["m"], 0), axis=1)   # (every in-range slice, before the pool is dealt)
    nofit = (3 * need + NS + (lz - la) > caps.lds) | (lz - la > caps.lamcap)
    assert np.array_equal(stg, ~nofit), "wavelengths are staged exactly where they fit beside the slices"
    assert np.all(p.lam[stg, 0] == la[stg]) and np.all(p.lam[stg, 1] == lz[stg])
    if caps.lamfit:
        # every window stages its wavelengths -- except one that cannot be made smaller (a single candidate interval:
        # at most one target of the reference row, the median factor's, or beyond its ends of the extreme rows) and
        # whose wavelengths, the rows' Doppler spread, still do not fit beside its slices
        un = ~stg
        if lamfit_all:
            assert not np.any(un)
        order = np.argsort(inp.shift, kind="stable")
        o_lo, o_hi, o_ref = order[0], order[-1], order[inp.n_rows // 2]
        single = (cnt[:, o_ref] <= 1) & ((cnt[:, o_ref] == 1) | ((cnt[:, o_lo] <= 1) & (cnt[:, o_hi] <= 1)))
        assert np.all(single[un])


def audit(inp, p, rp, old_rule=False, rare=None):
    stored = np.zeros((inp.n_rows, inp.n_wav), dtype=np.uint8)
    cnt = np.zeros(len(COUNTERS), dtype=np.int64)
    rare_a = None if rare is None else np.ascontiguousarray(rare, dtype=np.uint8)
    p.L.tw_audit(_dp(inp.wav), inp.n_wav, _dp(inp.shift), inp.n_rows, inp.ns, inp.Xp, inp.nxp, p.seg.ctypes.data,
                 _ip(p.row), _ip(p.lam), p.n_win, rp, int(old_rule), None if rare_a is None else rare_a.ctypes.data,
                 stored.ctypes.data, cnt.ctypes.data_as(C.POINTER(C.c_int64)))
    return dict(zip(COUNTERS, (int(c) for c in cnt))), stored


def check_audit(inp, p, rare=None):
    """4. the kernel index audit, both row groupings: no index out of range, every (row, wavelength) stored once."""
    out = {}
    for rp in (1, 2):
        c, stored = audit(inp, p, rp, rare=rare)
        for key in ("global_oor", "staged_oor", "guess_oor", "step_oor", "bracket_bad"):
            assert c[key] == 0, (rp, key, c)
        assert c["win_first"] + c["win_second"] == p.n_win
        assert np.all(stored == 1), "RP %d: %d points not stored exactly once" % (rp, int(np.sum(stored != 1)))
        out[rp] = c
    return out


def test_header_constants_and_small_functions(libs):
    hdr = open(os.path.join(CSRC, "prom_internal.h")).read()
    assert "#define PROM_TW_LDSD %d " % K_TW_LDS in hdr and "constexpr int kTwLamCap = %d;" % K_TW_LAMCAP in hdr
    L = libs()
    # waves per row or pair: 4 for one unit, 2 for two or three, 1 from four
    assert [L.tw_waves_per_unit(n) for n in (1, 2, 3, 4, 5, 8, 64)] == [4, 2, 2, 1, 1, 1, 1]
    # a pair: both, the first alone, the second alone, neither; an empty row is absent like a rare one
    assert [L.tw_pair_rows(a, b) for a, b in ((0, 0), (0, 1), (1, 0), (1, 1))] == [3, 1, 2, 0]
    assert [L.tw_row_absent(r, w0, w1) for r, w0, w1 in ((0, 0, 1), (1, 0, 1), (0, 0, 0), (0, 7, 7), (0, 5, 70))] == \
        [0, 1, 1, 1, 0]
    assert [L.tw_chunks(a, b) for a, b in ((0, 0), (0, 1), (0, 64), (0, 65), (100, 228), (100, 229))] == \
        [0, 1, 1, 2, 2, 3]
    # every chunk a non-empty row can be asked for reads inside the row (global) or from its first chunk on (staged)
    for w0, w1 in ((0, 1), (0, 64), (10, 75), (1000, 1100), (14500, 14561)):
        for k in range(0, 9):
            c = L.tw_chunk_read(w0, w1, k)
            assert w0 <= c < w1 and (c == w0 + 64 * k or (w0 + 64 * k >= w1 and c == w0))
            for lane in (0, 1, 63):
                assert w0 <= L.tw_lam_global(w0, w1, k, lane) < w1
                assert L.tw_lam_staged(w0, w1, k, lane, w0 - 5) == c + lane - (w0 - 5)


@pytest.mark.parametrize("tup", [()] + CAP_TUPLES, ids=lambda t: "-".join(t) or "default")
def test_plan_reduced_c3(libs, tup):
    inp = inputs("C3r")
    assert (inp.n_wav, inp.n_rows, inp.ns) == (351222, 16, 3)
    caps = Caps(inp.n_rows, tup)
    p = make_plan(libs, inp, caps)
    print(caps, debug_counts(p))
    check_plan(inp, p, caps, lamfit_all=True)
    c = check_audit(inp, p)
    print(c[2])
    if tup == ():
        # the documented plan (prom_internal.h): 1,859 windows, wavelengths staged in 1,830
        assert debug_counts(p)[0] == 1859 and debug_counts(p)[5] == 1830
        assert debug_counts(p)[3] > 0
    if tup == ("256", "8192", "16"):
        assert debug_counts(p)[2] > 0 and debug_counts(p)[4] > 0
    if tup == ("4", "32", "96"):
        assert debug_counts(p)[2] > 0 and debug_counts(p)[3] > 0


def test_plan_reduced_c3_lds_2560_documented(libs):
    """prom_internal.h's A/B figures: at 2,560 doubles 1,863 windows; with PROM_TW_LAMFIT=1 every window stages."""
    inp = inputs("C3r")
    p = make_plan(libs, inp, Caps(inp.n_rows, ("256", "8192", "2560")))
    assert p.n_win == 1863
    caps = Caps(inp.n_rows, ("256", "8192", "2560", "1024", "1"))
    p = make_plan(libs, inp, caps)
    assert debug_counts(p)[5] == p.n_win


def test_plan_deterministic_across_threads(libs):
    """5. reduced C3 plans on several host threads (candidate intervals / 65,536, here 5): the same plan twice, and
    the plan of a second copy of the library."""
    inp = inputs("C3r")
    assert inp.n_wav // 65536 >= 2
    caps = Caps(inp.n_rows)
    a, b = make_plan(libs, inp, caps), make_plan(libs, inp, caps)
    c = make_plan(libs, inp, Caps(inp.n_rows, ("256", "8192", "2816", "1024", "0", "1", "64")))   # (the defaults, spelt out)
    for q in (b, c):
        assert a.n_win == q.n_win and np.array_equal(a.row, q.row) and np.array_equal(a.lam, q.lam)
        assert a.seg.tobytes() == q.seg.tobytes()


FINE_CAPS = [(), ("256", "8192", "2816", "0"), ("100", "8192", "2816")]


@pytest.mark.parametrize("tup", FINE_CAPS + CAP_TUPLES, ids=lambda t: "-".join(t) or "default")
@pytest.mark.parametrize("name,n", [("C4fine", 2), ("C4fine", 3), ("C4fine", 5), ("C4fine", 8), ("C3fine", 3),
                                    ("C3fine", 6)])
def test_plan_fine_grids(libs, name, n, tup):
    inp = inputs(name, n)
    if name == "C4fine":
        assert (inp.n_wav, inp.n_wav % 64, inp.ns, int(inp.nx[0])) == (14561, 33, 1, 203863)
    else:
        assert (inp.n_wav, inp.ns) == (12001, 3)
    caps = Caps(inp.n_rows, tup)
    p = make_plan(libs, inp, caps)
    check_plan(inp, p, caps)
    c = check_audit(inp, p)
    print(name, n, caps, debug_counts(p), c[2])


def test_c4fine_holds_the_empty_row_cases_and_the_old_dispatch_reads_out_of_range(libs):
    """The audit's reason to exist.  C4fine's Doppler spread at the low end (~590 wavelengths) leaves rows without
    wavelengths in first-pass windows whose pair partner has some: at the grid's low end (w1 == 0), at its high end
    (w0 == n_wav) and in the interior.  With the pair dispatch as it was before such rows counted as absent, the
    audit reports staged offsets outside [0, (lw1 - lw0) + 64) (2 phases, default caps) and a read of wav[-1]
    (8 phases, wavelengths never staged); with tw_index.h's rule none (test_plan_fine_grids)."""
    seen = {"pair_empty_low": 0, "pair_empty_high": 0, "pair_empty_mid": 0}
    inp = inputs("C4fine", 2)
    p = make_plan(libs, inp, Caps(2))
    c_new, _ = audit(inp, p, 2)
    c_old, stored = audit(inp, p, 2, old_rule=True)
    print("C4fine 2 phases:", p.n_win, "windows;", c_old)
    # (seen: 143 windows, 13 with such a pair, 12 of them with staged offsets out of range, 884 lanes)
    assert c_old["pair_empty_win"] == c_new["pair_empty_win"] >= 1
    assert c_old["win_staged_oor"] >= 1 and c_old["staged_oor"] >= 64
    assert c_old["win_staged_oor"] <= c_old["pair_empty_win"]
    assert np.all(stored == 1)   # (nothing is stored from those lanes: R never showed it)
    assert c_new["staged_oor"] == 0 and c_new["global_oor"] == 0
    for key in seen:
        seen[key] += c_new[key]
    inp = inputs("C4fine", 8)
    p = make_plan(libs, inp, Caps(8, ("256", "8192", "2816", "0")))
    assert not np.any(p.lam[:, 1] > p.lam[:, 0])
    c_new, _ = audit(inp, p, 2)
    c_old, stored = audit(inp, p, 2, old_rule=True)
    print("C4fine 8 phases, global wavelengths:", p.n_win, "windows;", c_old)
    # (seen: 166 windows, 9 with such a pair, one reading wav[-1] on 128 lanes)
    assert c_new["pair_empty_low"] >= 1, c_new
    assert c_old["win_global_oor"] >= 1 and c_old["global_oor"] >= 64
    assert np.all(stored == 1)
    assert c_new["staged_oor"] == 0 and c_new["global_oor"] == 0
    for key in seen:
        seen[key] += c_new[key]
    # rows of 1: the single-row dispatch never ran an empty row
    c1, _ = audit(inp, p, 1, old_rule=True)
    assert c1["global_oor"] == 0
    for n in (3, 5, 8):
        c, _ = audit(inputs("C4fine", n), make_plan(libs, inputs("C4fine", n), Caps(n)), 2)
        for key in seen:
            seen[key] += c[key]
    print(seen)
    assert all(v >= 1 for v in seen.values()), seen


def test_plan_synthetic_end_rules_and_unguessed_slices(libs):
    inp = inputs("synthetic")
    assert inp.n_wav % 64 == 41
    for tup in [(), ("64", "8192", "2816"), ("256", "8192", "2816", "0"), ("100", "8192", "400")]:
        caps = Caps(inp.n_rows, tup)
        p = make_plan(libs, inp, caps)
        print(caps, debug_counts(p))
        check_plan(inp, p, caps)
        c = check_audit(inp, p)
        assert c[1]["win_second"] > 0 and c[1]["win_first"] > 0
        assert np.any(p.kind[:, 0] == 0) and np.any(p.kind[:, 0] == 1)   # table 0: outside below and above, staged
        assert np.any(p.kind[:, 1] == 3), "no slice across the change of node spacing"
        first = np.all((p.kind == 1) | (p.kind == 3), axis=1)
        assert np.any(first & (p.kind[:, 1] == 3)), "no first-pass window with a searched slice"
    # rows the second pass takes (curve header flags): their partners run alone, every point still stored once
    for rare in ([1, 0, 0, 0], [0, 1, 1, 0], [1, 1, 0, 1], [1, 1, 1, 1]):
        check_audit(inp, p, rare=rare)


def test_odd_row_counts_leave_the_last_row_alone(libs):
    """3 and 5 rows: the last row has no partner (ob >= n_rows); 2-3 rows or pairs share two waves each."""
    for n in (3, 5):
        inp = inputs("C4fine", n)
        p = make_plan(libs, inp, Caps(n))
        c = check_audit(inp, p)
        assert c[1]["lanes"] > 0 and c[2]["lanes"] > 0
        check_audit(inp, p, rare=[0] * (n - 1) + [1])
        check_audit(inp, p, rare=[1] + [0] * (n - 1))
