"""The stage records of the target windows (prometheus_amd/csrc/tw_stage.h), on the host.

prom_transit_set derives one 64-byte record per window from the finished plan (build_target_windows' SigSeg per
species and staged wavelength range), and k_sigma_tw's prologue stages the species' slices from it: pool entry i
belongs to the species whose number is the count of the record's boundaries <= i, is table record i + off[species]
and goes to fixed LDS slots.  tests/tw_stage_host.cpp compiles that header for the host with g++ (as
tests/helpers/window_host.cpp does the planner) and walks every pool entry of every window with its functions.

Checked against plain numpy on the raw plan (plan.seg, plan.lam): every pool entry below the staged total maps to
exactly one species -- the one whose [pad, pad + m) holds it -- to record lo + (i - pad) of that species and to the
LDS slots the first pass' lookups read (node k of species s at the x base + k, its {E, L} at the el base + 2 k);
species without a slice in the pool own no entry; nlam and lw0 are the plan's; the mode bits are what the slice
kinds imply; the slots of distinct entries, of the slices' last upper nodes and of the wavelengths do not collide and
end inside the LDS budget.

Plans: reduced C3, the fine low-end grids of C3 (2 and 8 phases) and C4 (2 phases) and the synthetic problem of
tests/test_window_plan_cpu.py, each under the default caps and every tuple of window_plan.CAP_TUPLES.  Each input
names the slice kinds and staging it is there for, and the test fails if no plan of that input reaches them; which
caps reach which (debug_counts: windows, slices staged / global / staged unguessed / outside the table, windows with
staged wavelengths), as found when the test was written:

  C3r        default: 1,859 windows, 5,543 staged and 34 staged unguessed slices, 1,830 windows' wavelengths staged
             (8, 64, 2560): 88,115 tiny windows, all staged, every window's wavelengths staged
             (4, 32, 96): 19 global, 20 unguessed, 14 outside-the-table slices (unguessed ones that fit no pool)
             (256, 8192, 16): 675,707 global slices, no wavelengths staged
             LAMCAP 0 tuples: no wavelengths staged; the LAMFIT tuple: every window's staged
  C3fine 2/8 100 windows by default, 2 unguessed slices, 10 windows' wavelengths staged (the Doppler spread);
             global slices under (256, 8192, 16) only
  C4fine 2   one species: 4 unguessed slices under every tuple; global and outside-the-table under (256, 8192, 16)
  synthetic  outside-the-table slices (table 0 narrower than the targets: rare windows) and 2 unguessed ones (table
             1's change of node spacing) under every tuple; global slices under (4, 32, 96) and (256, 8192, 16)
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import window_plan as WP

STAGE = np.dtype([("tot", "<i4"), ("lw0", "<i4"), ("nlam", "<i4"), ("mode", "<i4"), ("bnd", "<i4", 4),
                  ("off", "<i4", 4), ("base", "<i4", 4)])
RARE, SEARCH, EXACT = 1, 2, 4   # tw_stage.h kTwRare, kTwSearch, kTwExact

INPUTS = [("C3r", None), ("C3fine", 2), ("C3fine", 8), ("C4fine", 2), ("synthetic", None)]
CAPS = [()] + list(WP.CAP_TUPLES)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    return WP.Libs(tmp_path_factory.mktemp("tw"))


@pytest.fixture(scope="module")
def stage_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tw_stage") / "libtw_stage_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + WP.rocm_include(),
                    "-I" + WP.CSRC, "-fPIC", "-shared", os.path.join(WP.REPO, "tests", "tw_stage_host.cpp"), "-o", out],
                   check=True)
    L = C.CDLL(out)
    ip = C.POINTER(C.c_int32)
    L.tw_stage_records.argtypes = [C.c_void_p, ip, C.c_int32, C.c_int32, C.c_void_p]
    L.tw_stage_records.restype = None
    L.tw_stage_entries.argtypes = [C.c_void_p, C.c_int32, C.c_int32, ip, ip, ip, ip]
    L.tw_stage_entries.restype = None
    L.tw_stage_bases.argtypes = [C.c_void_p, C.c_int32, C.c_int32, ip, ip, ip]
    L.tw_stage_bases.restype = None
    assert L.tw_stage_sizeof() == STAGE.itemsize == 64
    return L


def records(L, p, ns):
    st = np.zeros(p.n_win, dtype=STAGE)
    L.tw_stage_records(p.seg.ctypes.data, WP._ip(p.lam), p.n_win, ns, st.ctypes.data)
    return st


def check_records(L, p, ns, caps, marked=False):
    seg, kind = p.seg, p.seg["kind"] & 3
    st = records(L, p, ns)
    staged = (seg["kind"] & 1) != 0                      # kinds 1 and 3: a slice in the pool
    m = np.where(staged, seg["m"], 0).astype(np.int64)
    tot = m.sum(axis=1)
    pad = np.cumsum(m, axis=1) - m                       # the planner's offsets: species order, no holes
    assert np.all(seg["pad"][staged] == pad[staged])
    # the header of the record
    assert np.array_equal(st["tot"], tot)
    assert np.array_equal(st["lw0"], p.lam[:, 0]) and np.array_equal(st["nlam"], p.lam[:, 1] - p.lam[:, 0])
    rare = np.any((kind == 0) | (kind == 2), axis=1)
    search = np.any(kind == 3, axis=1)
    exact = np.all((seg["kind"] & 4) != 0, axis=1)
    assert np.array_equal(st["mode"], rare * RARE + search * SEARCH + exact * EXACT)
    assert np.any(exact) == marked
    # every pool entry: one species, its record and its LDS slots, against the slices themselves
    n = int(tot.sum())
    sp, rec, xs, el = (np.full(n, -7, dtype=np.int32) for _ in range(4))
    L.tw_stage_entries(st.ctypes.data, p.n_win, ns, WP._ip(sp), WP._ip(rec), WP._ip(xs), WP._ip(el))
    first = np.cumsum(tot) - tot                         # a window's first entry in the concatenation
    win = np.repeat(np.arange(p.n_win), tot)
    i = np.arange(n) - first[win]                        # the entry's pool index
    owners = np.zeros(n, dtype=np.int64)
    x_base, el_base, lam_base = (np.zeros(s, dtype=np.int32) for s in ((p.n_win, ns), (p.n_win, ns), (p.n_win,)))
    L.tw_stage_bases(st.ctypes.data, p.n_win, ns, WP._ip(x_base), WP._ip(el_base), WP._ip(lam_base))
    for s in range(ns):
        own = staged[win, s] & (i >= pad[win, s]) & (i < pad[win, s] + m[win, s])
        owners += own
        k = (i - pad[win, s])[own]                       # the node's index in its slice
        assert np.all(sp[own] == s)
        assert np.array_equal(rec[own], seg["lo"][win, s][own] + k)
        assert np.array_equal(xs[own], x_base[win, s][own] + k), "the x slot is not the one the lookups read"
        assert np.array_equal(el[own], el_base[win, s][own] + 2 * k), "the {E, L} slot is not the one the lookups read"
        assert np.array_equal(xs[own], 2 * tot[win][own] + i[own] + s)
        assert not np.any(sp[~own] == s), "a species owns an entry outside its slice"
    assert np.all(owners == 1), "a pool entry without exactly one species"
    # the LDS: {E, L} pairs, then the x's with every slice's last upper node in the slot after its last entry, then
    # the wavelengths; nothing collides and everything ends inside the budget
    assert np.array_equal(el, 2 * i)
    assert np.all(xs >= 2 * tot[win]) and np.all(xs + 1 < lam_base[win])
    last = np.zeros(n, dtype=bool)
    for s in range(ns):
        last |= staged[win, s] & (i == pad[win, s] + m[win, s] - 1)
    slots = np.concatenate([win * 4096 + xs, (win * 4096 + xs + 1)[last]])
    assert len(np.unique(slots)) == len(slots), "two entries (or a last upper node) share an x slot"
    assert np.array_equal(lam_base, 3 * tot + ns)
    assert np.all(lam_base + st["nlam"] <= caps.lds) and caps.lds <= WP.K_TW_LDS
    assert np.all(st["nlam"] <= caps.lamcap)
    return st


# per input: what some plan of it must reach (indices into debug_counts: 1 staged, 2 global, 3 staged unguessed,
# 4 outside the table; "lam0" / "lam1": windows without / with staged wavelengths)
NEEDS = {("C3r", None): (1, 2, 3, 4, "lam0", "lam1"), ("C3fine", 2): (1, 2, 3, "lam0", "lam1"),
         ("C3fine", 8): (1, 2, 3, "lam0", "lam1"), ("C4fine", 2): (1, 2, 3, 4, "lam0", "lam1"),
         ("synthetic", None): (1, 2, 3, 4, "lam0", "lam1")}


@pytest.mark.parametrize("name,n", INPUTS, ids=["%s%s" % (a, b or "") for a, b in INPUTS])
def test_stage_records(name, n, libs, stage_lib):
    inp = WP.inputs(name, n)
    reached = set()
    for tup in CAPS:
        caps = WP.Caps(inp.n_rows, tup)
        p = WP.make_plan(libs, inp, caps)
        counts = WP.debug_counts(p)
        print(name, n, tup, counts)
        st = check_records(stage_lib, p, inp.ns, caps)
        reached |= {j for j in (1, 2, 3, 4) if counts[j] > 0}
        reached |= {"lam1"} if counts[5] > 0 else set()
        reached |= {"lam0"} if counts[5] < counts[0] else set()
        if len(tup) > 3 and tup[3] == "0":
            assert not np.any(st["nlam"] > 0)            # (LAMCAP 0: the global instance's windows)
        assert np.any(st["mode"] & RARE) == (counts[2] + counts[4] > 0)
        assert np.any(st["mode"] & SEARCH) == (counts[3] > 0)
    assert reached >= set(NEEDS[(name, n)]), (reached, NEEDS[(name, n)])


def test_stage_records_follow_exact_marks(libs, stage_lib):
    """k_tw_exact marks a window's guessed slices (kind |= 4) and sets the record's exact bit when every species'
    slice is a guessed one: the record derived from the marked slices says the same."""
    inp = WP.inputs("C3r")
    caps = WP.Caps(inp.n_rows)
    p = WP.make_plan(libs, inp, caps)
    kind = p.seg["kind"] & 3
    p.seg["kind"] = np.where(kind == 1, p.seg["kind"] | 4, p.seg["kind"])
    st = check_records(stage_lib, p, inp.ns, caps, marked=True)
    assert np.array_equal((st["mode"] & EXACT) != 0, np.all(kind == 1, axis=1))
    assert np.any(st["mode"] & EXACT) and not np.all(st["mode"] & EXACT)   # (C3r has searched slices too)
