"""The table-extent rule of the transmission-curve path (prometheus_amd/csrc/tc_phase.h), on the host.

k_tc_build folds a phase's 32-chord partials (maximum and minimum of the active finite columns, chord counts by class)
and derives the curve table's extent from the fold with tc_phase_extent.  The header is plain inline C++:
tests/helpers/tc_phase_host.cpp compiles it with g++.  Here numpy folds the partials (1, 2, 64, 65 and 75 of them, the
degenerate phases) and restates the rule independently:

    fin = no non-finite active column, N_max > 0, some active chord
    L1 = octaves(ybound N_max (1 + 2^-40))  (no bound: unlimited),  L2 = octaves(40 N_max / N_min)
    L2 <= L1 and L2 <= lg:  L = L2, opaque above the table;  else  L = min(L1, lg), truncated (flag 4) when L1 > lg
    octaves(q) = 0 below 2^-7, else floor(log2 q) + 8

Every quantity is a maximum, a minimum or an integer: the comparison is exact.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "prometheus_amd", "csrc")
PART = np.dtype([("nmax", "<f8"), ("nmin", "<f8"), ("nact", "<i4"), ("ntr", "<i4"), ("nbl", "<i4"), ("nnf", "<i4")])
INT_MAX = 0x7fffffff


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tcp") / "libtc_phase_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + CSRC, "-fPIC", "-shared",
                    os.path.join(REPO, "tests", "helpers", "tc_phase_host.cpp"), "-o", out], check=True)
    L = C.CDLL(out)
    L.tcp_octaves.argtypes = [C.c_double]
    L.tcp_octaves.restype = C.c_int32
    L.tcp_extent.argtypes = [C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_void_p]
    L.tcp_extent.restype = None
    assert L.tcp_sizeof_part() == PART.itemsize == 32
    return L


def octaves(q):
    if not q >= 2.0 ** -7:
        return 0
    if not q <= 1e300:
        return INT_MAX
    return int(np.frexp(q)[1]) - 1 + 8


def reference(p, ybound, lg):
    """The record of the partials p, in numpy."""
    nmax = max(0.0, float(p["nmax"].max()))
    nmin = min(np.inf, float(p["nmin"].min()))
    nact, ntr, nbl, nnf = (int(p[k].sum()) for k in ("nact", "ntr", "nbl", "nnf"))
    fin = nnf == 0 and nmax > 0.0 and nact > 0
    L = top = trunc = 0
    if fin:
        L1 = octaves(np.float64(ybound) * np.float64(nmax) * np.float64(1.0 + 2.0 ** -40)) if ybound > 0.0 else INT_MAX
        with np.errstate(divide="ignore", over="ignore"):
            L2 = octaves(np.float64(40.0) * (np.float64(nmax) / np.float64(nmin)))
        if L2 <= L1 and L2 <= lg:
            L, top = L2, 1
        else:
            L, trunc = min(L1, lg), (4 if L1 > lg else 0)
    return dict(nmax=nmax, nmin=nmin, nact=nact, ntr=ntr, nbl=nbl, nnf=nnf, fin=int(fin), L=L, top_opaque=top,
                trunc=trunc)


def check(lib, p, ybound, lg):
    """The header's extent of the partials p (folded here) against the numpy rule; returns the reference."""
    ref = reference(p, ybound, lg)
    out = np.zeros(4, dtype=np.int32)
    lib.tcp_extent(ref["nmax"], ref["nmin"], ref["nact"], ref["nnf"], ybound, lg, out.ctypes.data)
    got = dict(zip(("fin", "L", "top_opaque", "trunc"), (int(v) for v in out)))
    assert got == {k: ref[k] for k in got}, (got, ref)
    return ref


def partials(n, seed, lo=1e12, hi=1e17):
    """n partials of 32 chords: active / transparent / blocked counts, columns log-uniform in [lo, hi]."""
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=PART)
    p["nact"] = rng.integers(1, 33, n)
    p["ntr"] = rng.integers(0, 33 - p["nact"])
    p["nbl"] = 32 - p["nact"] - p["ntr"]
    a = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 2)))
    p["nmax"], p["nmin"] = a.max(axis=1), a.min(axis=1)
    return p


def test_octaves(lib):
    for q in [0.0, 2.0 ** -8, np.nextafter(2.0 ** -7, 0), 2.0 ** -7, 2.0 ** -6, 0.999, 1.0, 40.0, 1e300, 1.1e300, np.inf,
              np.nan, -1.0, 5e-324]:
        assert lib.tcp_octaves(q) == octaves(q), q
    rng = np.random.default_rng(0)
    for q in np.exp(rng.uniform(np.log(1e-4), np.log(1e30), 2000)):
        assert lib.tcp_octaves(q) == octaves(q), q


@pytest.mark.parametrize("n", [1, 2, 64, 65, 75])
def test_fold_counts(lib, n):
    """1, 2, 64, 65 and 75 (the workload's 2,400 chords) partials."""
    for seed in range(20):
        p = partials(n, 100 * n + seed)
        ref = check(lib, p, 1e-13 * (seed + 1), 24 + seed)
        assert ref["fin"] == 1 and ref["nact"] == p["nact"].sum()
    p = partials(n, 7)
    p["nmax"][-1], p["nmin"][-1] = 1e20, 1e3   # 40 * 1e17: 65 octaves, past the cap
    ref = check(lib, p, 0.0, 64)
    assert (ref["L"], ref["top_opaque"], ref["trunc"]) == (64, 0, 4)


def test_all_blocked(lib):
    p = np.zeros(75, dtype=PART)
    p["nbl"], p["nmin"] = 32, np.inf
    ref = check(lib, p, 1e-12, 24)
    assert (ref["fin"], ref["L"], ref["nbl"], ref["nmin"]) == (0, 0, 2400, np.inf)


def test_all_transparent(lib):
    p = np.zeros(75, dtype=PART)
    p["ntr"], p["nmin"] = 32, np.inf
    ref = check(lib, p, 1e-12, 24)
    assert (ref["fin"], ref["L"], ref["nact"], ref["ntr"]) == (0, 0, 0, 2400)


def test_nonfinite_column(lib):
    """One non-finite active column: it is counted, kept out of the maximum, and the phase has no table."""
    p = partials(75, 3)
    p["nnf"][40] = 1
    ref = check(lib, p, 1e-12, 24)
    assert (ref["fin"], ref["L"], ref["top_opaque"], ref["trunc"], ref["nnf"]) == (0, 0, 0, 0, 1)
    assert ref["nmax"] == p["nmax"].max() > 0


def test_equal_columns(lib):
    """nmin == nmax: the table ends where 40 N_max / N_min = 40 does, 13 octaves above 2^-7."""
    p = partials(3, 5)
    p["nmax"] = p["nmin"] = 3.7e15
    ref = check(lib, p, 0.0, 24)
    assert (ref["L"], ref["top_opaque"], ref["trunc"]) == (13, 1, 0)


def test_truncated_by_cap(lib):
    """Y's bound and the columns' spread both reach past the octave cap: L = lg, flag 4."""
    p = partials(8, 9, lo=1e5, hi=1e17)
    p["nmax"][0], p["nmin"][1] = 1e17, 1e5
    ref = check(lib, p, 1e-10, 12)   # q up to 1e7: 31 octaves; 40 N_max / N_min = 4e13: 53 octaves
    assert (ref["L"], ref["top_opaque"], ref["trunc"]) == (12, 0, 4)
    ref = check(lib, p, 1e-10, 40)   # the cap above Y's bound: not truncated
    assert (ref["L"], ref["top_opaque"], ref["trunc"]) == (31, 0, 0)
    ref = check(lib, p, 0.0, 40)     # no bound of Y: unlimited L1, the cap truncates
    assert (ref["L"], ref["top_opaque"], ref["trunc"]) == (40, 0, 4)


def test_ends_at_the_opaque_bound(lib):
    """40 N_max / N_min below Y's bound: the table ends there and everything above is opaque."""
    p = partials(8, 11, lo=1e15, hi=1e16)
    p["nmax"][0], p["nmin"][1] = 1e16, 1e15
    ref = check(lib, p, 1e-10, 40)   # 40 * 10 = 400: 16 octaves; Y's bound gives q up to 1e6
    assert (ref["L"], ref["top_opaque"], ref["trunc"]) == (16, 1, 0)
    ref = check(lib, p, 0.0, 16)     # exactly the cap
    assert (ref["L"], ref["top_opaque"], ref["trunc"]) == (16, 1, 0)
    ref = check(lib, p, 0.0, 15)     # one octave short of it: truncated
    assert (ref["L"], ref["top_opaque"], ref["trunc"]) == (15, 0, 4)
