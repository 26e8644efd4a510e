"""Python side of the host harness of the target-window planner (tests/helpers/window_host.cpp): builds and binds
the harness, makes the planner's inputs from the oracle (no device), mirrors prom_transit_set's caps and returns raw
plans.  Shared by tests/test_window_plan_cpu.py and tests/test_gpu_windows.py."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np

from oracle import prom_oracle as O
from prometheus_amd import configs

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(REPO, "prometheus_amd", "csrc")
SEG = np.dtype([("lo", "<i4"), ("m", "<i4"), ("kind", "<i4"), ("pad", "<i4"), ("xs", "<f8"), ("inv", "<f8")])
K_TW_LDS, K_TW_LAMCAP = 2816, 1024   # prom_internal.h kTwLds, kTwLamCap (checked against the header below)
COUNTERS = ["lanes", "global_oor", "staged_oor", "padding", "guess_oor", "step_oor", "bracket_bad", "win_first",
            "win_second", "pair_empty_low", "pair_empty_high", "pair_empty_mid", "pair_empty_win", "win_global_oor",
            "win_staged_oor"]
# the cap tuples of tests/test_gpu_windows.py::test_windows_small_caps_bitwise (rowcap, pmax, lds[, lamcap, lamfit,
# exact, align, rp])
CAP_TUPLES = [("8", "64", "2560"), ("4", "32", "96"), ("256", "8192", "16"), ("256", "8192", "2560", "0"),
              ("256", "8192", "2560", "1024", "1"), ("256", "8192", "2560", "0", "0", "0"),
              ("256", "8192", "2560", "1024", "0", "1", "0", "2"), ("100", "8192", "2560", "0", "0", "1", "64", "2")]


def rocm_include():
    """The ROCm include directory next to the hipcc the package's build finds."""
    from prometheus_amd import build as b
    cc = b.hipcc()
    for c in (cc, os.path.realpath(cc)):
        inc = os.path.join(os.path.dirname(os.path.dirname(c)), "include")
        if os.path.exists(os.path.join(inc, "hip", "hip_runtime.h")):
            return inc
    raise RuntimeError("no hip/hip_runtime.h next to " + cc)


def compile_harness(out, extra=()):
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + rocm_include(),
           "-I" + CSRC, *extra, "-x", "c++", os.path.join(CSRC, "prom_window.hip"),
           os.path.join(REPO, "tests", "helpers", "window_host.cpp"), "-pthread", "-o", str(out)]
    subprocess.run(cmd, check=True)


def bind(path):
    L = C.CDLL(str(path))
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    L.tw_plan.restype = C.c_void_p
    L.tw_plan.argtypes = [dp, C.c_int64, dp, C.c_int32, C.c_int32, C.POINTER(dp), lp, C.c_int32, C.c_int32, C.c_int32,
                          C.c_int64, ip]
    L.tw_plan_copy.argtypes = [C.c_void_p, C.c_void_p, ip, ip]
    L.tw_plan_copy.restype = None
    L.tw_plan_free.argtypes = [C.c_void_p]
    L.tw_plan_free.restype = None
    L.tw_guess_n.argtypes = [C.c_int64, dp, dp, dp, ip, ip]
    L.tw_guess_n.restype = None
    for f, n in (("tw_waves_per_unit", 1), ("tw_pair_rows", 2), ("tw_row_absent", 3), ("tw_chunks", 2),
                 ("tw_chunk_read", 3), ("tw_lam_staged", 5), ("tw_lam_global", 4)):
        getattr(L, f).argtypes = [C.c_int32] * n
        getattr(L, f).restype = C.c_int32
    L.tw_audit.argtypes = [dp, C.c_int64, dp, C.c_int32, C.c_int32, C.POINTER(dp), lp, C.c_void_p, ip, ip, C.c_int32,
                           C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, lp]
    L.tw_audit.restype = None
    assert L.tw_sizeof_seg() == SEG.itemsize and L.tw_audit_counters() == len(COUNTERS)
    return L


class Libs:
    """PROM_TW_ALIGN is read once per process and library: one copy of the harness per value (None: unset), built
    in directory d."""

    def __init__(self, d):
        self.d = str(d)
        self.base = os.path.join(self.d, "libwindow_host.so")
        compile_harness(self.base, ["-fPIC", "-shared"])
        self.loaded = {}

    def __call__(self, align=None):
        if align not in self.loaded:
            path = os.path.join(self.d, "libwindow_host_align_%s.so" % align)
            shutil.copy(self.base, path)
            self.loaded[align] = bind(path)
        return self.loaded[align]


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


class Inputs:
    def __init__(self, wav, shift, X):
        self.wav = np.ascontiguousarray(wav, dtype=np.float64)
        self.shift = np.ascontiguousarray(shift, dtype=np.float64)
        self.X = [np.ascontiguousarray(x, dtype=np.float64) for x in X]
        self.n_wav, self.n_rows, self.ns = len(self.wav), len(self.shift), len(self.X)
        self.Xp = (C.POINTER(C.c_double) * self.ns)(*[_dp(x) for x in self.X])
        self.nx = np.array([len(x) for x in self.X], dtype=np.int64)
        self.nxp = self.nx.ctypes.data_as(C.POINTER(C.c_int64))

    @functools.cached_property
    def t(self):
        """Every target fl(shift_o lambda_w), [n_rows, n_wav]."""
        return self.shift[:, None] * self.wav[None, :]

    @functools.cached_property
    def k(self):
        """numpy's bracket of every target in every table, [ns][n_rows, n_wav]."""
        return [np.clip(np.searchsorted(x, self.t, "right") - 1, 0, len(x) - 2).astype(np.int32) for x in self.X]


def oracle_inputs(cfg):
    """What prom_transit_set hands the planner, from the oracle: the grid, the atomic tables' node x's in constituent
    order and the planet's per-phase Doppler factors (the factors of optical_depth: doppler_shift(-v))."""
    scen, doppler, grids = O.from_setup(cfg)
    assert doppler
    wav = O.simulation_wavelengths(grids, O.atomic_species(scen))
    tabs = O.build_tables(scen, grids)
    v = O.planet_los_velocity(scen[0].planet, O.orbphase_axis(grids))
    return Inputs(wav, O.doppler_shift(-v), [tabs[key][0] for key in sorted(tabs)])


def c4fine_cfg(n):
    return configs.reduced(configs.get("C4"), orbphase_steps=n, res_low=1e-11, res_high=5e-12, lower_w=5888e-8,
                           upper_w=5898e-8)


def c3fine_cfg(n):
    return configs.reduced(configs.get("C3"), orbphase_steps=n, res_low=1e-11, res_high=5e-12, lower_w=3930e-8,
                           upper_w=3940e-8)


@functools.lru_cache(maxsize=None)
def inputs(name, n=None):
    if name == "C3r":
        return oracle_inputs(configs.reduced(configs.get("C3")))
    if name == "C4fine":
        return oracle_inputs(c4fine_cfg(n))
    if name == "C3fine":
        return oracle_inputs(c3fine_cfg(n))
    if name == "synthetic":
        # 4 rows, 9,001 wavelengths at 1e-11 (9,001 % 64 = 41).  Table 0 is narrower than the targets (numpy's end
        # rules below and above it: kind 0); table 1 covers them, its node spacing changing 20-fold at two nodes (the
        # candidate interval that holds such a node has no linear guess within one node: kind 3)
        wav = 5000e-8 + 1e-11 * np.arange(9001)
        shift = np.array([1.0 - 8e-5, 1.0 + 3e-5, 1.0 - 2e-5, 1.0 + 8e-5])
        x0 = np.arange(5002e-8, 5007e-8, 1e-12)
        x1 = np.concatenate([np.arange(4990e-8, 5003.5e-8, 5e-12), np.arange(5003.5e-8, 5005.5e-8, 2.5e-13),
                             np.arange(5005.5e-8, 5020e-8, 5e-12)])
        return Inputs(wav, shift, [x0, np.unique(x1)])
    raise KeyError(name)


class Caps:
    def __init__(self, n_orb, tup=(), **knobs):
        """prom_transit_set's caps (prom_api_transit.hip target_windows): the defaults from n_orb, or the PROM_TW_* knobs of tup
        (test_windows_small_caps_bitwise's order) or by name (ROWCAP="100")."""
        e = dict(zip(("ROWCAP", "PMAX", "LDS", "LAMCAP", "LAMFIT", "EXACT", "ALIGN", "RP"), tup), **knobs)
        self.rowcap = max(1, int(e["ROWCAP"])) if "ROWCAP" in e else max(256, min(768, (4096 // max(1, n_orb)) // 64 * 64))
        self.pmax = max(1, int(e["PMAX"])) if "PMAX" in e else max(8192, self.rowcap * n_orb)
        self.lamcap = max(0, min(K_TW_LAMCAP, int(e["LAMCAP"]))) if "LAMCAP" in e else K_TW_LAMCAP
        self.lds = max(16, min(K_TW_LDS, int(e["LDS"]))) if "LDS" in e else K_TW_LDS
        self.lamfit = int(e.get("LAMFIT", "0")) != 0
        self.align = e.get("ALIGN")
        self.tup = tup

    def __repr__(self):
        return "Caps(rowcap %d, pmax %d, lds %d, lamcap %d, lamfit %d, align %s)" % (
            self.rowcap, self.pmax, self.lds, self.lamcap, self.lamfit, self.align)


class Plan:
    pass


def make_plan(libs, inp, caps):
    L = libs(caps.align)
    old = {k: os.environ.pop(k, None) for k in ("PROM_TW_ALIGN", "PROM_TW_LAMFIT")}
    try:
        if caps.align is not None:
            os.environ["PROM_TW_ALIGN"] = caps.align   # (read by this copy's first call only)
        if caps.lamfit:
            os.environ["PROM_TW_LAMFIT"] = "1"
        nw = C.c_int32(0)
        h = L.tw_plan(_dp(inp.wav), inp.n_wav, _dp(inp.shift), inp.n_rows, inp.ns, inp.Xp, inp.nxp, caps.lds,
                      caps.lamcap, caps.rowcap, caps.pmax, C.byref(nw))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert h, "the planner declined the inputs"
    p = Plan()
    p.L, p.n_win = L, nw.value
    p.seg = np.zeros((p.n_win, inp.ns), dtype=SEG)
    p.row = np.zeros((p.n_win + 1, inp.n_rows), dtype=np.int32)
    p.lam = np.zeros((p.n_win, 2), dtype=np.int32)
    L.tw_plan_copy(h, p.seg.ctypes.data, _ip(p.row), _ip(p.lam))
    L.tw_plan_free(h)
    p.kind = p.seg["kind"] & 3
    return p


def debug_counts(p):
    """The figures of prom_transit_set's debug line: windows, slices staged / global / staged unguessed / outside
    the table, windows with staged wavelengths."""
    return (p.n_win, int(np.sum(p.kind == 1)), int(np.sum(p.kind == 2)), int(np.sum(p.kind == 3)),
            int(np.sum(p.kind == 0)), int(np.sum(p.lam[:, 1] > p.lam[:, 0])))


def dump_inputs(path, inp, caps):
    """The stand-alone harness' input file (window_host.cpp built with -DWINDOW_HOST_MAIN)."""
    with open(path, "wb") as f:
        np.array([inp.n_wav, inp.n_rows, inp.ns, caps.lds, caps.lamcap, caps.rowcap, caps.pmax], dtype=np.int64).tofile(f)
        inp.nx.tofile(f)
        inp.wav.tofile(f)
        inp.shift.tofile(f)
        for x in inp.X:
            x.tofile(f)


if __name__ == "__main__":
    # PYTHONPATH=. python tests/helpers/window_plan.py DIR [compiler flags, e.g. -fsanitize=address,undefined]:
    # build the stand-alone harness DIR/window_host and write its inputs (reduced C3, C4fine at 2 and 8 phases)
    import sys
    d = sys.argv[1]
    compile_harness(os.path.join(d, "window_host"), ["-g", "-DWINDOW_HOST_MAIN"] + sys.argv[2:])
    dump_inputs(os.path.join(d, "c3r.bin"), inputs("C3r"), Caps(16))
    dump_inputs(os.path.join(d, "c4fine2.bin"), inputs("C4fine", 2), Caps(2))
    dump_inputs(os.path.join(d, "c4fine8_lam0.bin"), inputs("C4fine", 8), Caps(8, ("256", "8192", "2816", "0")))
