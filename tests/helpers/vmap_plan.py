"""Python side of the host harness of k_vmap's index arithmetic (tests/helpers/vmap_host.cpp): builds and binds it
and walks a map.  Shared by tests/test_vmap_cpu.py and tools/vmap_bench.py (the bytes the kernel's tile plan
requests)."""
import ctypes as C
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(REPO, "prometheus_amd", "csrc")
HOST = os.path.join(REPO, "tests", "helpers", "vmap_host.cpp")
COUNTERS = ["lanes", "points", "staged", "fallback", "empty", "staged_oor", "global_oor", "stage_load_oor", "part_oor",
            "visit_err", "stage_max", "workgroups", "batches", "stage_values", "fallback_values", "full_searches",
            "bracket_searches", "bracket_width"]
ERRORS = ("staged_oor", "global_oor", "stage_load_oor", "part_oor", "visit_err")
DEFAULT_CAP = 256 << 20


def small_constants(tile, stage, chunk, trials):
    return ("-DPROM_VM_TILE=%d" % tile, "-DPROM_VM_STAGE=%d" % stage, "-DPROM_VM_CHUNK=%d" % chunk,
            "-DPROM_VM_TRIALS=%d" % trials)


def compile_harness(out, extra=("-O2", "-fPIC", "-shared"), defines=()):
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *extra, *defines, "-I" + CSRC, HOST, "-o", str(out)],
                   check=True)


def bind(path):
    L = C.CDLL(str(path))
    dp = C.POINTER(C.c_double)
    L.vm_audit.argtypes = [dp, C.c_int32, dp, dp, C.c_double, dp, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                           C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    L.vm_audit.restype = None
    assert L.vm_audit_counters() == len(COUNTERS)
    return L


def constants(L):
    return {"tile": L.vm_const(0), "stage": L.vm_const(1), "chunk": L.vm_const(2), "trials": L.vm_const(3),
            "lanes": L.vm_const(4)}


def audit(L, wav, lam, sig, k, F, cap_bytes=DEFAULT_CAP, supports=True):
    """(counters, supports [n_orb][n_trial][n_pix][2] or None) of one map, walked on the host."""
    dp = C.POINTER(C.c_double)
    wav, lam, sig = (np.ascontiguousarray(a, dtype=np.float64) for a in (wav, lam, sig))
    F = np.ascontiguousarray(F, dtype=np.float64)
    n_orb, n_trial = F.shape
    cnt = np.zeros(len(COUNTERS), dtype=np.int64)
    supp = np.zeros((n_orb, n_trial, len(lam), 2), dtype=np.int32) if supports else None
    L.vm_audit(wav.ctypes.data_as(dp), len(wav), lam.ctypes.data_as(dp), sig.ctypes.data_as(dp), float(k),
               F.ctypes.data_as(dp), len(lam), n_orb, n_trial, int(cap_bytes), cnt.ctypes.data_as(C.POINTER(C.c_int64)),
               supp.ctypes.data_as(C.POINTER(C.c_int32)) if supports else None)
    return dict(zip(COUNTERS, (int(v) for v in cnt))), supp
