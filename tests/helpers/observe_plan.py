"""Python side of the host harness of k_observe's index arithmetic (tests/helpers/observe_host.cpp): builds and
binds it and walks a launch.  Shared by tests/test_observe_cpu.py and tools/observe_bench.py (the bytes the kernel's
tile plan requests)."""
import ctypes as C
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(REPO, "prometheus_amd", "csrc")
HOST = os.path.join(REPO, "tests", "helpers", "observe_host.cpp")
COUNTERS = ["lanes", "points", "staged_pix", "fallback_pix", "empty_pix", "staged_oor", "global_oor", "stage_load_oor",
            "out_oor", "stage_max", "workgroups", "stage_points", "fallback_points", "stage_values", "fallback_values"]


def compile_harness(out, extra=("-O2", "-fPIC", "-shared")):
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *extra, "-I" + CSRC, HOST, "-o", str(out)], check=True)


def bind(path):
    L = C.CDLL(str(path))
    dp = C.POINTER(C.c_double)
    L.obs_audit.argtypes = [dp, C.c_int32, dp, dp, C.c_double, dp, C.c_int32, C.c_int32, C.POINTER(C.c_int64),
                            C.POINTER(C.c_int32)]
    L.obs_audit.restype = None
    assert L.obs_audit_counters() == len(COUNTERS)
    return L


def audit(L, wav, lam, sig, k, f, n_orb, supports=True):
    """(counters, supports [groups][n_pix][2] or None) of one launch of k_observe, walked on the host."""
    dp = C.POINTER(C.c_double)
    wav, lam, sig = (np.ascontiguousarray(a, dtype=np.float64) for a in (wav, lam, sig))
    fa = None if f is None else np.ascontiguousarray(f, dtype=np.float64)
    cnt = np.zeros(len(COUNTERS), dtype=np.int64)
    groups = n_orb if f is not None else (n_orb + L.obs_const(2) - 1) // L.obs_const(2)
    supp = np.zeros((groups, len(lam), 2), dtype=np.int32) if supports else None
    L.obs_audit(wav.ctypes.data_as(dp), len(wav), lam.ctypes.data_as(dp), sig.ctypes.data_as(dp), k,
                fa.ctypes.data_as(dp) if fa is not None else None, len(lam), n_orb,
                cnt.ctypes.data_as(C.POINTER(C.c_int64)),
                supp.ctypes.data_as(C.POINTER(C.c_int32)) if supports else None)
    return dict(zip(COUNTERS, (int(v) for v in cnt))), supp
