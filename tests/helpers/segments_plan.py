"""Python side of the host harness of prom_transit_set's pure planners (tests/helpers/segments_host.cpp): builds and
binds the harness and returns the raw sigma segments.  Used by tests/test_segments_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from helpers.window_plan import CSRC, REPO, SEG, _dp, _ip, rocm_include


def compile_harness(out, extra=()):
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + rocm_include(),
           "-I" + CSRC, *extra, "-x", "c++", os.path.join(CSRC, "prom_segments.hip"),
           os.path.join(REPO, "tests", "helpers", "segments_host.cpp"), "-pthread", "-o", str(out)]
    subprocess.run(cmd, check=True)


def bind(path):
    L = C.CDLL(str(path))
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    L.sg_build.restype = C.c_void_p
    L.sg_build.argtypes = [dp, C.c_int64, C.c_int32, C.POINTER(dp), lp, dp, C.c_int64, C.c_int32, C.c_int32, lp]
    L.sg_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, ip, ip, ip]
    L.sg_copy.restype = None
    L.sg_free.argtypes = [C.c_void_p]
    L.sg_free.restype = None
    L.sg_guess_n.argtypes = [C.c_int64, dp, dp, dp, ip, ip]
    L.sg_guess_n.restype = None
    L.sg_pair_mirrors.argtypes = [dp, dp, C.c_int64, ip]
    L.sg_pair_mirrors.restype = C.c_int64
    L.sg_star_slices.argtypes = [dp, C.c_int64, dp, C.c_int64, C.c_double, C.c_double, ip]
    L.sg_star_slices.restype = None
    L.sg_factor_range.argtypes = [dp, C.c_int64, dp, dp]
    L.sg_poly_degree.argtypes = [dp, C.c_int32, C.c_int32]
    L.sg_density_bounded.argtypes = [C.c_int32, dp]
    assert L.sg_sizeof_seg() == SEG.itemsize
    return L


class Problem:
    """The builder's inputs: the grid, per atomic slot its table's nodes and its n_orb Doppler factors."""

    def __init__(self, wav, X, shift):
        self.wav = np.ascontiguousarray(wav, dtype=np.float64)
        self.X = [np.ascontiguousarray(x, dtype=np.float64) for x in X]
        self.shift = np.ascontiguousarray(shift, dtype=np.float64).reshape(len(self.X), -1)
        self.n_wav, self.na, self.n_orb = len(self.wav), len(self.X), self.shift.shape[1]
        self.Xp = (C.POINTER(C.c_double) * self.na)(*[_dp(x) for x in self.X])
        self.nx = np.array([len(x) for x in self.X], dtype=np.int64)

    def dump(self, path):
        """The stand-alone harness' input file (segments_host.cpp built with -DSEGMENTS_HOST_MAIN)."""
        with open(path, "wb") as f:
            np.array([self.n_wav, self.na, self.n_orb], dtype=np.int64).tofile(f)
            self.nx.tofile(f)
            self.wav.tofile(f)
            self.shift.tofile(f)
            for x in self.X:
                x.tofile(f)


class Segments:
    pass


def build_segments(L, pr, use_dir=True, no_guess=False):
    """build_sigma_segments' outputs as arrays, or None where it builds none."""
    sz = np.zeros(7, dtype=np.int64)
    h = L.sg_build(_dp(pr.wav), pr.n_wav, pr.na, pr.Xp, pr.nx.ctypes.data_as(C.POINTER(C.c_int64)), _dp(pr.shift),
                   pr.n_orb, int(use_dir), int(no_guess), sz.ctypes.data_as(C.POINTER(C.c_int64)))
    if not h:
        return None
    g = Segments()
    g.seg = np.zeros(sz[0], dtype=SEG)
    g.seg4 = np.zeros(sz[1], dtype=SEG)
    g.sdir, g.fb, g.fb_tc = (np.zeros(n, dtype=np.int32) for n in sz[2:5])
    L.sg_copy(h, g.seg.ctypes.data, g.seg4.ctypes.data, _ip(g.sdir), _ip(g.fb), _ip(g.fb_tc))
    L.sg_free(h)
    g.n_dir, g.noguess = int(sz[5]), int(sz[6])
    g.seg = g.seg.reshape(-1, pr.na)
    return g


def seg_guess(L, t, xs, inv, m):
    """The device's seg_guess for targets t against one entry (scalars) or one entry each (arrays)."""
    t = np.ascontiguousarray(t, dtype=np.float64)
    xs, inv = (np.ascontiguousarray(np.broadcast_to(v, t.shape), dtype=np.float64) for v in (xs, inv))
    m = np.ascontiguousarray(np.broadcast_to(m, t.shape), dtype=np.int32)
    out = np.empty(t.shape, dtype=np.int32)
    L.sg_guess_n(t.size, _dp(t), _dp(xs), _dp(inv), _ip(m), _ip(out))
    return out


if __name__ == "__main__":
    # PYTHONPATH=.:tests python tests/helpers/segments_plan.py DIR [compiler flags, e.g. -fsanitize=address,undefined]:
    # build the stand-alone harness DIR/segments_host and write the test module's synthetic problems as its inputs
    import sys
    from test_segments_cpu import synthetic, wide
    d = sys.argv[1]
    compile_harness(os.path.join(d, "segments_host"), ["-g", "-DSEGMENTS_HOST_MAIN"] + sys.argv[2:])
    synthetic(2).dump(os.path.join(d, "two_species.bin"))
    synthetic(1).dump(os.path.join(d, "one_species.bin"))
    wide().dump(os.path.join(d, "wide.bin"))
