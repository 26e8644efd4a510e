"""References of the median high-pass (include/prom_hip.h, "median high-pass on the device").

median_f64 restates the definition in numpy: a Python loop over the positions of each segment, the window clipped at
the segment's ends, its values that are not NaN sorted by the order-preserving integer key of their bits (-0 below +0,
the infinities ordinary values), the middle one or fl(fl(lo + hi) 0.5) of the two middle ones, then M - B or M / B.
It is vectorised over the rows only (a NaN gets the largest key, so it sorts behind every value, and each row picks
by its own count).  It is the bitwise reference of the device's filtered model and of observation.high_pass.

median_np takes np.nanmedian of each window instead: an independent statement that knows nothing of keys.  Its B
agrees with the definition's under == (it cannot tell -0 from +0, and a NaN equals nothing, so compare with
median_equal); so does M', except under division where B is a zero, whose sign then decides the sign of an infinity.
"""
import warnings

import numpy as np

TOP = np.uint64(1) << np.uint64(63)
NO_KEY = ~np.uint64(0)


def keys_of(x):
    """The integer keys of float64 x: the bits with the sign bit set for a value whose sign bit is clear, all bits
    flipped otherwise; NaN: the largest key."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = x.view(np.uint64)
    return np.where(np.isnan(x), NO_KEY, np.where((b & TOP) != 0, ~b, b | TOP))


def values_of(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.ascontiguousarray(np.where((k & TOP) != 0, k ^ TOP, ~k)).view(np.float64)


def running_median_f64(x, h):
    """B[..., n] of x[..., n] along the last axis, half width h; NaN where the window holds no value."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    rows = x.reshape(-1, n)
    keys = keys_of(rows)
    B = np.full(rows.shape, np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            w = np.sort(keys[:, max(0, i - h):min(n - 1, i + h) + 1], axis=1)
            c = (w != NO_KEY).sum(axis=1)
            lo = values_of(np.take_along_axis(w, np.maximum((c - 1) // 2, 0)[:, None], axis=1)[:, 0])
            hi = values_of(np.take_along_axis(w, np.minimum(c // 2, w.shape[1] - 1)[:, None], axis=1)[:, 0])
            even = (lo + hi) * 0.5
            B[:, i] = np.where(c == 0, np.nan, np.where(c % 2 == 1, lo, even))
    return B.reshape(x.shape)


def running_median_np(x, h):
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    rows = x.reshape(-1, n)
    B = np.full(rows.shape, np.nan)
    with warnings.catch_warnings(), np.errstate(invalid="ignore", over="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)            # (an all-NaN window)
        for i in range(n):
            B[:, i] = np.nanmedian(rows[:, max(0, i - h):min(n - 1, i + h) + 1], axis=1)
    return B.reshape(x.shape)


def _apply(M, seg_first, perm, h, mode, running):
    M = np.asarray(M, dtype=np.float64)
    seg_first, perm = np.asarray(seg_first), np.asarray(perm)
    out = np.full(M.shape, np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(len(seg_first) - 1):
            idx = perm[seg_first[s]:seg_first[s + 1]]
            x = M[..., idx]
            B = running(x, h)
            out[..., idx] = x - B if mode == 0 else x / B
    return out


def median_B(M, seg_first, perm, h):
    """B of the definition for every value of M[..., n_pix] (device order)."""
    M = np.asarray(M, dtype=np.float64)
    seg_first, perm = np.asarray(seg_first), np.asarray(perm)
    B = np.full(M.shape, np.nan)
    for s in range(len(seg_first) - 1):
        idx = perm[seg_first[s]:seg_first[s + 1]]
        B[..., idx] = running_median_f64(M[..., idx], h)
    return B


def median_f64(M, seg_first, perm, h, mode):
    """M' float64 of the model M[..., n_pix] (device order): the definition, bit for bit."""
    return _apply(M, seg_first, perm, h, mode, running_median_f64)


def median_np(M, seg_first, perm, h, mode):
    """The same through np.nanmedian of each window; equal to median_f64 under == (see median_equal), in mode 1
    where B is not a zero."""
    return _apply(M, seg_first, perm, h, mode, running_median_np)


def same_bits(a, b):
    """Bit for bit, any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def median_equal(a, b):
    """Equal under == with NaN where NaN is."""
    return bool(np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True))
