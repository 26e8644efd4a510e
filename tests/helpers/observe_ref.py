"""Reference of the device observation (include/prom_hip.h, "observation of a spectrum on the device") in
numpy.longdouble (80-bit on x86-64), and the synthetic designs the tests share.

The reference applies the definition's float64 roundings first -- q = fl((hi - lo) / 2), L = fl(lam f), S = fl(sig f),
c = fl(k S) and the support test |fl(wav - L)| <= c -- and evaluates everything after them (z, exp, the products and
the sums) in longdouble.  It is written from the definition alone.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def q_weights(wav, edge_lo=np.nan, edge_hi=np.nan):
    """float64 trapezoid weights of the whole grid; the edges are the grid points just outside wav (NaN: none)."""
    wav = np.asarray(wav, dtype=np.float64)
    lo = np.concatenate([[wav[0] if np.isnan(edge_lo) else edge_lo], wav[:-1]])
    hi = np.concatenate([wav[1:], [wav[-1] if np.isnan(edge_hi) else edge_hi]])
    return (hi - lo) / 2.0


def support(wav, L, c):
    """Indices [a, b) of the support of a pixel at L with half-width c: membership by the float64 test only."""
    a = max(int(np.searchsorted(wav, L - c, "left")) - 2, 0)
    b = min(int(np.searchsorted(wav, L + c, "right")) + 2, len(wav))
    m = np.abs(wav[a:b] - L) <= c
    idx = np.nonzero(m)[0]
    if len(idx) == 0:
        return 0, 0
    assert np.all(m[idx[0]:idx[-1] + 1])
    return a + int(idx[0]), a + int(idx[-1]) + 1


def observe(wav, R, lam, sig, k, f=None, edge_lo=np.nan, edge_hi=np.nan):
    """(num, den, count): longdouble partial sums [n_orb][n_pix] and the support counts (int64)."""
    wav = np.asarray(wav, dtype=np.float64)
    R = np.atleast_2d(np.asarray(R, dtype=np.float64))
    lam, sig = np.asarray(lam, dtype=np.float64), np.asarray(sig, dtype=np.float64)
    n_orb, n_pix = R.shape[0], len(lam)
    q = q_weights(wav, edge_lo, edge_hi).astype(LD)
    Rl = R.astype(LD)
    wl = wav.astype(LD)
    num = np.zeros((n_orb, n_pix), dtype=LD)
    den = np.zeros((n_orb, n_pix), dtype=LD)
    cnt = np.zeros((n_orb, n_pix), dtype=np.int64)
    k = np.float64(k)
    groups = [(np.float64(1.0), slice(0, n_orb))] if f is None else [(np.float64(v), slice(o, o + 1))
                                                                       for o, v in enumerate(np.asarray(f, np.float64))]
    for fo, rows in groups:
        for p in range(n_pix):
            L = lam[p] * fo
            S = sig[p] * fo
            c = k * S
            a, b = support(wav, L, c)
            if b == a:
                continue
            z = (wl[a:b] - LD(L)) / LD(S)
            gq = np.exp(LD(-0.5) * z * z) * q[a:b]
            den[rows, p] = gq.sum()
            num[rows, p] = (Rl[rows, a:b] * gq[None, :]).sum(axis=1)
            cnt[rows, p] = b - a
    return num, den, cnt


def model(num, den):
    """M = num / den in the dtype given; NaN where den == 0."""
    num, den = np.asarray(num), np.asarray(den)
    out = np.full(num.shape, np.nan, dtype=num.dtype)
    ok = den != 0
    with np.errstate(invalid="ignore"):
        out[ok] = num[ok] / den[ok]
    return out


def chi2(M, den, data, ivar):
    """Longdouble chi-square per phase of the model M (any dtype) and the used counts."""
    M, den, data, ivar = (np.asarray(a) for a in (M, den, data, ivar))
    with np.errstate(invalid="ignore"):
        used = np.isfinite(ivar) & (ivar > 0) & np.isfinite(data) & (den > 0)
    out = np.zeros(M.shape[0], dtype=LD)
    for o in range(M.shape[0]):
        u = used[o]
        r = M[o, u].astype(LD) - data[o, u].astype(LD)
        out[o] = (ivar[o, u].astype(LD) * r * r).sum()
    return out, used.sum(axis=1).astype(np.int64)


def m_tolerance(k, n_max):
    """Relative bound of |M_dev - M_ref| (the issue's derivation): the terms are non-negative, so a sum of n terms
    in any order errs by at most (n - 1) u; z is exact up to two roundings and the exponent is at most k^2 / 2, so
    with a 1-ulp exp a weight is off by at most about (1.5 k^2 + 2) u; a ratio of positively weighted sums moves by
    at most twice the weights' relative error.  (3 k^2 + 2 n_max + 16) u."""
    return (3.0 * k * k + 2.0 * n_max + 16.0) * U


# ---- designs -------------------------------------------------------------------------------------------------
def grid_nonuniform(n_wav, seed=0):
    """Ascending grid of n_wav points near 5890 A: fine (0.001 A) and coarse (0.01 A) stretches alternate every 37
    points, so supports hold 10x spacing jumps, with a duplicated point every 29th."""
    steps = np.where((np.arange(n_wav) // 37) % 2 == 0, 1e-11, 1e-10)
    steps[::29] = 0.0
    rng = np.random.default_rng(seed)
    steps = steps * (1.0 + 0.2 * rng.random(n_wav))
    w = 5890e-8 + np.cumsum(steps)
    w[0] = 5890e-8
    return w


def grid_coarse_fine(n_fine=3000, n_coarse=200):
    """A C3-like grid: 0.2 A coarse, a 0.001 A core in the middle."""
    lo = 5880e-8 + 2e-9 * np.arange(n_coarse)
    mid = lo[-1] + 2e-9 + 1e-11 * np.arange(n_fine)
    hi = mid[-1] + 2e-9 * (1 + np.arange(n_coarse))
    return np.concatenate([lo, mid, hi])


def grid_dyadic(n):
    """wav_j = 2^-14 (1 + j 2^-16): every node, difference and multiple of the spacing is exact in float64."""
    return 2.0 ** -14 * (1.0 + np.arange(n) * 2.0 ** -16)


DYADIC_STEP = 2.0 ** -30


def spectrum(wav, n_orb, seed=1):
    """R[n_orb][n_wav] in (0.5, 1]: a smooth continuum with a line per phase and per-point noise."""
    rng = np.random.default_rng(seed)
    x = (wav - wav[0]) / max(wav[-1] - wav[0], 1e-30)
    R = np.empty((n_orb, len(wav)))
    for o in range(n_orb):
        c = 0.3 + 0.4 * (o + 1) / (n_orb + 1)
        R[o] = 1.0 - 0.05 * x - 0.3 * np.exp(-0.5 * ((x - c) / 0.02) ** 2) - 0.05 * rng.random(len(wav))
    return R


def pixels_over(wav, n_pix, seed=2, dup=True, outside=True):
    """Non-decreasing pixel centres over the grid (a few beyond both ends when ``outside``), with duplicates."""
    rng = np.random.default_rng(seed)
    span = wav[-1] - wav[0] if len(wav) > 1 else 1e-9
    lo, hi = (wav[0] - 0.05 * span - 3e-10, wav[-1] + 0.05 * span + 3e-10) if outside else (wav[0], wav[-1])
    lam = np.sort(lo + (hi - lo) * rng.random(n_pix))
    if dup and n_pix >= 4:
        lam[n_pix // 2] = lam[n_pix // 2 - 1]
    return lam
