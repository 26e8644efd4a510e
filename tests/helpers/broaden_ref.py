"""References of the broadened spectra (include/prom_hip.h, "broadened spectra on the device") and the designs the
tests share.

broaden_f64 is a numpy loop of the definition, rounding for rounding: every element-wise numpy operation rounds once,
and the sums run in ascending w' through a cumulative sum that starts from +0.  broaden_ld decides membership by the
float64 rule and evaluates everything after it (t, the kernel value, the weights and the sums) in numpy.longdouble.
bound is derived from the definition, not from any kernel.  All written from the definition alone.
"""
import numpy as np

from helpers import observe_ref as oref

LD = np.longdouble
U = 2.0 ** -53
C_LIGHT = 2.998e10   # cm/s (prometheus_amd.constants.c)


def _t64(wav, w, b0, s):
    """t of every candidate for output w, float64, one rounding per operation."""
    r = np.float64(1.0) / wav[w]
    d = wav - wav[w]
    u = d * r
    return (u - np.float64(b0)) * np.float64(s)


def support(wav, w, n_k, b0, s):
    """(a, b, t): the support [a, b) of output w by the float64 membership test, and t of its members."""
    t = _t64(wav, w, b0, s)
    m = (t >= 0.0) & (t <= np.float64(n_k - 1))
    idx = np.nonzero(m)[0]
    if len(idx) == 0:
        return 0, 0, t[:0]
    a, b = int(idx[0]), int(idx[-1]) + 1
    assert m[a:b].all(), "the support is one contiguous range"
    return a, b, t[a:b]


def broaden_f64(wav, R, K, b0, s):
    """R_b[n_orb][n_wav] of the definition, bit for bit."""
    wav = np.ascontiguousarray(wav, dtype=np.float64)
    R = np.atleast_2d(np.asarray(R, dtype=np.float64))
    K = np.asarray(K, dtype=np.float64)
    n_k = len(K)
    D = K[1:] - K[:-1]
    q = oref.q_weights(wav)
    out = np.full(R.shape, np.nan)
    zero = np.zeros((R.shape[0], 1))
    for w in range(len(wav)):
        a, b, t = support(wav, w, n_k, b0, s)
        if b == a:
            continue
        i = np.minimum(np.floor(t).astype(np.int64), n_k - 2)
        kern = K[i] + (t - i) * D[i]
        g = kern * q[a:b]
        den = np.cumsum(np.concatenate([[0.0], g]))[-1]
        with np.errstate(invalid="ignore", over="ignore"):
            num = np.cumsum(np.concatenate([zero, g[None, :] * R[:, a:b]], axis=1), axis=1)[:, -1]
            if den != 0.0:
                out[:, w] = num / den
    return out


def broaden_ld(wav, R, K, b0, s):
    """(R_b, n_support, rmax, gsum, qsum): longdouble R_b with the float64 membership, the supports' sizes, and what
    bound needs per output: max|R| over the support [n_orb][n_wav], the sum of the weights g and the sum of q."""
    wav = np.ascontiguousarray(wav, dtype=np.float64)
    R = np.atleast_2d(np.asarray(R, dtype=np.float64))
    K = np.asarray(K, dtype=np.float64)
    n_k = len(K)
    Kl, wl, Rl = K.astype(LD), wav.astype(LD), R.astype(LD)
    ql = oref.q_weights(wav).astype(LD)
    out = np.full(R.shape, np.nan, dtype=LD)
    cnt = np.zeros(len(wav), dtype=np.int64)
    rmax = np.zeros(R.shape)
    gsum = np.zeros(len(wav), dtype=LD)
    qsum = np.zeros(len(wav), dtype=LD)
    for w in range(len(wav)):
        a, b, _ = support(wav, w, n_k, b0, s)
        cnt[w] = b - a
        if b == a:
            continue
        t = ((wl[a:b] - wl[w]) / wl[w] - LD(b0)) * LD(s)
        i = np.clip(np.floor(t).astype(np.int64), 0, n_k - 2)
        kern = Kl[i] + (t - i.astype(LD)) * (Kl[i + 1] - Kl[i])
        g = kern * ql[a:b]
        den = g.sum()
        gsum[w], qsum[w] = den, ql[a:b].sum()
        with np.errstate(invalid="ignore"):
            rmax[:, w] = np.abs(R[:, a:b]).max(axis=1)
            if den != 0:
                out[:, w] = (g[None, :] * Rl[:, a:b]).sum(axis=1) / den
    return out, cnt, rmax, gsum, qsum


def bound(K, b0, s, cnt, rmax, gsum, qsum):
    """Absolute bound of |R_b(float64 definition) - R_b(longdouble)| per output [n_orb][n_wav], from the definition:

    t: d, r and their product carry one rounding each (3u relative on |u| <= |t| / s + |b0|), the difference and the
    product with s one each, so |dt| <= u (3 (|t| + |b0| s) + 2 |t|) <= 6 (n_k + |b0| s) u.
    kern = K[i] + a D[i]: |dkern| <= max|D| dt + 3u max K (the roundings of D, the product and the sum, each at most
    u max K); K is continuous across its nodes, so a changed i costs no more, and the reference extends the end
    segments linearly, which dt covers.  g = kern q adds u kern q.  So sum_i |dg_i| <= E = (|dkern| + u max K) sum q.
    The terms of den are non-negative: n of them summed one by one err by at most n u relative; num's terms carry one
    more rounding each, (n + 1) u relative to sum g |R|.  With G = sum g and |R| <= Rmax on the support,
    |d(num / den)| <= Rmax (2 E / G + (2 n + 2) u) + u Rmax; two more u absorb the second-order terms.
    Infinite where G = 0 (both sides are NaN there) or R is not finite on the support."""
    K = np.asarray(K, dtype=np.float64)
    dt = 6.0 * (len(K) + abs(b0) * s) * U
    dkern = np.abs(np.diff(K)).max() * dt + 3.0 * U * K.max()
    E = (dkern + U * K.max()) * qsum.astype(np.float64)
    G = gsum.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(G > 0, 2.0 * E / G, np.inf) + (2.0 * cnt + 5.0) * U
    return rmax * rel[None, :]


# ---- designs -------------------------------------------------------------------------------------------------
def kernel(n_k, v_lo, v_hi, shape="ring", seed=0):
    """(K, b0, s) of a kernel whose n_k nodes span the velocities [v_lo, v_hi] cm/s (K over beta, so reversed)."""
    x = np.linspace(-1.0, 1.0, n_k)
    if shape == "ring":                       # the double-horned profile, finite at the ends
        P = 1.0 / np.sqrt(1.0 + 0.02 - x * x)
    elif shape == "gauss":
        P = np.exp(-0.5 * (2.5 * x) ** 2)
    elif shape == "random":                   # with zeros: weight-zero members
        P = np.random.default_rng(seed).random(n_k)
        P[::3] = 0.0
        P[-1] = 0.5
    else:
        raise ValueError(shape)
    step = (v_hi - v_lo) / (n_k - 1)
    return np.ascontiguousarray(P[::-1]), -v_hi / C_LIGHT, C_LIGHT / step


KMS = 1e5


def designs():
    """name -> (wav, K, b0, s): the grids of observe_ref with kernels of 2, 33 and 1025 nodes (+-0.5, 3 and 15 km/s: supports of a
    few to about a hundred points on grid_nonuniform(1500)), one-point supports and the spacing jump of
    grid_coarse_fine, and exact nodes on grid_dyadic."""
    g = oref.grid_nonuniform(1500)
    out = {
        "nonuniform n_k=2": (g,) + kernel(2, -0.5 * KMS, 0.5 * KMS, "gauss"),
        "nonuniform n_k=33": (g,) + kernel(33, -3 * KMS, 3 * KMS, "ring"),
        "nonuniform n_k=65 random": (g,) + kernel(65, -3 * KMS, 3 * KMS, "random"),
        "nonuniform n_k=1025": (g,) + kernel(1025, -15 * KMS, 15 * KMS, "ring"),
        "coarse_fine n_k=33": (oref.grid_coarse_fine(700, 60),) + kernel(33, -3 * KMS, 3 * KMS, "ring"),
        "dyadic n_k=33": (oref.grid_dyadic(600), np.ascontiguousarray(kernel(33, -1, 1, "ring")[0]), -16 * 2.0 ** -16,
                          2.0 ** 16),
    }
    return out


def wide_design():
    """+-160 km/s on grid_nonuniform(3000): supports of 500 to 1,100 points, so every tile's union, also the cut ones
    of the first and the last tile, exceeds the stage and the global path runs everywhere (+-80 km/s would still fit
    the two end tiles' unions into the stage)."""
    return (oref.grid_nonuniform(3000),) + kernel(33, -160 * KMS, 160 * KMS, "ring")


def mixed_design():
    """+-10 km/s on a coarse/fine grid: the unions of the fine core's tiles exceed the stage, those of the coarse
    wings fit, so neighbouring tiles take different paths."""
    return (oref.grid_coarse_fine(1400, 300),) + kernel(33, -10 * KMS, 10 * KMS, "ring")


def shift_design():
    """A pure shift: the kernel spans +2 .. +4 km/s and does not cover beta = 0, so outputs near one end of the grid
    have an empty support."""
    return (oref.grid_nonuniform(1500),) + kernel(9, 2 * KMS, 4 * KMS, "gauss")
