"""The filter's weights by the device's definition (include/prom_hip.h, "the filter's weights on the device") restated
in numpy: a Python loop over e, i, j and k, vectorised over the pixels, every operation a numpy operation of its own
(numpy never fuses a multiply with an add), so weights_f64 gives the kernel's bits.  weights_ld is the same text in
longdouble, the yardstick of the accuracy tests.  designs() makes the four designs the definition was prototyped on."""
import numpy as np


def _weights(U, ivar, dt):
    U = np.asarray(U, dtype=np.float64)
    iv = np.asarray(ivar, dtype=np.float64)
    n_exp, K = U.shape
    n_pix = iv.shape[1]
    Ud = U.astype(dt)
    with np.errstate(all="ignore"):
        v = np.where(np.isfinite(iv) & (iv > 0), iv, 0.0).astype(dt)      # [n_exp][n_pix]
        on = v > 0
        cnt = on.sum(axis=0)
        zero = np.zeros(n_pix, dtype=dt)
        N = [[zero.copy() for _ in range(i + 1)] for i in range(K)]
        for e in range(n_exp):
            for i in range(K):
                t = v[e] * Ud[e, i]
                for j in range(i + 1):
                    N[i][j] = np.where(on[e], N[i][j] + t * Ud[e, j], N[i][j])
        dmax = N[0][0].copy()
        for i in range(1, K):
            dmax = np.where(N[i][i] > dmax, N[i][i], dmax)
        tol = (dt(K) * dt(2.0 ** -52)) * dmax
        regular = cnt >= K
        L = N
        for j in range(K):
            s = L[j][j]
            for k in range(j):
                s = s - L[j][k] * L[j][k]
            regular = regular & (s > tol)
            d = np.sqrt(s)
            L[j][j] = d
            for i in range(j + 1, K):
                t = L[i][j]
                for k in range(j):
                    t = t - L[i][k] * L[j][k]
                L[i][j] = t / d
        W = np.zeros((K, n_exp, n_pix), dtype=dt)
        for e in range(n_exp):
            x = [None] * K
            for i in range(K):
                s = v[e] * Ud[e, i]
                for k in range(i):
                    s = s - L[i][k] * x[k]
                x[i] = s / L[i][i]
            for i in range(K - 1, -1, -1):
                s = x[i]
                for k in range(K - 1, i, -1):
                    s = s - L[k][i] * x[k]
                x[i] = s / L[i][i]
            for k in range(K):
                W[k, e] = x[k]
        use = on & regular[None, :]
        finite = np.isfinite(np.where(use[None, :, :], W, 0)).all(axis=(0, 1))
        W = np.where((use & finite[None, :])[None, :, :], W, dt(0.0))
    return np.ascontiguousarray(W), regular & finite


def weights_f64(U, ivar):
    """W[K][n_exp][n_pix] by the definition in float64: the kernel's bits, signs of zero included."""
    return _weights(U, ivar, np.float64)[0]


def regular_f64(U, ivar):
    """The pixels the definition does not zero."""
    return _weights(U, ivar, np.float64)[1]


def weights_ld(U, ivar):
    """The same evaluation in longdouble."""
    return _weights(U, ivar, np.longdouble)[0]


DESIGNS = ((7, 1, 65), (12, 3, 130), (48, 6, 300), (70, 16, 129))


def design(n_exp, K, n_pix, seed=5):
    """(U, ivar) of one prototype design: a perturbed orthonormal basis, 10 % of ivar zeroed, and planted pixels with
    no, K - 1 and <= K weighted exposures (pixels 0, 1 and 2 .. 4)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n_exp, K)))
    U = Q + 0.05 * rng.standard_normal((n_exp, K))
    iv = rng.uniform(0.5, 2.0, (n_exp, n_pix))
    iv[rng.random((n_exp, n_pix)) < 0.1] = 0.0
    iv[:, 0] = 0.0
    if n_pix > 1:
        iv[:, 1] = 0.0
        iv[rng.permutation(n_exp)[:K - 1], 1] = 1.0
    for p in range(2, min(5, n_pix)):
        iv[:, p] = 0.0
        iv[rng.permutation(n_exp)[:max(K - (p - 2), 0)], p] = rng.uniform(0.5, 2.0, max(K - (p - 2), 0))
    return U, iv


def designs(seed=5):
    return [design(*d, seed=seed) for d in DESIGNS]
