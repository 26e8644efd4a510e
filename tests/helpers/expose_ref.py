"""Reference of the device exposures (include/prom_hip.h, "exposures on the device") in numpy.longdouble, written
from the definition alone on top of observe_ref.observe and vmap_ref, with the bounds the tests assert.

The bounds.  u = 2^-53, eps = observe_ref.m_tolerance(k, n_max) is the documented bound on a tap's model M_i.  The
models are positive and the weights non-negative, so M_e = sum of fl(a_i M_i) over the K_live live taps has
non-negative terms: every term carries M_i's error eps and one rounding of the product, eps + u, and a sum of K_live
non-negative terms in any order adds at most (K_live - 1) u.  M_e errs by at most

    eps_e = eps + (K_live + 1) u        relative

(one u to spare).  The moment bounds are vmap_ref.bounds' with eps_e in eps's place: they were derived for any model
with a relative error bound and positive data.  The model on request is within eps_e |M_e|.
"""
import numpy as np

from helpers import observe_ref as ref
from helpers import vmap_ref as vref

LD = np.longdouble
U = ref.U


def expose(wav, R, lam, sig, k, rows, a, F, data, ivar):
    """(mom [n_exp][n_trial][7] longdouble, n_used [n_exp][n_trial] int64, M [n_exp][n_trial][n_pix] longdouble (NaN
    where there is no model), n_max: the largest support of a live tap, k_live: the most live taps of an exposure)."""
    R = np.atleast_2d(np.asarray(R, dtype=np.float64))
    rows, a, F = np.asarray(rows), np.asarray(a, dtype=np.float64), np.asarray(F, dtype=np.float64)
    data, ivar = np.asarray(data, dtype=np.float64), np.asarray(ivar, dtype=np.float64)
    n_exp, n_trial, n_tap = F.shape
    n_pix = len(lam)
    mom = np.zeros((n_exp, n_trial, 7), dtype=LD)
    n_used = np.zeros((n_exp, n_trial), dtype=np.int64)
    Ms = np.full((n_exp, n_trial, n_pix), np.nan, dtype=LD)
    n_max = k_live = 0
    cache = {}
    for e in range(n_exp):
        live = [i for i in range(n_tap) if a[e, i] > 0]
        k_live = max(k_live, len(live))
        for j in range(n_trial):
            Me = np.zeros(n_pix, dtype=LD)
            covered = np.full(n_pix, bool(live))
            for i in live:
                key = (int(rows[e, i]), float(F[e, j, i]))
                if key not in cache:
                    num, den, cnt = ref.observe(wav, R[key[0]:key[0] + 1], lam, sig, k, [key[1]])
                    cache[key] = (num[0], den[0], int(cnt.max()) if cnt.size else 0)
                num, den, cnt = cache[key]
                n_max = max(n_max, cnt)
                covered &= den > 0
                with np.errstate(invalid="ignore", divide="ignore"):
                    Me = Me + LD(a[e, i]) * np.where(den > 0, num / np.where(den > 0, den, 1), np.nan)
            Ms[e, j, covered] = Me[covered]
            with np.errstate(invalid="ignore"):
                used = np.isfinite(ivar[e]) & (ivar[e] > 0) & np.isfinite(data[e]) & covered
            M = Me[used]
            iv, d = ivar[e, used].astype(LD), data[e, used].astype(LD)
            mom[e, j] = [iv.sum(), (iv * M).sum(), (iv * d).sum(), (iv * M * M).sum(), (iv * M * d).sum(),
                         (iv * d * d).sum(), (iv * (M - d) ** 2).sum()]
            n_used[e, j] = int(used.sum())
    return mom, n_used, Ms, n_max, k_live


def model_tolerance(k, n_max, k_live):
    """eps_e = eps + (K_live + 1) u, relative (the module's derivation)."""
    return ref.m_tolerance(k, n_max) + (k_live + 1.0) * U


def bounds(mom_ref, n_used, k, n_max, k_live):
    """vmap_ref.bounds with eps_e for eps: relative for m0 .. m5 (times |reference|), absolute for m6."""
    m = np.asarray(mom_ref, dtype=LD)
    eps = model_tolerance(k, n_max, k_live)
    nu = (np.asarray(n_used, dtype=np.float64) + 4.0) * U
    out = np.zeros(m.shape, dtype=np.float64)
    for i, e in zip(range(6), (0.0, eps, 0.0, 2 * eps, eps, 0.0)):
        out[..., i] = (np.abs(m[..., i]) * (e + nu)).astype(np.float64)
    out[..., 6] = (2 * eps * np.sqrt(np.abs(m[..., 6] * m[..., 3])) + eps * eps * np.abs(m[..., 3])
                   + nu * np.abs(m[..., 6])).astype(np.float64)
    return out


def fractions(mom, mom_ref, n_used, k, n_max, k_live):
    """|mom - reference| / bound per moment, the largest over (e, j): [7] (vmap_ref.fractions' rules for zero bounds
    and NaN)."""
    mom, m = np.asarray(mom, dtype=LD), np.asarray(mom_ref, dtype=LD)
    b = bounds(np.where(np.isnan(m), 0, m), n_used, k, n_max, k_live)
    both_nan = np.isnan(mom) & np.isnan(m)
    one_nan = np.isnan(mom) ^ np.isnan(m)
    diff = np.abs(np.where(both_nan | one_nan, 0, mom - m)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        fr = np.where(diff == 0.0, 0.0, diff / b)
    fr = np.where(one_nan, np.inf, fr)
    return np.array([float(np.max(fr[..., i])) if fr[..., i].size else 0.0 for i in range(7)])


def model_fraction(model, M_ref, k, n_max, k_live):
    """The largest |model - reference| / (eps_e |reference|) over the pixels that have a model; inf where the NaN
    patterns differ."""
    model, M = np.asarray(model, dtype=LD), np.asarray(M_ref, dtype=LD)
    if not np.array_equal(np.isnan(model), np.isnan(M)):
        return np.inf
    ok = ~np.isnan(M)
    if not ok.any():
        return 0.0
    d = np.abs(model[ok] - M[ok]).astype(np.float64)
    b = (np.abs(M[ok]) * model_tolerance(k, n_max, k_live)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(d == 0.0, 0.0, d / b)))


def float64_moments(wav, R, lam, sig, k, rows, a, F, data, ivar, reverse=False):
    """The moments in plain float64, every sum one term after the other, the support's points, the taps and the pixels
    in forward or reverse order: what any reasonable evaluation order gives."""
    q = ref.q_weights(wav)
    n_exp, n_trial, n_tap = F.shape
    order = slice(None, None, -1) if reverse else slice(None)
    mom = np.zeros((n_exp, n_trial, 7))
    n_used = np.zeros((n_exp, n_trial), dtype=np.int64)
    for e in range(n_exp):
        taps = [i for i in range(n_tap) if a[e, i] > 0][order]
        for j in range(n_trial):
            acc = [0.0] * 7
            for p in (range(len(lam) - 1, -1, -1) if reverse else range(len(lam))):
                iv, d = ivar[e, p], data[e, p]
                if not taps or not (np.isfinite(iv) and iv > 0 and np.isfinite(d)):
                    continue
                Me, covered = 0.0, True
                for i in taps:
                    L, S = lam[p] * F[e, j, i], sig[p] * F[e, j, i]
                    s0, s1 = ref.support(wav, L, k * S)
                    z = (wav[s0:s1] - L) / S
                    gq = np.exp(-0.5 * z * z) * q[s0:s1]
                    nm = dn = 0.0
                    for g, r in zip(gq[order], R[rows[e, i], s0:s1][order]):
                        dn += g
                        nm += g * r
                    if not dn > 0:
                        covered = False
                        break
                    Me += a[e, i] * (nm / dn)
                if not covered:
                    continue
                M = Me
                for i, term in enumerate((iv, iv * M, iv * d, iv * M * M, iv * M * d, iv * d * d, iv * (M - d) ** 2)):
                    acc[i] += term
                n_used[e, j] += 1
            mom[e, j] = acc
    return mom, n_used


def degenerate(F):
    """The exposure table that is the velocity map over F[n_orb][n_trial]: one tap of weight 1 on row e."""
    F = np.asarray(F, dtype=np.float64)
    n_orb = F.shape[0]
    return np.arange(n_orb, dtype=np.int32)[:, None], np.ones((n_orb, 1)), np.ascontiguousarray(F[:, :, None])
