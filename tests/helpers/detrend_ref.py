"""References of the detrended exposures (include/prom_hip.h, "detrended exposures on the device").

filter_f64 is the definition in numpy float64: a Python loop over e and k, vectorised over (j, p), in which every
product and every sum is a numpy operation of its own and therefore rounded on its own, and a term with W = 0 is
skipped with a mask.  It is the bitwise reference of the device's filtered model.  filter_ld is the same in
longdouble, moments_ld the moments of a model in longdouble.

The bounds.  u = 2^-53.  The device starts from its own unfiltered model Mt_e = M_e (1 + d_e), |d_e| <= eps_e, the
exposures' model bound (expose_ref.model_tolerance).  Write S_k = sum_e' |W_ke'| |M_e'| over the terms with W != 0.

  coefficients   ct_k is the float64 dot product of n_exp terms at most: |ct_k - sum W Mt| <= n_exp u sum |W| |Mt|
                 (the standard bound: one rounding per product and n_exp - 1 additions), and
                 |sum W Mt - sum W M| <= eps_e S_k, so |ct_k - c_k| <= (eps_e + (n_exp + 1) u) S_k, the spare u taking
                 the second-order terms
  apply          Mt'_e comes from Mt_e by n_comp products and n_comp subtractions.  A product errs by u |U_ek| |ct_k|,
                 a subtraction by u times its result, which is at most |M_e| + sum_k |U_ek| S_k:
                 (n_comp + 1) u (|M_e| + sum_k |U_ek| S_k) in all
  inputs         eps_e |M_e| from Mt_e itself and sum_k |U_ek| |ct_k - c_k| from the coefficients

  |M'_dev - M'_exact| <= eps_e |M_e| + sum_k |U_ek| (eps_e + (n_exp + 1) u) S_k
                         + (n_comp + 1) u (|M_e| + sum_k |U_ek| S_k)

It is absolute: the filtered model is signed and cancels, so no relative bound exists.

The moments are compared with the longdouble sums of the device's own filtered model, which leaves the roundings of the
terms (four at most, in m6: the difference, its square, the product with iv; the model is the same number on both
sides) and of the n_used - 1 additions, in any order: (n_used + 4) u sum |term| per moment.  The terms are signed
except in m0, m5 and m6, so the sum of their magnitudes stands in the bound, not the moment.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def _filter(M, Ub, W, dtype):
    M, Ub, W = (np.asarray(a, dtype=dtype) for a in (M, Ub, W))
    n_exp, n_comp = Ub.shape
    assert M.ndim == 3 and M.shape[0] == n_exp and W.shape == (n_comp, n_exp, M.shape[2])
    c = np.zeros((n_comp,) + M.shape[1:], dtype=dtype)
    ok = np.ones(M.shape[1:], dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for e in range(n_exp):
            reads = np.zeros(M.shape[2], dtype=bool)
            for k in range(n_comp):
                mask = W[k, e] != 0
                if not mask.any():
                    continue
                reads |= mask
                term = W[k, e][None, :] * M[e]
                c[k] = np.where(mask[None, :], c[k] + term, c[k])
            ok &= ~(reads[None, :] & np.isnan(M[e]))
        out = np.empty_like(M)
        for e in range(n_exp):
            m = M[e].copy()
            for k in range(n_comp):
                prod = Ub[e, k] * c[k]
                m = m - prod
            out[e] = np.where(ok, m, np.nan)
    return out, ok


def filter_f64(M, Ub, W):
    """(M' [n_exp][n_trial][n_pix] float64, filterable [n_trial][n_pix]) of the model M[n_exp][n_trial][n_pix], the
    basis Ub[n_exp][n_comp] and W[n_comp][n_exp][n_pix]: the definition, rounding for rounding."""
    return _filter(M, Ub, W, np.float64)


def filter_ld(M, Ub, W):
    """The same in longdouble."""
    return _filter(M, Ub, W, LD)


def model_bound(M_exact, Ub, W, eps_e):
    """The derived absolute bound [n_exp][n_trial][n_pix] on |M'_dev - M'_exact| (the module's derivation); NaN model
    values count as 0 where W = 0 (they are never read) and make the column NaN otherwise."""
    M = np.asarray(M_exact, dtype=LD)
    Ua, Wa = np.abs(np.asarray(Ub, dtype=LD)), np.abs(np.asarray(W, dtype=LD))
    n_exp, n_comp = Ua.shape
    S = np.zeros((n_comp,) + M.shape[1:], dtype=LD)
    for e in range(n_exp):
        for k in range(n_comp):
            mask = Wa[k, e] != 0
            S[k] += np.where(mask[None, :], Wa[k, e][None, :] * np.abs(M[e]), 0)
    US = np.einsum("ek,kjp->ejp", Ua, S)
    absM = np.abs(M)
    return (eps_e * absM + (eps_e + (n_exp + 1) * U) * US + (n_comp + 1) * U * (absM + US)).astype(np.float64)


def moments_ld(model, data, ivar):
    """(moments [n_exp][n_trial][7] longdouble, n_used int64, sum of |term| [n_exp][n_trial][7] longdouble) of a
    model [n_exp][n_trial][n_pix] against data and ivar [n_exp][n_pix], with the definition's used test: ivar finite
    and > 0, data finite, model not NaN (an unfilterable column's model is NaN)."""
    M = np.asarray(model, dtype=LD)
    d = np.asarray(data, dtype=LD)[:, None, :]
    iv = np.asarray(ivar, dtype=LD)[:, None, :]
    with np.errstate(invalid="ignore"):
        used = np.isfinite(iv) & (iv > 0) & np.isfinite(d) & ~np.isnan(M)
        z = lambda a: np.where(used, a, 0)
        Mz, dz, ivz = z(M), z(np.broadcast_to(d, M.shape)), z(np.broadcast_to(iv, M.shape))
        terms = np.stack([ivz, ivz * Mz, ivz * dz, ivz * Mz * Mz, ivz * Mz * dz, ivz * dz * dz,
                          ivz * (Mz - dz) * (Mz - dz)], axis=-1)
    return terms.sum(axis=2), used.sum(axis=2).astype(np.int64), np.abs(terms).sum(axis=2)


def moment_fractions(mom, mom_ld, n_used, abs_ld):
    """|mom - reference| / ((n_used + 4) u sum |term|) per moment: the largest over (e, j), [7].  Where the bound is 0
    the difference must be 0 too (fraction 0), else inf."""
    diff = np.abs(np.asarray(mom, dtype=LD) - mom_ld)
    b = (np.asarray(n_used, dtype=LD)[..., None] + 4) * U * abs_ld
    with np.errstate(invalid="ignore", divide="ignore"):
        fr = np.where(b > 0, diff / np.where(b > 0, b, 1), np.where(diff == 0, 0.0, np.inf)).astype(np.float64)
    return np.array([float(fr[..., i].max()) if fr[..., i].size else 0.0 for i in range(7)])


def model_fraction(model, M_exact_filtered, bound):
    """The largest |model - reference| / bound over the values that are not NaN in the reference; inf where the NaN
    patterns differ or a difference stands against a zero bound."""
    m, r = np.asarray(model, dtype=LD), np.asarray(M_exact_filtered, dtype=LD)
    if not np.array_equal(np.isnan(m), np.isnan(r)):
        return float("inf")
    live = ~np.isnan(r)
    if not live.any():
        return 0.0
    diff, b = np.abs(m[live] - r[live]), np.asarray(bound)[live]
    fr = np.where(b > 0, diff / np.where(b > 0, b, 1), np.where(diff == 0, 0.0, np.inf))
    return float(fr.max())
