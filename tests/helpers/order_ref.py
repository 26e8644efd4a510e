"""References of the per-order moments (include/prom_hip.h, "per-order moments on the device"), from the definition
and not from the kernel.

order_moments_f64 is the definition in numpy float64: per order the used rule and the seven terms, every product and
difference a numpy operation of its own, the positions cut into tiles of 32, each tile's 32-vector t reduced by the xor
butterfly t = t + t[idx ^ m] for m = 1, 2, 4, 8, 16, and the tiles' sums t[0] added in ascending tile order to a sum
that starts at +0.  It is the bitwise reference of the device's records.  order_moments_ld gives the longdouble sums
and the sums of the terms' magnitudes.

totals_f64 applies the definition's formulas to records, in the order observation.VelocityMap evaluates them, and adds
the entering orders (kept, n_used >= 2) in ascending order from +0.

The bound of the totals.  u = 2^-53.  chi2 (sum m6), chi2_scaled and the count are formed from +, -, * and / alone, each
rounded on its own in the same order on both sides, so they are numpy's bit for bit.  The logarithm's argument is
numpy's bit for bit as well, so an order's loglike_s = fl(fl(-0.5 N) ln(arg)) differs from numpy's only through the two
logarithms and the product's rounding:

  the device's ln   the installed ROCm documentation states no ulp bound for the double-precision log of the
                    device library, so the figure is OpenCL's for double log: LOG_ULP_DEVICE = 3 ulp
  numpy's ln        the reference's own error: the C library's log, at most LOG_ULP_NUMPY = 1 ulp
  one ulp of ln     at most 2 u |ln|, so |ln_dev - ln_np| <= 2 (3 + 1) u |ln|, times N / 2:  8 u |loglike_s|
  the product       both sides round fl(-0.5 N) ln once: the roundings differ by at most u |loglike_s| (first order)
  the sum           at most n_seg additions of which the first is exact; (n_seg + 1) u sum |loglike_s| covers them

  |total_dev - total_np| <= (2 (LOG_ULP_DEVICE + LOG_ULP_NUMPY) + 1) u sum |loglike_s| + (n_seg + 1) u sum |loglike_s|

over the entering orders.  An infinite or NaN statistic must agree exactly (NaN with NaN, an infinity with itself).
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TILE = 32
LOG_ULP_DEVICE = 3.0      # OpenCL's bound for double log (the installed ROCm documentation has no figure)
LOG_ULP_NUMPY = 1.0       # the reference's own logarithm


def _used_and_terms(model, data, ivar, flag, idx, dtype):
    """(used [E][J][n], terms 7 x [E][J][n]) of the positions idx; unused terms are +0."""
    M = np.asarray(model, dtype=np.float64)[..., idx]
    d = np.asarray(data, dtype=np.float64)[:, None, idx]
    iv = np.asarray(ivar, dtype=np.float64)[:, None, idx]
    with np.errstate(invalid="ignore", over="ignore"):
        used = np.isfinite(iv) & (iv > 0) & np.isfinite(d) & ~np.isnan(M)
        if flag is not None:
            used = used & (np.asarray(flag)[None, :, idx] != 0)
        M, d, iv = (np.broadcast_to(x, M.shape).astype(dtype) for x in (M, d, iv))
        ivM, ivd, df = iv * M, iv * d, M - d
        terms = [iv, ivM, ivd, ivM * M, ivM * d, ivd * d, iv * (df * df)]
    zero = np.zeros((), dtype=dtype)
    return used, [np.where(used, t, zero) for t in terms]


def order_moments_f64(model, data, ivar, flag, seg_first, perm, tile=TILE, reverse=False):
    """(moments [n_exp][n_trial][n_seg][7] float64, n_used [n_exp][n_trial][n_seg] int64) of model
    [n_exp][n_trial][n_pix] against data, ivar [n_exp][n_pix] with the columns' flags [n_trial][n_pix] (None: all set),
    in the device's pixel order: the definition, rounding for rounding.  ``reverse``: the positions of every order in
    descending order (another rounding order, for the bound's test).  ``tile``: the butterfly's width (a power of
    two; the device's is 32)."""
    model = np.asarray(model, dtype=np.float64)
    seg_first, perm = np.asarray(seg_first), np.asarray(perm)
    n_seg = len(seg_first) - 1
    mom = np.zeros(model.shape[:2] + (n_seg, 7))
    nu = np.zeros(model.shape[:2] + (n_seg,), dtype=np.int64)
    lanes = np.arange(tile)
    for s in range(n_seg):
        idx = perm[seg_first[s]:seg_first[s + 1]]
        if reverse:
            idx = idx[::-1]
        used, terms = _used_and_terms(model, data, ivar, flag, idx, np.float64)
        nu[:, :, s] = used.sum(axis=2)
        n = len(idx)
        n_tiles = (n + tile - 1) // tile
        for i, term in enumerate(terms):
            t = np.zeros(term.shape[:2] + (n_tiles * tile,))
            t[..., :n] = term
            t = t.reshape(term.shape[:2] + (n_tiles, tile))
            m = 1
            while m < tile:
                t = t + t[..., lanes ^ m]
                m *= 2
            acc = np.zeros(term.shape[:2])
            for k in range(n_tiles):
                acc = acc + t[..., k, 0]
            mom[:, :, s, i] = acc
    return mom, nu


def order_moments_ld(model, data, ivar, flag, seg_first, perm):
    """(moments longdouble, n_used, sums of |term| longdouble), the shapes of order_moments_f64's: the terms formed and
    added in longdouble."""
    model = np.asarray(model, dtype=np.float64)
    seg_first, perm = np.asarray(seg_first), np.asarray(perm)
    n_seg = len(seg_first) - 1
    mom = np.zeros(model.shape[:2] + (n_seg, 7), dtype=LD)
    mag = np.zeros(model.shape[:2] + (n_seg, 7), dtype=LD)
    nu = np.zeros(model.shape[:2] + (n_seg,), dtype=np.int64)
    for s in range(n_seg):
        idx = perm[seg_first[s]:seg_first[s + 1]]
        used, terms = _used_and_terms(model, data, ivar, flag, idx, LD)
        nu[:, :, s] = used.sum(axis=2)
        for i, term in enumerate(terms):
            mom[:, :, s, i] = term.sum(axis=2)
            mag[:, :, s, i] = np.abs(term).sum(axis=2)
    return mom, nu, mag


def moment_fraction(mom, mom_ld, n_terms, mag):
    """The largest |mom - mom_ld| / ((n_terms + 4) u sum |term|) per moment [7]; inf where a difference stands against
    a zero bound.  ``n_terms`` broadcasts against mom[..., 0]."""
    diff = np.abs(np.asarray(mom, dtype=LD) - mom_ld)
    bound = (np.asarray(n_terms, dtype=LD)[..., None] + 4) * LD(U) * mag
    fr = np.where(bound > 0, diff / np.where(bound > 0, bound, 1), np.where(diff == 0, 0.0, np.inf))
    return np.array([float(fr[..., i].max()) for i in range(7)])


def _ratio(a, b):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.where(b == 0.0, np.nan, a / np.where(b == 0.0, 1.0, b))


def order_stats_f64(mom, nu):
    """(loglike_s, chi2_scaled_s) of records: the definition's formulas, every operation rounded on its own in the
    order written."""
    mom = np.asarray(mom, dtype=np.float64)
    m0, m1, m2, m3, m4, m5 = (mom[..., i] for i in range(6))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        scaled = m5 - _ratio(m4 * m4, m3)
        sf = _ratio(m5 - _ratio(m2 * m2, m0), m0)
        sg = _ratio(m3 - _ratio(m1 * m1, m0), m0)
        c = _ratio(m4 - _ratio(m1 * m2, m0), m0)
        arg = (sf - 2.0 * c) + sg
        ll = (-0.5 * np.asarray(nu, dtype=np.float64)) * np.log(arg)
    return ll, scaled


def enters(nu, keep):
    return (np.asarray(keep) != 0) & (np.asarray(nu) >= 2)


def totals_f64(mom, nu, keep):
    """tot [...][4] = (sum loglike_s, sum m6_s, sum chi2_scaled_s, sum n_used_s) over the entering orders of the
    records mom [...][n_seg][7], nu [...][n_seg], in ascending s from +0."""
    mom = np.asarray(mom, dtype=np.float64)
    nu = np.asarray(nu, dtype=np.int64)
    ll, scaled = order_stats_f64(mom, nu)
    en = enters(nu, keep)
    tot = np.zeros(mom.shape[:-2] + (4,))
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(mom.shape[-2]):
            stats = (ll[..., s], mom[..., s, 6], scaled[..., s], nu[..., s].astype(np.float64))
            for i, x in enumerate(stats):
                tot[..., i] = np.where(en[..., s], tot[..., i] + x, tot[..., i])
    return tot


def loglike_bound(mom, nu, keep):
    """The bound of |sum loglike (device) - sum loglike (totals_f64)| per (...): the module's derivation.  0 where no
    order enters; not meaningful where an entering order's loglike is not finite (compare those exactly)."""
    ll, _ = order_stats_f64(mom, nu)
    en = enters(nu, keep)
    n_seg = np.asarray(mom).shape[-2]
    mag = np.where(en & np.isfinite(ll), np.abs(ll), 0.0).sum(axis=-1)
    return (2.0 * (LOG_ULP_DEVICE + LOG_ULP_NUMPY) + 1.0) * U * mag + (n_seg + 1) * U * mag
