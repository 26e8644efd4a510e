"""References of the high-pass filtered exposures (include/prom_hip.h, "high-pass filtered exposures on the device").

highpass_f64 is the definition in numpy float64: per segment a Python loop over the distance d = i' - i in ascending
order, vectorised over the rows and the positions i, in which every product and every sum is a numpy operation of its
own and therefore rounded on its own.  A NaN value (and a position outside the segment, which is padded with NaN) adds
+0 to num and den, which the definition says gives the bits of skipping it.  It is the bitwise reference of the
device's filtered model.  highpass_ld is the same in longdouble.

The bound.  u = 2^-53, g >= 0.  The device starts from its own unfiltered model Mt_i = M_i (1 + d_i), |d_i| <= eps_e,
the exposures' model bound (expose_ref.model_tolerance).  A window has at most 2 h + 1 terms.

  num     a float64 sum of at most 2 h + 1 products: one rounding per product and at most 2 h + 1 additions (the
          first onto +0 is exact) err by at most (2 h + 2) u sum g |Mt| to first order, and the inputs by
          eps_e sum g |M|
  den     at most 2 h additions that round: relative error 2 h u
  B       fl(num / den): one more u.  With |B| <= sum g |M| / sum g:
          dB <= (eps_e + (2 h + 2) u + 2 h u + u) sum g |M| / sum g <= (eps_e + 2 gamma + u) sum g |M| / sum g,
          gamma = (2 h + 3) u.  The spare 3 u of 2 gamma takes the second-order terms; no further factor is applied
  mode 0  M'_dev = fl(Mt - B_dev):  |M'_dev - M'| <= eps_e |M| + dB + u (|M'| + eps_e |M| + dB)
  mode 1  M'_dev = fl(Mt / B_dev) = (M / B) (1 + d) / (1 + r) (1 + u'), |r| <= rho = dB / |B|:
          |M'_dev - M'| <= |M'| (t + u (1 + t)), t = (eps_e + rho) / (1 - rho).  It is a statement about a quotient, so
          it is used only where rho <= 2^-10 (|B| far from 0); elsewhere the model is not compared

The subtracting bound is absolute: the filtered model is a small difference of the model and its mean, so no relative
bound exists.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
RHO_MAX = 2.0 ** -10


def one_segment(n_pix):
    """(seg_first, perm) of one order in the device's own pixel order."""
    return np.array([0, n_pix], dtype=np.int32), np.arange(n_pix, dtype=np.int32)


def _highpass(M, seg_first, perm, g, mode, dtype, reverse=False, bound_eps=None):
    M = np.asarray(M, dtype=dtype)
    g = np.asarray(g, dtype=dtype)
    seg_first, perm = np.asarray(seg_first), np.asarray(perm)
    h = len(g) - 1
    out = np.full(M.shape, np.nan, dtype=dtype)
    extra = np.full(M.shape, np.nan, dtype=dtype)      # B, or with bound_eps the bound
    live = np.zeros(M.shape, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(len(seg_first) - 1):
            idx = perm[seg_first[s]:seg_first[s + 1]]
            n = len(idx)
            x = M[..., idx]
            pad = np.full(x.shape[:-1] + (h,), np.nan, dtype=dtype)
            xp = np.concatenate([pad, x, pad], axis=-1)
            num, den, sab = (np.zeros(x.shape, dtype=dtype) for _ in range(3))
            ds = range(-h, h + 1)
            for d in (reversed(ds) if reverse else ds):
                src = xp[..., h + d:h + d + n]
                ok = ~np.isnan(src)
                term = g[abs(d)] * src
                num = num + np.where(ok, term, 0)
                den = den + np.where(ok, g[abs(d)], 0)
                if bound_eps is not None:
                    sab = sab + np.where(ok, np.abs(term), 0)
            B = num / den
            res = x - B if mode == 0 else x / B
            out[..., idx] = res
            if bound_eps is None:
                extra[..., idx] = B
                continue
            gamma = (2 * h + 3) * U
            dB = (bound_eps + 2 * gamma + U) * sab / den
            if mode == 0:
                b = bound_eps * np.abs(x) + dB + U * (np.abs(res) + bound_eps * np.abs(x) + dB)
                ok_b = ~np.isnan(x)
            else:
                rho = dB / np.abs(B)
                ok_b = ~np.isnan(x) & (rho <= RHO_MAX)
                t = (bound_eps + rho) / (1 - rho)
                b = np.abs(res) * (t + U * (1 + t))
            extra[..., idx] = b
            live[..., idx] = ok_b
    if bound_eps is None:
        return out, extra
    return out, extra, live


def highpass_f64(M, seg_first, perm, g, mode):
    """M' float64 of the model M[..., n_pix] (device order): the definition, rounding for rounding."""
    return _highpass(M, seg_first, perm, g, mode, np.float64)[0]


def highpass_f64_reversed(M, seg_first, perm, g, mode):
    """The same with every window summed in descending i' (another rounding order, for the bound's test)."""
    return _highpass(M, seg_first, perm, g, mode, np.float64, reverse=True)[0]


def highpass_ld(M, seg_first, perm, g, mode):
    """The same in longdouble."""
    return _highpass(M, seg_first, perm, g, mode, LD)[0]


def model_bound(M_exact, seg_first, perm, g, mode, eps_e):
    """(M' longdouble, bound on |M'_dev - M'|, where the bound applies) of the exact model M_exact: the module's
    derivation.  The bound applies at every value that is not NaN in mode 0, in mode 1 where also rho <= 2^-10."""
    return _highpass(M_exact, seg_first, perm, g, mode, LD, bound_eps=LD(eps_e))


def model_fraction(model, exact, bound, live):
    """The largest |model - exact| / bound over ``live``; inf where the NaN patterns differ or a difference stands
    against a zero bound."""
    m, r = np.asarray(model, dtype=LD), np.asarray(exact, dtype=LD)
    if not np.array_equal(np.isnan(m), np.isnan(r)):
        return float("inf")
    live = live & np.isfinite(r) & np.isfinite(m)
    if not live.any():
        return 0.0
    diff, b = np.abs(m[live] - r[live]), np.asarray(bound)[live]
    fr = np.where(b > 0, diff / np.where(b > 0, b, 1), np.where(diff == 0, 0.0, np.inf))
    return float(fr.max())


def interleaved(lengths, seed=0):
    """(seg_first, perm) of segments of the given lengths whose pixels are dealt over the device's order at random
    (overlapping orders), every second segment reversed in position."""
    n = int(sum(lengths))
    rng = np.random.default_rng(seed)
    owner = rng.permutation(np.repeat(np.arange(len(lengths)), lengths))
    perm = []
    for s in range(len(lengths)):
        idx = np.flatnonzero(owner == s)
        perm.append(idx[::-1] if s % 2 else idx)
    seg_first = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    assert seg_first[-1] == n
    return seg_first, np.concatenate(perm).astype(np.int32)
