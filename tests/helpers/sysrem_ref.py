"""References of the injection and SYSREM on the device (include/prom_hip.h, "injection and SYSREM on the device").

sysrem_f64 is the definition in numpy float64: every product, sum, quotient and square root is a numpy operation of
its own and therefore rounded on its own; the column fit runs in ascending e with the terms of weight 0 skipped by a
mask; the row fit adds its terms in the fixed shape of prometheus_amd/csrc/sysrem_index.h (a lane's consecutive
pixels, the butterfly over a tile's 64 lanes, the tiles dealt to 64 sums, the same butterfly), whose constants are read
from that header.  It is the bitwise reference of the device.  sysrem_ld is the same text in longdouble.

In the row shape a term of weight 0 "adds nothing"; here it adds +0.  That gives the same bits: every sum starts at +0
and no IEEE sum of round-to-nearest that starts at +0 is ever -0, so x + (+0) = x for every x a sum can hold.

inject_f64 is the injection formula, weights_of the weights and residuals."""
import os
import re

import numpy as np

LD = np.longdouble
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_HDR = open(os.path.join(REPO, "prometheus_amd", "csrc", "sysrem_index.h")).read()
VEC = int(re.search(r"#define PROM_SY_VEC (\d+)", _HDR).group(1))        # pixels of a lane
LANES = int(re.search(r"kSyBlock = (\d+);", _HDR).group(1))               # lanes of a tile
TILE = LANES * VEC                                                        # T: pixels of a tile
MAX_EXP = int(re.search(r"kSyMaxExp = (\d+);", _HDR).group(1))
assert LANES == 64 and "kSyTile = kSyBlock * kSyVec" in _HDR


def inject_f64(raw, M, scale):
    """D = fl(raw fl(1 + fl(scale fl(M - 1)))) where M is not NaN, raw elsewhere."""
    raw, M = np.asarray(raw, dtype=np.float64), np.asarray(M, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = M - 1.0
        t = np.float64(scale) * t
        t = 1.0 + t
        t = raw * t
    return np.where(np.isnan(M), raw, t)


def weights_of(D, ivar, dtype=np.float64):
    """(w, r): w = ivar where ivar is finite and > 0 and D is finite, else 0; r = D where w > 0, else +0."""
    D, iv = np.asarray(D, dtype=np.float64), np.asarray(ivar, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(iv) & (iv > 0) & np.isfinite(D)
    return np.where(ok, iv, 0.0).astype(dtype), np.where(ok, D, 0.0).astype(dtype)


def _butterfly(t):
    """t[..., 64]: for m = 1, 2, .., 32 every t[l] becomes t[l] + t[l ^ m]; returns t[..., 0]."""
    idx = np.arange(64)
    m = 1
    while m < 64:
        t = t + t[..., idx ^ m]
        m <<= 1
    return t[..., 0]


def row_sum(terms):
    """The sum over the pixels of terms[n_exp][n_pix] (+0 where w = 0) in the fixed shape."""
    n_exp, n_pix = terms.shape
    n_tiles = (n_pix + TILE - 1) // TILE
    t = np.zeros((n_exp, n_tiles * TILE), dtype=terms.dtype)
    t[:, :n_pix] = terms
    t = t.reshape(n_exp, n_tiles, 64, VEC)
    lane = np.zeros((n_exp, n_tiles, 64), dtype=terms.dtype)
    for v in range(VEC):
        lane = lane + t[..., v]
    part = _butterfly(lane)                                   # [n_exp][n_tiles]
    n_i = (n_tiles + 63) // 64
    p = np.zeros((n_exp, n_i * 64), dtype=terms.dtype)
    p[:, :n_tiles] = part
    p = p.reshape(n_exp, n_i, 64)
    s = np.zeros((n_exp, 64), dtype=terms.dtype)
    for i in range(n_i):
        s = s + p[:, i, :]
    return _butterfly(s)


def fit_c(w, r, a):
    n_exp, n_pix = w.shape
    num, den = np.zeros(n_pix, dtype=w.dtype), np.zeros(n_pix, dtype=w.dtype)
    for e in range(n_exp):
        live = w[e] > 0
        t = w[e] * r[e]
        t = t * a[e]
        num = np.where(live, num + t, num)
        q = a[e] * a[e]
        q = w[e] * q
        den = np.where(live, den + q, den)
    return np.where(den > 0, num / np.where(den > 0, den, 1), 0).astype(w.dtype)


def fit_a(w, r, c):
    """a[n_exp] of fit_a(c) before the normalisation."""
    live = w > 0
    t = w * r
    t = t * c[None, :]
    num = row_sum(np.where(live, t, 0).astype(w.dtype))
    q = c * c
    q = w * q[None, :]
    den = row_sum(np.where(live, q, 0).astype(w.dtype))
    return np.where(den > 0, num / np.where(den > 0, den, 1), 0).astype(w.dtype)


def norm_of(a):
    s = a.dtype.type(0)
    for e in range(len(a)):
        s = s + a[e] * a[e]
    return np.sqrt(s)


def _sysrem(D, ivar, n_comp, n_iter, ones, dtype):
    D = np.asarray(D, dtype=np.float64)
    n_exp, n_pix = D.shape
    assert n_comp >= 0 and 1 <= n_comp + bool(ones) <= 16 and n_iter >= 1 and n_exp <= MAX_EXP
    w, r = weights_of(D, ivar, dtype)
    one = dtype(1)
    cols = []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        if ones:
            a = np.ones(n_exp, dtype=dtype)
            c = fit_c(w, r, a)
            r = np.where(w > 0, r - a[:, None] * c[None, :], r)
            cols.append(a)
        for _ in range(n_comp):
            a = np.full(n_exp, one / np.sqrt(dtype(n_exp)), dtype=dtype)
            c = fit_c(w, r, a)
            ended = False
            for _ in range(n_iter):
                a = fit_a(w, r, c)
                norm = norm_of(a)
                if not norm > 0:
                    ended = True
                    break
                a = a / norm
                c = fit_c(w, r, a)
            if ended:
                cols.append(np.zeros(n_exp, dtype=dtype))
                continue
            r = np.where(w > 0, r - a[:, None] * c[None, :], r)
            cols.append(a)
    U = np.ascontiguousarray(np.stack(cols, axis=1))
    return U, np.where(w > 0, r, D.astype(dtype))


def sysrem_f64(D, ivar, n_comp, n_iter=30, ones=False):
    """(U [n_exp][n_comp + ones], cleaned [n_exp][n_pix]) of D and ivar in the device's pixel order: the definition,
    rounding for rounding."""
    return _sysrem(D, ivar, int(n_comp), int(n_iter), bool(ones), np.float64)


def sysrem_ld(D, ivar, n_comp, n_iter=30, ones=False):
    """The same in longdouble."""
    return _sysrem(D, ivar, int(n_comp), int(n_iter), bool(ones), LD)


# ---- designs shared by the CPU and the GPU tests -------------------------------------------------------------------
def planted(n_exp, n_pix, seed):
    """(D, ivar) with planted, well-separated systematics: three rank-one terms of amplitude 1, 0.3 and 0.1 on a unit
    continuum and noise of 1e-3, with a few entries masked through NaN data or ivar = 0."""
    rng = np.random.default_rng(seed)
    D = 1.0 + 1e-3 * rng.normal(size=(n_exp, n_pix))
    for amp in (1.0, 0.3, 0.1):
        a, c = rng.normal(size=n_exp), rng.normal(size=n_pix)
        D = D + amp * (a / np.sqrt((a * a).mean()))[:, None] * (c / np.sqrt((c * c).mean()))[None, :]
    ivar = np.full((n_exp, n_pix), 1e6)
    hole = rng.random((n_exp, n_pix))
    D[hole < 0.01] = np.nan
    ivar[(hole > 0.01) & (hole < 0.02)] = 0.0
    return D, ivar


def distance(cleaned, cleaned_ld, w):
    """d(x) = max |cleaned_x - cleaned_ld| over the weighted entries."""
    live = np.asarray(w) > 0
    return float(np.max(np.abs(np.asarray(cleaned, dtype=LD)[live] - np.asarray(cleaned_ld, dtype=LD)[live])))


def margin(D, n_pix):
    """The floor of the accuracy yardstick: n_pix 2^-53 max |D| over the finite entries."""
    return n_pix * 2.0 ** -53 * float(np.nanmax(np.abs(np.where(np.isfinite(D), D, np.nan))))


PLANET_TRIAL = 6        # j*: the injected trial of the planted planet (Vsys = +20 km/s)
PLANET_CFG = dict(orbphase_border=0.02, orbphase_steps=3)


def planet_design(planet, orb, seed=4):
    """The planted-planet design on the reduced C1 problem: 12 exposures, 400 pixels about Na D2 and D1 in two
    interleaved orders given in descending wavelength, 9 trials in Vsys at the planet's Kp, raw data with a blaze per
    order, two planted systematics (an airmass-like trend times a telluric-like pattern, a drift times a slope) and
    noise of 2e-4.  The planet is not in ``raw``: the pipelines inject trial PLANET_TRIAL at scale 1."""
    from prometheus_amd import constants as const
    from prometheus_amd import observation as obs
    n_exp, n_pix = 12, 400
    px = 5889.0e-8 + 2e-10 * np.arange(n_pix)
    orders = ((np.arange(n_pix) // 5) % 2)[::-1].copy()
    ins = obs.Instrument(px[::-1], resolving_power=140000.0, truncate=5.0)
    base = obs.planet_frame_shifts(planet, orb)
    Kp = np.sqrt(const.G * planet.hostStar.M / planet.a)
    mid = np.linspace(orb[0], orb[-1], n_exp + 2)[1:-1]
    width = np.full(n_exp, 0.25 * (orb[1] - orb[0]))
    vsys = 1e5 * np.linspace(-40.0, 40.0, 9)
    rows, a, F = obs.exposure_taps(orb, base, mid, width, n_sub=2, Kp=[Kp], Vsys=vsys)
    rng = np.random.default_rng(seed)
    x = np.linspace(-1.0, 1.0, n_pix)
    blaze = np.where(orders == 0, 1.0 + 0.2 * x, 0.8 - 0.1 * x * x)
    airmass = 1.0 + 0.5 * np.linspace(-1.0, 1.0, n_exp) ** 2
    telluric = 0.05 * np.exp(-0.5 * ((np.arange(n_pix)[:, None] - np.array([60, 170, 310])[None, :]) / 3.0) ** 2).sum(1)
    drift = np.linspace(-1.0, 1.0, n_exp)
    raw = blaze[None, :] * (1.0 - airmass[:, None] * telluric[None, :]) * (1.0 + 0.01 * drift[:, None] * x[None, :])
    raw = raw * (1.0 + 2e-4 * rng.normal(size=(n_exp, n_pix)))
    err = np.full((n_exp, n_pix), 2e-4) * raw
    raw[3, 7] = np.nan
    return dict(ins=ins, orders=orders, rows=rows, a=a, F=F, raw=raw, err=err, taps=obs.gaussian_taps(8.0),
                mode="divide", n_comp=2, ones=True, n_iter=30, n_exp=n_exp, n_pix=n_pix)


def numpy_recovery(d, model, cleaned, Ub):
    """The summed log-likelihood per trial of the models model[n_exp][n_trial][n_pix] (caller's pixel order) against
    the cleaned data with the basis Ub, all in numpy: high_pass, the filter of Ub, the moments, VelocityMap.loglike."""
    from helpers import detrend_ref as dref
    from prometheus_amd import observation as obs
    ins = d["ins"]
    ex = obs.Exposures(ins, d["rows"], d["a"], d["F"], cleaned, d["err"])
    M = obs.high_pass(model, d["taps"], orders=d["orders"], mode=d["mode"])
    W = obs.filter_weights(Ub, ex.ivar)
    Mf, _ = dref.filter_f64(ins.sort(M), Ub, W)
    mom, nu, _ = dref.moments_ld(Mf, ex.data, ex.ivar)
    vm = obs.VelocityMap(mom.astype(np.float64), nu, d["F"])
    return vm.loglike.sum(axis=0)
