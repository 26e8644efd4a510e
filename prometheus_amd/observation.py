"""Observing a transit spectrum: the instrument's line-spread function, the detector's pixels, chi-square.

The model grid is far finer than any detector (0.001 A in the line cores).  Before R meets data it is convolved
with the spectrograph's Gaussian line-spread function and sampled on the detector's pixels, often in the planet's
rest frame (one Doppler factor per phase), and a chi-square is formed.  Here that runs on the device over R as it
stays in HBM after the run (prom_transit_observe; the definition is in include/prom_hip.h): a likelihood evaluation
brings back a few numbers per phase, or a pixel spectrum far smaller than R.  The host forms the O(n_pix) pixel
tables and combines the partial sums of wavelength shards and chunks.
"""
from __future__ import annotations

import math

import numpy as np

FWHM_PER_SIGMA = 2.0 * math.sqrt(2.0 * math.log(2.0))


class Instrument:
    """Detector pixels and the Gaussian line-spread function at each of them.

    ``pixels``: pixel centres in cm, in any order (echelle orders overlap): they are sorted for the device and
    results come back in the caller's order.  The width is ``sigma`` (cm, scalar or per pixel) or follows from
    ``resolving_power`` (scalar or per pixel) as sigma = pixel / (resolving_power 2 sqrt(2 ln 2)).  The pixel's own
    width is not modelled: fold it into sigma.  ``truncate``: the support of the kernel in units of sigma."""

    def __init__(self, pixels, resolving_power=None, sigma=None, truncate: float = 5.0):
        px = np.array(pixels, dtype=np.float64).reshape(-1)
        if (resolving_power is None) == (sigma is None):
            raise ValueError("Instrument: give resolving_power or sigma")
        if sigma is None:
            sg = px / (np.asarray(resolving_power, dtype=np.float64) * FWHM_PER_SIGMA)
        else:
            sg = np.asarray(sigma, dtype=np.float64)
        sg = np.array(np.broadcast_to(sg, px.shape), dtype=np.float64)
        if not (np.all(np.isfinite(px)) and np.all(np.isfinite(sg)) and np.all(sg > 0)):
            raise ValueError("Instrument: pixels must be finite and sigma positive")
        if not (truncate > 0 and math.isfinite(truncate)):
            raise ValueError("Instrument: truncate must be positive")
        self.pixels, self.sigma, self.truncate = px, sg, float(truncate)
        self.order = np.argsort(px, kind="stable")
        self.lam = np.ascontiguousarray(px[self.order])   # what the device sees
        self.sig = np.ascontiguousarray(sg[self.order])

    @property
    def n_pix(self) -> int:
        return len(self.pixels)

    def sort(self, a):
        """[..., n_pix] in the caller's pixel order -> the device's (ascending) order."""
        return np.ascontiguousarray(np.asarray(a, dtype=np.float64)[..., self.order])

    def unsort(self, a):
        """[..., n_pix] in the device's order -> the caller's."""
        a = np.asarray(a)
        out = np.empty_like(a)
        out[..., self.order] = a
        return out

    def full_weight(self, frame=None):
        """The integral of the truncated kernel, sigma sqrt(2 pi) erf(k / sqrt 2) per pixel ([n_pix], or
        [n_orb][n_pix] with the phases' frame factors): den of a pixel whose support the grid covers densely."""
        s = self.sigma if frame is None else np.asarray(frame, dtype=np.float64)[:, None] * self.sigma[None, :]
        return s * (math.sqrt(2.0 * math.pi) * math.erf(self.truncate / math.sqrt(2.0)))


class Observation:
    """What stays resident on the device between likelihood evaluations: the instrument's pixels, the phases' frame
    factors ``frame_shifts`` [n_orb] (None: the model's own frame) and ``data`` with its standard error ``err``
    ([n_orb][n_pix] in the caller's pixel order, or anything that broadcasts to it; a pixel with non-finite data or
    err, or err <= 0, is masked).  Sorting, the inverse variances and the content key that lets a device skip the
    upload are computed once here: a retrieval loop builds one Observation and hands it to every Transit.observe
    call, which then neither hashes nor uploads the data again.  The arrays are copied: later changes to the
    caller's arrays need a new Observation."""

    def __init__(self, instrument: Instrument, n_orb: int, frame_shifts=None, data=None, err=None):
        from .gasProperties import _content_fingerprint
        self.instrument, self.n_orb = instrument, int(n_orb)
        self.f = None
        if frame_shifts is not None:
            self.f = np.array(frame_shifts, dtype=np.float64)
            if self.f.shape != (self.n_orb,):
                raise ValueError("Observation: frame_shifts must have one factor per orbital phase")
        if (data is None) != (err is None):
            raise ValueError("Observation: data and err come together")
        self.data = self.ivar = None
        if data is not None:
            shape = (self.n_orb, instrument.n_pix)
            self.data = instrument.sort(np.broadcast_to(np.asarray(data, dtype=np.float64), shape))
            e = instrument.sort(np.broadcast_to(np.asarray(err, dtype=np.float64), shape))
            with np.errstate(divide="ignore", invalid="ignore"):
                self.ivar = np.where(np.isfinite(e) & (e > 0), 1.0 / (e * e), 0.0)
        arrays = [instrument.lam, instrument.sig] + [a for a in (self.f, self.data, self.ivar) if a is not None]
        self.key = (self.n_orb, instrument.truncate, self.f is None, self.data is None) + _content_fingerprint(*arrays)


class Exposures:
    """Data at any phase, smeared over its duration: what stays resident on the device between Transit.expose calls.
    An exposure is a weighted sum of taps; a tap is a row of the model's R read at a factor (include/prom_hip.h,
    "exposures on the device").  ``rows`` and ``weights`` are [n_exp][n_tap] (rows: indices into the model's phase
    axis; a tap of weight 0 is padding and is skipped), ``factors`` [n_exp][n_trial][n_tap], or [n_exp][n_tap] for one
    trial (exposure_taps makes all three), ``data`` and its standard error ``err`` [n_exp][n_pix] in the caller's
    pixel order, or anything that broadcasts to it (a pixel with non-finite data or err, or err <= 0, is masked).
    Sorting, the inverse variances and the content key that lets a device skip the upload are computed once here.
    The arrays are copied.  ValueError for a bad shape or value; that the rows lie inside the transit's phases is
    checked by Transit.expose."""

    def __init__(self, instrument: Instrument, rows, weights, factors, data, err):
        from .gasProperties import _content_fingerprint
        self.instrument = instrument
        r = np.asarray(rows)
        if r.ndim != 2 or r.shape[0] < 1 or r.shape[1] < 1:
            raise ValueError("Exposures: rows must be [n_exp][n_tap] with n_exp, n_tap >= 1")
        if not (np.issubdtype(r.dtype, np.integer) or (np.issubdtype(r.dtype, np.floating) and np.all(r == np.rint(r)))):
            raise ValueError("Exposures: rows must be integers")
        if np.any(r < 0) or np.any(r > 65534):
            raise ValueError("Exposures: rows must lie in [0, n_orb)")
        self.rows = np.ascontiguousarray(r, dtype=np.int32)
        self.n_exp, self.n_tap = self.rows.shape
        a = np.array(weights, dtype=np.float64)
        if a.shape != self.rows.shape:
            raise ValueError("Exposures: weights must be [n_exp][n_tap] like rows")
        if not (np.all(np.isfinite(a)) and np.all(a >= 0)):
            raise ValueError("Exposures: weights must be finite and >= 0")
        self.weights = np.ascontiguousarray(a)
        F = np.array(factors, dtype=np.float64)
        if F.ndim == 2:
            F = F[:, None, :]
        if F.ndim != 3 or F.shape[0] != self.n_exp or F.shape[2] != self.n_tap or F.shape[1] < 1:
            raise ValueError("Exposures: factors must be [n_exp][n_trial][n_tap] (or [n_exp][n_tap] for one trial)")
        if not (np.all(np.isfinite(F)) and np.all(F > 0)):
            raise ValueError("Exposures: factors must be finite and positive")
        self.factors = np.ascontiguousarray(F)
        self.n_trial = F.shape[1]
        if data is None or err is None:
            raise ValueError("Exposures: data and err are needed")
        shape = (self.n_exp, instrument.n_pix)
        try:
            d = np.broadcast_to(np.asarray(data, dtype=np.float64), shape)
            e = np.broadcast_to(np.asarray(err, dtype=np.float64), shape)
        except ValueError:
            raise ValueError("Exposures: data and err must be [n_exp][n_pix] = [%d][%d]" % shape) from None
        self.data = instrument.sort(d)
        e = instrument.sort(e)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.ivar = np.where(np.isfinite(e) & (e > 0), 1.0 / (e * e), 0.0)
        self.key = ("exposures", instrument.truncate) + _content_fingerprint(
            instrument.lam, instrument.sig, self.rows, self.weights, self.factors, self.data, self.ivar)
        self._pixels = {}

    def pixels(self, n_orb: int) -> "Observation":
        """The Observation that carries only the pixels, for a model of n_orb phases (made once per n_orb)."""
        if n_orb not in self._pixels:
            self._pixels[n_orb] = Observation(self.instrument, n_orb)
        return self._pixels[n_orb]


def _weights_of(data, err):
    """(data with masked entries 0, inverse variances with masked entries 0) of data and its standard error."""
    d = np.asarray(data, dtype=np.float64)
    e = np.broadcast_to(np.asarray(err, dtype=np.float64), d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ok = np.isfinite(d) & np.isfinite(e) & (e > 0)
        return np.where(ok, d, 0.0), np.where(ok, 1.0 / (e * e), 0.0)


def sysrem(data, err, n_comp: int, n_iter: int = 30, ones: bool = False, orders=None):
    """SYSREM (Tamuz, Mazeh & Zucker 2005) on the host, once per data set: ``n_comp`` times the weighted rank-one fit
    a[e] c[p] that minimises sum (r - a c)^2 / err^2 over the residuals r is found by ``n_iter`` alternating
    least-squares steps (c from a, then a from c; a starts at ones and is scaled to unit length, the scale going to
    c) and subtracted.  ``data`` and ``err`` are [n_exp][n_pix] (err anything that broadcasts); an entry with
    non-finite data or err, or err <= 0, has no weight.  Returns (U [n_exp][n_comp], the cleaned data, masked entries
    as they came).  With ``ones`` every pixel's weighted mean over the exposures is removed first and U gets a leading
    column of ones for it: U is then [n_exp][n_comp + 1].  U is the basis the model must be filtered with
    (filter_weights, Detrend).  With ``orders`` (an integer label per pixel, as for Orders) every echelle order is
    cleaned on its own, as every published analysis does: the call is a loop of itself over the orders' columns in
    ascending label order, U is [n_ord][n_exp][n_comp + ones] and every pixel's cleaned data come from its own
    order."""
    d0 = np.asarray(data, dtype=np.float64)
    if d0.ndim != 2 or d0.shape[0] < 1:
        raise ValueError("sysrem: data must be [n_exp][n_pix]")
    if orders is not None:
        members = _order_members(orders, d0.shape[1], "sysrem")
        try:
            e0 = np.broadcast_to(np.asarray(err, dtype=np.float64), d0.shape)
        except ValueError:
            raise ValueError("sysrem: err must broadcast to data") from None
        cleaned = np.array(d0)
        Us = []
        for idx in members:
            U, cl = sysrem(d0[:, idx], e0[:, idx], n_comp, n_iter, ones)
            Us.append(U)
            cleaned[:, idx] = cl
        return np.ascontiguousarray(np.stack(Us)), cleaned
    n_comp, n_iter = int(n_comp), int(n_iter)
    if n_comp < 0 or n_iter < 1 or n_comp + bool(ones) < 1:
        raise ValueError("sysrem: n_comp >= 1 (0 with ones) and n_iter >= 1")
    try:
        r, iv = _weights_of(d0, err)
    except ValueError:
        raise ValueError("sysrem: err must broadcast to data") from None
    cols = []

    def fit_c(a):
        den = (iv * (a * a)[:, None]).sum(axis=0)
        return np.where(den > 0, (iv * r * a[:, None]).sum(axis=0) / np.where(den > 0, den, 1.0), 0.0)

    if ones:
        a = np.ones(d0.shape[0])
        r = r - a[:, None] * fit_c(a)[None, :]
        cols.append(a)
    for _ in range(n_comp):
        a = np.ones(d0.shape[0]) / np.sqrt(d0.shape[0])
        c = fit_c(a)
        for _ in range(n_iter):
            den = (iv * (c * c)[None, :]).sum(axis=1)
            a = np.where(den > 0, (iv * r * c[None, :]).sum(axis=1) / np.where(den > 0, den, 1.0), 0.0)
            norm = np.sqrt((a * a).sum())
            if not norm > 0:
                break
            a = a / norm
            c = fit_c(a)
        r = r - a[:, None] * c[None, :]
        cols.append(a)
    return np.ascontiguousarray(np.stack(cols, axis=1)), np.where(iv > 0, r, d0)


def filter_weights(U, ivar, orders=None) -> np.ndarray:
    """W[n_comp][n_exp][n_pix] of the basis U[n_exp][n_comp] under the inverse variances ivar[n_exp][n_pix]: at pixel
    p, W_p = (U^T L_p U)^-1 U^T L_p with L_p = diag(ivar[:, p]), the weighted least-squares pseudo-inverse, so that
    m' = m - U (W_p m) removes from a column m what a fit of the basis finds in it.  Entries with ivar = 0 (or not
    finite, or < 0) are exactly 0.  A pixel whose normal matrix U^T L_p U is singular (its smallest eigenvalue not
    above n_comp 2^-52 times its largest: too few weighted exposures, or dependent columns) gets W = 0: it is then
    filtered by nothing and stays usable.  With ``orders`` (an integer label per pixel, as for Orders) U is
    [n_ord][n_exp][n_comp], a basis per order in ascending label order, and a pixel's W is formed with its own order's
    basis: a loop of this function over the orders' columns."""
    U = np.asarray(U, dtype=np.float64)
    iv = np.asarray(ivar, dtype=np.float64)
    if orders is not None:
        if iv.ndim != 2:
            raise ValueError("filter_weights: ivar must be [n_exp][n_pix]")
        members = _order_members(orders, iv.shape[1], "filter_weights")
        if U.ndim != 3 or U.shape[0] != len(members) or U.shape[2] < 1 or U.shape[1] != iv.shape[0]:
            raise ValueError("filter_weights: with orders U must be [n_ord][n_exp][n_comp] = [%d][%d][n_comp]"
                             % (len(members), iv.shape[0]))
        W = np.zeros((U.shape[2], iv.shape[0], iv.shape[1]))
        for s, idx in enumerate(members):
            W[:, :, idx] = filter_weights(U[s], iv[:, idx])
        return W
    if U.ndim != 2 or U.shape[1] < 1 or iv.ndim != 2 or iv.shape[0] != U.shape[0]:
        raise ValueError("filter_weights: U must be [n_exp][n_comp] and ivar [n_exp][n_pix]")
    if not np.all(np.isfinite(U)):
        raise ValueError("filter_weights: U must be finite")
    n_exp, K = U.shape
    with np.errstate(invalid="ignore"):
        iv = np.where(np.isfinite(iv) & (iv > 0), iv, 0.0)
    B = U.T[None, :, :] * iv.T[:, None, :]                     # [n_pix][K][n_exp]: U^T L_p
    N = B @ U                                                  # [n_pix][K][K]
    lam = np.linalg.eigvalsh(N)
    good = np.isfinite(lam).all(axis=1) & (lam[:, 0] > K * 2.0 ** -52 * lam[:, -1])
    W = np.zeros((iv.shape[1], K, n_exp))
    if good.any():
        W[good] = np.linalg.solve(N[good], B[good])
    W[~np.isfinite(W).all(axis=(1, 2))] = 0.0
    W = np.ascontiguousarray(W.transpose(1, 2, 0))
    W[:, iv == 0.0] = 0.0
    return W


class Detrend:
    """The filter of Transit.expose(detrend=...): the basis ``U`` [n_exp][n_comp] (1 <= n_comp <= 16) the data of
    ``exposures`` were cleaned with (sysrem) and its pseudo-inverse per pixel ``W`` [n_comp][n_exp][n_pix] in the
    caller's pixel order (None: filter_weights with the exposures' inverse variances).  The model of every trial is
    filtered per pixel column, m' = m - U (W_p m), before it meets the data (include/prom_hip.h, "detrended exposures
    on the device").  Sorting W into the device's pixel order and the content key that lets a device skip the upload
    are computed once here; the arrays are copied.  ValueError for a bad shape or a non-finite value.

    With ``on_device`` no W is formed or kept on the host (``W`` is then None, and giving one is a ValueError): the
    device forms it from U and the exposures' inverse variances when the filter is uploaded (include/prom_hip.h, "the
    filter's weights on the device"; a Cholesky rule of the device's own, which agrees with filter_weights to
    rounding on pixels that are not borderline), and the key is made of the exposures' key and U's fingerprint.

    With ``orders`` (an observation.Orders made for the same exposures) the filter has a basis per echelle order, as
    Transit.clean(sysrem_orders=...) returns it: ``U`` is [n_ord][n_exp][n_comp] in the Orders' order of labels, and
    every pixel is filtered with the basis of its own order (include/prom_hip.h, "SYSREM per order on the device").
    ``W`` keeps its shape; None forms it with filter_weights(orders=...), or on the device with ``on_device``."""

    MAX_COMP = 16

    def __init__(self, exposures: Exposures, U, W=None, on_device: bool = False, orders=None):
        from .gasProperties import _content_fingerprint
        if not isinstance(exposures, Exposures):
            raise TypeError("Detrend: exposures must be an observation.Exposures")
        self.orders = orders
        if orders is not None:
            return self._init_per_order(exposures, U, W, bool(on_device), orders)
        u = np.array(U, dtype=np.float64)
        if u.ndim != 2 or u.shape[0] != exposures.n_exp:
            raise ValueError("Detrend: U must be [n_exp][n_comp] with n_exp = %d" % exposures.n_exp)
        if not 1 <= u.shape[1] <= self.MAX_COMP:
            raise ValueError("Detrend: n_comp must lie in [1, %d]" % self.MAX_COMP)
        if not np.all(np.isfinite(u)):
            raise ValueError("Detrend: U must be finite")
        self.U = np.ascontiguousarray(u)
        self.n_exp, self.n_comp = self.U.shape
        self.on_device = bool(on_device)
        self.exposures_key = exposures.key
        if self.on_device:
            if W is not None:
                raise ValueError("Detrend: on_device forms W on the device; give no W")
            self.W = None
            self.key = ("detrend on device", exposures.key) + _content_fingerprint(self.U)
            return
        shape = (self.n_comp, self.n_exp, exposures.instrument.n_pix)
        if W is None:
            w = filter_weights(self.U, exposures.ivar)          # (the exposures' ivar is in the device's order)
        else:
            w = np.asarray(W, dtype=np.float64)
            if w.shape != shape:
                raise ValueError("Detrend: W must be [n_comp][n_exp][n_pix] = [%d][%d][%d]" % shape)
            w = exposures.instrument.sort(w)
        if not np.all(np.isfinite(w)):
            raise ValueError("Detrend: W must be finite")
        self.W = np.ascontiguousarray(w)                        # what the device sees
        self.key = ("detrend", exposures.key) + _content_fingerprint(self.U, self.W)

    def _init_per_order(self, exposures, U, W, on_device, orders):
        from .gasProperties import _content_fingerprint
        if not isinstance(orders, Orders):
            raise TypeError("Detrend: orders must be an observation.Orders")
        if orders.exposures_key != exposures.key:
            raise ValueError("Detrend: the Orders were made for other exposures (another table, pixels or data)")
        u = np.array(U, dtype=np.float64)
        if u.ndim != 3 or u.shape[:2] != (orders.n_seg, exposures.n_exp):
            raise ValueError("Detrend: with orders U must be [n_ord][n_exp][n_comp] = [%d][%d][n_comp]"
                             % (orders.n_seg, exposures.n_exp))
        if not 1 <= u.shape[2] <= self.MAX_COMP:
            raise ValueError("Detrend: n_comp must lie in [1, %d]" % self.MAX_COMP)
        if not np.all(np.isfinite(u)):
            raise ValueError("Detrend: U must be finite")
        self.U = np.ascontiguousarray(u)
        _, self.n_exp, self.n_comp = self.U.shape
        self.on_device = on_device
        self.exposures_key = exposures.key
        n_pix = exposures.instrument.n_pix
        self.seg_of = np.zeros(n_pix, dtype=np.int32)           # the order of every device pixel
        for s in range(orders.n_seg):
            self.seg_of[orders.perm[orders.seg_first[s]:orders.seg_first[s + 1]]] = s
        if on_device:
            if W is not None:
                raise ValueError("Detrend: on_device forms W on the device; give no W")
            self.W = None
            self.key = ("detrend per order on device", orders.key) + _content_fingerprint(self.U)
            return
        shape = (self.n_comp, self.n_exp, n_pix)
        if W is None:
            w = filter_weights(self.U, exposures.ivar, orders=self.seg_of)   # (ivar and seg_of: the device's order)
        else:
            w = np.asarray(W, dtype=np.float64)
            if w.shape != shape:
                raise ValueError("Detrend: W must be [n_comp][n_exp][n_pix] = [%d][%d][%d]" % shape)
            w = exposures.instrument.sort(w)
        if not np.all(np.isfinite(w)):
            raise ValueError("Detrend: W must be finite")
        self.W = np.ascontiguousarray(w)
        self.key = ("detrend per order", orders.key) + _content_fingerprint(self.U, self.W)


MAX_HALF_WIDTH = 512   # of a high-pass' taps (the device's rolling window)


def gaussian_taps(sigma_pix: float, truncate: float = 4.0) -> np.ndarray:
    """Taps g[half_width + 1] of a Gaussian running mean along the pixels: g[d] = exp(-d^2 / (2 sigma_pix^2)) at
    distance d, cut at half_width = int(truncate sigma_pix + 1/2) <= 512.  g[0] = 1; the filter normalises by the
    weights it meets, so the taps need no norm."""
    sigma_pix, truncate = float(sigma_pix), float(truncate)
    if not (math.isfinite(sigma_pix) and sigma_pix > 0 and math.isfinite(truncate) and truncate >= 0):
        raise ValueError("gaussian_taps: sigma_pix must be positive and truncate >= 0")
    h = int(truncate * sigma_pix + 0.5)
    if h > MAX_HALF_WIDTH:
        raise ValueError("gaussian_taps: half width %d exceeds %d pixels" % (h, MAX_HALF_WIDTH))
    d = np.arange(h + 1, dtype=np.float64)
    return np.exp(-0.5 * (d / sigma_pix) ** 2)


def box_taps(half_width: int) -> np.ndarray:
    """Taps of a box running mean over 2 half_width + 1 pixels: ones[half_width + 1], half_width in [0, 512]."""
    h = int(half_width)
    if h != half_width or not 0 <= h <= MAX_HALF_WIDTH:
        raise ValueError("box_taps: half_width must be an integer in [0, %d]" % MAX_HALF_WIDTH)
    return np.ones(h + 1)


class MedianWindow:
    """The window of a running median high-pass: ``half_width`` positions either side of a pixel.  Given wherever
    taps are: high_pass(a, median_window(h), ...) and HighPass(exposures, median_window(h), ...)."""

    def __init__(self, half_width: int):
        if isinstance(half_width, (bool, np.bool_)) or not isinstance(half_width, (int, np.integer)):
            raise ValueError("median_window: half_width must be an integer in [0, %d]" % MAX_HALF_WIDTH)
        if not 0 <= int(half_width) <= MAX_HALF_WIDTH:
            raise ValueError("median_window: half_width must be an integer in [0, %d]" % MAX_HALF_WIDTH)
        self.half_width = int(half_width)

    def __repr__(self):
        return "MedianWindow(%d)" % self.half_width


def median_window(half_width: int) -> MedianWindow:
    """A running median over 2 half_width + 1 pixels, half_width an integer in [0, 512] (ValueError otherwise), in the
    place of taps: the continuum is then the median of the values within half_width positions that are not NaN."""
    return MedianWindow(half_width)


def _median_keys(x):
    """The order-preserving integer keys of float64 x (-0 below +0, the infinities ordinary values); a NaN gets the
    largest key of all."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    return np.where(np.isnan(x), ~np.uint64(0), np.where(b >> np.uint64(63) != 0, ~b, b | top))


def _median_values(k):
    top = np.uint64(1) << np.uint64(63)
    return np.where(k & top != 0, k ^ top, ~k).astype(np.uint64).view(np.float64)


def _running_median(x, h):
    """B of the definition (include/prom_hip.h, "median high-pass on the device") along the last axis of x[..., n]:
    the windows clipped at the ends, NaN skipped, the values in the order of their integer keys; NaN where the
    window holds no value."""
    n = x.shape[-1]
    rows = x.reshape(-1, n)
    B = np.empty_like(rows)
    h = min(h, max(n - 1, 0))                                    # (a wider window holds nothing more)
    for r, row in enumerate(rows):
        keys = np.full(n + 2 * h, ~np.uint64(0), dtype=np.uint64)
        keys[h:h + n] = _median_keys(row)
        win = np.sort(np.lib.stride_tricks.sliding_window_view(keys, 2 * h + 1), axis=-1)      # [n][2 h + 1]
        c = (win != ~np.uint64(0)).sum(axis=-1)
        pick = lambda k: _median_values(np.take_along_axis(win, np.maximum(k, 0)[:, None], axis=-1)[:, 0])
        lo, hi = pick((c - 1) // 2), pick(c // 2)
        with np.errstate(invalid="ignore", over="ignore"):
            B[r] = np.where(c == 0, np.nan, np.where(c % 2 == 1, lo, (lo + hi) * 0.5))
    return B.reshape(x.shape)


def _check_taps(taps, who) -> np.ndarray:
    g = np.array(taps, dtype=np.float64)
    if g.ndim != 1 or not 1 <= len(g) <= MAX_HALF_WIDTH + 1:
        raise ValueError("%s: taps must be [half_width + 1] with half_width in [0, %d]" % (who, MAX_HALF_WIDTH))
    if not (np.all(np.isfinite(g)) and np.all(g >= 0) and g[0] > 0):
        raise ValueError("%s: taps must be finite and >= 0, the first > 0" % who)
    return g


def _check_mode(mode, who) -> int:
    if mode not in ("subtract", "divide"):
        raise ValueError("%s: mode must be 'subtract' or 'divide'" % who)
    return 0 if mode == "subtract" else 1


def _order_members(orders, n_pix, who):
    """The pixels of every order, in the caller's order, as a list of index arrays (ascending label)."""
    if orders is None:
        return [np.arange(n_pix)]
    o = np.asarray(orders)
    if o.shape != (n_pix,):
        raise ValueError("%s: orders must hold one label per pixel" % who)
    if not (np.issubdtype(o.dtype, np.integer) or (np.issubdtype(o.dtype, np.floating) and np.all(o == np.rint(o)))):
        raise TypeError("%s: orders must be integer labels" % who)
    o = o.astype(np.int64)
    return [np.flatnonzero(o == label) for label in np.unique(o)]


def high_pass(a, taps, orders=None, mode: str = "subtract") -> np.ndarray:
    """The high-pass of Transit.expose(highpass=...) in numpy, over a[..., n_pix] in the caller's pixel order: what a
    user runs on the data before sysrem.  ``orders``: an integer label per pixel (None: one order); a pixel's position
    inside its order is its rank among that order's pixels.  At every position the running mean B over the positions
    within half_width = len(taps) - 1 of it, weighted with taps[distance] and normalised by the weights of the
    values that are not NaN, is subtracted from the value or divided out of it; NaN stays NaN.  The sums run in
    ascending position and every product and sum is rounded on its own, which is the device's definition
    (include/prom_hip.h, "high-pass filtered exposures on the device") bit for bit.  With a median_window in the place
    of taps B is the running median of the values that are not NaN in the same window (the mean of the two middle
    ones when their count is even), in the order that puts -0 below +0: "median high-pass on the device" there, bit for
    bit."""
    median = isinstance(taps, MedianWindow)
    g = None if median else _check_taps(taps, "high_pass")
    m = _check_mode(mode, "high_pass")
    a = np.asarray(a, dtype=np.float64)
    if a.ndim < 1:
        raise ValueError("high_pass: a must be [..., n_pix]")
    out = np.empty_like(a)
    if median:
        for idx in _order_members(orders, a.shape[-1], "high_pass"):
            x = a[..., idx]
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                B = _running_median(x, taps.half_width)
                out[..., idx] = x - B if m == 0 else x / B
        return out
    h = len(g) - 1
    for idx in _order_members(orders, a.shape[-1], "high_pass"):
        x = a[..., idx]
        n = len(idx)
        num, den = np.zeros_like(x), np.zeros_like(x)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            for d in range(-min(h, n - 1), min(h, n - 1) + 1):        # i' = i + d, ascending
                lo, hi = max(0, -d), min(n, n - d)                    # the outputs i with 0 <= i + d < n
                src = x[..., lo + d:hi + d]
                ok = ~np.isnan(src)
                num[..., lo:hi] = np.where(ok, num[..., lo:hi] + g[abs(d)] * src, num[..., lo:hi])
                den[..., lo:hi] = np.where(ok, den[..., lo:hi] + g[abs(d)], den[..., lo:hi])
            B = num / den
            out[..., idx] = x - B if m == 0 else x / B
    return out


class HighPass:
    """The high-pass of Transit.expose(highpass=...): every exposure's model is filtered along the pixels of each
    order as high_pass filters data, on the device, before the SYSREM filter (if any) and the moments.  ``taps``:
    gaussian_taps, box_taps or any [half_width + 1] weights (finite, >= 0, the first > 0, half_width <= 512), or a
    median_window for a running median (``kind`` is then "median" and ``taps`` None, otherwise "mean");
    ``orders``: an integer label per pixel of ``exposures`` in the caller's order (None: one order); ``mode``:
    'subtract' or 'divide'.  The segments in the device's pixel order (``seg_first``, ``perm``) and the content key that
    lets a device skip the upload are computed once here; the arrays are copied.  ValueError / TypeError for bad
    arguments."""

    def __init__(self, exposures: Exposures, taps, orders=None, mode: str = "subtract"):
        from .gasProperties import _content_fingerprint
        if not isinstance(exposures, Exposures):
            raise TypeError("HighPass: exposures must be an observation.Exposures")
        if isinstance(taps, MedianWindow):
            self.kind, self.taps, self.half_width = "median", None, taps.half_width
        else:
            self.kind, self.taps = "mean", np.ascontiguousarray(_check_taps(taps, "HighPass"))
            self.half_width = len(self.taps) - 1
        self.mode = mode
        self.mode_id = _check_mode(mode, "HighPass")
        ins = exposures.instrument
        members = _order_members(orders, ins.n_pix, "HighPass")
        self.orders = None if orders is None else np.array(orders, dtype=np.int64)
        where = np.empty(ins.n_pix, dtype=np.int64)
        where[ins.order] = np.arange(ins.n_pix)                 # the device's index of the caller's pixel
        self.perm = np.ascontiguousarray(np.concatenate([where[idx] for idx in members]) if ins.n_pix
                                         else np.zeros(0), dtype=np.int32)
        if ins.n_pix:
            self.seg_first = np.concatenate([[0], np.cumsum([len(idx) for idx in members])]).astype(np.int32)
        else:
            self.seg_first = np.zeros(2, dtype=np.int32)
        self.n_seg = len(self.seg_first) - 1
        self.exposures_key = exposures.key
        if self.kind == "median":
            self.key = (("highpass", exposures.key, self.mode_id, "median", self.half_width)
                        + _content_fingerprint(self.perm, self.seg_first))
        else:
            self.key = (("highpass", exposures.key, self.mode_id)
                        + _content_fingerprint(self.taps, self.perm, self.seg_first))


class Orders:
    """The echelle orders of Transit.expose(orders=...): the moments of every (exposure, trial) are then also formed per
    order on the device (include/prom_hip.h, "per-order moments on the device").  ``orders``: an integer label per
    pixel of ``exposures`` in the caller's order, as for HighPass (None: one order); ``keep``: a bool per label in
    ascending label order, whether the order enters the totals (None: every order).  ``labels`` holds the labels in
    ascending order; the segments in the device's pixel order (``seg_first``, ``perm``) and the content key that lets
    a device skip the upload are computed once here; the arrays are copied.  The object is independent of a HighPass:
    either may be used without the other.  ValueError / TypeError for bad arguments."""

    def __init__(self, exposures: Exposures, orders, keep=None):
        from .gasProperties import _content_fingerprint
        if not isinstance(exposures, Exposures):
            raise TypeError("Orders: exposures must be an observation.Exposures")
        ins = exposures.instrument
        members = _order_members(orders, ins.n_pix, "Orders")
        self.orders = None if orders is None else np.array(orders, dtype=np.int64)
        self.labels = np.zeros(1, dtype=np.int64) if orders is None else np.unique(self.orders)
        where = np.empty(ins.n_pix, dtype=np.int64)
        where[ins.order] = np.arange(ins.n_pix)                 # the device's index of the caller's pixel
        self.perm = np.ascontiguousarray(np.concatenate([where[idx] for idx in members]) if ins.n_pix
                                         else np.zeros(0), dtype=np.int32)
        if ins.n_pix:
            self.seg_first = np.concatenate([[0], np.cumsum([len(idx) for idx in members])]).astype(np.int32)
        else:
            self.seg_first = np.zeros(2, dtype=np.int32)
            self.labels = np.zeros(1, dtype=np.int64)
        self.n_seg = len(self.seg_first) - 1
        if keep is None:
            self.keep = np.ones(self.n_seg, dtype=bool)
        else:
            k = np.asarray(keep)
            if k.shape != (self.n_seg,):
                raise ValueError("Orders: keep must hold one entry per order label (%d)" % self.n_seg)
            if not (k.dtype == bool or (np.issubdtype(k.dtype, np.integer) and np.all((k == 0) | (k == 1)))):
                raise TypeError("Orders: keep must be bool (or 0 / 1)")
            self.keep = k.astype(bool)
        self.exposures_key = exposures.key
        self.key = ("orders", exposures.key) + _content_fingerprint(self.perm, self.seg_first,
                                                                    self.keep.astype(np.uint8))


class Injection:
    """The raw exposures of Transit.clean / Transit.inject: ``raw`` [n_exp][n_pix] in the caller's pixel order, the
    data of ``exposures`` before any cleaning (any value; NaN marks a bad pixel).  A model is multiplied into them, and
    the high-pass and SYSREM run on them, on the device (include/prom_hip.h, "injection and SYSREM on the device");
    the exposures' inverse variances are the weights.  Sorting into the device's pixel order and the content key that
    lets a device skip the upload are computed once here; the array is copied.  TypeError / ValueError for bad
    arguments."""

    MAX_EXP = 4096

    def __init__(self, exposures: Exposures, raw):
        from .gasProperties import _content_fingerprint
        if not isinstance(exposures, Exposures):
            raise TypeError("Injection: exposures must be an observation.Exposures")
        try:
            d = np.array(raw, dtype=np.float64)
        except (TypeError, ValueError):
            raise TypeError("Injection: raw must be an array of numbers") from None
        shape = (exposures.n_exp, exposures.instrument.n_pix)
        if d.shape != shape:
            raise ValueError("Injection: raw must be [n_exp][n_pix] = [%d][%d]" % shape)
        if exposures.n_exp > self.MAX_EXP:
            raise ValueError("Injection: more than %d exposures" % self.MAX_EXP)
        self.exposures = exposures
        self.raw = exposures.instrument.sort(d)                 # what the device sees
        self.exposures_key = exposures.key
        self.key = ("injection", exposures.key) + _content_fingerprint(self.raw)


class Cleaned:
    """What Transit.clean / Transit.inject return: ``U`` [n_exp][n_comp + ones], the basis SYSREM found (the input of
    Detrend; with ``sysrem_orders`` [n_ord][n_exp][n_comp + ones], a basis per echelle order), ``data`` [n_exp][n_pix], the cleaned exposures in the caller's pixel order (the input of Exposures;
    entries without weight as they came), and ``injected`` (None unless asked for): the data after the injection and
    the high-pass, before SYSREM."""

    def __init__(self, U, data, injected=None):
        self.U, self.data, self.injected = U, data, injected


class CleanedGrid:
    """What Transit.inject_grid returns: ``trials`` and ``scales`` [n_inj], ``U`` [n_inj][n_exp][n_comp + ones]
    ([n_inj][n_ord][n_exp][n_comp + ones] with ``sysrem_orders``) and
    ``data`` [n_inj][n_exp][n_pix] in the caller's pixel order (None when the data were not asked for).  ``grid[b]`` is
    the Cleaned that Transit.inject returns for (trials[b], scales[b])."""

    def __init__(self, trials, scales, U, data=None):
        self.trials, self.scales, self.U, self.data = trials, scales, U, data

    def __len__(self):
        return len(self.trials)

    def __getitem__(self, b):
        b = range(len(self))[b]
        return Cleaned(self.U[b], None if self.data is None else self.data[b])


class RecoveryGrid:
    """What Transit.recover_grid returns: ``trials`` and ``scales`` [n_inj], ``moments`` [n_inj][n_exp][n_trial][7],
    ``n_used`` [n_inj][n_exp][n_trial], ``U`` [n_inj][n_exp][n_comp + ones], the exposures' ``factors`` and, when
    orders were given, ``order_totals``: one OrderTotals per injection (None otherwise).  ``grid[b]`` is the
    VelocityMap that Transit.recover returns for (trials[b], scales[b]), without a model and per-order records."""

    def __init__(self, trials, scales, moments, n_used, U, factors, order_totals=None):
        self.trials, self.scales, self.moments, self.n_used, self.U = trials, scales, moments, n_used, U
        self.factors = factors
        self.order_totals = None if order_totals is None else [OrderTotals(t) for t in order_totals]

    def __len__(self):
        return len(self.trials)

    def __getitem__(self, b):
        b = range(len(self))[b]
        vm = VelocityMap(self.moments[b], self.n_used[b], self.factors)
        if self.order_totals is not None:
            vm.by_order = None
            vm.order_totals = self.order_totals[b]
        vm.U = self.U[b]
        return vm

    def total(self, stat="chi2"):
        """The statistic (a name of VelocityMap's) summed over the exposures, per injection: [n_inj][n_trial]."""
        return np.array([self[b].total(stat) for b in range(len(self))]).reshape(len(self), self.moments.shape[2])


def injection_grid(trials, scales):
    """The cross product of ``trials`` and ``scales`` as the two flat lists of Transit.inject_grid / recover_grid,
    trial-major: entry i * len(scales) + k is (trials[i], scales[k])."""
    t = np.asarray(trials)
    s = np.asarray(scales, dtype=np.float64)
    if t.ndim != 1 or s.ndim != 1:
        raise ValueError("injection_grid: trials and scales must be one-dimensional")
    if t.dtype.kind not in "iu" and t.size:
        raise TypeError("injection_grid: trials must be integers")
    return np.repeat(t.astype(np.int64), len(s)), np.tile(s, len(t))


def _check_grid_list(who, inj, trials, scales):
    """The list of Transit.inject_grid / recover_grid as (int64 trials, float64 scales) of one length; a scalar is
    broadcast against the other.  TypeError / ValueError as Transit.inject's for a single point."""
    try:
        t = np.atleast_1d(np.asarray(trials))
        s = np.atleast_1d(np.asarray(scales, dtype=np.float64))
    except (TypeError, ValueError):
        raise TypeError("%s: trials must be integers and scales numbers" % who) from None
    if t.dtype.kind not in "iu" and t.size:
        raise TypeError("%s: trials must be integers" % who)
    if t.ndim != 1 or s.ndim != 1:
        raise ValueError("%s: trials and scales must be scalars or one-dimensional" % who)
    if len(t) != len(s):
        if np.ndim(trials) == 0:
            t = np.repeat(t, len(s))
        elif np.ndim(scales) == 0:
            s = np.repeat(s, len(t))
        else:
            raise ValueError("%s: %d trials and %d scales" % (who, len(t), len(s)))
    t = t.astype(np.int64)
    n_trial = inj.exposures.n_trial
    for b in range(len(t)):
        if not 0 <= t[b] < n_trial:
            raise ValueError("%s: trial %d of entry %d lies outside [0, %d)" % (who, t[b], b, n_trial))
        if not np.isfinite(s[b]):
            raise ValueError("%s: scale of entry %d must be finite" % (who, b))
    return t, s


def _check_sysrem_args(who, inj, n_comp, n_iter, ones, highpass, sysrem_orders=None):
    """The refusals of Transit.clean / Transit.inject that need no device: (n_comp, n_iter, ones) as integers."""
    if not isinstance(inj, Injection):
        raise TypeError("%s: inj must be an observation.Injection" % who)
    if sysrem_orders is not None:
        if not isinstance(sysrem_orders, Orders):
            raise TypeError("%s: sysrem_orders must be an observation.Orders" % who)
        if sysrem_orders.exposures_key != inj.exposures_key:
            raise ValueError("%s: the Orders of sysrem_orders were made for other exposures (another table, pixels or "
                             "data)" % who)
    if highpass is not None:
        if not isinstance(highpass, HighPass):
            raise TypeError("%s: highpass must be an observation.HighPass" % who)
        if highpass.exposures_key != inj.exposures_key:
            raise ValueError("%s: the HighPass was made for other exposures (another table, pixels or data)" % who)
    for name, v in (("n_comp", n_comp), ("n_iter", n_iter)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError("%s: %s must be an integer" % (who, name))
    if not isinstance(ones, (bool, np.bool_)):
        raise TypeError("%s: ones must be a bool" % who)
    n_comp, n_iter, ones = int(n_comp), int(n_iter), bool(ones)
    if n_comp < 0 or not 1 <= n_comp + ones <= Detrend.MAX_COMP:
        raise ValueError("%s: n_comp >= 0 and 1 <= n_comp + ones <= %d" % (who, Detrend.MAX_COMP))
    if n_iter < 1:
        raise ValueError("%s: n_iter must be >= 1" % who)
    return n_comp, n_iter, ones


MAX_BROADENING_NODES = 1025   # of a velocity kernel (the device's record stage)


class Broadening:
    """The velocity kernel of Transit.observe / velocity_map / expose(broaden=...) and Transit.broadened: ``weights``
    [n] (finite and >= 0, not all zero) are the shares of the absorbing gas at the line-of-sight velocities
    ``velocities`` [n] in cm/s (positive: away from the observer), uniform and ascending, 2 <= n <= 1025; between the
    nodes the distribution is linear, outside them zero.  R is convolved with it on the device, on the model's own
    grid, before the instrument sees it (include/prom_hip.h, "broadened spectra on the device").  Gas at velocity v
    moves a line to lambda (1 + v / c), so the device's kernel over the Doppler offset beta is K(beta) = P(-beta c):
    the weights reversed, first node b0 = -velocities[-1] / c, s = c / step nodes per unit beta.  These and the content
    key that lets a device skip the upload are computed once here; the arrays are copied.  TypeError or ValueError for
    a bad shape or value, before a device is touched."""

    def __init__(self, velocities, weights):
        from . import constants as const
        from .gasProperties import _content_fingerprint
        try:
            v = np.array(velocities, dtype=np.float64)
            p = np.array(weights, dtype=np.float64)
        except (TypeError, ValueError):
            raise TypeError("Broadening: velocities and weights must be arrays of numbers") from None
        if v.ndim != 1 or p.shape != v.shape:
            raise ValueError("Broadening: velocities and weights must be 1-D arrays of one length")
        if not 2 <= len(v) <= MAX_BROADENING_NODES:
            raise ValueError("Broadening: between 2 and %d nodes, not %d" % (MAX_BROADENING_NODES, len(v)))
        if not (np.all(np.isfinite(v)) and np.all(np.isfinite(p))):
            raise ValueError("Broadening: velocities and weights must be finite")
        if np.any(p < 0) or not np.any(p > 0):
            raise ValueError("Broadening: weights must be >= 0 and not all zero")
        step = (v[-1] - v[0]) / (len(v) - 1)
        if not (step > 0 and np.all(np.diff(v) > 0)):
            raise ValueError("Broadening: velocities must be ascending")
        if np.max(np.abs(v - (v[0] + step * np.arange(len(v))))) > 1e-9 * step * len(v):
            raise ValueError("Broadening: velocities must be uniformly spaced")
        self.velocities, self.weights = v, p
        self.K = np.ascontiguousarray(p[::-1])       # what the device sees
        self.b0 = float(-v[-1] / const.c)
        self.s = float(const.c / step)
        if not (math.isfinite(self.s) and self.s > 0):
            raise ValueError("Broadening: the velocity step is too small")
        self.key = ("broaden", self.b0, self.s) + _content_fingerprint(self.K)


def rotation_kernel(v_eq: float, n: int = 65, wind: float = 0.0, east_west=(1.0, 1.0)):
    """(velocities, weights) of the terminator ring of a rigid rotator with equatorial speed ``v_eq`` [cm/s]: gas on
    the ring has P(v) ~ 1 / sqrt(v_eq^2 - v^2), the double-horned profile.  ``n`` uniform nodes span [-v_eq, v_eq]; a
    node's weight is the exact integral of P over its cell (a difference of arcsines), so the horns stay integrable.
    ``wind`` [cm/s] shifts all velocities (a day-to-night flow is negative: towards the observer).  ``east_west``
    weighs the receding (v > 0) and the approaching (v < 0) half of the ring.  The weights sum to 1."""
    v_eq, wind, n = float(v_eq), float(wind), int(n)
    if not (math.isfinite(v_eq) and v_eq > 0 and math.isfinite(wind)):
        raise ValueError("rotation_kernel: v_eq must be positive and wind finite")
    if not 2 <= n <= MAX_BROADENING_NODES:
        raise ValueError("rotation_kernel: between 2 and %d nodes" % MAX_BROADENING_NODES)
    ew = np.array(east_west, dtype=np.float64)
    if ew.shape != (2,) or not (np.all(np.isfinite(ew)) and np.all(ew >= 0) and np.any(ew > 0)):
        raise ValueError("rotation_kernel: east_west must be two weights >= 0, not both zero")
    x = np.linspace(-1.0, 1.0, n)                                  # nodes in units of v_eq
    h = 1.0 / (n - 1)
    lo, hi = np.clip(x - h, -1.0, 1.0), np.clip(x + h, -1.0, 1.0)  # the cells' ends
    share = lambda a, b: (np.arcsin(b) - np.arcsin(a)) / math.pi   # of the ring between a <= b
    w = ew[0] * share(np.maximum(lo, 0.0), np.maximum(hi, 0.0)) + ew[1] * share(np.minimum(lo, 0.0), np.minimum(hi, 0.0))
    return x * v_eq + wind, w / w.sum()


def gaussian_velocity_kernel(sigma_v: float, truncate: float = 4.0, n: int = 65):
    """(velocities, weights) of a Gaussian velocity distribution of standard deviation ``sigma_v`` [cm/s] on ``n``
    uniform nodes over [-truncate sigma_v, truncate sigma_v]; the weights sum to 1."""
    sigma_v, truncate, n = float(sigma_v), float(truncate), int(n)
    if not (math.isfinite(sigma_v) and sigma_v > 0 and math.isfinite(truncate) and truncate > 0):
        raise ValueError("gaussian_velocity_kernel: sigma_v and truncate must be positive")
    if not 2 <= n <= MAX_BROADENING_NODES:
        raise ValueError("gaussian_velocity_kernel: between 2 and %d nodes" % MAX_BROADENING_NODES)
    z = np.linspace(-truncate, truncate, n)
    w = np.exp(-0.5 * z * z)
    return z * sigma_v, w / w.sum()


def tidally_locked_speed(planet) -> float:
    """Equatorial rotation speed [cm/s] of a planet that rotates once per orbit: R_p sqrt(G M_star / a^3)."""
    from . import constants as const
    return float(planet.R * math.sqrt(const.G * planet.hostStar.M / planet.a ** 3))


def model_spectrum(num, den) -> np.ndarray:
    """M = num / den; NaN where den == 0 (no model coverage)."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den == 0.0, np.nan, num / np.where(den == 0.0, 1.0, den))


def chi_square(model, den, data, ivar):
    """(chi2[n_orb], n_used[n_orb]) on the host, with the device's rule: a pixel is used when ivar is finite and
    > 0, data is finite and den > 0; a used pixel with NaN model makes the phase's chi2 NaN."""
    model, den, data, ivar = (np.asarray(a, dtype=np.float64) for a in (model, den, data, ivar))
    with np.errstate(invalid="ignore"):
        used = np.isfinite(ivar) & (ivar > 0) & np.isfinite(data) & (den > 0)
        r = np.where(used, model - data, 0.0)
        terms = np.where(used, np.where(used, ivar, 0.0) * (r * r), 0.0)
    return terms.sum(axis=-1), used.sum(axis=-1).astype(np.int64)


def coadd(model, weights=None) -> np.ndarray:
    """Weighted mean over phases of model[n_orb][n_pix], over the phases whose model is finite at the pixel: the
    planet-frame co-addition that ``frame_shifts`` exists for.  ``weights``: [n_orb] or [n_orb][n_pix] (default
    1).  NaN where no phase has a finite model or the weights sum to 0."""
    m = np.asarray(model, dtype=np.float64)
    w = np.ones(m.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64)
    w = np.broadcast_to(w[:, None] if w.ndim == 1 else w, m.shape)
    ok = np.isfinite(m) & np.isfinite(w)
    ws = np.where(ok, w, 0.0)
    tot = ws.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(tot != 0.0, (ws * np.where(ok, m, 0.0)).sum(axis=0) / np.where(tot != 0.0, tot, 1.0), np.nan)


def planet_frame_shifts(planet, orbphase) -> np.ndarray:
    """Per-phase frame factors of the planet's rest frame (lightcurve.planet_shifts): a pixel at rest wavelength
    lambda sits at lambda * factor in the model's frame."""
    from . import lightcurve
    return lightcurve.planet_shifts(planet, orbphase)


def trial_factors(base, velocities) -> np.ndarray:
    """Trial table F[n_orb][n_trial] = base[:, None] * calculateDopplerShift(velocities)[None, :]: every phase's own
    frame factor ``base`` [n_orb] (e.g. planet_frame_shifts; None: ones, with one row) scanned over a grid of trial
    line-of-sight velocities [cm/s]."""
    from . import constants as const
    d = const.calculateDopplerShift(np.asarray(velocities, dtype=np.float64).reshape(-1))
    b = np.ones(1) if base is None else np.asarray(base, dtype=np.float64).reshape(-1)
    return np.ascontiguousarray(b[:, None] * d[None, :])


def kp_vsys_factors(orbphase, Kp, Vsys) -> np.ndarray:
    """Trial table F[n_orb][nKp * nVsys], Kp-major, of a (Kp, Vsys) grid [cm/s]:
    calculateDopplerShift(-Kp_i sin(orbphase_o) + Vsys_l), Planet.getLOSvelocity's convention.  With
    Kp = [sqrt(G M_star / a)] and Vsys = [0] it is planet_frame_shifts bit for bit."""
    from . import constants as const
    orb = np.asarray(orbphase, dtype=np.float64).reshape(-1)
    kp = np.asarray(Kp, dtype=np.float64).reshape(-1)
    vs = np.asarray(Vsys, dtype=np.float64).reshape(-1)
    v = (-np.sin(orb))[:, None, None] * kp[None, :, None] + vs[None, None, :]
    return np.ascontiguousarray(const.calculateDopplerShift(v).reshape(len(orb), len(kp) * len(vs)))


def exposure_taps(orbphase, base, mid, width, n_sub: int = 1, Kp=None, Vsys=None):
    """(rows [n_exp][2 n_sub], weights [n_exp][2 n_sub], factors [n_exp][n_trial][2 n_sub]) of exposures centred at the
    orbital phases ``mid`` [n_exp] that last ``width`` [n_exp] (>= 0), both in radians like ``orbphase``, the model's
    ascending phase axis (at least 2 entries).  ``base`` [n_orb] holds each row's own planet factor
    (planet_frame_shifts).

    An exposure is the mean of ``n_sub`` sub-samples at phi = mid + width ((s + 1/2) / n_sub - 1/2); a sub-sample is
    interpolated linearly between the two model phases that bracket it: with r the bracket's lower row and
    t = (phi - orbphase[r]) / (orbphase[r + 1] - orbphase[r]) the taps are (r, (1 - t) / n_sub) and
    (r + 1, t / n_sub).  A sub-sample outside the axis raises ValueError: there is no extrapolation.

    factors[e][j][tap] = base[row] / calculateDopplerShift(-Kp_j sin(phi) + Vsys_j) over a (Kp, Vsys) grid [cm/s],
    Kp-major as in kp_vsys_factors.  With ``Kp`` and ``Vsys`` both None there is one trial, whose denominator is
    ``base`` interpolated linearly to phi between the bracket's rows (with the same t).

    The pixels are in the frame the model is computed in.  The factor moves the planet's lines from the row's velocity
    to the sub-sample's; features that do not move with the planet, such as a stellar spectrum with centre-to-limb
    variation or the Rossiter-McLaughlin effect, are displaced by the same amount.  This is the approximation of
    interpolating between phases."""
    from . import constants as const
    orb = np.asarray(orbphase, dtype=np.float64).reshape(-1)
    n_orb = len(orb)
    if n_orb < 2 or not np.all(np.isfinite(orb)) or not np.all(np.diff(orb) > 0):
        raise ValueError("exposure_taps: orbphase must be ascending with at least 2 entries")
    b = np.asarray(base, dtype=np.float64).reshape(-1)
    if b.shape != (n_orb,):
        raise ValueError("exposure_taps: base must have one factor per orbital phase")
    mid = np.asarray(mid, dtype=np.float64).reshape(-1)
    wid = np.asarray(width, dtype=np.float64).reshape(-1)
    if wid.shape != mid.shape or len(mid) < 1:
        raise ValueError("exposure_taps: mid and width must be [n_exp] with n_exp >= 1")
    if not (np.all(np.isfinite(mid)) and np.all(np.isfinite(wid)) and np.all(wid >= 0)):
        raise ValueError("exposure_taps: mid must be finite and width finite and >= 0")
    n_sub = int(n_sub)
    if n_sub < 1:
        raise ValueError("exposure_taps: n_sub must be >= 1")
    if (Kp is None) != (Vsys is None):
        raise ValueError("exposure_taps: Kp and Vsys come together")
    phi = mid[:, None] + wid[:, None] * ((np.arange(n_sub) + 0.5) / n_sub - 0.5)[None, :]   # [n_exp][n_sub]
    if np.any(phi < orb[0]) or np.any(phi > orb[-1]):
        raise ValueError("exposure_taps: a sub-sample lies outside the model's phases [%r, %r] (no extrapolation)"
                         % (orb[0], orb[-1]))
    r = np.minimum(np.searchsorted(orb, phi, "right") - 1, n_orb - 2)
    t = (phi - orb[r]) / (orb[r + 1] - orb[r])
    n_exp = len(mid)
    rows = np.empty((n_exp, 2 * n_sub), dtype=np.int32)
    rows[:, 0::2], rows[:, 1::2] = r, r + 1
    weights = np.empty((n_exp, 2 * n_sub))
    weights[:, 0::2], weights[:, 1::2] = (1.0 - t) / n_sub, t / n_sub
    if Kp is None:
        den = ((1.0 - t) * b[r] + t * b[r + 1])[:, None, :]                                  # [n_exp][1][n_sub]
    else:
        kp = np.asarray(Kp, dtype=np.float64).reshape(-1)
        vs = np.asarray(Vsys, dtype=np.float64).reshape(-1)
        v = (-np.sin(phi))[:, None, None, :] * kp[None, :, None, None] + vs[None, None, :, None]
        den = const.calculateDopplerShift(v).reshape(n_exp, len(kp) * len(vs), n_sub)
    factors = b[rows][:, None, :] / np.repeat(den, 2, axis=2)
    return rows, weights, np.ascontiguousarray(factors)


def _ratio(a, b):
    """a / b, NaN where b == 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(b == 0.0, np.nan, a / np.where(b == 0.0, 1.0, b))


class _MomentStats:
    """The statistics of seven moments ``moments`` [..., 7] and ``n_used`` [...]: shared by VelocityMap (per phase or
    exposure and trial) and OrderMap (per exposure, trial and order).  NaN where a denominator is 0."""

    STATS = ("chi2", "chi2_scaled", "scale", "ccf", "loglike")

    def _m(self, i):
        return self.moments[..., i]

    @property
    def chi2(self):
        """sum iv (M - d)^2: m6."""
        return self._m(6)

    @property
    def scale(self):
        """The scale a that minimises sum iv (a M - d)^2: m4 / m3."""
        return _ratio(self._m(4), self._m(3))

    @property
    def chi2_scaled(self):
        """The minimum over a of sum iv (a M - d)^2: m5 - m4^2 / m3."""
        return self._m(5) - _ratio(self._m(4) * self._m(4), self._m(3))

    @property
    def ccf(self):
        """Weighted cross-covariance sum iv (M - <M>)(d - <d>) with weighted means: m4 - m1 m2 / m0."""
        return self._m(4) - _ratio(self._m(1) * self._m(2), self._m(0))

    @property
    def loglike(self):
        """Brogi & Line (2019) with inverse-variance weights: N = n_used, s_f^2 = (m5 - m2^2 / m0) / m0,
        s_g^2 = (m3 - m1^2 / m0) / m0, C = ccf / m0; logL = -N / 2 ln(s_f^2 - 2 C + s_g^2)."""
        m0, m1, m2, m3, m5 = (self._m(i) for i in (0, 1, 2, 3, 5))
        sf = _ratio(m5 - _ratio(m2 * m2, m0), m0)
        sg = _ratio(m3 - _ratio(m1 * m1, m0), m0)
        c = _ratio(self.ccf, m0)
        with np.errstate(invalid="ignore", divide="ignore"):
            return -0.5 * self.n_used * np.log(sf - 2.0 * c + sg)

    def _stat(self, stat):
        if isinstance(stat, str):
            if stat not in self.STATS:
                raise ValueError("%s: unknown statistic %r (one of %s)" % (type(self).__name__, stat,
                                                                           ", ".join(self.STATS)))
            return getattr(self, stat)
        return np.asarray(stat, dtype=np.float64)

    def grid(self, stat, n_kp: int, n_vsys: int):
        """A Kp-major statistic ([..., nKp * nVsys], e.g. over a kp_vsys_factors table) as [..., nKp, nVsys]."""
        s = self._stat(stat)
        if s.shape[-1] != n_kp * n_vsys:
            raise ValueError("%s.grid: %d trials are no %d x %d grid" % (type(self).__name__, s.shape[-1], n_kp, n_vsys))
        return s.reshape(s.shape[:-1] + (n_kp, n_vsys))


class VelocityMap(_MomentStats):
    """Result of Transit.velocity_map: ``moments`` [n_orb][n_trial][7] and ``n_used`` [n_orb][n_trial] of the model in
    every trial frame against the data (include/prom_hip.h, "velocity maps on the device"; m0 = sum iv,
    m1 = sum iv M, m2 = sum iv d, m3 = sum iv M^2, m4 = sum iv M d, m5 = sum iv d^2, m6 = sum iv (M - d)^2 over the
    used pixels) and the table ``factors`` they belong to.  The statistics are per (phase, trial), NaN where their
    denominator is 0.  From Transit.expose the first axis counts exposures, ``factors`` is the exposures'
    [n_exp][n_trial][n_tap] table and ``model`` [n_exp][n_trial][n_pix] holds the exposures' model spectra in the
    caller's pixel order when they were asked for (None otherwise, and from velocity_map).  From
    Transit.expose(orders=...) it also carries ``by_order`` (an OrderMap, or None when the records were not asked for)
    and ``order_totals`` (OrderTotals, formed on the device)."""

    def __init__(self, moments, n_used, factors, model=None):
        self.model = model
        self.moments = np.asarray(moments, dtype=np.float64)
        self.n_used = np.asarray(n_used, dtype=np.int64)
        self.factors = np.asarray(factors, dtype=np.float64)
        if self.moments.ndim != 3 or self.moments.shape[2] != 7 or self.n_used.shape != self.moments.shape[:2]:
            raise ValueError("VelocityMap: moments must be [n_orb][n_trial][7] and n_used [n_orb][n_trial]")

    def total(self, stat="chi2"):
        """The statistic (a name or an array [n_orb][n_trial]) summed over the phases: [n_trial]."""
        return self._stat(stat).sum(axis=0)


class OrderMap(_MomentStats):
    """The per-order moments of Transit.expose(orders=...): ``moments`` [n_exp][n_trial][n_seg][7] and ``n_used``
    [n_exp][n_trial][n_seg] of the final model against the data over each order's pixels (include/prom_hip.h,
    "per-order moments on the device"), the orders' ``labels`` [n_seg] in ascending order and ``keep`` [n_seg].  The
    statistics are VelocityMap's, per (exposure, trial, order)."""

    def __init__(self, moments, n_used, labels, keep):
        self.moments = np.asarray(moments, dtype=np.float64)
        self.n_used = np.asarray(n_used, dtype=np.int64)
        self.labels = np.asarray(labels, dtype=np.int64)
        self.keep = np.asarray(keep, dtype=bool)
        if self.moments.ndim != 4 or self.moments.shape[3] != 7 or self.n_used.shape != self.moments.shape[:3]:
            raise ValueError("OrderMap: moments must be [n_exp][n_trial][n_seg][7] and n_used [n_exp][n_trial][n_seg]")
        if self.labels.shape != self.moments.shape[2:3] or self.keep.shape != self.labels.shape:
            raise ValueError("OrderMap: labels and keep must be [n_seg]")

    def enters(self, keep=None):
        """Whether (exposure, trial, order) enters a total: the order is kept (``keep`` [n_seg], None: the map's own)
        and has two used pixels at least."""
        k = self.keep if keep is None else np.asarray(keep, dtype=bool)
        if k.shape != self.keep.shape:
            raise ValueError("OrderMap: keep must be [n_seg]")
        return k[None, None, :] & (self.n_used >= 2)

    def total(self, stat="chi2", keep=None):
        """The statistic (a name or an array [n_exp][n_trial][n_seg]) summed over the exposures and the entering
        orders: [n_trial].  A NaN statistic of an entering order makes the total NaN."""
        return np.where(self.enters(keep), self._stat(stat), 0.0).sum(axis=(0, 2))

    def grid(self, stat, n_kp: int, n_vsys: int):
        """A Kp-major statistic as a grid: [n_exp][nKp * nVsys][n_seg] (a name, or an array of that shape) becomes
        [n_exp][nKp][nVsys][n_seg]; any other array, a total [nKp * nVsys] say, is taken along its last axis as in
        VelocityMap.grid."""
        s = self._stat(stat)
        if s.shape != self.n_used.shape:
            return super().grid(s, n_kp, n_vsys)
        if s.shape[1] != n_kp * n_vsys:
            raise ValueError("OrderMap.grid: %d trials are no %d x %d grid" % (s.shape[1], n_kp, n_vsys))
        return s.reshape(s.shape[:1] + (n_kp, n_vsys) + s.shape[2:])


class OrderTotals:
    """The totals of Transit.expose(orders=...) as the device formed them, each [n_exp][n_trial] over the entering
    orders (kept, n_used >= 2) in ascending label: ``loglike``, ``chi2``, ``chi2_scaled`` and ``n_used`` (int64)."""

    def __init__(self, totals):
        t = np.asarray(totals, dtype=np.float64)
        if t.ndim != 3 or t.shape[2] != 4:
            raise ValueError("OrderTotals: totals must be [n_exp][n_trial][4]")
        self.loglike, self.chi2, self.chi2_scaled = t[..., 0], t[..., 1], t[..., 2]
        self.n_used = t[..., 3].astype(np.int64)


class Observed:
    """Result of Transit.observe, in the caller's pixel order: ``model`` [n_orb][n_pix] (None when not asked),
    ``coverage`` = den / (sigma sqrt(2 pi) erf(k / sqrt 2)) (1 where the grid covers a pixel's support densely, less
    at the grid's ends, 0 outside), ``chi2`` and ``n_used`` [n_orb] (None without data), ``spectrum`` R (None
    unless asked)."""

    def __init__(self, model=None, coverage=None, chi2=None, n_used=None, spectrum=None):
        self.model, self.coverage, self.chi2, self.n_used, self.spectrum = model, coverage, chi2, n_used, spectrum
