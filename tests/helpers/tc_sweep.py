"""Designs and the reference of the transmission-curve sweep (tests/test_tc_sweep_cpu.py, tests/test_gpu_tc_sweep.py).

The curve path (prom_tcurve.hip, prom_tc.h) evaluates R(o, w) = T_o(Y(o, w)) with T_o built per phase from the
chords' columns: a tail polynomial for q = Y N_max < 2^-7, 16 Chebyshev coefficients per octave of q above it, and
"every chord opaque" (or, for a table truncated at the 64-octave cap, the exact chord sum) above the table.  The
designs here choose the columns N(phase, chord) and the cross-sections Y(wavelength) so that one run visits every
branch, both sides of every hand-off between them, and the chord counts at which k_tc_build changes its front end,
its number of parts or its chord source.  Pure numpy: nothing here touches the device or the product's library.

How a design reaches the device: a PROM_DENSITY_TABULATED scenario with n_x = 8, delta_x = 1, chi = 1 and the
column in sample 0 (so N is the stored density, exactly), and a lookup table with one node per wavelength,
x_i = lambda_i, y_i = log10(Y_i + offset).  Without Doppler shift every lookup lands on a node.

What "Y_i" means.  The table holds y as float64, and |y| is 18 .. 29 here (ulp(y) = 2^-48), so the cross-sections
a table can express near a given Y are ln10 ulp(y) = 37 ulp(Y) apart.  The reference therefore takes Y from the
table (10^y - offset in longdouble), never from the design's target, and the octave boundaries q = 2^j get, besides
the targets the design asks for, the two expressible values nearest the boundary on either side (BOUNDARY_ULPS).
"""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53                      # unit roundoff of float64
OFFSET = 1e-50                      # the tables' offset (sigma = 10^y - offset), as the product's own tables
LAM0, DLAM, PAD = 5.9e-5, 1e-10, 40  # wavelength grid [cm]; table nodes beyond it at either end (Doppler spread: 18)
K_EPS_EXP = -7                      # prom_tc.h: the tail ends at q = 2^-7
K_SAT = 40.0                        # ... a chord with tau >= 40 is opaque
K_MAX_OCTAVES = 64                  # prom_internal.h kTcMaxOctaves
N_EQUAL = 2.0 ** 60
N_TWO_HI, N_TWO_LO = 2.0 ** 83, 2.0 ** 17   # ratio 2^66: top = 40 2^66, 79 octaves > the cap
# the expressible cross-sections next to a boundary lie within ln10 ulp(y) / ulp(Y) = 2.303 * 2^-48 / 2^-52 ulp of it
BOUNDARY_ULPS = 40
KINDS = ("equal", "loguniform", "two")


# ---- tolerance (derivation: tests/test_gpu_tc_sweep.py's docstring) -----------------------------------------------
LEBESGUE_16 = 2.0 / math.pi * math.log(16.0) + 0.9625
TOL_TAIL = 2.0 ** -42 / 720.0 + 6 * U
TOL_OCTAVE = (31 * LEBESGUE_16 + 48) * U
TOL_OPAQUE = math.exp(-K_SAT)
TOL_LOOKUP = {"static": 2 * U / math.e, "doppler": (2.0 ** -53 + (14 + 4) * U) / math.e}


def tol_exact_sum(nact):
    """Beyond a truncated table: nact terms (F_c / F_sum) exp(-N_c Y) added in chord order.  Sequential summation of
    positive terms: (nact - 1) u of their sum; each term: the weight's product, N_c Y, ocml exp (1 ulp = 2 u) and
    tau's own rounding through tau e^-tau <= 1/e -- 5 u in all."""
    return (nact + 4) * U


# ---- columns ---------------------------------------------------------------------------------------------------
def pinned_chord(n_pr):
    """The chord that holds exactly N_max in the log-uniform design (three quarters round the ring: never behind
    the planet of phase 2)."""
    return (3 * n_pr) // 4


def design_columns(kind, n_pr, n_orb):
    """N[n_orb, n_pr], every chord active, the same columns in every phase."""
    if kind == "equal":
        n = np.full(n_pr, N_EQUAL)
    elif kind == "loguniform":
        u = np.random.default_rng(60012).random(n_pr)
        n = N_EQUAL * 10.0 ** (-12.0 * u)
        n[pinned_chord(n_pr)] = N_EQUAL
    elif kind == "two":
        n = np.where(np.arange(n_pr) % 2 == 0, N_TWO_HI, N_TWO_LO)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(np.broadcast_to(n.astype(np.float64), (n_orb, n_pr)))


def table_octaves(n_max, n_min):
    """k_tc_build's table extent for finite columns when Y reaches past the top: octaves [0, L) of q from 2^-7 up to
    the octave that holds top = 40 N_max / N_min, capped at 64 (then truncated: the exact sum above it)."""
    top = K_SAT * (n_max / n_min)
    return min(math.frexp(top)[1] - 1 - K_EPS_EXP + 1, K_MAX_OCTAVES)


# ---- chord geometry of the chord-count matrix -------------------------------------------------------------------
PLANET_R = 1.3
PLANET_FAR = 1.0e3


def ring(n_pr):
    """Chords on the unit ring, chord c at angle 2 pi (c + 1/2) / n_pr: (y, z)."""
    th = 2.0 * np.pi * (np.arange(n_pr) + 0.5) / n_pr
    return np.sin(th), np.cos(th)


def blocked_by(y, z, planet_y, planet_R=PLANET_R):
    """The kernel's rule: sqrt((y - y_p)^2 + z^2) < R.  The designs keep every chord 1e-6 away from the rim, so the
    device's rounding of the distance cannot change a chord's side."""
    d = np.sqrt((y - planet_y) ** 2 + z ** 2)
    assert np.all(np.abs(d - planet_R) > 1e-6)
    return d < planet_R


def chord_fout(n_pr):
    return np.random.default_rng(77003).uniform(0.5, 1.5, n_pr)


def matrix_problem(n_pr):
    """The chord-count matrix' four phases over log-uniform columns: 0 every chord active; 1 every density zero;
    2 the planet over the chords with sin(angle) > 0.155 (about 45 %); 3 one active chord (the pinned one, N_max)
    among zero densities.  Returns dict(N [4, n_pr] as stored (zero = transparent), blocked [4, n_pr], planet_y [4],
    y, z, fout)."""
    N = design_columns("loguniform", n_pr, 4)
    y, z = ring(n_pr)
    planet_y = np.array([PLANET_FAR, PLANET_FAR, 1.0, PLANET_FAR])
    blocked = np.stack([blocked_by(y, z, p) for p in planet_y])
    N[1] = 0.0
    one = pinned_chord(n_pr)
    keep = N[3, one]
    N[3] = 0.0
    N[3, one] = keep
    assert not blocked[2, one]
    return {"N": N, "blocked": blocked, "planet_y": planet_y, "y": y, "z": z, "fout": chord_fout(n_pr)}


# ---- the sweep over q -------------------------------------------------------------------------------------------
def _pow10(v):
    return np.power(LD(10.0), np.asarray(v, dtype=LD))


def _real_Y(y):
    """The cross-section a table node y expresses: 10^y - offset, longdouble."""
    return _pow10(y) - LD(OFFSET)


def _node_of(Y):
    return np.asarray(np.log10(np.asarray(Y, dtype=LD) + LD(OFFSET)), dtype=np.float64)


def _step(y, k):
    for _ in range(abs(k)):
        y = np.nextafter(y, np.inf if k > 0 else -np.inf)
    return y


def design_sweep(n_max, n_min, L):
    """The table nodes and wavelengths of one sweep.  n_max must be a power of two (Y = q / N_max is then exact).

    Targets: 16 points per octave of q from 2^-12 to 4 top (geometric, seeded jitter); for every boundary q = 2^j,
    j = -7 .. L - 7, the doubles 2^j (1 +- 2^-52), 2^j (1 +- 2^-50) and 2^j; three points straddling top =
    40 N_max / N_min.  Each target becomes the node y = fl(log10(Y + offset)); each boundary also gets the nearest
    node on either side of it (see the module docstring).  Returns a dict:
      y [n] float64 strictly increasing, Y [n] longdouble (what the nodes express), q [n] longdouble = Y N_max,
      targets [m] float64 (the q asked for), wav [n], tx / ty (the padded table), L, top, n_max, cap (2^(L-7))."""
    assert math.frexp(n_max)[0] == 0.5
    top = K_SAT * (n_max / n_min)
    rng = np.random.default_rng(160007)
    q = []
    e = -12
    while 2.0 ** e < 4.0 * top:
        for i in range(16):
            v = 2.0 ** (e + (i + rng.uniform(0.1, 0.9)) / 16.0)
            if v <= 4.0 * top:
                q.append(v)
        e += 1
    snapped = []
    for j in range(K_EPS_EXP, L + K_EPS_EXP + 1):
        b = 2.0 ** j
        q += [b * (1 - 2.0 ** -52), b * (1 + 2.0 ** -52), b * (1 - 2.0 ** -50), b * (1 + 2.0 ** -50), b]
        y0 = float(_node_of(b / n_max))
        cand = np.array([_step(y0, k) for k in range(-6, 7)])
        qr = _real_Y(cand) * LD(n_max)
        snapped.append(cand[qr < b][-1])
        snapped.append(cand[qr >= b][0])
    q += [top * (1 - 1e-9), top, top * (1 + 1e-9)]
    targets = np.unique(np.array(q, dtype=np.float64))
    y = np.unique(np.concatenate([_node_of(targets / n_max), np.array(snapped)]))
    Y = _real_Y(y)
    n = len(y)
    grid = LAM0 + DLAM * (np.arange(n + 2 * PAD) - PAD)
    ty = np.concatenate([np.full(PAD, y[0]), y, np.full(PAD, y[-1])])
    return {"y": y, "Y": Y, "q": Y * LD(n_max), "targets": targets, "wav": grid[PAD:PAD + n].copy(), "tx": grid,
            "ty": ty, "L": L, "top": top, "n_max": n_max, "cap": 2.0 ** (L + K_EPS_EXP)}


def sweep_for(kind, N):
    """design_sweep for the columns N[n_pr] of a design's full phase."""
    n_max, n_min = float(N.max()), float(N[N > 0].min())
    return design_sweep(n_max, n_min, table_octaves(n_max, n_min))


# ---- the reference ------------------------------------------------------------------------------------------------
def reference_Y(tx, ty, offset, factors, wav):
    """Y[n_orb, n_wav] in longdouble from the float64 targets t = factor * wavelength (the kernel's own product):
    numpy.interp's bracket (the largest j <= n - 2 with x_j <= t; the end values outside the table), then
    slope (t - x_j) + f_j with slope = (f_j+1 - f_j) / (x_j+1 - x_j) and 10^(.) - offset, all in longdouble
    (oracle.interp_log's operand order)."""
    t = np.asarray(factors, dtype=np.float64)[:, None] * np.asarray(wav, dtype=np.float64)[None, :]
    n = len(tx)
    j = np.clip(np.searchsorted(tx, t, side="right") - 1, 0, n - 2)
    xl, fl = np.asarray(tx, dtype=LD), np.asarray(ty, dtype=LD)
    slope = (fl[j + 1] - fl[j]) / (xl[j + 1] - xl[j])
    v = slope * (t.astype(LD) - xl[j]) + fl[j]
    v = np.where(t >= tx[-1], fl[-1], np.where(t < tx[0], fl[0], v))
    return _pow10(v) - LD(offset)


def reference_R(fout, blocked, N, Y, chunk=1 << 21):
    """R[o, w] = sum_{c not blocked} F_c exp(-N[o, c] Y[o, w]) / sum_{all c} F_c, exp and sums in longdouble
    (oracle/prom_oracle.py transit_depth: Fin / Fout).  fout [n_pr], blocked and N [n_orb, n_pr], Y [n_orb, n_wav]
    or [n_wav].  Two shortcuts that keep every digit the comparison can see: a chord with N = 0 adds F_c itself, and
    a term with tau > 200 (e^-200 = 1e-87 of its weight) adds 0 without calling exp."""
    F = np.asarray(fout, dtype=LD)
    N = np.asarray(N, dtype=LD)
    n_orb, n_pr = N.shape
    Y = np.broadcast_to(np.asarray(Y, dtype=LD), (n_orb, np.shape(Y)[-1]))
    fsum = F.sum()
    R = np.empty(Y.shape, dtype=LD)
    with np.errstate(under="ignore"):
        for o in range(n_orb):
            live = ~np.asarray(blocked[o], dtype=bool)
            clear = live & (N[o] == 0)
            live &= ~clear
            Fo, No = F[live], N[o][live]
            R[o] = F[clear].sum()
            step = max(1, chunk // max(1, len(No)))
            for w0 in range(0, Y.shape[1] if len(No) else 0, step):
                tau = No[:, None] * Y[o, None, w0:w0 + step]
                e = np.zeros(tau.shape, dtype=LD)
                np.exp(-tau, out=e, where=tau <= 200)
                R[o, w0:w0 + step] += (Fo[:, None] * e).sum(axis=0)
    return R / fsum


def regions(q, L):
    """The branch prom_tc.h's tc_eval takes at each q (longdouble, of the reference): -1 tail, j = 0 .. L - 1 the
    octave, L above the table ("opaque" or the exact sum)."""
    e = np.frexp(np.asarray(q, dtype=LD))[1].astype(np.int64)   # q = m 2^e, m in [0.5, 1)
    return np.clip(e - 1 - K_EPS_EXP, -1, L)


def near_boundary(q, rel=2.0 ** -40):
    """Points within rel of a power of two: the device's q = fl(Y N_max) may fall on the other side."""
    q = np.asarray(q, dtype=LD)
    m = np.frexp(q)[0]          # [0.5, 1)
    return (m < 0.5 * (1 + rel)) | (m > 1 - rel)


# ---- which k_tc_build configuration a chord count reaches (prom_api_transit.hip, prom_transit.hip, prom_tcurve.hip) --
def build_config(n_pr, parts_env=None):
    """(front end, parts, chord source) for n_pr chords: the partials of k_columns8 when n_pr % 32 == 0, else sweeps
    of 3,072 chords; (n_pr + 299) / 300 parts capped at 16 unless PROM_TC_PARTS; a part of <= 1,024 chords is staged
    in LDS, a longer one reads global memory."""
    parts = max(1, min(16, (n_pr + 299) // 300))
    if parts_env:
        parts = min(16, int(parts_env))
    lens = [n_pr * (p + 1) // parts - n_pr * p // parts for p in range(parts)]
    src = {(True,): "LDS", (False,): "global"}.get(tuple(sorted({l <= 1024 for l in lens})), "mixed")
    front = "partials" if n_pr % 32 == 0 else "sweep x%d" % -(-n_pr // 3072)
    return front, parts, src, lens
