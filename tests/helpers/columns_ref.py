"""References and designs for the column stage (k_columns8, k_ntot + k_columns): plain numpy, no GPU.

columns_numpy      the upstream expression itself, np.sum(n * chi, axis=1) * delta_x (gasProperties.py:940): the
                   reference of everything bitwise in tests/test_gpu_columns.py
columns_emulated   numpy's pairwise order written out in scalar float64, so that tests/test_columns_ref_cpu.py can
                   show that the numpy at hand still sums this way, and so that the order can be mutated
blocked_mask       the reference's two forms of the blocking test (gasProperties.py:1224-1230)
density_ld         the four analytic densities in longdouble with the relative error budget of one float64 sample
design_rows        the rows the bitwise tests sum: log-uniform over 16 decades, about a quarter exact zeros
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53

NX_SMALL = list(range(1, 18)) + [23, 24, 25, 31, 32, 33, 47, 48, 63, 64]
NX_LARGE = [65, 72, 127, 128, 129, 136, 137, 255, 256, 257, 300]
# (chords per phase, phases) of the bitwise tests: 33 is no multiple of 32 (no phase partials, the last 8-lane groups
# of a workgroup partly invalid), 64 is (partials on); one phase and three
GRIDS = [(33, 1), (33, 3), (64, 3)]
CHIS = [1.0, 0.3]
DELTA_X = 0.7   # not a power of two: the final product rounds

MUTATIONS = ["sequential", "drop_last", "remainder_first", "combine_sequential", "swap_duplicate", "split_unrounded",
             "chi_after"]


# ---- the sums --------------------------------------------------------------------------------------------------------
def columns_numpy(n, chi, delta_x):
    n = np.ascontiguousarray(n, dtype=np.float64)
    assert n.ndim == 2
    return np.sum(n * chi, axis=1) * delta_x


def _leaf(p, lo, n, mutation):
    """numpy's pairwise_sum below its block size of 128 (loops_utils.h.src)."""
    if n < 8:
        r = 0.0
        for i in range(lo, lo + n):
            r += p[i]
        return r
    r = [p[lo + j] for j in range(8)]
    lim = n - n % 8
    for i in range(8, lim, 8):
        for j in range(8):
            r[j] += p[lo + i + j]
    if mutation == "remainder_first":      # the remainder lands in lane 0's partial sum, before the combination
        for i in range(lim, n):
            r[0] += p[lo + i]
    if mutation == "combine_sequential":
        res = r[0]
        for j in range(1, 8):
            res += r[j]
    else:
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    if mutation != "remainder_first":
        for i in range(lim, n):
            res += p[lo + i]
    return res


def _pairwise(p, lo, n, mutation):
    if n <= 128:
        return _leaf(p, lo, n, mutation)
    n2 = n // 2
    if mutation != "split_unrounded":
        n2 -= n2 % 8
    return _pairwise(p, lo, n2, mutation) + _pairwise(p, lo + n2, n - n2, mutation)


def mutation_applies(mutation, n_x, chi):
    """Where a mutation is another computation than the true order (elsewhere it is the same sequence of roundings,
    and no design can see it):
      sequential, combine_sequential   from 8 samples on: below, the true order is the sequential one
      remainder_first                  a remainder beside eight partial sums: n_x >= 9, n_x % 8 != 0
      swap_duplicate                   samples 0 and 1 exchanged and sample 2 overwritten by sample 1: n_x >= 3
      split_unrounded                  a recursion whose half is no multiple of 8: n_x > 128, (n_x // 2) % 8 != 0
      chi_after                        chi != 1 (a product with 1.0 is exact wherever it stands)
      drop_last                        n_x >= 2."""
    if mutation in ("sequential", "combine_sequential"):
        return n_x >= 8
    if mutation == "remainder_first":
        return n_x >= 9 and n_x % 8 != 0
    if mutation == "swap_duplicate":
        return n_x >= 3
    if mutation == "split_unrounded":
        return n_x > 128 and (n_x // 2) % 8 != 0
    if mutation == "chi_after":
        return n_x >= 2 and chi != 1.0
    if mutation == "drop_last":
        return n_x >= 2
    raise ValueError(mutation)


def columns_emulated(n, chi, delta_x, mutation=None):
    """The kernels' order: n < 8 sequential from 0.0; otherwise eight strided accumulators combined as
    ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder in order; above 128 split at n/2 rounded down to a
    multiple of 8; then 0.0 + the result, times delta_x.  Python floats are IEEE binary64."""
    n = np.asarray(n, dtype=np.float64)
    chi, delta_x = float(chi), float(delta_x)
    out = np.empty(n.shape[0])
    for c in range(n.shape[0]):
        a = [float(v) for v in n[c]]
        if mutation == "drop_last":
            a = a[:-1]
        if mutation == "swap_duplicate":
            a[0], a[1] = a[1], a[0]
            a[2] = a[0]
        p = a if mutation == "chi_after" else [v * chi for v in a]
        if mutation == "sequential":
            s = 0.0
            for v in p:
                s += v
        else:
            s = _pairwise(p, 0, len(p), mutation)
        s = 0.0 + s
        if mutation == "chi_after":
            s = s * chi
        out[c] = s * delta_x
    return out


# ---- designs ---------------------------------------------------------------------------------------------------------
def design_rows(n_chords, n_x, seed):
    """[n_chords, n_x] float64: 10^U(0, 16) with about a quarter of the samples exactly 0.  A sum over magnitudes spread
    over 16 decades rounds at nearly every addition, so another order of the same samples gives other bits."""
    rng = np.random.default_rng([int(seed), int(n_chords), int(n_x)])
    a = 10.0 ** rng.uniform(0.0, 16.0, size=(n_chords, n_x))
    a[rng.random((n_chords, n_x)) < 0.25] = 0.0
    return np.ascontiguousarray(a)


def design_seed(n_x):
    return 1000 + n_x


def grid(n_pr, n_orb):
    """Chords on a zigzag across the disk and a planet that covers a few of them, other ones in every phase."""
    i = np.arange(n_pr)
    g = {"y": np.linspace(-10.0, 10.0, n_pr), "z": 0.5 * ((i % 5) - 2.0), "planet_y": np.array([-6.0, 0.25, 7.0])[:n_orb],
         "planet_R": 2.0}
    g["blocked"] = blocked_mask(g["y"], g["z"], g["planet_y"], g["planet_R"], np.zeros((0, n_orb)), [])
    return g


def table_design(n_pr, n_orb, n_x):
    """The tabulated density of the bitwise tests on grid(n_pr, n_orb): rows [n_pr, n_orb, n_x] in the C-ABI's layout
    n[(ip * n_orb + o) * n_x + ix] (every phase its own rows), with a +inf sample in the first chord that no phase
    blocks (first phase, middle sample) and a NaN in the second (last phase, last sample).  `witness` [n_pr, n_orb]
    marks the unblocked finite rows: the ones that can show a wrong order."""
    g = grid(n_pr, n_orb)
    rows = design_rows(n_pr * n_orb, n_x, design_seed(n_x)).reshape(n_pr, n_orb, n_x)
    free = np.where(~g["blocked"].any(axis=0))[0]
    ia, ib = int(free[0]), int(free[1])
    witness = ~g["blocked"].T.copy()
    rows[ia, 0, n_x // 2] = np.inf
    rows[ib, n_orb - 1, n_x - 1] = np.nan
    witness[ia, 0] = witness[ib, n_orb - 1] = False
    g.update(rows=rows, witness=witness, special=[(ia, 0), (ib, n_orb - 1)])
    return g


# ---- blocking --------------------------------------------------------------------------------------------------------
def blocked_mask(y, z, planet_y, planet_R, moon_y, moon_R):
    """[n_orb, n_pr]: the planet as sqrt(dy^2 + z^2) < R, every moon as dy^2 + z^2 < R_m^2 (gasProperties.py:1224-1230)."""
    y, z = np.asarray(y, dtype=np.float64)[None, :], np.asarray(z, dtype=np.float64)[None, :]
    planet_y = np.asarray(planet_y, dtype=np.float64)[:, None]
    blocked = np.sqrt((y - planet_y) ** 2 + z ** 2) < planet_R
    moon_y = np.asarray(moon_y, dtype=np.float64).reshape(len(moon_R), planet_y.shape[0])
    for m, R_m in enumerate(np.asarray(moon_R, dtype=np.float64)):
        blocked = blocked | ((y - moon_y[m][:, None]) ** 2 + z ** 2 < R_m ** 2)
    return blocked


# ---- densities -------------------------------------------------------------------------------------------------------
BAROMETRIC, HYDROSTATIC, POWERLAW, TORUS = 1, 2, 3, 4
RHO = 3.5      # r = sqrt((dx^2 + dy^2) + z^2) in float64, relative, in units of u: see density_ld
RHO_A = 3.0    # the torus' a = sqrt(dx^2 + dy^2)
E_EXP = 4.0    # ocml exp and pow: 2 ulp = 4 u each (supposed: the installed ROCm states no bound)
E_POW = 4.0
LD_SHARE = 2.0 ** -9   # the longdouble reference's own error, as a share of the float64 budget (2^-64 against 2^-53,
#                        four times over for its own handful of roundings)


def density_ld(kind, p, x, y, z, bx, by):
    """(sample, eps) in longdouble, broadcasting x, y, z, bx, by: the formulas of prom_density_kind, and the bound
    eps(x) on a float64 evaluation's relative error in units of u = 2^-53 (first order in u), from the arithmetic:

      dx = x - bx, dy = y - by     one rounding each: the squares carry 2 u + 1 u
      r = sqrt((dx^2 + dy^2) + z^2)  sums of positive terms add 1 u each: 5 u under the root, halved, + 1 u: RHO = 3.5
      barometric   n0 exp((R - r) / H) heaviside(r - R): R - r has the absolute error RHO r u + |R - r| u, the quotient
                   adds |arg| u; exp turns the exponent's absolute error into a relative one and adds E_EXP; one
                   product with n0 (the product with heaviside's 0 or 1 is exact):
                     eps = RHO r / |H| + 2 |arg| + E_EXP + 1
      hydrostatic  jeans = p2 / (p3 r) heaviside: RHO + 2 relative; arg = jeans - J0 rounds once:
                     eps = (RHO + 2) |jeans| + |jeans - J0| + E_EXP + 1
      power law    xr = R / r: RHO + 1.  Integral q <= 8 by binary exponentiation: q (RHO + 1) carried, q - 1 from the
                   rounded products (a factor b^(2^k) carries 2^k - 1, the popcount(q) - 1 products between them one
                   each), one product with n0: eps = q (RHO + 2), and 1 at q = 0.  Otherwise pow:
                     eps = |q| (RHO + 1) + E_POW + 1
      torus        a to RHO_A = 3; ta = (a - p1) / p2 has the absolute error (3 a / |p2| + 2 |ta|) u; ta^2 doubles it
                   times |ta| and rounds; tz = z / p3 and its square: 3 tz^2 u; two exp, their product, n0:
                     eps = 6 |ta| a / |p2| + 5 ta^2 + 3 tz^2 + 2 E_EXP + 2
    each widened by LD_SHARE for the reference's own rounding.  Where the sample is 0, inf or NaN the class must
    match and eps is not used."""
    p = [LD(v) for v in p]
    x, y, z, bx, by = np.broadcast_arrays(*[np.asarray(v, dtype=np.float64).astype(LD) for v in (x, y, z, bx, by)])
    dx, dy = x - bx, y - by
    with np.errstate(all="ignore"):
        if kind == TORUS:
            a = np.sqrt(dx * dx + dy * dy)
            ta = (a - p[1]) / p[2]
            tz = z / p[3]
            val = p[0] * (np.exp(-(ta * ta)) * np.exp(-(tz * tz)))
            eps = 6 * np.abs(ta) * a / abs(p[2]) + 5 * ta * ta + 3 * tz * tz + 2 * E_EXP + 2
        else:
            r = np.sqrt((dx * dx + dy * dy) + z * z)
            h = np.where(r - p[1] < 0, LD(0), LD(1))
            if kind == BAROMETRIC:
                arg = (p[1] - r) / p[2]
                val = (p[0] * np.exp(arg)) * h
                eps = RHO * r / abs(p[2]) + 2 * np.abs(arg) + E_EXP + 1
            elif kind == HYDROSTATIC:
                jeans = p[2] / (p[3] * r) * h
                val = p[0] * np.exp(jeans - p[4])
                eps = (RHO + 2) * np.abs(jeans) + np.abs(jeans - p[4]) + E_EXP + 1
            elif kind == POWERLAW:
                q = float(p[2])
                val = (p[0] * np.power(p[1] / r, p[2])) * h
                if 0.0 <= q <= 8.0 and q == np.floor(q):
                    e = q * (RHO + 2) if q >= 1 else 1.0
                else:
                    e = abs(q) * (RHO + 1) + E_POW + 1
                eps = np.full(r.shape, e, dtype=LD)
            else:
                raise ValueError(kind)
    return val, (eps * (1 + LD_SHARE) + LD_SHARE).astype(np.float64)
