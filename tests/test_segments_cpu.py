"""prom_transit_set's pure planners (prometheus_amd/csrc/prom_segments.hip) on the host: the sigma segments of the
Doppler rows, the chords' mirror pairs, the star table's node slices, the polynomial degree of the sigma rows and the
boundedness rule of the built-in densities.

tests/helpers/segments_host.cpp links the planners, compiled as C++ with g++, and returns their raw outputs.  The
segments are audited by brute force: for every block, slot, row and wavelength (the clamped lanes of a partial last
block among them) the target fl(shift lambda) and numpy's bracket are formed as the kernels form them, and every
slice, guess, bucket directory, per-wavefront slice, kind bit, oversize-block list and count is checked against them.
The synthetic problems between them reach every class of entry; the tests assert that each occurs.  The wide one
has enough blocks for the builder's thread split.
"""
import math
from collections import Counter

import numpy as np
import pytest

from helpers.segments_plan import Problem, bind, build_segments, compile_harness, seg_guess
from helpers.window_plan import _dp, _ip

BW = 256   # kSigBlockW


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    path = tmp_path_factory.mktemp("sg") / "libsegments_host.so"
    compile_harness(path, ["-fPIC", "-shared"])
    lib = bind(path)
    assert lib.sg_const(0, 0) == BW
    return lib


def stretches(x0, *parts):
    """Nodes from x0 on: (stop, h) stretches of uniform spacing h, or arrays of spacings."""
    x = [np.array([x0])]
    for p in parts:
        last = x[-1][-1]
        d = np.full(int(round((p[0] - last) / p[1])), p[1]) if isinstance(p, tuple) else p
        x.append(last + np.cumsum(d))
    return np.unique(np.concatenate(x))


def synthetic(na):
    """2,341 wavelengths at 0.01 (nine blocks and a partial tenth of 37) and three rows.  Table 0: uniform at 0.01 (LDS
    slices with a guess) around a line core whose spacing shrinks to 1e-5 (no linear guess: per-wavefront slices and a
    directory), then 0.005 (more than kSigSeg nodes a block: a global slice with a guess), 0.002 (more than 1,024), 0.01
    again, ending three blocks before the wavelengths do (no slice).  Table 1, for two species: 0.02, then 0.0025."""
    wav = 5000.0 + 0.01 * np.arange(2341)
    core = 0.01 * 0.8 ** np.arange(1, 32)
    x0 = stretches(4999.0, (5003.95, 0.01), np.concatenate([core, core[::-1]]), (5007.4, 0.01), (5010.5, 0.005),
                   (5015.6, 0.002), (5019.0, 0.01))
    x1 = stretches(4998.0, (5012.0, 0.02), (5030.0, 0.0025))
    sh = [[1.0 - 3e-5, 1.0, 1.0 + 3e-5], [1.0 - 1e-5, 1.0 + 2e-5, 1.0 + 1e-5]]
    return Problem(wav, [x0, x1][:na], sh[:na])


def wide():
    """33,061 wavelengths at 0.01 (129 blocks and a partial one of 37: the builder splits them over two threads) and
    three rows; one table that repeats, every 16 blocks, a stretch at 0.01, the line core, a stretch whose spacing
    alternates between 0.01 and 0.005 every 0.3 (no wave of 64 wavelengths has a linear guess: a directory only), a
    stretch whose spacing grows by 3e-4 a node (the guess drifts ~3 nodes over a block's ~290 nodes, ~0.3 over a
    wave's ~95: per-wavefront slices on all four waves) and a stretch at 0.005."""
    wav = 5000.0 + 0.01 * np.arange(129 * BW + 37)
    core = 0.01 * 0.8 ** np.arange(1, 32)
    parts, x = [], 4999.0
    for _ in range(9):
        alt = [(x + 8.0 + 0.3 * (j + 1), 0.005 if j % 2 else 0.01) for j in range(20)]
        parts += [(x + 4.95, 0.01), np.concatenate([core, core[::-1]]), (x + 8.0, 0.01)] + alt
        parts += [0.008 * 1.0003 ** np.arange(1400), (x + 40.96, 0.005)]   # (the chirp: 8 -> 12.2e-3 over ~13.9)
        x += 40.96
    return Problem(wav, [stretches(4999.0, *parts)], [[1.0 - 3e-5, 1.0, 1.0 + 3e-5]])


def audit(L, pr, g, use_dir=True):
    """Every assertion of the brute-force audit on segments built without no_guess; returns the classes seen."""
    nb, na = (pr.n_wav + BW - 1) // BW, pr.na
    k_seg, cap = L.sg_const(1, 0), L.sg_const(2, na)
    widx = np.minimum(np.arange(nb * BW), pr.n_wav - 1).reshape(nb, BW)   # (the kernels' clamped lanes)
    seen = Counter()
    assert g.seg.shape == (nb, na) and len(g.seg4) == nb * na * 4 + g.n_dir
    w4 = g.seg4[:nb * na * 4].reshape(nb, na, 4)
    zero = np.zeros((), dtype=g.seg.dtype)
    dir_buckets = 0
    for a in range(na):
        X = pr.X[a]
        t = pr.shift[a][None, :, None] * pr.wav[widx][:, None, :]   # [block, row, lane]
        k = np.clip(np.searchsorted(X, t, "right") - 1, 0, len(X) - 2)
        e = g.seg[:, a]
        kind, m = e["kind"], e["m"].astype(np.int64)
        inside = (t.min(axis=(1, 2)) >= X[0]) & (t.max(axis=(1, 2)) < X[-1])
        has = m >= 2
        assert np.array_equal(has, inside), "a slice exactly where every target lies inside the table"
        assert np.all(e[~has] == zero)
        seen["no slice"] += int(np.sum(~has))
        seen["past the table"] += int(np.sum(pr.shift[a].min() * pr.wav[widx].min(axis=1) >= X[-1]))
        rel = k - e["lo"][:, None, None]
        assert np.all(rel[has] >= 0) and np.all(rel[has] <= (m[has] - 2)[:, None, None]), "a bracket outside its slice"
        guessed = (kind & 3) != 0
        assert not np.any(kind & ~(3 | 8 | 32 | 64)) and not np.any(guessed & ~has)
        assert np.array_equal((kind & 3)[guessed], np.where(m[guessed] <= k_seg, 1, 2))
        assert np.array_equal((kind & 64) != 0, guessed & (m <= cap)), "bit 64: a guess and m <= tc_slice_cap"
        assert not np.any(guessed & ((kind & (8 | 32)) != 0))
        if not use_dir:
            assert not np.any(kind & 32)
        for b in range(nb):
            if guessed[b]:
                gg = seg_guess(L, t[b], e["xs"][b], e["inv"][b], e["m"][b])
                assert np.abs(gg - rel[b]).max() <= 1, "a guess more than one node off"
                seen["lds guess" if (kind[b] & 3) == 1 else "global guess"] += 1
                seen["global guess within the curve cap"] += int((kind[b] & 67) == 66)
                seen["guess over more than 1024 nodes"] += int(m[b] > 1024)
            if kind[b] & 32:
                assert nb * na * 4 <= e["pad"][b] < len(g.seg4)
                de = g.seg4[e["pad"][b]]
                B = int(de["m"]) - 1
                assert de["kind"] == 32 and de["lo"] == e["lo"][b] and B >= 4 * m[b]
                assert 0 <= de["pad"] and de["pad"] + B <= len(g.sdir)
                j = seg_guess(L, t[b], de["xs"], de["inv"], de["m"])
                assert j.min() >= 0 and j.max() <= B - 1
                assert np.abs(g.sdir[de["pad"] + j] - rel[b]).max() <= 1, "a directory bucket more than one node off"
                dir_buckets += B
                seen["directory"] += 1
                seen["directory only"] += int(not kind[b] & 8)
            if kind[b] & 8:
                live = 0
                for q in range(4):
                    ew = w4[b, a, q]
                    if ew["m"] == 0:
                        assert ew == zero
                        continue
                    assert ew["kind"] == 2
                    tq, relq = t[b][:, 64 * q:64 * q + 64], k[b][:, 64 * q:64 * q + 64] - ew["lo"]
                    assert relq.min() >= 0 and relq.max() <= ew["m"] - 2
                    assert np.abs(seg_guess(L, tq, ew["xs"], ew["inv"], ew["m"]) - relq).max() <= 1
                    live += 1
                assert live >= 1
                seen["per wavefront"] += 1
                seen["per wavefront, some waves without"] += int(live < 4)
                seen["per wavefront, all four waves"] += int(live == 4)
            else:
                assert np.all(w4[b, a] == zero)
    assert dir_buckets == len(g.sdir) and g.n_dir == int(np.sum((g.seg["kind"] & 32) != 0))
    kinds = g.seg["kind"]
    assert np.array_equal(g.fb, np.nonzero(np.any((kinds & ~64) != 1, axis=1))[0])
    assert np.array_equal(g.fb_tc, np.nonzero(np.any((kinds & 64) == 0, axis=1))[0])
    assert g.noguess == int(np.sum(((kinds & 3) == 0) & ((kinds & 32) == 0)))
    seen["partial last block"] += int(pr.n_wav % BW != 0)
    return seen


@pytest.fixture(scope="module")
def built(L):
    return {na: (synthetic(na), build_segments(L, synthetic(na))) for na in (1, 2)}


@pytest.mark.parametrize("na", [1, 2])
def test_segment_audit(L, built, na):
    pr, g = built[na]
    seen = audit(L, pr, g)
    print(dict(seen))
    for c in ("lds guess", "global guess", "guess over more than 1024 nodes", "no slice", "past the table",
              "per wavefront", "directory", "partial last block", "global guess within the curve cap"):
        assert seen[c] >= 1, c + ": the input reaches no such entry"
    if na == 2:   # (the second table's entries are there, and differ from the first's)
        assert np.any(g.seg["m"][:, 1] >= 2) and np.any(g.seg["m"][:, 0] != g.seg["m"][:, 1])
    assert len(g.fb) >= 1 and len(g.fb_tc) >= 1 and len(g.fb) < g.seg.shape[0]


def test_segment_audit_two_threads(L):
    """128 blocks or more: the blocks are split over threads that append their directories in the order they finish.
    The audit follows every entry's pad into seg4 and on into sdir, so it holds whatever that order is."""
    pr = wide()
    nb = (pr.n_wav + BW - 1) // BW
    assert nb // 64 >= 2, "one thread"
    g = build_segments(L, pr)
    seen = audit(L, pr, g)
    print(dict(seen))
    for c in ("lds guess", "global guess", "directory", "directory only", "per wavefront",
              "per wavefront, some waves without", "per wavefront, all four waves", "partial last block"):
        assert seen[c] >= 1, c + ": the input reaches no such entry"
    with_dir = np.nonzero(g.seg["kind"][:, 0] & 32)[0]
    half = nb // 2   # (two threads: blocks [0, nb / 2) and [nb / 2, nb))
    assert np.any(with_dir < half) and np.any(with_dir >= half), "directories from one thread only"
    assert len(set(g.seg["pad"][with_dir, 0])) == len(with_dir) == g.n_dir
    audit(L, pr, build_segments(L, pr, use_dir=False), use_dir=False)


@pytest.mark.parametrize("na", [1, 2])
def test_switches(L, built, na):
    pr, g = built[na]
    plain = build_segments(L, pr, use_dir=False)
    assert plain.n_dir == 0 and len(plain.sdir) == 0 and len(plain.seg4) == g.seg.size * 4
    audit(L, pr, plain, use_dir=False)
    want = g.seg.copy()
    want["pad"] = 0
    want["kind"] &= ~32
    assert np.array_equal(plain.seg, want) and np.array_equal(plain.seg4, g.seg4[:g.seg.size * 4])
    ng = build_segments(L, pr, no_guess=True)
    nb = g.seg.shape[0]
    assert np.all(ng.seg["kind"] == 0), "no_guess leaves a guess"
    assert np.array_equal(ng.seg["lo"], g.seg["lo"]) and np.array_equal(ng.seg["m"], g.seg["m"])
    assert ng.noguess == ng.seg.size
    assert np.array_equal(ng.fb, np.arange(nb)) and np.array_equal(ng.fb_tc, np.arange(nb))


def test_no_segments(L):
    pr = synthetic(1)
    five = Problem(pr.wav, pr.X * 5, np.tile(pr.shift, (5, 1)))
    assert build_segments(L, five) is None
    # a factor that is not positive and finite: no slice anywhere for that slot
    for bad in (0.0, -1.0, np.nan, np.inf):
        g = build_segments(L, Problem(pr.wav, pr.X, [[1.0, bad, 1.0]]))
        assert np.all(g.seg["m"] == 0) and g.noguess == g.seg.size and len(g.fb) == g.seg.shape[0]
    lo, hi = np.zeros(1), np.zeros(1)
    v = np.array([1.5, 0.5, 2.0])
    assert L.sg_factor_range(_dp(v), 3, _dp(lo), _dp(hi)) == 1 and (lo[0], hi[0]) == (0.5, 2.0)
    assert L.sg_factor_range(_dp(np.array([1.0, np.nan])), 2, _dp(lo), _dp(hi)) == 0


# ---- mirror pairs ----------------------------------------------------------------------------------------------------
def mirrors_ref(cy, cz):
    """The rule restated: sorted by y, each unpaired chord with z != 0 takes the first later unpaired chord within the
    relative 1e-9 of (y, -z)."""
    n = len(cy)
    mir = np.full(n, -1, dtype=np.int32)
    order = sorted(range(n), key=lambda i: (cy[i], i))
    pairs = 0
    for a, i in enumerate(order):
        if mir[i] >= 0 or not cz[i] != 0.0 or not (math.isfinite(cy[i]) and math.isfinite(cz[i])):
            continue
        tol = 1e-9 * max(abs(cy[i]), abs(cz[i]))
        for j in order[a + 1:]:
            if not cy[j] - cy[i] <= tol:
                break
            if mir[j] < 0 and abs(cz[j] + cz[i]) <= tol:
                mir[i], mir[j] = j, i
                pairs += 1
                break
    return mir, pairs


def pair(L, cy, cz):
    cy, cz = np.ascontiguousarray(cy, dtype=np.float64), np.ascontiguousarray(cz, dtype=np.float64)
    mir = np.full(len(cy), -7, dtype=np.int32)
    n = L.sg_pair_mirrors(_dp(cy), _dp(cz), len(cy), _ip(mir))
    i = np.nonzero(mir >= 0)[0]
    assert np.all(mir >= -1) and np.all(mir[mir[i]] == i) and np.all(mir[i] != i), "not an involution"
    assert 2 * n == len(i)
    return mir, n


def test_mirror_pairs(L):
    y, z = np.meshgrid(np.linspace(-3.0, 3.0, 7), np.linspace(-3.0, 3.0, 7))   # symmetric in z, with a z = 0 row
    cy, cz = list(y.ravel()), list(z.ravel())
    cy += [1.0, 10.0, 10.0, 11.0, 11.0, 12.0, 12.0]
    cz += [2.0,             # a duplicate of the chord (1, 2)
           1.0, -1.0 - 2e-8,   # a partner just outside the tolerance 1e-9 * 10
           1.0, -1.0 - 5e-9,   # ... and one just inside
           np.nan, 1.0]        # a NaN and the chord that would be its partner
    perm = np.random.default_rng(5).permutation(len(cy))
    cy, cz = np.array(cy)[perm], np.array(cz)[perm]
    mir, n = pair(L, cy, cz)
    ref, n_ref = mirrors_ref(cy, cz)
    assert np.array_equal(mir, ref) and n == n_ref == 7 * 3 + 1
    assert np.all(mir[cz == 0.0] == -1) and np.all(mir[cy == 10.0] == -1) and np.all(mir[cy == 11.0] >= 0)
    assert np.all(mir[cy == 12.0] == -1) and np.sum(mir[(cy == 1.0) & (np.abs(cz) == 2.0)] >= 0) == 2
    # a ring of 64 chords at angles (k + 1/4) 2 pi / 64: no chord is another's mirror image
    th = 2.0 * np.pi * (np.arange(64) + 0.25) / 64
    mir, n = pair(L, 2.0 * np.cos(th), 2.0 * np.sin(th))
    assert n == 0 and np.all(mir == -1) and mirrors_ref(2.0 * np.cos(th), 2.0 * np.sin(th))[1] == 0


# ---- polynomial degree -----------------------------------------------------------------------------------------------
def remainder(am, D):
    am *= 1.0 + 1e-6
    return math.exp(am) * am ** (D + 1) / math.factorial(D + 1)


@pytest.mark.parametrize("amax, want", [([1e-3], 4), ([0.01], 6), ([0.03], 8), ([0.0866], 10), ([0.2], 12),
                                        ([1e-3, 0.2, 0.01], 12), ([0.45], 14), ([1.0], 0)])
def test_poly_degree(L, amax, want):
    a = np.array(amax)
    D = L.sg_poly_degree(_dp(a), len(a), 1)
    assert D == want
    if D:
        assert remainder(a.max(), D) <= 2.0 ** -53 < remainder(a.max(), D - 2)
    else:
        assert remainder(a.max(), 14) > 2.0 ** -53
    assert L.sg_poly_degree(_dp(a), len(a), 0) == 0
    assert L.sg_poly_degree(_dp(np.append(a, np.nan)), len(a) + 1, 1) == 0


# ---- star slices -----------------------------------------------------------------------------------------------------
def test_star_slices(L):
    wav = 5000.0 + 0.01 * np.arange(300)   # two tiles: 256 and 44 wavelengths
    smin, smax = 1.0 - 1e-5, 1.0 + 1e-5
    cap = L.sg_const(3, 0)

    def slices(X, lo_s=smin, hi_s=smax):
        sl = np.full((2, 3), -7, dtype=np.int32)
        L.sg_star_slices(_dp(wav), len(wav), _dp(X), len(X), lo_s, hi_s, _ip(sl))
        return sl

    def covered(X, sl, tiles=(0, 1)):
        for tl in tiles:
            lo, m, half = (int(v) for v in sl[tl])
            w = wav[256 * tl:256 * tl + 256]
            P = 1 << max(m - 1, 0).bit_length()
            assert 2 <= m <= cap and half == P // 2 and P >= m > P // 2
            for s in (smin, smax):
                k = np.clip(np.searchsorted(X, w / s, "right") - 1, 0, len(X) - 2)
                assert k.min() >= lo and k.max() + 1 <= lo + m - 1
    # the table ends inside the second tile's targets (the slice's last node is the table's)
    X = stretches(4999.0, (5002.5, 0.01), (5002.9, 0.0005))
    sl = slices(X)
    covered(X, sl)
    assert sl[1, 0] + sl[1, 1] == len(X)
    # the second tile reaches more than kRmStarMax nodes: global lookups (m = 0)
    X = stretches(4999.0, (5002.5, 0.01), (5003.2, 0.0005))
    sl = slices(X)
    covered(X, sl, tiles=(0,))
    assert np.all(sl[1] == 0)
    reach = np.searchsorted(X, wav[-1] / smin, "right") - np.searchsorted(X, wav[256] / smax, "right") + 2
    assert reach > cap and wav[-1] / smin < X[-1]
    # factors that are not positive and finite: no slices
    for lo_s, hi_s in ((0.0, 1.0), (np.nan, np.nan), (1.0, np.inf)):
        assert np.all(slices(X, lo_s, hi_s) == 0)


# ---- the boundedness rule of the built-in densities ------------------------------------------------------------------
@pytest.mark.parametrize("kind, p, want", [
    (1, [1e9, 7e9, 1e8], True), (1, [1e9, 7e9, -1e8], False), (1, [-1.0, 7e9, 1e8], False), (1, [np.inf, 7e9, 1e8], False),
    (2, [1e9, 7e9, 2.0, 1.0, 1.0], True),        # J_0 >= J(R) = p2 / (p3 p1)
    (2, [1e9, 7e9, 2.0, 1e-10, 1.0], False),     # J_0 below J(R)
    (2, [1e9, 7e9, 2.0, 0.0, 1.0], False), (2, [1e9, 7e9, 2.0, 1.0, -1.0], False),
    (3, [1e9, 7e9, 6.0], True), (3, [1e9, 7e9, -1.0], False), (3, [1e9, 0.0, 6.0], False),
    (4, [1e9, 4e10, 4e9, 1e9], True), (4, [np.nan, 4e10, 4e9, 1e9], False)])
def test_density_bounded(L, kind, p, want):
    assert L.sg_density_bounded(kind, _dp(np.array(p + [0.0] * (8 - len(p))))) == int(want)
