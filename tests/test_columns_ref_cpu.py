"""The column stage's references (tests/helpers/columns_ref.py) on the CPU: numpy at hand still sums in the order
the kernels restate, the designs of tests/test_gpu_columns.py can see every wrong order listed there, the sample
counts cover every class of the kernels' index arithmetic, and the longdouble densities agree with mpmath."""
import numpy as np
import pytest

from helpers import columns_ref as CR

NX_ALL = CR.NX_SMALL + CR.NX_LARGE


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("chi", CR.CHIS)
def test_emulation_is_numpy_bitwise(chi):
    for n_x in NX_ALL:
        rows = CR.design_rows(64 * 3, n_x, CR.design_seed(n_x))
        want = CR.columns_numpy(rows, chi, CR.DELTA_X)
        got = CR.columns_emulated(rows, chi, CR.DELTA_X)
        assert np.array_equal(bits(got), bits(want)), "n_x %d chi %g: %d rows differ" % (
            n_x, chi, np.count_nonzero(bits(got) != bits(want)))


@pytest.mark.parametrize("n_pr,n_orb", CR.GRIDS)
def test_designs_see_every_mutation(n_pr, n_orb):
    """A condition on the designs: on every grid the GPU test runs, for every n_x >= 2 and every mutation that is
    another computation there (columns_ref.mutation_applies), at least one chord's column changes its bits -- with the
    chi the GPU test's first term carries (1.0), except chi_after, which only a chi != 1 term can show (0.3)."""
    weak = []
    for n_x in NX_ALL:
        if n_x < 2:
            continue
        d = CR.table_design(n_pr, n_orb, n_x)
        rows = d["rows"][d["witness"]]   # the unblocked finite rows: what the GPU test compares bit for bit
        assert len(rows) >= 20 and np.all(np.isfinite(rows))
        for mut in CR.MUTATIONS:
            chi = 0.3 if mut == "chi_after" else 1.0
            if not CR.mutation_applies(mut, n_x, chi):
                continue
            true = CR.columns_emulated(rows, chi, CR.DELTA_X)
            m = CR.columns_emulated(rows, chi, CR.DELTA_X, mut)
            if np.array_equal(bits(true), bits(m)):
                weak.append((n_x, mut))
    assert not weak, weak


def test_every_mutation_applies_somewhere():
    for mut in CR.MUTATIONS:
        assert any(CR.mutation_applies(mut, n, 0.3) for n in NX_ALL), mut


def test_sample_counts_cover_the_classes():
    small, large = set(CR.NX_SMALL), set(CR.NX_LARGE)
    assert max(small) == 64 and min(large) == 65          # the kernel switch
    assert {n % 8 for n in small if n >= 8} == set(range(8))
    assert {n % 8 for n in large} >= {0, 1, 7}
    assert {n for n in small if n < 8} == set(range(1, 8))   # the shuffle loop at every length
    for lo, hi in ((1, 8), (9, 16), (17, 32), (33, 64)):     # k_columns8's samples per lane: 1, 2, 4, 8
        assert any(lo <= n <= hi for n in small)
    for b in (8, 16, 32, 64):
        assert b in small and (b + 1 in small or b + 1 in large)
    assert 128 in large and 129 in large and 256 in large and 257 in large
    halves = {(n // 2) % 8 == 0 for n in large if n > 128}
    assert halves == {True, False}                       # a split on a multiple of 8, and one rounded down to it
    # krem, the slot of the remainder samples, takes every value a lane can hold
    assert {n // 8 for n in small if n >= 8 and n % 8} >= {1, 2, 3, 4, 5, 7}


def test_design_rows_shape():
    a = CR.design_rows(99, 30, CR.design_seed(30))
    assert a.flags.c_contiguous and a.shape == (99, 30)
    zero = np.count_nonzero(a == 0.0) / a.size
    assert 0.2 < zero < 0.3
    nz = a[a > 0]
    assert nz.min() >= 1.0 and nz.max() <= 1e16 and np.log10(nz.max() / nz.min()) > 15
    # a plain sequential sum has other bits than numpy's in a good share of such rows
    seq = CR.columns_emulated(a, 1.0, CR.DELTA_X, "sequential")
    assert np.count_nonzero(bits(seq) != bits(CR.columns_numpy(a, 1.0, CR.DELTA_X))) >= 20


@pytest.mark.parametrize("n_pr,n_orb", CR.GRIDS)
def test_table_design_layout(n_pr, n_orb):
    d = CR.table_design(n_pr, n_orb, 30)
    assert d["rows"].shape == (n_pr, n_orb, 30) and d["blocked"].shape == (n_orb, n_pr)
    per_phase = d["blocked"].sum(axis=1)
    assert np.all(per_phase >= 2) and np.all(per_phase <= n_pr // 4)     # every phase blocks a few chords
    if n_orb > 1:
        assert len({tuple(b) for b in d["blocked"]}) == n_orb             # other ones in every phase
        assert not np.array_equal(d["rows"][:, 0], d["rows"][:, 1])       # a transposed (ip, o) index reads other rows
    (ia, oa), (ib, ob) = d["special"]
    assert ia != ib and not d["blocked"][:, [ia, ib]].any()
    assert np.isinf(d["rows"][ia, oa]).sum() == 1 and np.isnan(d["rows"][ib, ob]).sum() == 1
    assert np.isfinite(d["rows"][d["witness"]]).all() and d["witness"].sum() == n_pr * n_orb - d["blocked"].sum() - 2


def test_blocked_mask_forms():
    # (3, 4) against R = 5: on the limb in either form, not blocked; one ulp more: blocked
    y, z = np.array([3.0, 30.0]), np.array([4.0, 40.0])
    up = np.nextafter(5.0, 6.0)
    assert not CR.blocked_mask(y, z, [0.0], 5.0, np.zeros((0, 1)), []).any()
    assert CR.blocked_mask(y, z, [0.0], up, np.zeros((0, 1)), []).tolist() == [[True, False]]
    assert not CR.blocked_mask(y, z, [100.0], 5.0, [[0.0]], [5.0]).any()
    assert CR.blocked_mask(y, z, [100.0], 5.0, [[0.0]], [up]).tolist() == [[True, False]]
    # a moon at y = 27 in the first phase only: 24^2 + 4^2 = 592 < 1600 < 3^2 + 40^2
    assert CR.blocked_mask(y, z, [100.0, 50.0], 1.0, [[27.0, 100.0]], [40.0]).tolist() == [[True, False], [False, False]]


MP_CASES = {
    CR.BAROMETRIC: [(1e10, 7.0e9, 4.0e8)],
    CR.HYDROSTATIC: [(1e8, 7.0e9, 6.67e-8 * 2.3 * 1.661e-24 * 1.9e30, 1.381e-16 * 1500.0, 12.5)],
    CR.POWERLAW: [(1e5, 7.0e9, 0.0), (1e5, 7.0e9, 6.0), (1e5, 7.0e9, 6.5), (1e5, 7.0e9, 9.0)],
    CR.TORUS: [(1e4, 4.2e10, 4 * 2.0e9, 2.0e9)],
}


@pytest.mark.parametrize("kind", sorted(MP_CASES))
def test_density_ld_against_mpmath(kind):
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(kind)
    for p in MP_CASES[kind]:
        scale = p[1]
        x = rng.uniform(-3, 3, 12) * scale
        y = rng.uniform(-1.2, 1.2, 12) * scale
        z = rng.uniform(-1.2, 1.2, 12) * scale
        bx, by = 0.01 * scale, -0.02 * scale
        val, eps = CR.density_ld(kind, p, x, y, z, bx, by)
        P = [mp.mpf(float(v)) for v in p]
        for i in range(12):
            dx, dy, zz = mp.mpf(float(x[i])) - mp.mpf(bx), mp.mpf(float(y[i])) - mp.mpf(by), mp.mpf(float(z[i]))
            if kind == CR.TORUS:
                a = mp.sqrt(dx * dx + dy * dy)
                want = P[0] * mp.exp(-((a - P[1]) / P[2]) ** 2) * mp.exp(-(zz / P[3]) ** 2)
            else:
                r = mp.sqrt(dx * dx + dy * dy + zz * zz)
                h = 0 if r < P[1] else 1
                if kind == CR.BAROMETRIC:
                    want = P[0] * mp.exp((P[1] - r) / P[2]) * h
                elif kind == CR.HYDROSTATIC:
                    want = P[0] * mp.exp(P[2] / (P[3] * r) * h - P[4])
                else:
                    want = P[0] * (P[1] / r) ** P[2] * h
            hi = float(val[i])   # a longdouble is the exact sum of two doubles
            got = mp.mpf(hi) + mp.mpf(float(val[i] - CR.LD(hi)))
            if want == 0:
                assert got == 0
                continue
            err = abs(got - want) / abs(want)
            # the share of the budget that density_ld claims for itself
            assert err <= CR.LD_SHARE * (eps[i] + 1) * CR.U, (kind, p, i, float(err), eps[i])
