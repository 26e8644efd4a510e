"""The molecular path's reference and designs (helpers/mol_ref.py) on the CPU: the longdouble reference against the
oracle's scipy interpolation, every design's own assertions (the edges it is named for, sensitivity, list lengths, the
stage rule, merged and unmerged pairs), and the mutation check -- each wrong computation listed in mol_ref.MUTATIONS,
applied to the reference itself, moves R by more than a hundred times the tolerance tests/test_gpu_mol.py allows the
device, so a kernel that made the mistake could not pass there."""
import numpy as np
import pytest

from helpers import mol_ref as M


@pytest.mark.parametrize("name", M.NAMES)
def test_design_reaches_its_edges(name):
    facts = M.check_design(name)
    assert facts["sensitive"] >= 0.5
    bound, parts = M.tolerance(M.design(name))
    # |v| <= 40 in every design: a few 1e-13, and below 2e-12 with the merging term
    assert 5e-15 < bound < (2e-12 if parts["merge"] else 5e-13), (name, bound, parts)


@pytest.mark.parametrize("name", M.NAMES)
def test_reference_against_the_oracle(name):
    """tau and R from oracle.prom_oracle's RegularGridInterpolator (molecular_interpolator / molecular_sigma and
    optical_depth's two lines around them) in float64: R within 1e-12 of the longdouble reference (scipy's float64
    trilinear value carries ~8 |v| ln10 u < 1e-13 relative into sigma), NaN in the same places, sigma exactly 0 at the
    fill value and nowhere else."""
    from oracle import prom_oracle as O
    d = M.design(name)
    ref = M.reference(d)
    n_pr, n_orb, n_wav = d["n_pr"], d["n_orb"], len(d["wav"])
    tau = np.zeros((n_orb, n_pr, n_wav))
    with np.errstate(invalid="ignore"):
        for s in M.mol_slots(d):
            tab = d["tables"][s["table"]]
            rgi = O.molecular_interpolator(tab, offset=s["offset"])
            assert all(np.array_equal(a, b) for a, b in zip(rgi.grid, (tab["P"], tab["T"], tab["W"])))
            assert np.array_equal(rgi.values, tab["V"])
            rows = d["scenarios"][s["sc"]]["rows"]
            inT, _ = M.brackets(tab["T"], s["T"])
            for o in range(n_orb):
                P = (rows[:, o, :] * M.KB) * s["T"]                       # gasProperties.py:925  n_tot k_B T
                lam = np.broadcast_to(s["shift"][o] * d["wav"], (n_pr, n_wav))
                sig = O.molecular_sigma(rgi, P, s["T"], lam, offset=s["offset"])
                inP, _ = M.brackets(tab["P"], M.pressure(rows[:, o, :], s["T"]))
                inW, _ = M.brackets(tab["W"], lam[0])
                inside = inP[:, :, None] & inW[None, None, :] & bool(inT)
                fin = ~np.isnan(rows[:, o, :])
                assert np.all(sig[~inside & fin[:, :, None]] == 0.0), "sigma is not exactly 0 at the fill value"
                assert np.all(sig[inside] > 0.0)
                assert np.all(np.isnan(sig[~fin]))                          # scipy: a NaN coordinate gives NaN
                tau[o] += np.einsum("cx,cxw->cw", rows[:, o, :] * s["chi"], sig) * d["dx"]
        for a in M.atom_slots(d):
            rows = d["scenarios"][a["sc"]]["rows"]
            y = np.log10(M.ATOM_SIGMA[a["atom"]] + M.ATOM_OFFSET)
            sg = O.interp_log(np.array([2.0e-4]), M.ATOM_W, np.array([y, y]), M.ATOM_OFFSET)[0]
            tau += ((np.sum(rows * a["chi"], axis=2) * d["dx"]).T * sg)[:, :, None]
        blocked = ref["blocked"]
        F = d["fout"] / d["fout"].sum()
        R = np.einsum("c,ocw->ow", F, np.where(blocked[:, :, None], 0.0, np.exp(-tau)))
    Rr = ref["R"].astype(np.float64)
    assert np.array_equal(np.isnan(R), np.isnan(Rr))
    unb = ~blocked[:, :, None] & np.ones(tau.shape, dtype=bool)
    assert np.array_equal(np.isnan(tau)[unb], np.isnan(ref["tau"].astype(np.float64))[unb])
    ok = ~np.isnan(R)
    err = float(np.abs(R[ok] - Rr[ok]).max())
    assert err < 1e-12, (name, err)
    t64 = ref["tau"].astype(np.float64)
    m = unb & ~np.isnan(tau) & (t64 > 0)
    assert np.array_equal(tau[unb & ~np.isnan(tau)] == 0.0, t64[unb & ~np.isnan(tau)] == 0.0)
    assert not m.any() or float(np.abs(tau[m] / t64[m] - 1.0).max()) < 1e-12


def test_stage_rule_restated():
    """stage_plan's rule is the kernel's: n_ * n_int * 2 <= 1216 double2 of LDS, n_int = n_p - 1 = 3 intervals: at most
    202 nodes; the 700-node design's first workgroup needs more, its second (44 live lanes) less."""
    assert M.STAGE_D2 == 1216 and 202 * 3 * 2 <= M.STAGE_D2 < 203 * 3 * 2
    d = M.design("stage-wide")
    p = M.stage_plan(d, 1)
    assert p["staged"][(0, 0)] is None
    lo, n = p["staged"][(0, 1)]
    assert 3 <= n <= 202 and lo + n <= len(d["tables"][0]["W"]) - 1


def test_list_lengths_cover_every_tail():
    """K mod 4 = 0, 1, 2, 3 and K = 0 (k_tau_mol reads fours, then a pair, then a single), with and without atoms."""
    for name in ("lists-mod4", "lists-atoms"):
        K = M.listing(M.design(name))["K"]
        assert [int(k) % 4 for k in K[:4]] == [0, 1, 2, 3], (name, K)
    assert M.listing(M.design("lists-mod4"))["K"][4] == 0


def test_every_instance_is_reached():
    """k_tau_mol<NSA in {0, 1, 4}, EXPK in {0, 1}, M1 in {true, false}>: the slot designs' counts (each runs on both exp
    paths in tests/test_gpu_mol.py)."""
    got = {(len(M.atom_slots(M.design(n))), len(M.mol_slots(M.design(n))) == 1) for n in M.SLOT_NAMES}
    assert got == {(a, m1) for a in (0, 1, 4) for m1 in (True, False)}


MUTATION_DESIGNS = {
    "excl_P": ["axes-T512-uniform", "axes-T1024-clipnode"], "excl_T": ["axes-T300-uniform", "axes-T1100-geometric"],
    "excl_W": ["axes-T512-uniform"], "no_clip": ["axes-T512-uniform", "axes-T1024-clipnode"],
    "prev_iw": ["brackets-uniform", "brackets-geometric"], "prev_tw": ["brackets-uniform"],
    "slot_T": ["slots-2m0a", "slots-4m1a"], "slot_offset": ["slots-2m0a"], "slot_chi": ["slots-2m0a"],
    "slot_shift": ["slots-2m0a"], "drop_last_1": ["lists-mod4"], "drop_last_2": ["lists-mod4"],
    "drop_last_3": ["lists-mod4"], "quadratic": ["poly"], "swap_t": ["axes-T512-uniform"], "merge_2m30": ["mirror"],
    "nan_dropped": ["nan-mol"]}


@pytest.mark.parametrize("mut", M.MUTATIONS)
def test_mutation_is_detected(mut):
    """In every design listed for it, the mutated reference leaves the true one by more than 100 bounds (a NaN that
    appears or disappears counts as such)."""
    assert sorted(MUTATION_DESIGNS) == sorted(M.MUTATIONS)
    for name in MUTATION_DESIGNS[mut]:
        d = M.design(name)
        a, b = M.reference(d)["R"], M.reference(d, mut=mut)["R"]
        bound, _ = M.tolerance(d)
        if not np.array_equal(np.isnan(a), np.isnan(b)):
            continue
        ok = ~np.isnan(a)
        ratio = float(np.abs(a[ok] - b[ok]).max()) / bound
        print("%s on %s: %.3g bounds" % (mut, name, ratio))
        assert ratio > 100.0, (mut, name, ratio)
