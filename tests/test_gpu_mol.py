"""The molecular path (k_mol_prep, k_columns, k_mol_gt, k_mol_list, k_tau_mol) against the longdouble trilinear reference
of helpers/mol_ref.py, through the raw C-ABI with tabulated densities, at tiny shapes (33 / 64 chords, n_x = 7 / 8,
5 phases, 300 wavelengths, 4 x 3-node tables).  tests/test_mol_ref_cpu.py checks the reference against the oracle,
every design's edges and sensitivity, and that each mistake of mol_ref.MUTATIONS moves R by more than 100 bounds.

The bound (mol_ref.tolerance; u = 2^-53, first order in u, worst case, nothing cancels).  Vmax = max |V| of the
design's tables, Y = Vmax 1024 log2 10, tau's relative error eta gives |dR| <= max(tau e^-tau) eta <= eta / e.

  k_mol_gt   a node value y = ((1 - t_T) V0 + t_T V1) 1024 log2 10: the complement, two products, the sum, the scaling
             and its rounded constant: 6 u Y.  s_i = y(i, w + 1) - y(i, w): two such and a rounding of |s| <= 2 Y:
             14 u Y.  dg = g_{i+1} - g_i likewise 14 u Y; ds = s_{i+1} - s_i: 2 x 14 + 4 = 32 u Y (the cancellation
             in s and ds is why these are absolute, in Y, and not relative to the small differences).
  k_tau_mol  fma(t_w, ds, dg): 32 + 14 + 2 = 48 u Y; fma(t_w, s, g): 14 + 6 + 1 = 21 u Y; fma(t_P, ., .): 48 + 21 + 1 =
             70 u Y; the weights t_w and t_P, each (a - b) / (c - b) in float64, 3 u relative, times what they
             multiply (|s| + |ds| <= 6 Y, |dg + t_w ds| <= 2 Y): 24 u Y.  Sum: 94 u Y in y, that is 94 u Vmax in v and
             E_v = 94 Vmax ln10 u relative in 10^v (the argument scaling |v| ln10 u, ninety-four times over).
             10^v - offset from the LDS table: e = (y - k) ln2 / 1024 (1 u), the cubic's three FMAs (1.5 u), its
             truncation e^4 / 24 <= 5.5e-16 (5 u), the table entry (1 u), the final FMA (0.5 u): E_exp = 9 u, relative
             to 10^v = sigma + offset, so both times A_off = max 10^v / (10^v - offset) over the table (1.01 at most).
             The record's sum: n_abs = fl(n chi) and K = n_mol n_x FMAs of positive terms: (K + 1) u.  Atoms add
             N sigma: N's pairwise sum n_x u, sigma's exp10 and offset 5 u (ocml, supposed), product and sum 3 u:
             (n_x + 8) u on their share, so E_tau = max(mol, atoms) + (n_atoms + 1) u for the sums + 3 u for
             -tau 1024 / ln2 (delta_x's product, the constant, the product with the sum).
             exp of tau: the same table exp, 9 u, and F's product 1 u: 10 u on e^-tau <= 1; F = fout / sum (sums of
             small integers: exact) 1 u; the disk sum over at most n_pr records, the transparent share and the folded
             weight sum: (n_pr + 3) u on R <= 1.  E_disk = (n_pr + 14) u.
  bound      (E_tau / e + E_disk) u (1 + 2^-9) (the longdouble reference's own share), plus, where mirror pairs merge,
             DESIGN.md's 2^-40 (1 + D ln10) / e with D the largest step between the table's adjacent P rows.
  ocml path  (PROM_OPT_OCML_EXP) exp2 and exp at 2 ulp = 4 u each are supposed, as in test_gpu_columns.py: the installed
             ROCm states no bound.  4 u + 1 u <= E_exp, so the same bound serves.
For |v| <= 22 this is 1.9e-13, with the 1e-38 table of the slot designs 3.6e-13, for the flat table of `poly` 1e-14.

Measured worst error over bound per design and path: profiles/mol_errors.txt (written from this module's output when
PROM_MOL_RECORD names a file).  A ratio above 1 is a finding to explain, not a reason to loosen.

Route: every run asserts tau_kernel_variant (10 + atoms on the table-exp path, atoms with the ocml option), the count
of exact phases, and exp_evals = listed in-table samples x in-table lanes (mol_ref.predicted_evals), which shows
which mirror pairs merged and which samples were listed (the stats add one e^-tau per record and lane).  k_tau_mol<NSA, EXPK, M1>: the slot designs run NSA in
{0, 1, 4} with one slot (M1) and with two and four (not M1) on both exp paths -- 12 of the 20 instances; NSA = 2, 3
differ by the unrolled atom loop alone.
"""
import copy
import os

import numpy as np
import pytest

from helpers import mol_ref as M

pytestmark = pytest.mark.gpu

ENV_KEYS = ("PROM_MOL_STAGE", "PROM_MOL_PPG", "PROM_MOL_MIRROR", "PROM_GRAPH", "PROM_DEBUG")


@pytest.fixture(scope="module")
def dev():
    from prometheus_amd import _native
    return _native.get_device(0)


class Tables:
    """The design's molecular tables and the atoms' flat tables on the device."""

    def __init__(self, dev, d):
        self.dev, self.mol, self.atom = dev, [], {}
        with dev.lock:
            for t in d["tables"]:
                self.mol.append(dev.molecular_upload(t["P"], t["T"], t["W"], t["V"], t["offset"]))
            for a in M.atom_slots(d):
                if a["atom"] not in self.atom:
                    y = np.log10(M.ATOM_SIGMA[a["atom"]] + M.ATOM_OFFSET)
                    self.atom[a["atom"]] = dev.table_upload(M.ATOM_W, np.array([y, y]), M.ATOM_OFFSET)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        with self.dev.lock:
            for t in self.mol:
                self.dev.table_free(t, molecular=True)
            for t in self.atom.values():
                self.dev.table_free(t)


def problem(d, tb, options=0, wav=None):
    from prometheus_amd import _native
    scs = []
    for sc in d["scenarios"]:
        cons = [{"table_id": tb.mol[c["table"]], "chi": c["chi"], "is_molecule": True} if c["kind"] == "mol" else
                {"table_id": tb.atom[c["atom"]], "chi": c["chi"]} for c in sc["cons"]]
        scs.append({"kind": _native.DENSITY_TABULATED, "params": [], "shift": sc["shift"], "T": sc["T"],
                    "n_tabulated": np.ascontiguousarray(sc["rows"]).ravel(), "constituents": cons})
    n_orb = d["n_orb"]
    return _native.TransitInputs(
        wavelength=d["wav"] if wav is None else wav, chord_y=d["y"], chord_z=d["z"], chord_fout=d["fout"], n_orb=n_orb,
        x=np.arange(float(d["n_x"])), delta_x=d["dx"], planet_y=d["planet_y"], planet_R=d["planet_R"],
        moon_y=np.zeros((0, n_orb)), moon_R=np.zeros(0), scenarios=scs, options=options, k_B=M.KB)


def run(dev, monkeypatch, d, tb, env=(), ocml=False, wav=None, runs=1):
    """One set, `runs` runs (the last one a stats run): (stats, R).  A HIP error ends the session: nothing more is
    started on a device that has faulted."""
    from prometheus_amd import _native
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    try:
        with dev.lock:
            dev.transit_set(problem(d, tb, options=_native.OPT_OCML_EXP if ocml else 0, wav=wav))
            for _ in range(runs - 1):
                dev.transit_run()
            st = dev.transit_run(stats=True)
            R = dev.transit_result()
    except _native.NativeError as e:
        if "PROM_E_HIP" in str(e):
            pytest.exit("HIP error in %s: %s" % (d["name"], e), returncode=3)
        raise
    return st, R


def check_route(d, st, ocml):
    na = len(M.atom_slots(d))
    L = M.listing(d)
    what = (d["name"], ocml, st)
    assert st["tau_kernel_variant"] == (na if ocml else 10 + na), what
    assert st["exact_phases"] == int(L["exact"].sum()), what
    assert st["blocked_chords"] == int(L["blocked"].sum()) and st["active_chords"] == int(L["active"].sum()), what
    # (exp_evals: the 10^v of every listed in-table sample on its in-table lanes, and one e^-tau per record and lane)
    n_wav = len(d["wav"])
    assert st["tau_records"] == int(L["active"].sum()), what
    assert st["exp_evals"] - st["tau_records"] * n_wav == M.predicted_evals(d, table_exp=not ocml), what


def record(line):
    print(line)
    path = os.environ.get("PROM_MOL_RECORD")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def check_accuracy(d, R, path):
    ref = M.reference(d)["R"]
    bound, _ = M.tolerance(d)
    nan = np.isnan(ref)
    err = np.abs(R.astype(M.LD) - ref)[~nan]
    worst = float(err.max()) if err.size else 0.0
    record("%-30s %-8s worst |R - R_ref| %.3e  bound %.3e  ratio %.4f  (NaN points %d)" % (
        d["name"], path, worst, bound, worst / bound, int(nan.sum())))
    assert np.all(np.isnan(R[nan])), "%s %s: the reference is NaN at %d points, the device at %d of them" % (
        d["name"], path, int(nan.sum()), int(np.isnan(R[nan]).sum()))
    assert not np.isnan(R[~nan]).any(), "%s %s: NaN where the reference is finite" % (d["name"], path)
    assert worst <= bound, "%s %s: |R - R_ref| = %.3e, %.2f of the bound" % (d["name"], path, worst, worst / bound)


# ---- accuracy and route --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ocml", [False, True], ids=["table", "ocml"])
@pytest.mark.parametrize("name", M.NAMES)
def test_accuracy_and_route(dev, monkeypatch, name, ocml):
    d = M.design(name)
    with Tables(dev, d) as tb:
        st, R = run(dev, monkeypatch, d, tb, ocml=ocml)
    check_accuracy(d, R, "ocml" if ocml else "table")
    check_route(d, st, ocml)


# ---- bitwise invariants --------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", M.STAGE)
def test_stage_off_bitwise(dev, monkeypatch, name):
    """PROM_MOL_STAGE=0 (every record from global memory) against the LDS stage, with one group per phase and with all
    five phases in one group (where later phases' waves leave the staged range or find nothing staged)."""
    d = M.design(name)
    with Tables(dev, d) as tb:
        for ppg in ((), (("PROM_MOL_PPG", "5"),)):
            _, R1 = run(dev, monkeypatch, d, tb, env=ppg)
            _, R0 = run(dev, monkeypatch, d, tb, env=ppg + (("PROM_MOL_STAGE", "0"),))
            assert np.array_equal(bits(R0), bits(R1)), (name, ppg)
            check_accuracy(d, R1, "ppg5" if ppg else "ppg-def")


@pytest.mark.parametrize("name", list(M.BRACKETS) + M.STAGE + ["slots-2m1a", "slots-4m0a", "lists-mod4"])
def test_phase_groups_bitwise(dev, monkeypatch, name):
    """PROM_MOL_PPG = 1, 2, 5: a phase's bracket searched afresh (first phase of a group) or walked from the previous
    phase's (cached nodes, repeated Doppler factors skipped): the same bits."""
    d = M.design(name)
    with Tables(dev, d) as tb:
        R = [run(dev, monkeypatch, d, tb, env=(("PROM_MOL_PPG", p),))[1] for p in ("1", "2", "5")]
    assert np.array_equal(bits(R[0]), bits(R[1])) and np.array_equal(bits(R[0]), bits(R[2])), name
    check_accuracy(d, R[2], "ppg5")


@pytest.mark.parametrize("name", ["axes-T512-uniform", "slots-4m4a", "mirror", "lists-atoms"])
def test_pipelined_runs_bitwise(dev, monkeypatch, name):
    """Four runs back to back over the pipeline slots: the last one's R is the single run's."""
    d = M.design(name)
    with Tables(dev, d) as tb:
        st1, R1 = run(dev, monkeypatch, d, tb)
        st4, R4 = run(dev, monkeypatch, d, tb, runs=4)
    assert np.array_equal(bits(R1), bits(R4)) and st1["exp_evals"] == st4["exp_evals"], name


@pytest.mark.parametrize("name", ["axes-T700-geometric-clipnode", "stage-clamp", "slots-2m0a", "lists-mod4"])
def test_mirror_off_bitwise(dev, monkeypatch, name):
    """Without mergeable pairs PROM_MOL_MIRROR=0 changes nothing (64-chord designs have no pair at all, and none of the
    33-chord ones)."""
    d = M.design(name)
    assert not d["mergeable"]
    with Tables(dev, d) as tb:
        st1, R1 = run(dev, monkeypatch, d, tb)
        st0, R0 = run(dev, monkeypatch, d, tb, env=(("PROM_MOL_MIRROR", "0"),))
    assert np.array_equal(bits(R1), bits(R0)) and st1["exp_evals"] == st0["exp_evals"], name


def test_mirror_merging_counts(dev, monkeypatch):
    """The mirror design: exp_evals with merging is the prediction with the pairs mol_ref.listing merges (equal and
    2^-41 pairs; not the 2^-39 and 2^-30 ones, the pair with another count, the pair half behind the planet);
    without, every active chord's samples."""
    d = M.design("mirror")
    with Tables(dev, d) as tb:
        st1, R1 = run(dev, monkeypatch, d, tb)
        st0, R0 = run(dev, monkeypatch, d, tb, env=(("PROM_MOL_MIRROR", "0"),))
    rec = st1["tau_records"] * len(d["wav"])
    assert st1["tau_records"] == st0["tau_records"]
    assert st1["exp_evals"] - rec == M.predicted_evals(d) < st0["exp_evals"] - rec == M.predicted_evals(d, table_exp=False)
    nomerge = dict(d, mergeable=False)
    bound0, _ = M.tolerance(nomerge)
    ref = M.reference(d)["R"]
    assert float(np.abs(R0.astype(M.LD) - ref).max()) <= bound0
    check_accuracy(d, R1, "merged")


@pytest.mark.parametrize("name", ["brackets-geometric", "brackets-uniform", "stage-wide", "slots-2m0a"])
def test_wavelength_order_bitwise(dev, monkeypatch, name):
    """The wavelengths in descending order (k_tau_mol's wave reduction instead of the first and last lane): R reversed."""
    d = M.design(name)
    with Tables(dev, d) as tb:
        _, Ra = run(dev, monkeypatch, d, tb, env=(("PROM_MOL_PPG", "5"),))
        _, Rd = run(dev, monkeypatch, d, tb, env=(("PROM_MOL_PPG", "5"),), wav=np.ascontiguousarray(d["wav"][::-1]))
    assert np.array_equal(bits(Ra), bits(Rd[:, ::-1])), name


# ---- a slot whose T lies outside its table, after a run that left overflowing records behind --------------------------------
def hot_variant(d):
    """The same shapes with every table value 400 (2^(y / 1024) overflows) and every temperature inside the table."""
    h = copy.deepcopy({k: v for k, v in d.items() if k != "_ref"})
    for t in h["tables"]:
        t["V"] = np.full_like(t["V"], 400.0)
    for sc in h["scenarios"]:
        sc["T"] = 512.0
    return h


@pytest.mark.parametrize("ocml", [False, True], ids=["table", "ocml"])
@pytest.mark.parametrize("name", ["axes-Tout-hi", "axes-Tout-lo", "slots-2m0a-tout", "slots-4m1a-tout"])
def test_temperature_outside_after_overflowing_records(dev, monkeypatch, name, ocml):
    """k_mol_gt's records of an earlier problem must not reach R through a slot whose T is outside its table: sigma is
    exactly 0 there (10^fill - offset).  First a run of the same shapes whose records overflow, then the design."""
    d = M.design(name)
    h = hot_variant(d)
    with Tables(dev, h) as th:
        st, Rh = run(dev, monkeypatch, h, th, ocml=ocml)     # (the upload accepts 400.0: no range check)
        assert st["tau_kernel_variant"] % 10 == len(M.atom_slots(d))
        with Tables(dev, d) as tb:
            st, R = run(dev, monkeypatch, d, tb, ocml=ocml)
    check_accuracy(d, R, "hot-" + ("ocml" if ocml else "table"))
    if name.startswith("axes"):
        # one slot, outside: R is the unblocked flux share
        share = 1.0 - M.listing(d)["blocked"].sum(axis=1) / d["n_pr"]
        assert float(np.abs(R - share[:, None]).max()) <= M.tolerance(d)[0]
    check_route(d, st, ocml)


# ---- a NaN density sample ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ocml", [False, True], ids=["table", "ocml"])
@pytest.mark.parametrize("name", ["nan-mol", "nan-mol-atom"])
def test_nan_sample(dev, monkeypatch, name, ocml):
    """One NaN sample on one unblocked chord of one phase: that phase's R is NaN at every wavelength, in-table or not,
    as in the reference (scipy's interpolator returns NaN for a NaN coordinate and n_abs is NaN as well); the other
    phases stay within the bound.  With an atom the phase is an exact one (the atom's column is NaN)."""
    d = M.design(name)
    o, _ip = d["nan"]
    with Tables(dev, d) as tb:
        st, R = run(dev, monkeypatch, d, tb, ocml=ocml, env=(("PROM_MOL_PPG", "5"),))
    assert np.isnan(R[o]).all(), "%d of %d points of the NaN phase are finite" % (int((~np.isnan(R[o])).sum()), R.shape[1])
    assert st["exact_phases"] == (1 if name.endswith("atom") else 0)
    check_route(d, st, ocml)
    check_accuracy(d, R, "nan-" + ("ocml" if ocml else "table"))
