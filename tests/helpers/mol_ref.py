"""Designs and a longdouble reference for the molecular path (k_mol_prep, k_columns, k_mol_gt, k_mol_list, k_tau_mol):
plain numpy, no GPU.

A design is a tiny transit problem in the raw C-ABI's terms: tabulated densities n[ip][o][x] (so the device integrates
exactly the stored samples), molecular tables of n_p = 4 x n_t = 3 nodes, atoms with a flat two-node table of known
sigma, and k_B = 2^-60.  With a slot temperature that is a power of two, P = fl(fl(n k_B) T) = n 2^-60 T exactly, so a
density sample can be put on a table node, one ulp inside or outside either end, or below the clip at 1e-4.

reference(d)   Bracket decisions as the upstream code makes them, in float64: P = fl(fl(n k_B) T) clipped below at 1e-4,
               lambda' = fl(shift_o lambda_w), scipy's bracket (searchsorted-left minus one clipped to [0, n - 2]), both
               table ends inclusive, the fill value (sigma = 0 exactly) outside any axis.  Everything after the bracket in
               np.longdouble: the weights, the trilinear value, 10^v - offset, tau_c = dx sum_x n chi sigma over the slots
               plus the atoms' N sigma, R = sum_unblocked F_c e^-tau_c / sum_all F_c.  NaN propagates as in numpy: a NaN
               density sample makes its chord's tau, and so the phase's R, NaN at every wavelength.
               `mut` names one wrong computation (MUTATIONS); tests/test_mol_ref_cpu.py shows that each moves R by more
               than a hundred times the GPU test's tolerance somewhere in the designs.
tolerance(d)   The bound of tests/test_gpu_mol.py (derived in that module's docstring) for this design.
listing(d)     The device's sample lists restated (float64, k_mol_prep's and k_mol_list's rules): active chords, each
               phase's entries and their count K, the mirror pairs that merge, and from them exp_evals.
stage_plan(d)  k_tau_mol's LDS stage restated: which workgroups stage their node range (n_ n_int 2 <= 1216), where the
               margin is clamped, and which waves of later phases leave the staged range.

Every design asserts on the CPU (check_design) that it reaches the edges it is named for and that R is sensitive:
at least half of the (phase, lambda) points with any in-table sample have sum_c (F_c / sum F) tau_c e^-tau_c >= 0.05,
which is what lets a tolerance on R pin the per-sample arithmetic (|dR| = tau e^-tau |dtau / tau|).

A record without an in-table sample and without atoms cannot be active with finite tables (its bound is 0: the chord is
transparent), so no design reaches k_mol_list's folded weight sum; with atoms such a record is listed as one zero-weight
entry (design lists-atoms).
"""
import functools

import numpy as np

from helpers import columns_ref as CR

LD = np.longdouble
U = 2.0 ** -53
LN10 = float(np.log(10.0))
KB = 2.0 ** -60
T_AXIS = np.array([300.0, 700.0, 1100.0])
DX = 0.7
N_WAV = 300
KBLOCK = 256
STAGE_D2 = 1216            # kMolStageD2
STAGE_MARGIN = 1           # kMolStageMargin
MIRROR_TOL = 2.0 ** -40    # kMolMirrorTol
CULL = 2.0 ** -60          # prom_transit_set's default cull_tau
KAPPA = 1024.0 * float(np.log2(10.0))
ATOM_SIGMA = [1e-20, 3e-21, 2e-20, 5e-21]
ATOM_OFFSET = 1e-50
ATOM_W = np.array([1.0e-5, 1.0e-2])

MUTATIONS = ["excl_P", "excl_T", "excl_W", "no_clip", "prev_iw", "prev_tw", "slot_T", "slot_offset", "slot_chi",
             "slot_shift", "drop_last_1", "drop_last_2", "drop_last_3", "quadratic", "swap_t", "merge_2m30",
             "nan_dropped"]


# ---- tables ------------------------------------------------------------------------------------------------------------
def make_table(n_w, wkind, p0, vbase, vspread, offset, seed, w_lo=1.0e-4, flat=None):
    """A table in the upstream file's terms (p, t, bin_edges, xsecarr) and in the device's (P = p 10, W = 1 / bin_edges
    reversed, V = log10(xsecarr reversed + offset)), derived the way gasProperties.py:774-781 derives them, so that
    oracle.prom_oracle.molecular_interpolator sees the same nodes bit for bit."""
    rng = np.random.default_rng([int(seed), int(n_w)])
    p = np.array([p0, 1e-2, 1.0, 1e2]) / 10.0
    if wkind == "uniform":
        wt = np.linspace(w_lo, 1.2 * w_lo, n_w)
    elif wkind == "geometric":
        wt = np.geomspace(w_lo, 4.0 * w_lo, n_w)
    else:
        raise ValueError(wkind)
    be = np.ascontiguousarray((1.0 / wt)[::-1])
    vt = np.full((4, 3, n_w), float(flat)) if flat is not None else vbase + rng.uniform(0.0, vspread, (4, 3, n_w))
    xs = np.ascontiguousarray((10.0 ** vt)[:, :, ::-1])
    t = {"p": p, "t": T_AXIS.copy(), "bin_edges": be, "xsecarr": xs, "offset": float(offset), "wkind": wkind}
    t["P"] = p * 10.0
    t["T"] = t["t"]
    t["W"] = np.ascontiguousarray(1.0 / be[::-1])
    t["V"] = np.ascontiguousarray(np.log10(xs[:, :, ::-1] + offset))
    assert np.all(np.diff(t["W"]) > 0) and np.all(np.diff(t["P"]) > 0)
    return t


def brackets(g, v, exclusive=False):
    """scipy's RegularGridInterpolator: (inside, i) for float64 v on the ascending grid g; NaN is never inside."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = (v > g[0]) & (v < g[-1]) if exclusive else (v >= g[0]) & (v <= g[-1])
    i = np.clip(np.searchsorted(g, v, side="left") - 1, 0, len(g) - 2)
    return inside, i


def weight_ld(g, v, i):
    g = np.asarray(g, dtype=np.float64).astype(LD)
    return (np.asarray(v, dtype=np.float64).astype(LD) - g[i]) / (g[i + 1] - g[i])


def weight_f64(g, v, i):
    """The device's weight: (v - g[i]) / (g[i + 1] - g[i]) in float64 (rgi_bracket)."""
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (np.asarray(v, dtype=np.float64) - g[i]) / (g[i + 1] - g[i])


# ---- geometry ------------------------------------------------------------------------------------------------------------
PLANET_Y = np.array([-6.0, 0.25, 7.0, -2.5, 3.3])
PLANET_R = 2.0


def geometry(n_pr, n_orb, mirror=False):
    """33 (or any count of) chords on a zigzag, none the mirror image of another; `mirror`: 64 chords, 16 exact pairs
    (y, +-z) and 32 unpaired ones on z = 0."""
    if mirror:
        assert n_pr == 64
        k = np.arange(16)
        yp = -9.5 + 1.2 * k
        zp = 0.3 + 0.1 * (k % 4)
        y = np.concatenate([yp, yp, np.linspace(-10.0, 10.0, 32) + 0.05])
        z = np.concatenate([zp, -zp, np.zeros(32)])
    else:
        i = np.arange(n_pr)
        y = np.linspace(-10.0, 10.0, n_pr)
        z = 0.5 * ((i % 5) - 2.0) + 0.01 * (i % 3)
    return {"y": y, "z": z, "planet_y": PLANET_Y[:n_orb].copy(), "planet_R": PLANET_R, "fout": np.ones(n_pr)}


def mirror_pairs(y, z):
    """prom_transit_set's pairing: sorted by y, each unpaired chord with z != 0 takes the first later chord within 1e-9
    (relative to its radius) of (y, -z).  mirror[ip] = partner or -1."""
    n = len(y)
    mir = np.full(n, -1, dtype=np.int64)
    order = sorted(range(n), key=lambda a: (y[a], a))
    for a, i in enumerate(order):
        if mir[i] >= 0 or not (z[i] != 0.0):
            continue
        tol = 1e-9 * max(abs(y[i]), abs(z[i]))
        for j in order[a + 1:]:
            if not (y[j] - y[i] <= tol):
                break
            if mir[j] < 0 and abs(z[j] + z[i]) <= tol:
                mir[i], mir[j] = j, i
                break
    return mir


# ---- densities -----------------------------------------------------------------------------------------------------------
def n_for_P(P, T):
    """n with fl(fl(n k_B) T) = P exactly, for T a power of two."""
    m, _ = np.frexp(T)
    assert m == 0.5, "exact P needs a power-of-two temperature"
    return np.asarray(P, dtype=np.float64) / (KB * T)


def special_P(tab):
    """The P edges of a table: every node, one ulp inside and outside each end, two values below the clip, and 0."""
    P = tab["P"]
    return np.concatenate([P, [np.nextafter(P[0], 0.0), np.nextafter(P[0], 1.0), np.nextafter(P[-1], 0.0),
                               np.nextafter(P[-1], np.inf), 3.0e-5, 2.0e-6, 0.0]])


def design_rows(n_pr, n_orb, n_x, T, tab, seed, specials=True, spread=1.0):
    """[n_pr, n_orb, n_x]: most samples with P log-uniform in the table's top two decades times a factor per chord
    (10^-spread .. 1: the chords' tau spread), a quarter (with `specials`) on the table's P edges."""
    rng = np.random.default_rng([int(seed), n_pr, n_orb, n_x])
    scale = 10.0 ** rng.uniform(-spread, 0.0, (n_pr, 1, 1))
    P = scale * 10.0 ** rng.uniform(0.3, 1.95, (n_pr, n_orb, n_x))
    pow2 = np.frexp(T)[0] == 0.5
    rows = n_for_P(P, T) if pow2 else P / (KB * T)
    if specials:
        sp = special_P(tab)
        pick = rng.random((n_pr, n_orb, n_x)) < 0.25
        which = rng.integers(0, len(sp), (n_pr, n_orb, n_x))
        ns = n_for_P(sp, T) if pow2 else sp / (KB * T)
        rows = np.where(pick, ns[which], rows)
        # every special value at least once, in chords that no phase blocks
        free = np.where(~CR.blocked_mask(geometry(n_pr, n_orb)["y"], geometry(n_pr, n_orb)["z"], PLANET_Y[:n_orb],
                                         PLANET_R, np.zeros((0, n_orb)), []).any(axis=0))[0]
        for k in range(len(sp)):
            rows[free[k % len(free)], k % n_orb, k % n_x] = ns[k]
    return np.ascontiguousarray(rows)


SHIFT_A = np.array([1.0, 1.0, 1.0 + 1e-7, 1.1, 0.93])          # repeat, inside the bracket, many nodes up, many down
SHIFT_B = np.array([1.0 - 1e-6, 2.0, 1.0, 1.0 + 2e-4, 1.0 + 2e-4])   # out of the table at one phase and back; one node


def wav_for(tab, n_wav=N_WAV, margin=0.03, descending=False, inside=False):
    """Wavelengths across the table: a margin outside both ends (lanes in and out of the table within one wave) and,
    in place of the nearest grid values, the ends, one ulp inside and outside each, and two interior nodes."""
    W = tab["W"]
    if inside:    # two per cent inside both ends: no lane leaves the table, no staged range touches an end
        w = np.linspace(W[0] * 1.02, W[-1] * 0.98, n_wav)
    else:
        w = np.linspace(W[0] * (1 - margin), W[-1] * (1 + margin), n_wav)
        sp = [W[0], np.nextafter(W[0], 0.0), np.nextafter(W[0], 1.0), W[-1], np.nextafter(W[-1], 0.0),
              np.nextafter(W[-1], 1.0), W[5], W[len(W) // 2]]
        used = set()
        for v in sp:
            k = next(int(j) for j in np.argsort(np.abs(w - v)) if int(j) not in used)
            used.add(k)
            w[k] = v
        w = np.sort(w)
        assert len(np.unique(w)) == n_wav
    return np.ascontiguousarray(w[::-1] if descending else w)


# ---- designs -------------------------------------------------------------------------------------------------------------
def _finish(d):
    d["n_pr"], d["n_orb"], d["n_x"] = d["scenarios"][0]["rows"].shape
    d.setdefault("dx", DX)
    d.setdefault("mergeable", False)
    d.setdefault("nan", False)
    return d


def _scale_chi(d, target=0.7):
    """Mixing ratios so that the chords' median tau (at the in-table wavelengths, molecules with chi as drawn relative
    to each other) is `target`; atoms then add 0.3 of that each."""
    for sc in d["scenarios"]:
        for c in sc["cons"]:
            c["chi"] = c.get("rel", 1.0)
    ref = reference(d, _raw=True)
    tau = ref["tau"].astype(np.float64)
    ok = ~ref["blocked"][:, :, None] & np.isfinite(tau) & (tau > 0)
    med = float(np.median(tau[ok])) if ok.any() else 1.0
    for sc in d["scenarios"]:
        rows = np.where(np.isfinite(sc["rows"]), sc["rows"], 0.0)
        for c in sc["cons"]:
            if c["kind"] == "mol":
                c["chi"] = c["chi"] * target / med
            else:
                colmed = float(np.median(rows.sum(axis=2))) * d["dx"]
                c["chi"] = 0.3 * target / (colmed * ATOM_SIGMA[c["atom"]])
    return d


def single(name, n_pr, n_x, T, wkind, n_w, p0=1e-5, seed=1, shift=SHIFT_A, descending=False, specials=True, atoms=0,
           n_orb=5, inside=False, offset=1e-50, margin=0.03, vbase=-21.0, vspread=1.5, flat=None, spread=1.0,
           mirror=False):
    """One molecular slot (k_tau_mol's M1 instances) in one scenario, `atoms` atomic constituents beside it."""
    tab = make_table(n_w, wkind, p0, vbase, vspread, offset, seed, flat=flat)
    g = geometry(n_pr, n_orb, mirror=mirror)
    rows = design_rows(n_pr, n_orb, n_x, T, tab, seed, specials=specials, spread=spread)
    cons = [{"kind": "mol", "table": 0}] + [{"kind": "atom", "atom": k} for k in range(atoms)]
    d = dict(g, name=name, wav=wav_for(tab, descending=descending, inside=inside, margin=margin), tables=[tab],
             scenarios=[{"rows": rows, "T": float(T), "shift": np.asarray(shift, dtype=np.float64)[:n_orb].copy(),
                         "cons": cons}])
    return _finish(d)


def d_axes(name, n_pr, n_x, T, wkind, p0):
    return _scale_chi(single(name, n_pr, n_x, T, wkind, 40, p0=p0, seed=len(name)))


def d_brackets(name, wkind, descending=False):
    d = single(name, 33, 7, 512.0, wkind, 40, seed=11, descending=descending, shift=SHIFT_B if "out" in name else SHIFT_A)
    return _scale_chi(d)


def d_stage(name):
    if name == "stage-wide":      # 700 nodes under 300 wavelengths: the first workgroup's range exceeds the stage
        d = single(name, 33, 7, 512.0, "uniform", 700, seed=21)
    elif name == "stage-fit":     # every range fits; nothing touches a table end
        d = single(name, 33, 8, 512.0, "uniform", 40, seed=22, inside=True, shift=np.array([1.0, 1.0, 1 + 1e-7, 1 + 2e-7, 1.0]))
    elif name == "stage-move":    # 200 nodes: the first workgroup's range fits; 1.004 moves lambda' by several nodes
        d = single(name, 33, 7, 512.0, "uniform", 200, seed=23, inside=True, shift=np.array([1.0, 1.004, 1.0, 0.997, 1.0]))
    elif name == "stage-clamp":   # the staged ranges touch node 0 and node n_w - 2: the margin is clamped
        d = single(name, 64, 8, 512.0, "uniform", 40, seed=24)
    elif name == "stage-late":    # the group's first phase has no in-table lane (shift 2): nothing staged by it
        d = single(name, 33, 7, 512.0, "uniform", 40, seed=25, shift=np.array([2.0, 1.0, 1.0 + 1e-7, 2.0, 1.001]))
    else:
        raise ValueError(name)
    return _scale_chi(d)


def d_lists(name):
    if name == "lists-300":       # n_act crosses 256: k_mol_list loops by kBlock
        d = single(name, 340, 7, 512.0, "uniform", 40, seed=31, n_orb=2)
        return _scale_chi(d)
    atoms = 1 if name == "lists-atoms" else 0
    d = single(name, 33, 7, 512.0, "uniform", 40, seed=32 + atoms, atoms=atoms)
    rows, tab = d["scenarios"][0]["rows"], d["tables"][0]
    out = float(n_for_P(np.nextafter(tab["P"][-1], np.inf), 512.0))
    blocked = CR.blocked_mask(d["y"], d["z"], d["planet_y"], d["planet_R"], np.zeros((0, 5)), [])
    rows[:, 4, :] = 0.0 if not atoms else rows[:, 4, :]     # no atoms: phase 4 has no active chord, K = 0
    if atoms:
        rows[:, 4, :] = out                                  # atoms: every record of phase 4 is a zero-weight entry
        free = np.where(~blocked[2])[0]
        rows[free[:3], 2, :] = out                           # ... and three records of phase 2
    d = _scale_chi(d)
    # K mod 4 = 0, 1, 2, 3 at phases 0..3: samples of unblocked chords moved out of the table until the count fits
    for o in range(4):
        for _ in range(3):
            if listing(d)["K"][o] % 4 == o:
                break
            P = np.where(rows[:, o, :] * KB * 512.0 < 1e-4, 1e-4, rows[:, o, :] * KB * 512.0)
            inside, _i = brackets(tab["P"], P)
            cnt = inside.sum(axis=1)
            ip = int(np.where(~blocked[o] & (cnt >= 3))[0][0])
            rows[ip, o, int(np.where(inside[ip])[0][0])] = out
        assert listing(d)["K"][o] % 4 == o
    return d


SLOT_REL = [1.0, 0.6, 0.8, 1.3]


def d_slots(n_mol, atoms, t_out=False, one_sc=False):
    """n_mol molecular slots and `atoms` atoms over one scenario (n_mol = 1) or two: other T, other Doppler rows,
    offsets 1e-50 and 1e-40 (the second table's sigma ~ 1e-38, where the offset matters), other chi; with four slots,
    slots 0 and 1 share table 0 and slots 2 and 3 table 1.  `t_out`: slot 1's scenario temperature lies outside the table."""
    name = "slots-%dm%da%s" % (n_mol, atoms, "-tout" if t_out else "")
    n_pr, n_x = (33, 7) if (n_mol + atoms) % 2 else (64, 8)
    tabs = [make_table(40, "uniform", 1e-5, -21.0, 1.5, 1e-50, 41),
            make_table(33, "geometric", 1e-4, -38.5, 1.5, 1e-40, 42, w_lo=0.9e-4)]
    g = geometry(n_pr, 5)
    n_sc = 1 if n_mol == 1 or one_sc else 2
    T = [512.0, float(np.nextafter(1100.0, np.inf)) if t_out else 1024.0]
    scs = []
    for s in range(n_sc):
        scs.append({"rows": design_rows(n_pr, 5, n_x, 512.0 if s == 0 else 1024.0, tabs[s], 43 + s), "T": T[s],
                    "shift": (SHIFT_A if s == 0 else SHIFT_B).copy(), "cons": []})
    # constituent m: scenario m % n_sc and that scenario's table
    order = []
    for m in range(n_mol):
        order.append((m % n_sc, {"kind": "mol", "table": m % 2 if n_mol > 1 else 0, "rel": SLOT_REL[m]}))
    for a in range(atoms):
        order.append((a % n_sc, {"kind": "atom", "atom": a}))
    # interleave: atoms first in scenario 0, molecules first in scenario 1
    for s, c in order:
        if s == 0 and c["kind"] == "atom":
            scs[0]["cons"].append(c)
    for s, c in order:
        if s == 0 and c["kind"] == "mol":
            scs[0]["cons"].append(c)
    for s, c in order:
        if s == 1:
            scs[1]["cons"].append(c)
    # the second table's sigma is 1e17 times smaller: its slots' relative chi makes up for it
    for sc in scs:
        for c in sc["cons"]:
            if c["kind"] == "mol" and c["table"] == 1:
                c["rel"] = c["rel"] * 10.0 ** 17.5
    d = dict(g, name=name, wav=wav_for(tabs[0]), tables=tabs, scenarios=scs)
    return _scale_chi(_finish(d))


def d_mirror():
    """64 chords, 16 mirror pairs (pair k: chords k and 16 + k), weights 8 on the pairs (64 on the upper chords of the
    2^-30 pairs, so that merging them by mistake shows), a table whose adjacent P rows differ by at most 0.3 decades.  Pair k's second chord carries
    the first one's samples: k % 4 = 0 equal; 1: every n larger by 2^-41 relative (merged); 2: by 2^-39 (not merged);
    3: by 2^-30 (not merged: the mutation's pair).  Pair 12 loses one in-table sample on one side at phase 0 (other
    counts); pair 13's second chord sits 5e-10 (relative) further out in z and the planet's radius is that chord's
    distance at phase 1, so the planet covers the first chord only."""
    d = single("mirror", 64, 8, 512.0, "uniform", 40, seed=51, mirror=True, specials=False, spread=0.5, vspread=0.3)
    rows, tab = d["scenarios"][0]["rows"], d["tables"][0]
    for k in range(16):
        f = [1.0, 1.0 + 2.0 ** -41, 1.0 + 2.0 ** -39, 1.0 + 2.0 ** -30][k % 4]
        rows[16 + k] = rows[k] * f
    rows[16 + 12, 0, 3] = float(n_for_P(np.nextafter(tab["P"][-1], np.inf), 512.0))
    d["z"][16 + 13] = -d["z"][13] * (1.0 + 5e-10)
    d["planet_y"][1] = d["y"][13] + 1.9
    d["planet_R"] = float(np.sqrt((d["y"][16 + 13] - d["planet_y"][1]) ** 2 + d["z"][16 + 13] ** 2))
    d["fout"][:32] = 8.0
    d["fout"][[16 + k for k in (3, 7, 11, 15)]] = 64.0     # (sum F = 512: the 2^-30 pairs' upper chords carry half of it)
    d["mergeable"] = True
    return _scale_chi(d)


def d_nan(atoms):
    d = single("nan-mol" + ("-atom" if atoms else ""), 33, 7, 512.0, "uniform", 40, seed=61, atoms=atoms)
    d = _scale_chi(d)
    blocked = CR.blocked_mask(d["y"], d["z"], d["planet_y"], d["planet_R"], np.zeros((0, 5)), [])
    ip = int(np.where(~blocked[2])[0][4])
    d["scenarios"][0]["rows"][ip, 2, 3] = np.nan
    d["nan"] = (2, ip)
    return d


def d_poly():
    """A flat table whose exponent argument y = v 1024 log2 10 lies 0.49 from an integer at every sample, small |v|, and
    every tau near 1: the cubic term of the table exp's polynomial, e^3 / 6 = 6e-12 relative, stands above the bound."""
    v0 = (1700.0 + 0.49) / KAPPA
    d = single("poly", 33, 7, 512.0, "uniform", 40, seed=71, flat=v0, specials=False, spread=0.15, inside=True,
               shift=np.ones(5))
    y = d["tables"][0]["V"] * KAPPA
    fr = np.abs(y - np.rint(y))
    assert fr.min() > 0.48 and fr.max() < 0.4999, (fr.min(), fr.max())
    return _scale_chi(d, target=1.0)


AXES = {"axes-T512-uniform": (33, 7, 512.0, "uniform", 1e-5),                      # T between nodes, clip inside
        "axes-T700-geometric-clipnode": (64, 8, 700.0, "geometric", 1e-4),        # T on a node, clip on the first node
        "axes-T300-uniform": (33, 8, 300.0, "uniform", 1e-5),                      # T on the first node
        "axes-T1100-geometric": (64, 7, 1100.0, "geometric", 1e-5),               # T on the last node
        "axes-T1024-clipnode": (33, 7, 1024.0, "uniform", 1e-4),                   # T between, exact P, clip on a node
        "axes-Tout-hi": (33, 7, float(np.nextafter(1100.0, np.inf)), "uniform", 1e-5),
        "axes-Tout-lo": (33, 7, float(np.nextafter(300.0, 0.0)), "geometric", 1e-5)}
BRACKETS = {"brackets-uniform": ("uniform", False), "brackets-geometric": ("geometric", False),
            "brackets-out-and-back": ("uniform", False), "brackets-descending": ("geometric", True)}
STAGE = ["stage-wide", "stage-fit", "stage-move", "stage-clamp", "stage-late"]
LISTS = ["lists-mod4", "lists-atoms", "lists-300"]
SLOTS = [(m, a, False, False) for m in (1, 2, 4) for a in (0, 1, 4)] + [(2, 0, True, False), (4, 1, True, False),
                                                                         (2, 1, False, True)]
SLOT_NAMES = ["slots-%dm%da%s" % (m, a, "-tout" if t else "-onesc" if o else "") for m, a, t, o in SLOTS]
NAMES = list(AXES) + list(BRACKETS) + STAGE + LISTS + SLOT_NAMES + ["mirror", "nan-mol", "nan-mol-atom", "poly"]


@functools.lru_cache(maxsize=None)
def design(name):
    if name in AXES:
        return d_axes(name, *AXES[name])
    if name in BRACKETS:
        return d_brackets(name, *BRACKETS[name])
    if name in STAGE:
        return d_stage(name)
    if name in LISTS:
        return d_lists(name)
    if name in SLOT_NAMES:
        return d_slots(*SLOTS[SLOT_NAMES.index(name)])
    if name == "mirror":
        return d_mirror()
    if name.startswith("nan-mol"):
        return d_nan(1 if name.endswith("atom") else 0)
    if name == "poly":
        return d_poly()
    raise KeyError(name)


# ---- slots -----------------------------------------------------------------------------------------------------------------
def mol_slots(d):
    """The device's molecular slots: scenario order, then constituent order."""
    return [dict(sc=s, table=c["table"], chi=c["chi"], T=sc["T"], shift=sc["shift"], offset=d["tables"][c["table"]]["offset"])
            for s, sc in enumerate(d["scenarios"]) for c in sc["cons"] if c["kind"] == "mol"]


def atom_slots(d):
    return [dict(sc=s, atom=c["atom"], chi=c["chi"]) for s, sc in enumerate(d["scenarios"]) for c in sc["cons"]
            if c["kind"] == "atom"]


def blocked_of(d):
    return CR.blocked_mask(d["y"], d["z"], d["planet_y"], d["planet_R"], np.zeros((0, d["n_orb"])), [])


def pressure(rows, T, clip=True):
    with np.errstate(invalid="ignore"):
        P = (rows * KB) * T
        return np.where(P < 1e-4, 1e-4, P) if clip else P


# ---- the device's lists, restated ----------------------------------------------------------------------------------------
def listing(d, merge_tol=MIRROR_TOL, merged=True):
    """k_mol_prep, k_columns' flags and k_mol_list in float64.  Returns
      active [n_orb, n_pr]   unblocked chords whose bound exceeds the cull (a NaN bound stays active)
      entries[o]             the phase's list: (ip, slot, x) in record order, merged pairs' upper records listing nothing
      K [n_orb]              its length, the zero-weight entries of empty records (atoms or exact phases) included
      pairs[o]               the (lower chord, upper chord) pairs that merge (`merged`, table-exp path without atoms)
      exact [n_orb]          phases with a non-finite atomic column (k_chords' nnf)
    A NaN density sample is listed as an in-table entry (k_mol_prep keeps it, so that tau is NaN as in the reference)."""
    n_pr, n_orb, n_x = d["n_pr"], d["n_orb"], d["n_x"]
    ms, at = mol_slots(d), atom_slots(d)
    blocked = blocked_of(d)
    inP, iP, tP, nabs = [], [], [], []
    bound = np.zeros((n_orb, n_pr))
    for s in ms:
        rows, tab = d["scenarios"][s["sc"]]["rows"], d["tables"][s["table"]]
        P = pressure(rows, s["T"])
        ins, i = brackets(tab["P"], P)
        nan = np.isnan(rows)
        ins = ins | nan
        i = np.where(nan, 0, i)
        t = np.where(nan, 0.0, weight_f64(tab["P"], P, i))
        na = rows * s["chi"]
        inP.append(ins), iP.append(i), tP.append(t), nabs.append(na)
        vmax = max(float(d["tables"][q["table"]]["V"].max()) for q in ms)
        with np.errstate(invalid="ignore"):
            bound += (np.where(ins, na * d["dx"], 0.0).sum(axis=2) * 10.0 ** vmax).T
    exact = np.zeros(n_orb, dtype=bool)
    for a in at:
        rows = d["scenarios"][a["sc"]]["rows"]
        N = np.stack([CR.columns_numpy(rows[:, o, :], a["chi"], d["dx"]) for o in range(n_orb)])
        with np.errstate(invalid="ignore"):
            bound += N * ((10.0 ** np.log10(ATOM_SIGMA[a["atom"]] + ATOM_OFFSET) - ATOM_OFFSET) * (1.0 + 1e-9))
        exact |= (~np.isfinite(N) & ~blocked).any(axis=1)
    with np.errstate(invalid="ignore"):
        active = ~blocked & ~(bound <= CULL)
        near = ~blocked & (bound > CULL / 100.0) & (bound < CULL * 100.0)
    assert not near.any(), "a chord's bound lies within a factor of 100 of the cull"
    mir = mirror_pairs(d["y"], d["z"])
    entries, pairs, K = [], [], np.zeros(n_orb, dtype=np.int64)
    for o in range(n_orb):
        fold = merged and not at and not exact[o]
        skip, pr = set(), []
        if fold and (mir >= 0).any():
            for ip in range(n_pr):
                q = int(mir[ip])
                if q <= ip or not (active[o, ip] and active[o, q]):
                    continue
                eq = True
                for m in range(len(ms)):
                    a, b = inP[m][ip, o], inP[m][q, o]
                    if a.sum() != b.sum():
                        eq = False
                        break
                    ta, tb = tP[m][ip, o][a], tP[m][q, o][b]
                    na_, nb_ = nabs[m][ip, o][a], nabs[m][q, o][b]
                    with np.errstate(invalid="ignore"):
                        eq = bool(np.all(iP[m][ip, o][a] == iP[m][q, o][b]) and np.all(np.abs(ta - tb) <= merge_tol) and
                                  np.all(np.abs(na_ - nb_) <= merge_tol * np.maximum(np.abs(na_), np.abs(nb_))))
                    if not eq:
                        break
                if eq and sum(int(inP[m][ip, o].sum()) for m in range(len(ms))) > 0:
                    pr.append((ip, q))
                    skip.add(q)
        ent, k = [], 0
        for ip in np.where(active[o])[0]:
            if ip in skip:
                continue
            mine = [(int(ip), m, int(x)) for m in range(len(ms)) for x in np.where(inP[m][ip, o])[0]]
            ent += mine
            k += len(mine) if (mine or fold) else 1
        entries.append(ent), pairs.append(pr)
        K[o] = k
    return dict(active=active, entries=entries, K=K, pairs=pairs, exact=exact, blocked=blocked)


def lanes_in_table(d):
    """[n_mol, n_orb, n_wav]: lambda' = fl(shift lambda) inside the slot's W axis and the slot's T inside its T axis."""
    out = []
    for s in mol_slots(d):
        tab = d["tables"][s["table"]]
        inT, _ = brackets(tab["T"], s["T"])
        lam = s["shift"][:, None] * d["wav"][None, :]
        inW, _ = brackets(tab["W"], lam)
        out.append(inW & bool(inT))
    return np.stack(out)


def predicted_evals(d, table_exp=True):
    """exp_evals of a stats run: per phase and slot, the listed samples times the slot's in-table lanes (k_tau_mol's
    npow).  The ocml path (`table_exp` false) merges nothing."""
    L = listing(d, merged=table_exp)
    lanes = lanes_in_table(d).sum(axis=2)
    tot = 0
    for o, ent in enumerate(L["entries"]):
        for _ip, m, _x in ent:
            tot += int(lanes[m, o])
    return tot


# ---- the LDS stage, restated ---------------------------------------------------------------------------------------------
def stage_plan(d, ppg):
    """One slot, table exp.  Per (group, workgroup): `staged` (lo, n) or None by the kernel's rule
    n_ * n_int * 2 <= kMolStageD2 at the group's first table-exp phase, with the margin's clamps; per (phase, workgroup,
    wave): whether the wave's samples come from the stage."""
    s = mol_slots(d)[0]
    tab = d["tables"][s["table"]]
    n_int, nw1 = len(tab["P"]) - 1, len(tab["W"]) - 1
    n_wav, n_orb = len(d["wav"]), d["n_orb"]
    exact = listing(d)["exact"]
    inT, _ = brackets(tab["T"], s["T"])
    n_wg = (n_wav + KBLOCK - 1) // KBLOCK
    lam = d["wav"][np.minimum(np.arange(n_wg * KBLOCK), n_wav - 1)]     # lanes past n_wav take the last wavelength
    staged, use, clamp_lo, clamp_hi = {}, {}, False, False
    for g0 in range(0, n_orb, ppg):
        for b in range(n_wg):
            st, done = None, False
            for o in range(g0, min(n_orb, g0 + ppg)):
                if exact[o]:
                    continue
                lw = s["shift"][o] * lam[b * KBLOCK:(b + 1) * KBLOCK]
                inW, iW = brackets(tab["W"], lw)
                inW = inW & bool(inT)
                if not done:
                    done = True
                    if inW.any():
                        gmn, gmx = int(iW[inW].min()), int(iW[inW].max())
                        lo, hi = max(0, gmn - STAGE_MARGIN), min(nw1 - 1, gmx + STAGE_MARGIN)
                        if (hi - lo + 1) * n_int * 2 <= STAGE_D2:
                            st = (lo, hi - lo + 1)
                            clamp_lo |= gmn - STAGE_MARGIN < 0
                            clamp_hi |= gmx + STAGE_MARGIN > nw1 - 1
                    staged[(g0, b)] = st
                for v in range(KBLOCK // 64):
                    m = inW[v * 64:(v + 1) * 64]
                    i = iW[v * 64:(v + 1) * 64][m]
                    use[(o, b, v)] = st is not None and (not m.any() or (st[0] <= i.min() and i.max() < st[0] + st[1]))
    return dict(staged=staged, use=use, clamp_lo=clamp_lo, clamp_hi=clamp_hi)


# ---- the reference -------------------------------------------------------------------------------------------------------
def reference(d, mut=None, _raw=False):
    """R [n_orb, n_wav] (longdouble), tau [n_orb, n_pr, n_wav], the sensitivity S [n_orb, n_wav] =
    sum_c (F_c / sum F) tau_c e^-tau_c and `any_in` [n_orb, n_wav] (some slot's lambda' and T inside its table)."""
    if mut is None and not _raw and "_ref" in d:
        return d["_ref"]
    n_pr, n_orb, n_x = d["scenarios"][0]["rows"].shape
    n_wav = len(d["wav"])
    ms, at = mol_slots(d), atom_slots(d)
    blocked = blocked_of(dict(d, n_orb=n_orb))
    eff = [dict(s) for s in ms]
    if mut in ("slot_T", "slot_offset", "slot_chi", "slot_shift"):
        key = mut[5:]
        assert len(ms) > 1
        for m in range(len(ms)):
            eff[m][key] = ms[(m + 1) % len(ms)][key]
    keep = None
    if mut and mut.startswith("drop_last_"):
        L = listing(d, merged=False)
        keep = [np.ones((n_pr, n_orb, n_x), dtype=bool) for _ in ms]
        for o, ent in enumerate(L["entries"]):
            for ip, m, x in ent[len(ent) - int(mut[-1]):]:
                keep[m][ip, o, x] = False
    tau = np.zeros((n_orb, n_pr, n_wav), dtype=LD)
    any_in = np.zeros((n_orb, n_wav), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for m, s in enumerate(eff):
            tab = d["tables"][s["table"]]
            rows = d["scenarios"][s["sc"]]["rows"]
            P = pressure(rows, s["T"], clip=mut != "no_clip")
            inP, iP = brackets(tab["P"], P, exclusive=mut == "excl_P")
            tP = weight_ld(tab["P"], np.where(np.isnan(P), tab["P"][0], P), iP)
            inT, iT = brackets(tab["T"], s["T"], exclusive=mut == "excl_T")
            tT = weight_ld(tab["T"], s["T"], iT)
            V = tab["V"].astype(LD)
            GT = (1 - tT) * V[:, int(iT), :] + tT * V[:, int(iT) + 1, :]
            nabs = rows.astype(LD) * LD(s["chi"])
            if mut == "nan_dropped":
                nabs = np.where(np.isnan(nabs), LD(0), nabs)
            if keep is not None:
                nabs = np.where(keep[m], nabs, LD(0))
            iW_prev = tW_prev = None
            for o in range(n_orb):
                lam = s["shift"][o] * d["wav"]
                inW, iW = brackets(tab["W"], lam, exclusive=mut == "excl_W")
                tW = weight_ld(tab["W"], lam, iW)
                cur = (iW, tW)
                if mut == "prev_iw" and iW_prev is not None:
                    iW = iW_prev
                    tW = weight_ld(tab["W"], lam, iW)
                if mut == "prev_tw" and tW_prev is not None:
                    tW = tW_prev
                iW_prev, tW_prev = cur
                ok = inW & bool(inT)
                any_in[o] |= ok
                a, b = tP[:, o, :, None], tW[None, None, :]
                i0, w0 = iP[:, o, :, None], iW[None, None, :]
                if mut == "swap_t":
                    a, b = np.broadcast_to(b, (n_pr, n_x, n_wav)), np.broadcast_to(a, (n_pr, n_x, n_wav))
                v = ((1 - a) * ((1 - b) * GT[i0, w0] + b * GT[i0, w0 + 1]) +
                     a * ((1 - b) * GT[i0 + 1, w0] + b * GT[i0 + 1, w0 + 1]))
                pw = np.power(LD(10), v)
                if mut == "quadratic":
                    y = (v * LD(KAPPA)).astype(np.float64)
                    e = (y - np.rint(y)) * (np.log(2.0) / 1024.0)
                    pw = pw * (1 - LD(1) * e ** 3 / 6)
                sig = np.where(inP[:, o, :, None] & ok[None, None, :], pw - LD(s["offset"]), LD(0))
                tau[o] += LD(d["dx"]) * (nabs[:, o, :, None] * sig).sum(axis=1)
        for a in at:
            rows = d["scenarios"][a["sc"]]["rows"]
            y = np.log10(ATOM_SIGMA[a["atom"]] + ATOM_OFFSET)     # the uploaded flat table's node value
            sg = np.power(LD(10), LD(y)) - LD(ATOM_OFFSET)
            N = (rows.astype(LD) * LD(a["chi"])).sum(axis=2) * LD(d["dx"])
            tau += (N.T * sg)[:, :, None]
        if mut == "merge_2m30":
            L = listing(d, merge_tol=2.0 ** -29.5)
            for o, pr in enumerate(L["pairs"]):
                for lo, hi in pr:
                    tau[o, hi] = tau[o, lo]
        F = d["fout"].astype(LD)
        w = np.where(blocked, LD(0), F[None, :] / F.sum())
        et = np.exp(-tau)
        R = (w[:, :, None] * np.where(blocked[:, :, None], LD(0), et)).sum(axis=1)
        S = (w[:, :, None] * np.where(blocked[:, :, None] | ~np.isfinite(tau), LD(0), tau * et)).sum(axis=1)
    out = dict(R=R, tau=tau, S=S.astype(np.float64), any_in=any_in, blocked=blocked)
    if mut is None and not _raw:
        d["_ref"] = out
    return out


# ---- the bound -------------------------------------------------------------------------------------------------------------
def tolerance(d):
    """|R - R_ref| of a float64 evaluation by k_mol_gt / k_tau_mol's arithmetic; tests/test_gpu_mol.py derives the terms.
    Returns (bound, parts)."""
    ms, at = mol_slots(d), atom_slots(d)
    e_v = a_off = 0.0
    D = 0.0
    for s in ms:
        V, off = d["tables"][s["table"]]["V"], s["offset"]
        assert V.min() >= np.log10(off) + 1.0
        e_v = max(e_v, 94.0 * float(np.abs(V).max()) * LN10)
        a_off = max(a_off, 1.0 / (1.0 - off * 10.0 ** -float(V.min())))
        D = max(D, float(np.abs(np.diff(V, axis=0)).max()))
    K = len(ms) * d["n_x"]
    e_mol = (e_v + 9.0) * a_off + K + 1.0
    e_atom = d["n_x"] + 8.0
    e_tau = max(e_mol, e_atom if at else 0.0) + len(at) + 1.0 + 3.0
    e_disk = 10.0 + 1.0 + d["n_pr"] + 3.0
    merge = MIRROR_TOL * (1.0 + D * LN10) / np.e if d["mergeable"] else 0.0
    bound = (e_tau / np.e + e_disk) * U * (1.0 + 2.0 ** -9) + merge
    return bound, dict(e_v=e_v, a_off=a_off, e_tau=e_tau, e_disk=e_disk, merge=merge, D=D)


# ---- design assertions ---------------------------------------------------------------------------------------------------
def check_design(name):
    """Every design: sensitivity.  Named designs: the edges they are named for.  Returns the facts it found."""
    d = design(name)
    ref = reference(d)
    facts = {}
    pts = ref["any_in"] & np.isfinite(ref["S"])
    for o in range(d["n_orb"]):
        pts[o] &= bool(listing(d)["active"][o].any())
    sens = float((ref["S"][pts] >= 0.05).mean()) if pts.any() else 1.0    # (no in-table point: R is the flux share)
    facts["sensitive"] = sens
    assert sens >= 0.5, "%s: only %.2f of the in-table points have sum F tau e^-tau >= 0.05" % (name, sens)
    tau = ref["tau"].astype(np.float64)
    act = listing(d)["active"]
    sel = tau[act & ~np.isnan(tau).any(axis=2)]
    sel = sel[sel > 0]
    facts["tau_5_50_95"] = [float(np.percentile(sel, q)) for q in (5, 50, 95)] if sel.size else []
    s0 = mol_slots(d)[0]
    tab = d["tables"][s0["table"]]
    rows = d["scenarios"][s0["sc"]]["rows"]
    unb = ~blocked_of(d).T[:, :, None]                     # [n_pr, n_orb, 1]
    if name in AXES:
        T = s0["T"]
        inT, _ = brackets(tab["T"], T)
        facts["T_in"] = bool(inT)
        assert bool(inT) == ("Tout" not in name)
        lam = s0["shift"][:, None] * d["wav"][None, :]
        W = tab["W"]
        for v in (W[0], W[-1], np.nextafter(W[0], 0.0), np.nextafter(W[0], 1.0), np.nextafter(W[-1], 0.0),
                  np.nextafter(W[-1], 1.0), W[5], W[len(W) // 2]):
            assert (lam == v).any(), "%s: no lambda' at %r" % (name, v)
        inW, _ = brackets(W, lam)
        waves = inW[:, :256].reshape(d["n_orb"], 4, 64)
        assert (waves.any(axis=2) & ~waves.all(axis=2)).any(), "no wave with lanes in and out of the table"
        assert not inW[0, 0] and not inW[0, -1]
        if np.frexp(T)[0] == 0.5:
            P = pressure(rows, T)
            Praw = (rows * KB) * T
            for v in special_P(tab):
                hit = (Praw == v) & unb
                assert hit.any(), "%s: no unblocked sample at P = %r" % (name, v)
        Praw = (rows * KB) * T
        assert ((Praw < 1e-4) & (pressure(rows, T) == 1e-4) & unb).any() and ((rows == 0) & unb).any()
        facts["clip_on_node"] = bool(tab["P"][0] == 1e-4)
        assert facts["clip_on_node"] == ("clipnode" in name)
    if name in BRACKETS:
        W = tab["W"]
        idx = [brackets(W, s0["shift"][o] * d["wav"])[1] for o in range(d["n_orb"])]
        inw = [brackets(W, s0["shift"][o] * d["wav"])[0] for o in range(d["n_orb"])]
        # the kernel's linear guess on the first phase: kept on a uniform grid, failing on a geometric one
        lw = (s0["shift"][0] * d["wav"])[inw[0]]
        gss = np.clip(((lw - W[0]) * ((len(W) - 1) / (W[-1] - W[0]))).astype(np.int64), 0, len(W) - 2)
        good = (W[gss] < lw) & (lw <= W[gss + 1])
        facts["guess_kept"] = float(good.mean())
        assert (good.mean() > 0.9) if tab["wkind"] == "uniform" else (good.mean() < 0.5)
        if "out" in name:
            assert inw[0].any() and not inw[1].any() and inw[2].any()
            step = np.abs(idx[3] - idx[2])[inw[2] & inw[3]]
            assert (step == 1).any() and (step == 0).any()
        else:
            assert s0["shift"][1] == s0["shift"][0]
            both = inw[1] & inw[2]
            assert (idx[2] == idx[1])[both].mean() > 0.9                      # inside the cached bracket
            assert ((idx[3] - idx[2])[inw[2] & inw[3]] >= 2).any()            # many nodes up
            assert ((idx[4] - idx[3])[inw[3] & inw[4]] <= -2).any()           # many nodes down
        assert (np.diff(d["wav"]) < 0).all() == ("descending" in name)
    if name in STAGE:
        p1, p5 = stage_plan(d, 1), stage_plan(d, 5)
        facts["staged_ppg1"] = {k: v for k, v in p1["staged"].items()}
        if name == "stage-wide":
            assert p1["staged"][(0, 0)] is None and p1["staged"][(0, 1)] is not None
            n_int = len(tab["P"]) - 1
            assert (len(tab["W"]) - 1) * n_int * 2 > STAGE_D2
        if name == "stage-fit":
            assert all(v is not None for v in p1["staged"].values()) and all(p5["use"].values())
            assert not p1["clamp_lo"] and not p1["clamp_hi"]
        if name == "stage-move":
            assert all(v is not None for v in p5["staged"].values())
            assert not all(p5["use"].values()) and any(p5["use"].values())
        if name == "stage-clamp":
            assert p1["clamp_lo"] and p1["clamp_hi"]
        if name == "stage-late":
            assert not lanes_in_table(d)[0, 0].any() and p5["staged"][(0, 0)] is None and p1["staged"][(1, 0)] is not None
    if name in ("lists-mod4", "lists-atoms"):
        L = listing(d)
        facts["K"] = [int(k) for k in L["K"]]
        assert [int(k) % 4 for k in L["K"][:4]] == [0, 1, 2, 3]
        if name == "lists-mod4":
            assert L["K"][4] == 0 and not L["active"][4].any()
        else:
            empty = [sum(1 for ip in np.where(L["active"][o])[0] if not any(e[0] == ip for e in L["entries"][o]))
                     for o in range(d["n_orb"])]
            assert empty[4] == int(L["active"][4].sum()) > 0 and empty[2] >= 3
    if name == "lists-300":
        assert (listing(d)["active"].sum(axis=1) > 256).all()
    if name in SLOT_NAMES:
        ms = mol_slots(d)
        facts["slots"] = [(s["sc"], s["table"], s["T"], s["offset"]) for s in ms]
        if len(ms) > 1:
            assert len({s["offset"] for s in ms}) == 2 and len({s["chi"] for s in ms}) == len(ms)
            if "onesc" in name:
                assert len({s["sc"] for s in ms}) == 1 and len({s["table"] for s in ms}) == 2
            else:
                assert len({s["sc"] for s in ms}) == 2 and len({s["T"] for s in ms}) == 2
                assert not np.array_equal(ms[0]["shift"], ms[-1]["shift"])
        if len(ms) == 4:
            assert ms[0]["table"] == ms[1]["table"] and ms[2]["table"] == ms[3]["table"]
        t_in = [bool(brackets(d["tables"][s["table"]]["T"], s["T"])[0]) for s in ms]
        assert t_in[0] and all(t_in) == ("tout" not in name)
    if name == "mirror":
        L = listing(d)
        mir = mirror_pairs(d["y"], d["z"])
        assert all(mir[k] == 16 + k for k in range(16)) and (mir[32:] < 0).all()
        for o in range(d["n_orb"]):
            got = {p[0] for p in L["pairs"][o]}
            for k in range(16):
                both = L["active"][o, k] and L["active"][o, 16 + k]
                want = both and k % 4 in (0, 1) and not (k == 12 and o == 0)
                assert (k in got) == bool(want), (o, k, got)
        assert L["blocked"][1, 13] and not L["blocked"][1, 16 + 13]
        assert sum(len(p) for p in L["pairs"]) >= 20
        loose = listing(d, merge_tol=2.0 ** -29.5)
        assert any(p[0] % 4 == 3 for o in range(d["n_orb"]) for p in loose["pairs"][o])
        facts["pairs"] = [len(p) for p in L["pairs"]]
    if name.startswith("nan-mol"):
        o, ip = d["nan"]
        assert not blocked_of(d)[o, ip] and np.isnan(ref["R"][o]).all()
        assert np.isfinite(ref["R"][[k for k in range(d["n_orb"]) if k != o]].astype(np.float64)).all()
    elif not d["nan"]:
        assert np.isfinite(ref["R"].astype(np.float64)).all()
    if not d["mergeable"]:
        assert not any(listing(d)["pairs"][o] for o in range(d["n_orb"]))
    return facts
