#!/usr/bin/env python3
"""Latency of an injection grid, a loop of single calls against one grid call (GPU box), on C3 with the inputs
resident: the set-up of tools/recover_bench.py (pixels of 0.01 A at R = 140,000, 48 exposures of 6 taps, a Gaussian
high-pass of sigma = 40 pixels cut at h = 160 over one order, dividing, SYSREM with 6 components of 30 iterations), at
2,000 pixels x 1,024 trials and at 320,000 pixels x 8 trials, for grids of 16 and 64 points (trial x scale):

  recover  (a)  a loop of transit_recover over the points        (b)  one transit_recover_grid
  inject   (a)  a loop of transit_inject, the cleaned data back  (b)  one transit_inject_grid, the cleaned data back

(a) runs on the package and library of the tree given with --parent-tree (a checkout of the parent commit with its
own build), or on this tree's when none is given; (b) on this tree's.  A package's table caches belong to one library,
so every (way, round) is a child process of its own, under its own time limit, and the ways are alternated ROUNDS
times (a b a b ...): drifts of the box show as the spread between rounds.  A child sets the problem up, warms up on
the 16-point grid and times one evaluation per grid and kind; the outputs' digests are compared across the ways.  The
last (b) child also runs the 64-point recover grid under a sweep of the sub-batch cap PROM_GRID_SCRATCH_MB, which the
library reads at every grid call.

  python tools/grid_bench.py [--config C3] [--rounds 4] [--parent-tree PATH] [--out profiles/inject_grid_latency.txt]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SIZES = ((2000, 1024), (320000, 8))
GRIDS = (16, 64)
LIMIT_S = {2000: 150, 320000: 200}
N_COMP, N_ITER, SIGMA_PIX = 6, 30, 40.0
CAPS_MB = (1024, 4096, 16384, 65536)
CAP = "PROM_GRID_SCRATCH_MB"


def child(n_pix, n_trial, config, way, sweep):
    import numpy as np
    from prometheus_amd import _native, configs, setupfile
    from prometheus_amd import lightcurve as lc
    from prometheus_amd import observation as obs
    from detrend_bench import N_EXP, tables
    from sysrem_bench import pixels
    tr = setupfile.build_transit(configs.get(config))
    dev = _native.get_device(0)
    host = tr._host_inputs()
    wav = np.asarray(tr.wavelength)
    n_orb = len(host["orb"])
    lam = pixels(np, lc, tr, n_pix)
    ins = obs.Instrument(lam, resolving_power=140000.0)
    rng = np.random.default_rng(0)
    x = np.linspace(-1.0, 1.0, n_pix)
    raw = (1.0 + 0.2 * x)[None, :] * (1.0 + 0.05 * np.linspace(-1, 1, N_EXP)[:, None] * np.sin(40.0 * x)[None, :])
    raw = raw * (1.0 + 1e-3 * rng.normal(size=(N_EXP, n_pix)))
    err = np.full(raw.shape, 1e-3)
    rows, a, F = tables(tr, 1024)
    F = np.ascontiguousarray(F[:, :n_trial])
    g = obs.gaussian_taps(SIGMA_PIX)
    ex = obs.Exposures(ins, rows, a, F, raw, err)
    dev.transit_set(tr._problem(dev, host, 0, len(wav), 0.0))
    dev.transit_run()
    dev.observe_set(ins.lam, ins.sig, ins.truncate, n_orb)
    dev.expose_set(ex.rows, ex.weights, ex.factors, ex.data, ex.ivar)
    dev.highpass_set([0, n_pix], np.arange(n_pix), g, 1)
    dev.sysrem_set(ex.data)
    res = {"n_orb": n_orb, "n_wav": len(wav), "n_pix": n_pix, "n_trial": n_trial, "n_exp": N_EXP,
           "n_tap": int(rows.shape[1]), "half_width": len(g) - 1, "ms": {}, "digest": {}}
    kw = dict(n_comp=N_COMP, n_iter=N_ITER, highpass=True)
    os.environ.pop(CAP, None)

    def points(n_grid):   # n / 4 trials x four scales, trial-major
        return (np.repeat(np.linspace(0, n_trial - 1, n_grid // 4).astype(int), 4),
                np.tile([0.5, 1.0, 1.5, 2.0], n_grid // 4))
    if way == "a":
        ways = {"recover": lambda t, s: np.stack([dev.transit_recover(int(tt), float(ss), **kw)[0] for tt, ss in zip(t, s)]),
                "inject": lambda t, s: np.stack([dev.transit_inject(int(tt), float(ss), **kw)[1] for tt, ss in zip(t, s)])}
    else:
        ways = {"recover": lambda t, s: dev.transit_recover_grid(t, s, **kw)[0],
                "inject": lambda t, s: dev.transit_inject_grid(t, s, **kw)[1]}
    for f in ways.values():                                    # warm-up, untimed
        f(*points(GRIDS[0]))
    for n_grid in GRIDS:
        t, s = points(n_grid)
        for kind, f in ways.items():
            t0 = time.perf_counter()
            out = f(t, s)                                      # every way ends in a stream synchronise (the copy back)
            res["ms"]["%s %d" % (kind, n_grid)] = (time.perf_counter() - t0) * 1e3
            res["digest"]["%s %d" % (kind, n_grid)] = hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()
            out = None
    if sweep:
        res["sweep"] = {}
        t, s = points(GRIDS[-1])
        for mb in CAPS_MB:
            os.environ[CAP] = str(mb)
            v = []
            for _ in range(2):
                t0 = time.perf_counter()
                ways["recover"](t, s)
                v.append((time.perf_counter() - t0) * 1e3)
            res["sweep"][str(mb)] = v
        os.environ.pop(CAP, None)
    print("GRID_BENCH " + json.dumps(res), flush=True)


def run_child(n_pix, n_trial, a, way, sweep):
    tree = os.path.abspath(a.parent_tree) if way == "a" and a.parent_tree else REPO
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n_pix), str(n_trial), "--config", a.config,
           "--way", way, "--tree", tree] + (["--sweep"] if sweep else [])
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[n_pix])
    except subprocess.TimeoutExpired:
        sys.stderr.write("(%d pixels, %s) did not finish within its limit of %d s: no result\n" % (n_pix, way, LIMIT_S[n_pix]))
        return None                      # the child is killed; nothing more is started on the device
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("GRID_BENCH ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        return None                      # a failed child ends the session
    return json.loads(line[-1][len("GRID_BENCH "):])


def run_size(n_pix, n_trial, a):
    """{"ms": {"recover 16": {"a": [per round], "b": [...]}, ...}, "equal": {...}, "sweep": {...}} of one size."""
    out = {"ms": {}, "equal": {}}
    for r in range(a.rounds):
        for way in ("a", "b"):
            x = run_child(n_pix, n_trial, a, way, way == "b" and r == a.rounds - 1)
            if x is None:
                return None
            for k, v in x["ms"].items():
                out["ms"].setdefault(k, {"a": [], "b": []})[way].append(v)
            out.setdefault("digest_" + way, x["digest"])
            out.update({k: x[k] for k in ("n_orb", "n_wav", "n_exp", "n_tap", "half_width")})
            if "sweep" in x:
                out["sweep"] = x["sweep"]
    out["equal"] = {k: out["digest_a"][k] == out["digest_b"][k] for k in out["digest_a"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--way", default="b")
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "inject_grid_latency.txt"))
    ap.add_argument("--child", type=int, nargs=2, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "tools"))
    if a.child is not None:
        sys.path.insert(0, a.tree)       # the package (and its library) of the tree this way measures
        child(a.child[0], a.child[1], a.config, a.way, a.sweep)
        return 0
    a.rounds = max(3, a.rounds)
    runs = {}
    for n, nt in SIZES:
        runs[n] = run_size(n, nt, a)
        if runs[n] is None:
            return 1
    x0 = runs[SIZES[0][0]]
    lines = ["Latency of an injection grid, %s with the inputs resident and R in device memory (tools/grid_bench.py):"
             % a.config,
             "pixels of 0.01 A at R = 140,000, %d exposures over the %d phases (%d taps), a Gaussian high-pass of sigma = "
             "%g pixels cut at h = %d" % (x0["n_exp"], x0["n_orb"], x0["n_tap"], SIGMA_PIX, x0["half_width"]),
             "over one order, dividing; SYSREM with %d components of %d iterations; %d wavelengths.  A grid is n / 4 "
             "trials x the scales 0.5, 1, 1.5, 2." % (N_COMP, N_ITER, x0["n_wav"]),
             "One evaluation per way, kind and round by the host clock, each (way, round) in a process of its own after a "
             "warm-up on the 16-point grid; the ways alternated a b ... for %d rounds." % a.rounds,
             "  recover (a)  a loop of transit_recover, %s" % (
                 "the parent commit's tree and library" if a.parent_tree else "this tree's library (no parent tree given)"),
             "          (b)  one transit_recover_grid, this tree's library: moments, n_used and U come back",
             "  inject  (a)  a loop of transit_inject, the same library as recover (a): U and the cleaned data come back",
             "          (b)  one transit_inject_grid: U and the cleaned data come back", ""]
    for n, nt in SIZES:
        x = runs[n]
        for n_grid in GRIDS:
            lines.append("%d pixels x %d trials, %d points:" % (n, nt, n_grid))
            for kind in ("recover", "inject"):
                med, spread = {}, {}
                for w in ("a", "b"):
                    v = x["ms"]["%s %d" % (kind, n_grid)][w]
                    med[w], spread[w] = statistics.median(v), max(v) - min(v)
                    lines.append("  %-7s (%s) ms per round: %s   median %.3f   spread (max - min) %.3f"
                                 % (kind, w, " ".join("%.3f" % t for t in v), med[w], spread[w]))
                gain = med["a"] - med["b"]
                lines.append("  %-7s (a) - (b) = %.3f ms against spreads of %.3f and %.3f ms, (a) / (b) = %.2f: (b) %s; the "
                             "outputs of (a) and (b) are bitwise equal: %s"
                             % (kind, gain, spread["a"], spread["b"], med["a"] / med["b"],
                                "beats (a) by more than the two spreads" if gain > spread["a"] + spread["b"] else
                                "does NOT beat (a) by more than the two spreads", x["equal"]["%s %d" % (kind, n_grid)]))
        lines.append("  the 64-point recover grid under %s (two evaluations each, ms): %s"
                     % (CAP, "   ".join("%s MB: %s" % (mb, " ".join("%.1f" % t for t in v))
                                        for mb, v in x["sweep"].items())))
        lines.append("")
    lines += ["Not measured: hardware counters (no rocprofv3 --pmc run); the kernels' own device durations inside a grid "
              "call (the *_kernel_ms aids refuse after one); several orders; other n_comp and n_iter than %d and %d."
              % (N_COMP, N_ITER)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
