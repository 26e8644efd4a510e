#!/usr/bin/env python3
"""Latency of SYSREM per echelle order (GPU box), on C3 with R in device memory: 48 exposures of 6 taps, 8 trials,
SYSREM with 6 components of 30 iterations, no high-pass, at 24 orders x 2,000 pixels and at the 320,000-pixel table cut
into 80 orders (contiguous orders of equal length):

  clean   (a)  the parent's route: a loop over the orders of sysrem_clean on per-order tables
          (b)  one sysrem_clean_orders on the whole table
  inject  (a)  a loop over the orders of transit_inject on per-order tables    (b)  one transit_inject_orders

A context holds one table, so (a) uploads every order's pixels, table and raw exposures before its call; the calls
alone and the calls with their uploads are timed separately.  (a) runs on the package and library of the tree given
with --parent-tree (a checkout of the parent commit with its own build), or on this tree's when none is given; (b) on
this tree's.  Every (way, round) is a child process of its own, under its own time limit, and the ways are alternated
ROUNDS times (a b a b ...): drifts of the box show as the spread between rounds.  A child warms up once and times
EVALS evaluations per kind (the median counts); U and the cleaned data are compared across the ways by digest.

The last (b) child of a size also measures the cost of per-lane loads of U in the filter: prom_detrend_kernel_ms and
prom_filter_kernel_ms of the single-basis instantiations against the per-order ones on identical data, with every U_s
equal, alternated three times.

  python tools/sysrem_orders_bench.py [--config C3] [--rounds 3] [--parent-tree PATH]
                                      [--out profiles/sysrem_orders_latency.txt]
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
SIZES = ((24, 2000), (80, 4000))                 # (orders, pixels of an order)
LIMIT_S = {24: 200, 80: 400}
EVALS = {24: 5, 80: 2}
N_COMP, N_ITER, N_TRIAL, TRIAL = 6, 30, 8, 5


def child(n_seg, n_s, config, way, filt):
    import numpy as np
    from prometheus_amd import _native, configs, setupfile
    from prometheus_amd import lightcurve as lc
    from prometheus_amd import observation as obs
    from detrend_bench import N_EXP, basis, tables
    from sysrem_bench import pixels
    n_pix = n_seg * n_s
    tr = setupfile.build_transit(configs.get(config))
    dev = _native.get_device(0)
    host = tr._host_inputs()
    wav = np.asarray(tr.wavelength)
    n_orb = len(host["orb"])
    ins = obs.Instrument(pixels(np, lc, tr, n_pix), resolving_power=140000.0)
    rng = np.random.default_rng(0)
    x = np.linspace(-1.0, 1.0, n_pix)
    raw = (1.0 + 0.2 * x)[None, :] * (1.0 + 0.05 * np.linspace(-1, 1, N_EXP)[:, None] * np.sin(40.0 * x)[None, :])
    raw = raw * (1.0 + 1e-3 * rng.normal(size=(N_EXP, n_pix)))
    rows, a, F = tables(tr, 1024)
    F = np.ascontiguousarray(F[:, :N_TRIAL])
    ex = obs.Exposures(ins, rows, a, F, raw, np.full(raw.shape, 1e-3))
    dev.transit_set(tr._problem(dev, host, 0, len(wav), 0.0))
    dev.transit_run()
    seg = (n_s * np.arange(n_seg + 1)).astype(np.int32)
    kw = dict(n_comp=N_COMP, n_iter=N_ITER)
    res = {"n_orb": n_orb, "n_wav": len(wav), "n_exp": N_EXP, "n_tap": int(rows.shape[1]), "ms": {}, "digest": {}}

    def table(lo, hi):
        dev.observe_set(ins.lam[lo:hi], ins.sig[lo:hi], ins.truncate, n_orb)
        dev.expose_set(ex.rows, ex.weights, ex.factors, np.ascontiguousarray(ex.data[:, lo:hi]),
                       np.ascontiguousarray(ex.ivar[:, lo:hi]))
        dev.sysrem_set(np.ascontiguousarray(ex.data[:, lo:hi]))

    def digest(U, cleaned):
        h = hashlib.sha256(np.ascontiguousarray(U).tobytes())
        h.update(np.ascontiguousarray(cleaned).tobytes())
        return h.hexdigest()

    if way == "a":
        calls = {"clean": lambda: dev.sysrem_clean(**kw), "inject": lambda: dev.transit_inject(TRIAL, 1.0, **kw)}

        def evaluate(kind):   # (ms of the calls alone, ms with the uploads, digest)
            t_call, Us, cs = 0.0, [], []
            t0 = time.perf_counter()
            for s in range(n_seg):
                table(seg[s], seg[s + 1])
                t1 = time.perf_counter()
                U, cleaned, _ = calls[kind]()              # (ends in a stream synchronise: the copy back)
                t_call += time.perf_counter() - t1
                Us.append(U)
                cs.append(cleaned)
            total = time.perf_counter() - t0
            return t_call * 1e3, total * 1e3, digest(np.stack(Us), np.concatenate(cs, axis=1))
    else:
        table(0, n_pix)
        dev.orders_set(seg, np.arange(n_pix))
        calls = {"clean": lambda: dev.sysrem_clean_orders(**kw),
                 "inject": lambda: dev.transit_inject_orders(TRIAL, 1.0, **kw)}

        def evaluate(kind):
            t0 = time.perf_counter()
            U, cleaned, _ = calls[kind]()
            t = (time.perf_counter() - t0) * 1e3
            return t, t, digest(U, cleaned)
    for kind in ("clean", "inject"):
        evaluate(kind)                                     # warm-up, untimed
        runs = [evaluate(kind) for _ in range(EVALS[n_seg])]
        res["ms"][kind] = statistics.median(r[0] for r in runs)
        res["ms"][kind + " with uploads"] = statistics.median(r[1] for r in runs)
        res["digest"][kind] = runs[-1][2]
    if filt and way == "b":
        # the filter: one basis against a basis per order with every U_s equal, identical data
        Ub = basis()
        res["filter"] = {"k_detrend single": [], "k_detrend per order": [], "k_filter_weights single": [],
                         "k_filter_weights per order": []}
        models = []
        for _ in range(3):
            for name, build in (("single", lambda: dev.detrend_build(Ub)),
                                ("per order", lambda: dev.detrend_build_orders(np.stack([Ub] * n_seg)))):
                build()
                res["filter"]["k_filter_weights " + name].append(dev.filter_kernel_ms(5))
                out = dev.transit_expose_detrended()
                if len(models) < 2:
                    models.append(hashlib.sha256(out[0].tobytes()).hexdigest())
                res["filter"]["k_detrend " + name].append(dev.detrend_kernel_ms(5)[0])
        res["filter_equal"] = models[0] == models[1]
    print("ORDERS_BENCH " + json.dumps(res), flush=True)


def run_child(n_seg, n_s, a, way, filt):
    tree = os.path.abspath(a.parent_tree) if way == "a" and a.parent_tree else REPO
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n_seg), str(n_s), "--config", a.config, "--way", way,
           "--tree", tree] + (["--filter"] if filt else [])
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[n_seg])
    except subprocess.TimeoutExpired:
        sys.stderr.write("(%d orders, %s) did not finish within its limit of %d s: no result\n"
                         % (n_seg, way, LIMIT_S[n_seg]))
        return None                      # the child is killed; nothing more is started on the device
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ORDERS_BENCH ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        return None                      # a failed child ends the session
    return json.loads(line[-1][len("ORDERS_BENCH "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--way", default="b")
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--filter", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sysrem_orders_latency.txt"))
    ap.add_argument("--child", type=int, nargs=2, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "tools"))
    if a.child is not None:
        sys.path.insert(0, a.tree)       # the package (and its library) of the tree this way measures
        child(a.child[0], a.child[1], a.config, a.way, a.filter)
        return 0
    a.rounds = max(3, a.rounds)
    runs = {}
    for n_seg, n_s in SIZES:
        out = {"ms": {}, "digest": {}}
        for r in range(a.rounds):
            for way in ("a", "b"):
                x = run_child(n_seg, n_s, a, way, way == "b" and r == a.rounds - 1)
                if x is None:
                    return 1
                for k, v in x["ms"].items():
                    out["ms"].setdefault(k, {"a": [], "b": []})[way].append(v)
                out["digest"][way] = x["digest"]
                out.update({k: x[k] for k in ("n_orb", "n_wav", "n_exp", "n_tap", "filter", "filter_equal") if k in x})
        runs[n_seg] = out
    x0 = runs[SIZES[0][0]]
    launches = 2 + N_COMP + N_COMP * (2 * N_ITER + 1)
    lines = ["Latency of SYSREM per echelle order, %s with R in device memory (tools/sysrem_orders_bench.py):" % a.config,
             "pixels spread over the grid at R = 140,000, %d exposures over the %d phases (%d taps), %d trials, no "
             "high-pass;" % (x0["n_exp"], x0["n_orb"], x0["n_tap"], N_TRIAL),
             "SYSREM with %d components of %d iterations (%d launches a call); %d wavelengths; contiguous orders of "
             "equal length." % (N_COMP, N_ITER, launches, x0["n_wav"]),
             "The median of %s evaluations per way, kind and round by the host clock, each (way, round) in a process of "
             "its own after a warm-up;" % " / ".join(str(EVALS[n]) for n, _ in SIZES),
             "the ways alternated a b ... for %d rounds." % a.rounds,
             "  (a)  the parent's route, %s: a loop over the orders of sysrem_clean / transit_inject on"
             % ("the parent commit's tree and library" if a.parent_tree else "this tree's library (no parent tree given)"),
             "       per-order tables.  'calls': the n_seg calls alone; 'with uploads': with every order's pixels, table "
             "and raw exposures going up before its call",
             "  (b)  one sysrem_clean_orders / transit_inject_orders on the whole table, this tree's library", ""]
    for n_seg, n_s in SIZES:
        x = runs[n_seg]
        lines.append("%d orders x %d pixels (%d pixels):" % (n_seg, n_s, n_seg * n_s))
        for kind in ("clean", "inject"):
            med, spread = {}, {}
            for label, key in (("calls", kind), ("with uploads", kind + " with uploads")):
                for w in ("a", "b"):
                    if w == "b" and label != "calls":
                        continue
                    v = x["ms"][key][w]
                    med[w, label], spread[w, label] = statistics.median(v), max(v) - min(v)
                    lines.append("  %-6s (%s) %-12s ms per round: %s   median %.3f   spread (max - min) %.3f"
                                 % (kind, w, label if w == "a" else "one call", " ".join("%.3f" % t for t in v),
                                    med[w, label], spread[w, label]))
            for label in ("calls", "with uploads"):
                gain = med["a", label] - med["b", "calls"]
                lines.append("  %-6s (a) %s / (b) = %.2f, (a) - (b) = %.3f ms against spreads of %.3f and %.3f ms: (b) %s"
                             % (kind, label, med["a", label] / med["b", "calls"], gain, spread["a", label],
                                spread["b", "calls"],
                                "beats (a) by more than the two spreads" if gain > spread["a", label] + spread["b", "calls"]
                                else "does NOT beat (a) by more than the two spreads"))
            lines.append("  %-6s U and the cleaned data of (a) and (b) are bitwise equal: %s"
                         % (kind, x["digest"]["a"][kind] == x["digest"]["b"][kind]))
        if "filter" in x:
            lines.append("  the filter, one basis against a basis per order with every U_s equal (device durations in ms of "
                         "5 launches each, alternated three times; the moments of the two filters are bitwise equal: %s):"
                         % x["filter_equal"])
            for k in ("k_filter_weights", "k_detrend"):
                s1, s2 = x["filter"][k + " single"], x["filter"][k + " per order"]
                m1, m2 = statistics.median(s1), statistics.median(s2)
                sp = (max(s1) - min(s1)) + (max(s2) - min(s2))
                lines.append("    %-16s single %s   per order %s   per order / single = %.3f, difference %.4f ms against "
                             "spreads of %.4f ms together: %s"
                             % (k, " ".join("%.4f" % t for t in s1), " ".join("%.4f" % t for t in s2), m2 / m1, m2 - m1, sp,
                                "the per-lane loads of U cost more than the spread" if m2 - m1 > sp else
                                "inside the spread"))
        lines.append("")
    lines += ["Not measured: hardware counters (no rocprofv3 --pmc run); other n_comp and n_iter than %d and %d; unequal "
              "orders (every item is as wide as the longest order); interleaved orders; the high-pass." % (N_COMP, N_ITER)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
