#!/usr/bin/env python3
"""Latency of one likelihood evaluation against median-filtered exposures with and without the median on the device
(GPU box), on C3 with the inputs resident: the setup of tools/highpass_bench.py (2,000 pixels of 0.01 A about Na D at
R = 140,000, 48 exposures over the 16 phases, three sub-samples each) with a running median of half width h = 160 over
one order, subtracting, for one trial and for 1,024 trials:

  (a)  what a user has without it: transit_expose with the model brought back ([n_exp][n_trial][n_pix] doubles), then
       the median (observation.high_pass with a median_window) and the seven moments in numpy.  For 1,024 trials
       high_pass over all 49,152 rows takes the better part of an hour, so the clock runs over the whole transfer, the
       whole moments and the median of ONE trial's rows (48 of them): a lower bound of (a), measured.  The line
       "extrapolated" adds the other trials' medians at the measured cost per row
  (b)  transit_expose_highpass with the median resident, moments only
  (c)  transit_expose_highpass with the Gaussian mean of the same half width resident, moments only: the floor

One child process per trial count, under its own time limit; inside it the ways are alternated ROUNDS times
(a b c a b ...), so drifts of the box show as the spread between rounds.  The resident high-pass is swapped (untimed)
before (b) and (c).  Also reported: the device durations of k_median and k_highpass (prom_highpass_kernel_ms).

  python tools/median_bench.py [--config C3] [--rounds 4] [--out profiles/median_latency.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
WAYS = ("a", "b", "c")
TRIALS = (1, 1024)
LIMIT_S = {1: 240, 1024: 560}
EVALS = {1: dict(a=2, b=20, c=20), 1024: dict(a=1, b=5, c=5)}
N_EXP, HALF = 48, 160


def child(n_trial, config, rounds):
    import numpy as np
    from prometheus_amd import _native, configs, setupfile
    from prometheus_amd import lightcurve as lc
    from prometheus_amd import observation as obs
    from detrend_bench import tables
    from highpass_bench import host_moments
    tr = setupfile.build_transit(configs.get(config))
    dev = _native.get_device(0)
    host = tr._host_inputs()
    wav = np.asarray(tr.wavelength)
    dev.transit_set(tr._problem(dev, host, 0, len(wav), 0.0))
    dev.transit_run()
    n_orb = len(host["orb"])
    lam = 0.5 * (lc.NA_D2 + lc.NA_D1) + 1e-10 * (np.arange(2000) - 1000)
    sig = lam / (140000.0 * 2.3548200450309493)
    rng = np.random.default_rng(0)
    data = 1e-4 * rng.normal(size=(N_EXP, len(lam)))
    ivar = np.full(data.shape, 1e6)
    rows, a, F = tables(tr, n_trial)
    g = obs.gaussian_taps(HALF / 4.0)
    assert len(g) - 1 == HALF
    win = obs.median_window(HALF)
    seg, perm = [0, len(lam)], np.arange(len(lam))
    dev.observe_set(lam, sig, 5.0, n_orb)
    dev.expose_set(rows, a, F, data, ivar)
    res = {"n_orb": n_orb, "n_wav": len(wav), "n_pix": len(lam), "n_trial": n_trial, "n_exp": N_EXP,
           "n_tap": int(rows.shape[1]), "half_width": HALF, "model_bytes": 8 * N_EXP * n_trial * len(lam)}
    row_ms = []

    def way_a():
        M = dev.transit_expose(moments=False, model=True)[2]
        t0 = time.perf_counter()
        first = obs.high_pass(M[:, :1], win)                  # one trial's rows
        row_ms.append((time.perf_counter() - t0) * 1e3 / N_EXP)
        Mf = first if n_trial == 1 else np.concatenate([first, M[:, 1:]], axis=1)    # (the others stay unfiltered)
        return host_moments(Mf, data, ivar)

    def resident(kind):
        if kind == "median":
            dev.highpass_set_median(seg, perm, HALF, 0)
        else:
            dev.highpass_set(seg, perm, g, 0)
    steps = {"a": way_a, "b": lambda: dev.transit_expose_highpass()[0], "c": lambda: dev.transit_expose_highpass()[0]}
    before = {"a": lambda: None, "b": lambda: resident("median"), "c": lambda: resident("mean")}
    last = {}
    for w in WAYS:                                             # warm-up, untimed
        before[w]()
        for _ in range(1 if w == "a" else 2):
            last[w] = steps[w]()
    per_round = {w: [] for w in WAYS}
    for _ in range(rounds):
        for w in WAYS:
            before[w]()
            t = []
            for _ in range(EVALS[n_trial][w]):
                t0 = time.perf_counter()
                last[w] = steps[w]()     # ends in a stream synchronise (the copy back)
                t.append((time.perf_counter() - t0) * 1e3)
            per_round[w].append(statistics.median(t))
    res["ms"] = per_round
    res["row_ms"] = statistics.median(row_ms)
    res["chi2_sum"] = {w: float(np.sum(last[w][..., 6])) for w in WAYS}
    resident("median")
    dev.transit_expose_highpass()
    res["k_median_ms"] = [dev.highpass_kernel_ms(10) for _ in range(rounds)]
    resident("mean")
    dev.transit_expose_highpass()
    res["k_highpass_ms"] = [dev.highpass_kernel_ms(10) for _ in range(rounds)]
    print("MEDIAN_BENCH " + json.dumps(res), flush=True)


def run_child(n_trial, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n_trial), "--config", a.config, "--rounds",
           str(a.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[n_trial])
    except subprocess.TimeoutExpired:
        sys.stderr.write("(%d trials) did not finish within its limit of %d s: no result\n" % (n_trial, LIMIT_S[n_trial]))
        return None                      # the child is killed; nothing more is started on the device
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("MEDIAN_BENCH ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        return None                      # a failed child ends the session
    return json.loads(line[-1][len("MEDIAN_BENCH "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "median_latency.txt"))
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "tools"))
    if a.child is not None:
        child(a.child, a.config, a.rounds)
        return 0
    a.rounds = max(4, a.rounds)
    runs = {}
    for n in TRIALS:
        runs[n] = run_child(n, a)
        if runs[n] is None:
            return 1
    x0 = runs[1]
    lines = ["Latency of one likelihood evaluation against median-filtered exposures, %s with the inputs resident and R in "
             "device memory" % a.config,
             "(tools/median_bench.py): %d pixels of 0.01 A about Na D at R = 140,000, %d exposures over the %d phases, "
             "%d taps," % (x0["n_pix"], x0["n_exp"], x0["n_orb"], x0["n_tap"]),
             "a running median of half width h = %d over one order, subtracting; %d wavelengths."
             % (x0["half_width"], x0["n_wav"]),
             "Per round the median of the evaluations by the host clock (each ends in a stream synchronise); one process "
             "per trial count,",
             "in it the ways alternated %s ... for %d rounds; the resident high-pass is swapped before (b) and (c), "
             "outside the clock." % (" ".join(WAYS), a.rounds),
             "  (a)  transit_expose with the model brought back, observation.high_pass with the window and the moments "
             "in numpy;",
             "       at 1,024 trials the median of ONE trial's 48 rows only (a measured lower bound of (a))",
             "  (b)  transit_expose_highpass with the median resident, moments only",
             "  (c)  transit_expose_highpass with the Gaussian mean of the same half width resident: the floor", ""]
    for n in TRIALS:
        x = runs[n]
        med, spread = {}, {}
        lines.append("%d trial(s):" % n)
        for w in WAYS:
            v = x["ms"][w]
            med[w], spread[w] = statistics.median(v), max(v) - min(v)
            lines.append("  (%-1s, %2d evaluations a round) ms per round: %s   median %.4f   spread (max - min) %.4f"
                         % (w, EVALS[n][w], " ".join("%.4f" % t for t in v), med[w], spread[w]))
        cost, sc = med["b"] - med["c"], max(spread["b"], spread["c"])
        gain, sg = med["a"] - med["b"], max(spread["a"], spread["b"])
        km, kh = statistics.median(x["k_median_ms"]), statistics.median(x["k_highpass_ms"])
        lines += ["  (a) - (b) = %.4f ms against a spread of %.4f ms, (a) / (b) = %.1f: (b) is %s" % (
                      gain, sg, med["a"] / med["b"], "faster than (a) by more than the spread" if gain > sg else
                      "NOT faster than (a) by more than the spread"),
                  "  the median's cost over the mean (b) - (c) = %.4f ms against a spread of %.4f ms, (b) / (c) = %.3f"
                  % (cost, sc, med["b"] / med["c"])]
        if n > 1:
            lines.append("  (a) extrapolated: + %d trials x %d rows x %.2f ms a row (numpy, measured) = %.0f s an evaluation"
                         % (n - 1, x["n_exp"], x["row_ms"], (n - 1) * x["n_exp"] * x["row_ms"] / 1e3))
        lines += ["  (a) brings %.1f MB of model over the bus an evaluation, the others 64 bytes per (exposure, trial)"
                  % (x["model_bytes"] / 1e6),
                  "  sum of chi2 over the table: " + "  ".join("(%s) %.17g" % (w, x["chi2_sum"][w]) for w in WAYS)
                  + ("" if n == 1 else "   ((a): one trial filtered)"),
                  "  k_median by device events, means of 10, one per round: %s ms, median %.4f ms"
                  % (" ".join("%.4f" % v for v in x["k_median_ms"]), km),
                  "  k_highpass likewise: %s ms, median %.4f ms; k_median / k_highpass = %.2f"
                  % (" ".join("%.4f" % v for v in x["k_highpass_ms"]), kh, km / kh), ""]
    lines += ["Not measured: hardware counters (no rocprofv3 --pmc run), so neither LDS bank conflicts nor the share of "
              "the sort, the ranks and the bisection", "inside k_median; observation.high_pass over all rows at 1,024 "
              "trials; several orders; mode 1; half widths other than %d." % x0["half_width"]]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
