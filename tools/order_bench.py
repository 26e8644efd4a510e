#!/usr/bin/env python3
"""Latency of one likelihood evaluation with per-order moments on the device (GPU box), on C3 with the inputs resident
(one transit_run, then R, the pixels, the exposure table, the high-pass, the SYSREM filter and the orders stay in device
memory): the setup of tools/highpass_bench.py (2,000 pixels of 0.01 A about Na D at R = 140,000, 48 exposures over the
16 phases, three sub-samples each, a basis of 6 components, a Gaussian high-pass of sigma = 40 pixels) with the 2,000
pixels cut into 4 orders of 500 and into 40 orders of 50, for one trial and for 1,024 trials:

  (x)  transit_expose_orders with the high-pass and the filter: the lumped moments and the totals, no records
  (y)  the same with the records brought back
  (bd) transit_expose_highpass with detrend = 1, moments only: untouched code, the floor
  (a)  what a user has without it: transit_expose_highpass(detrend = 1) with the final model brought back
       ([n_exp][n_trial][n_pix] doubles) and the per-order moments in numpy (the orders are contiguous here, so one
       reshape and seven sums)

One child process per trial count, under its own time limit; inside it the ways are alternated ROUNDS times
(bd x4 y4 a4 x40 y40 a40 bd ...), so drifts of the box show as the spread between rounds; the orders of a cut are set
before the clock starts.  Also reported: the device durations of k_order_moments and k_order_totals
(prom_orders_kernel_ms) and the bytes the algorithm needs.

  python tools/order_bench.py [--config C3] [--rounds 4] [--out profiles/order_moments_latency.txt]
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
CUTS = (4, 40)
WAYS = ("bd",) + tuple("%s%d" % (w, c) for c in CUTS for w in ("x", "y", "a"))
TRIALS = (1, 1024)
LIMIT_S = {1: 240, 1024: 560}
N_EXP, N_SUB, N_COMP, SIGMA_PIX, N_PIX = 48, 3, 6, 40.0, 2000


def evals(n_trial, way):
    if n_trial == 1:
        return 20
    return 1 if way.startswith("a") else 5


def host_order_moments(M, data, ivar, n_seg):
    """The seven moments per (exposure, trial, order) of contiguous orders of equal length, in numpy."""
    import numpy as np
    E, J, P = M.shape
    M = M.reshape(E, J, n_seg, P // n_seg)
    iv, d = ivar.reshape(E, 1, n_seg, -1), data.reshape(E, 1, n_seg, -1)
    one = np.broadcast_to
    return np.stack([one(iv, M.shape).sum(-1), (iv * M).sum(-1), one(iv * d, M.shape).sum(-1), (iv * M * M).sum(-1),
                     (iv * M * d).sum(-1), one(iv * d * d, M.shape).sum(-1), (iv * (M - d) ** 2).sum(-1)], axis=-1)


def child(n_trial, config, rounds):
    import numpy as np
    from prometheus_amd import _native, configs, setupfile
    from prometheus_amd import lightcurve as lc
    from prometheus_amd import observation as obs
    from detrend_bench import basis, tables
    tr = setupfile.build_transit(configs.get(config))
    dev = _native.get_device(0)
    host = tr._host_inputs()
    wav = np.asarray(tr.wavelength)
    dev.transit_set(tr._problem(dev, host, 0, len(wav), 0.0))
    dev.transit_run()
    n_orb = len(host["orb"])
    lam = 0.5 * (lc.NA_D2 + lc.NA_D1) + 1e-10 * (np.arange(N_PIX) - N_PIX // 2)
    sig = lam / (140000.0 * 2.3548200450309493)
    rng = np.random.default_rng(0)
    data = 1e-4 * rng.normal(size=(N_EXP, len(lam)))          # cleaned data scatter about 0
    ivar = np.full(data.shape, 1e6)
    rows, a, F = tables(tr, n_trial)
    U = basis()
    W = obs.filter_weights(U, ivar)
    g = obs.gaussian_taps(SIGMA_PIX)
    dev.observe_set(lam, sig, 5.0, n_orb)
    dev.expose_set(rows, a, F, data, ivar)
    dev.detrend_set(U, W)
    dev.highpass_set([0, len(lam)], np.arange(len(lam)), g, 0)
    perm = np.arange(len(lam))
    segs = {c: np.arange(0, len(lam) + 1, len(lam) // c) for c in CUTS}
    model_bytes = 8 * N_EXP * n_trial * len(lam)
    res = {"n_orb": n_orb, "n_wav": len(wav), "n_pix": len(lam), "n_trial": n_trial, "n_exp": N_EXP,
           "n_tap": int(rows.shape[1]), "n_comp": N_COMP, "half_width": len(g) - 1, "model_bytes": model_bytes}

    def way_a(c):
        M = dev.transit_expose_highpass(detrend=True, moments=False, model=True)[2]
        if np.isnan(M).any():
            raise RuntimeError("the bench's model holds NaN: the plain sums of (a) do not apply")
        return host_order_moments(M, data, ivar, c)[..., 6].sum(axis=2)
    steps = {"bd": lambda: dev.transit_expose_highpass(detrend=True)[0][..., 6]}
    for c in CUTS:
        steps["x%d" % c] = lambda: dev.transit_expose_orders(highpass=True, detrend=True, records=False)[4][..., 1]
        steps["y%d" % c] = lambda: dev.transit_expose_orders(highpass=True, detrend=True)[2][..., 6].sum(axis=2)
        steps["a%d" % c] = lambda c=c: way_a(c)

    def prepare(w):                                           # (untimed: the orders of the way's cut)
        if w != "bd":
            dev.orders_set(segs[int(w[1:])], perm)
    last = {}
    for w in WAYS:                                             # warm-up, untimed
        prepare(w)
        for _ in range(1 if (w.startswith("a") and n_trial > 1) else 2):
            last[w] = steps[w]()
    per_round = {w: [] for w in WAYS}
    for _ in range(rounds):
        for w in WAYS:
            prepare(w)
            t = []
            for _ in range(evals(n_trial, w)):
                t0 = time.perf_counter()
                last[w] = steps[w]()     # ends in a stream synchronise (the copy back)
                t.append((time.perf_counter() - t0) * 1e3)
            per_round[w].append(statistics.median(t))
    res["ms"] = per_round
    res["chi2_sum"] = {w: float(np.sum(last[w])) for w in WAYS}
    res["k_ms"] = {}
    for c in CUTS:
        prepare("x%d" % c)
        steps["x%d" % c]()
        res["k_ms"][str(c)] = [dev.orders_kernel_ms(10) for _ in range(rounds)]
    print("ORDER_BENCH " + json.dumps(res), flush=True)


def run_child(n_trial, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n_trial), "--config", a.config, "--rounds",
           str(a.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[n_trial])
    except subprocess.TimeoutExpired:
        sys.stderr.write("(%d trials) did not finish within its limit of %d s: no result\n" % (n_trial, LIMIT_S[n_trial]))
        return None                      # the child is killed; nothing more is started on the device
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ORDER_BENCH ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        return None                      # a failed child ends the session
    return json.loads(line[-1][len("ORDER_BENCH "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "order_moments_latency.txt"))
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
        print("%d trial(s): done" % n, flush=True)
    x0 = runs[1]
    lines = ["Latency of one likelihood evaluation with per-order moments, %s with the inputs resident and R in device "
             "memory" % a.config,
             "(tools/order_bench.py): %d pixels of 0.01 A about Na D at R = 140,000, %d exposures over the %d phases, "
             "%d sub-samples (%d taps)," % (x0["n_pix"], x0["n_exp"], x0["n_orb"], N_SUB, x0["n_tap"]),
             "a Gaussian high-pass of sigma = %g pixels cut at h = %d over one segment, subtracting; a basis of %d "
             "components; %d wavelengths;" % (SIGMA_PIX, x0["half_width"], x0["n_comp"], x0["n_wav"]),
             "the pixels cut into %s contiguous orders of equal length, all kept." % " and into ".join(map(str, CUTS)),
             "Per round the median of the evaluations by the host clock (each ends in a stream synchronise); one process "
             "per trial count,",
             "in it the ways alternated %s ... for %d rounds; everything resident is set once, the orders of a cut before "
             "the clock." % (" ".join(WAYS), a.rounds),
             "  (xN) transit_expose_orders(highpass = 1, detrend = 1) with N orders: lumped moments and totals, no records",
             "  (yN) the same with the records brought back",
             "  (bd) transit_expose_highpass(detrend = 1), moments only: untouched code, the floor",
             "  (aN) transit_expose_highpass(detrend = 1) with the final model brought back and the per-order moments in "
             "numpy", ""]
    for n in TRIALS:
        x = runs[n]
        med, spread = {}, {}
        lines.append("%d trial(s):" % n)
        for w in WAYS:
            v = x["ms"][w]
            med[w], spread[w] = statistics.median(v), max(v) - min(v)
            lines.append("  (%-3s, %2d evaluations a round) ms per round: %s   median %.4f   spread (max - min) %.4f"
                         % (w, evals(n, w), " ".join("%.4f" % t for t in v), med[w], spread[w]))
        for c in CUTS:
            xs, ys, as_ = "x%d" % c, "y%d" % c, "a%d" % c
            cost, sc = med[xs] - med["bd"], max(spread[xs], spread["bd"])
            rec, sr = med[ys] - med[xs], max(spread[ys], spread[xs])
            gain, sg = med[as_] - med[xs], max(spread[as_], spread[xs])
            km = statistics.median(k[0] for k in x["k_ms"][str(c)])
            kt = statistics.median(k[1] for k in x["k_ms"][str(c)])
            rec_bytes = 64 * x["n_exp"] * n * c
            lines += ["  %d orders: the feature's cost (x) - (bd) = %.4f ms against a spread of %.4f ms, (x) / (bd) = %.4f: %s"
                      % (c, cost, sc, med[xs] / med["bd"], "above the spread" if abs(cost) > sc else
                         "NOT told apart from the spread"),
                      "    the records (y) - (x) = %.4f ms against a spread of %.4f ms (%.2f MB over the bus)"
                      % (rec, sr, rec_bytes / 1e6),
                      "    (a) - (x) = %.4f ms against a spread of %.4f ms, (a) / (x) = %.1f: (x) is %s"
                      % (gain, sg, med[as_] / med[xs], "faster than (a) by more than the spread" if gain > sg else
                         "NOT faster than (a) by more than the spread"),
                      "    k_order_moments by device events, means of 10, one per round: %s ms, median %.4f ms"
                      % (" ".join("%.4f" % k[0] for k in x["k_ms"][str(c)]), km),
                      "    k_order_totals likewise: %s ms, median %.4f ms"
                      % (" ".join("%.4f" % k[1] for k in x["k_ms"][str(c)]), kt),
                      "    the algorithm needs %.1f MB (the model read once, a flag byte per value of a trial, the records "
                      "written): %.3f TB/s if that were" % ((x["model_bytes"] + x["model_bytes"] / 8 / x["n_exp"]
                                                              + rec_bytes) / 1e6,
                                                             (x["model_bytes"] + x["model_bytes"] / 8 / x["n_exp"]
                                                              + rec_bytes) / (km * 1e-3) / 1e12),
                      "    the traffic (a derived count, not an HBM figure: no counter was read)"]
        lines += ["  (a) brings %.1f MB of model over the bus an evaluation, (x) 88 bytes per (exposure, trial)"
                  % (x["model_bytes"] / 1e6),
                  "  sum of chi2 over the table and the orders: " + "  ".join("(%s) %.17g" % (w, x["chi2_sum"][w])
                                                                              for w in WAYS), ""]
    lines += ["Not measured: hardware counters (no rocprofv3 --pmc run), so neither the traffic that reaches HBM nor the L1 "
              "hit rate of the", "gathered reads; orders that interleave in the device's pixel order (perm is the "
              "identity here); orders of unequal length; a record", "buffer above the scratch cap (several batches); "
              "the call without the lumped moments."]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
