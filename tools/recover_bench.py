#!/usr/bin/env python3
"""Latency of one point of an injection grid, the injection with its recovery, through the host and on the device (GPU
box), on C3 with the inputs resident: the set-up of tools/sysrem_bench.py (pixels of 0.01 A at R = 140,000, 48
exposures of 6 taps, a Gaussian high-pass of sigma = 40 pixels cut at h = 160 over one order, dividing, SYSREM with 6
components of 30 iterations), at 2,000 pixels x 1,024 trials and at 320,000 pixels x 8 trials:

  (a)  today's route: transit_inject with the cleaned data brought back, observation.Exposures of them,
       observation.Detrend with the host's filter_weights, the uploads of the table, the high-pass and the filter,
       transit_expose_highpass(detrend=1)
  (b)  transit_recover: the same on the device; the moments and U come back

One child process per size, under its own time limit; inside it the ways are alternated ROUNDS times (a b a b ...), so
drifts of the box show as the spread between rounds.  Also reported: the host time of filter_weights alone, and the
device duration of k_filter_weights (prom_filter_kernel_ms) at K in {1, 6, 16} with the bytes and operations its text
implies.

  python tools/recover_bench.py [--config C3] [--rounds 4] [--out profiles/recover_latency.txt]
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
WAYS = ("a", "b")
SIZES = ((2000, 1024), (320000, 8))
LIMIT_S = {2000: 400, 320000: 1000}
EVALS = {2000: dict(a=3, b=10), 320000: dict(a=1, b=3)}
N_COMP, N_ITER, SIGMA_PIX = 6, 30, 40.0
KS = (1, 6, 16)


def child(n_pix, n_trial, config, rounds):
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
    dev.transit_set(tr._problem(dev, host, 0, len(wav), 0.0))
    dev.transit_run()
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
    trial = n_trial // 2
    g = obs.gaussian_taps(SIGMA_PIX)
    ex = obs.Exposures(ins, rows, a, F, raw, err)
    dev.observe_set(ins.lam, ins.sig, ins.truncate, n_orb)
    res = {"n_orb": n_orb, "n_wav": len(wav), "n_pix": n_pix, "n_trial": n_trial, "n_exp": N_EXP,
           "n_tap": int(rows.shape[1]), "half_width": len(g) - 1, "trial": trial}

    def table():   # what both ways start from: the raw table, the high-pass and the raw exposures resident
        dev.expose_set(ex.rows, ex.weights, ex.factors, ex.data, ex.ivar)
        dev.highpass_set([0, n_pix], np.arange(n_pix), g, 1)
        dev.sysrem_set(ex.data)

    def way_a():
        U, cleaned, _ = dev.transit_inject(trial, 1.0, N_COMP, N_ITER, highpass=True)
        ex2 = obs.Exposures(ins, rows, a, F, ins.unsort(cleaned), err)
        dt = obs.Detrend(ex2, U)
        dev.expose_set(ex2.rows, ex2.weights, ex2.factors, ex2.data, ex2.ivar)
        dev.highpass_set([0, n_pix], np.arange(n_pix), g, 1)
        dev.detrend_set(dt.U, dt.W)
        mom, nu, _ = dev.transit_expose_highpass(detrend=True)
        return mom, nu, U

    def way_b():
        out = dev.transit_recover(trial, 1.0, N_COMP, N_ITER, highpass=True)
        return out[0], out[1], out[6]
    steps = {"a": way_a, "b": way_b}
    last = {}
    for w in WAYS:                                             # warm-up, untimed
        table()
        last[w] = steps[w]()
    per_round = {w: [] for w in WAYS}
    for _ in range(rounds):
        for w in WAYS:
            t = []
            for _ in range(EVALS[n_pix][w]):
                table()                                        # (way a leaves another table behind)
                t0 = time.perf_counter()
                last[w] = steps[w]()                           # both end in a stream synchronise (the copy back)
                t.append((time.perf_counter() - t0) * 1e3)
            per_round[w].append(statistics.median(t))
    res["ms"] = per_round
    ok = np.isfinite(last["a"][0]) & np.isfinite(last["b"][0])
    scale = np.abs(last["a"][0][ok]).max()
    res["max_rel_diff_moments"] = float(np.abs(last["a"][0][ok] - last["b"][0][ok]).max() / scale)
    res["n_used_equal"] = bool(np.array_equal(last["a"][1], last["b"][1]))
    table()
    way_b()
    res["filter_ms_in_b"] = [dev.filter_kernel_ms(5) for _ in range(rounds)]
    U = last["b"][2]
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        obs.filter_weights(U, ex.ivar)
        t.append((time.perf_counter() - t0) * 1e3)
    res["host_filter_weights_ms"] = t
    res["kernel_ms"] = {}
    for K in KS:
        Q, _ = np.linalg.qr(rng.standard_normal((N_EXP, K)))
        dev.detrend_build(Q + 0.05 * rng.standard_normal((N_EXP, K)))
        res["kernel_ms"][str(K)] = [dev.filter_kernel_ms(5) for _ in range(rounds)]
    print("RECOVER_BENCH " + json.dumps(res), flush=True)


def run_child(n_pix, n_trial, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n_pix), str(n_trial), "--config", a.config,
           "--rounds", str(a.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[n_pix])
    except subprocess.TimeoutExpired:
        sys.stderr.write("(%d pixels) did not finish within its limit of %d s: no result\n" % (n_pix, LIMIT_S[n_pix]))
        return None                      # the child is killed; nothing more is started on the device
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RECOVER_BENCH ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        return None                      # a failed child ends the session
    return json.loads(line[-1][len("RECOVER_BENCH "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "recover_latency.txt"))
    ap.add_argument("--child", type=int, nargs=2, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "tools"))
    if a.child is not None:
        child(a.child[0], a.child[1], a.config, a.rounds)
        return 0
    a.rounds = max(4, a.rounds)
    runs = {}
    for n, nt in SIZES:
        runs[n] = run_child(n, nt, a)
        if runs[n] is None:
            return 1
    x0 = runs[SIZES[0][0]]
    lines = ["Latency of one injection with its recovery, %s with the inputs resident and R in device memory" % a.config,
             "(tools/recover_bench.py): pixels of 0.01 A at R = 140,000, %d exposures over the %d phases (%d taps), the "
             "middle trial at scale 1," % (x0["n_exp"], x0["n_orb"], x0["n_tap"]),
             "a Gaussian high-pass of sigma = %g pixels cut at h = %d over one order, dividing; SYSREM with %d components "
             "of %d iterations; %d wavelengths." % (SIGMA_PIX, x0["half_width"], N_COMP, N_ITER, x0["n_wav"]),
             "Per round the median of the evaluations by the host clock; one process per size, in it the ways alternated "
             "a b ... for %d rounds;" % a.rounds,
             "the raw table, the high-pass and the raw exposures are set before the clock of every evaluation.",
             "  (a)  transit_inject with the cleaned data brought back, observation.Exposures, observation.Detrend "
             "(filter_weights on the host),",
             "       expose_set, highpass_set, detrend_set, transit_expose_highpass(detrend=1)",
             "  (b)  transit_recover with the high-pass: the moments, n_used and U come back", ""]
    for n, nt in SIZES:
        x = runs[n]
        med, spread = {}, {}
        lines.append("%d pixels x %d trials:" % (n, nt))
        for w in WAYS:
            v = x["ms"][w]
            med[w], spread[w] = statistics.median(v), max(v) - min(v)
            lines.append("  (%s, %2d evaluations a round) ms per round: %s   median %.3f   spread (max - min) %.3f"
                         % (w, EVALS[n][w], " ".join("%.3f" % t for t in v), med[w], spread[w]))
        gain, sg = med["a"] - med["b"], max(spread["a"], spread["b"])
        fb = statistics.median(x["filter_ms_in_b"])
        lines += ["  (a) - (b) = %.3f ms against a spread of %.3f ms, (a) / (b) = %.1f: (b) is %s" % (
                      gain, sg, med["a"] / med["b"], "faster than (a) by more than the spread" if gain > sg else
                      "NOT faster than (a) by more than the spread"),
                  "  moments of (a) and (b) differ by at most %.3g of the largest (two rules for W, the host's LU and "
                  "the device's Cholesky); n_used equal: %s" % (x["max_rel_diff_moments"], x["n_used_equal"]),
                  "  observation.filter_weights alone on the host (K = %d): %s ms" % (
                      N_COMP, " ".join("%.1f" % t for t in x["host_filter_weights_ms"])),
                  "  k_filter_weights inside (b) (K = %d), by device events, means of 5, the median of one per round: "
                  "%.4f ms = %.2f %% of (b)" % (N_COMP, fb, 100.0 * fb / med["b"])]
        for K in KS:
            ms = statistics.median(x["kernel_ms"][str(K)])
            entries = x["n_exp"] * n
            byts = (3 * 8 + K * 8) * entries                      # ivar read in three walks, W written once
            ops = entries * (K * (K + 1) // 2 + 2 * K * K) + n * (K * (K + 1) * (K + 2) // 6)   # N, two solves, the factor
            divs = entries * 2 * 2 * K
            lines.append("  k_filter_weights at K = %2d: %.4f ms; by its text %.1f MB (ivar read three times, W written "
                         "once): %.3f TB/s if that were the traffic; %.3g multiply-add pairs, %.3g divisions: %.2f "
                         "Tpairs/s" % (K, ms, byts / 1e6, byts / (ms * 1e-3) / 1e12, ops, divs, ops / (ms * 1e-3) / 1e12))
        lines.append("")
    lines += ["The byte and operation counts are derived from the kernel's text, not measured: no counter was read.",
              "Not measured: hardware counters (no rocprofv3 --pmc run); several orders; other n_comp and n_iter of "
              "SYSREM than %d and %d; the Python layer's share (Transit.recover against Transit.inject + Transit.expose)."
              % (N_COMP, N_ITER)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
