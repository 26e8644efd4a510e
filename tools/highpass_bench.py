#!/usr/bin/env python3
"""Latency of one likelihood evaluation against high-pass filtered exposures with and without the filter on the device
(GPU box), on C3 with the inputs resident (one transit_run, then R, the pixels, the exposure table, the high-pass and
the SYSREM filter stay in device memory): the setup of tools/detrend_bench.py (2,000 pixels of 0.01 A about Na D at
R = 140,000, 48 exposures over the 16 phases, three sub-samples each, a basis of 6 components) with a Gaussian
high-pass of sigma = 40 pixels cut at 4 sigma (h = 160) over one order, for one trial and for 1,024 trials:

  (a)  what a user has without it: transit_expose with the model brought back ([n_exp][n_trial][n_pix] doubles), then
       the high-pass and the seven moments in numpy.  For one trial the high-pass is observation.high_pass; for 1,024
       trials that loop (321 numpy passes over 786 MB) takes minutes, so the stand-in is the fastest numpy form of the
       same filter for a model without NaN, one matrix product M - M K^T with the banded, row-normalised K
  (b)  transit_expose_highpass, moments only
  (c)  transit_expose, moments only: no filter at all, the floor
  (bd) transit_expose_highpass with detrend = 1, moments only
  (cd) transit_expose_detrended, moments only: the SYSREM filter alone

One child process per trial count, under its own time limit; inside it the ways are alternated ROUNDS times
(a b c bd cd a b ...), so drifts of the box show as the spread between rounds.  Also reported: the device duration of
k_highpass (prom_highpass_kernel_ms) and the bytes the algorithm needs.

  python tools/highpass_bench.py [--config C3] [--rounds 4] [--out profiles/highpass_latency.txt]
  python tools/highpass_bench.py --kernel-only     (k_highpass' duration alone, e.g. of a variant library named by
                                                    PROMETHEUS_AMD_LIB)
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
WAYS = ("a", "b", "c", "bd", "cd")
TRIALS = (1, 1024)
LIMIT_S = {1: 240, 1024: 560}
EVALS = {1: dict(a=20, b=20, c=20, bd=20, cd=20), 1024: dict(a=1, b=5, c=5, bd=5, cd=5)}
N_EXP, N_SUB, N_COMP, SIGMA_PIX = 48, 3, 6, 40.0


def host_moments(M, data, ivar):
    import numpy as np
    iv, d = ivar[:, None, :], data[:, None, :]
    return np.stack([np.broadcast_to(iv, M.shape).sum(-1), (iv * M).sum(-1), np.broadcast_to(iv * d, M.shape).sum(-1),
                     (iv * M * M).sum(-1), (iv * M * d).sum(-1), np.broadcast_to(iv * d * d, M.shape).sum(-1),
                     (iv * (M - d) ** 2).sum(-1)], axis=-1)


def band_matrix(g, n):
    """K[n][n] with K[i][i'] = g[|i - i'|] / sum over the window: B = M K^T for a model without NaN."""
    import numpy as np
    d = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    K = np.where(d < len(g), g[np.minimum(d, len(g) - 1)], 0.0)
    return np.ascontiguousarray(K / K.sum(axis=1, keepdims=True))


def child(n_trial, config, rounds, kernel_only):
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
    lam = 0.5 * (lc.NA_D2 + lc.NA_D1) + 1e-10 * (np.arange(2000) - 1000)
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
    model_bytes = 8 * N_EXP * n_trial * len(lam)
    res = {"n_orb": n_orb, "n_wav": len(wav), "n_pix": len(lam), "n_trial": n_trial, "n_exp": N_EXP,
           "n_tap": int(rows.shape[1]), "n_comp": N_COMP, "half_width": len(g) - 1, "model_bytes": model_bytes,
           "lib": os.environ.get("PROMETHEUS_AMD_LIB", "")}
    if kernel_only:
        dev.transit_expose_highpass()
        res["k_highpass_ms"] = [dev.highpass_kernel_ms(10) for _ in range(max(1, rounds))]
        print("HIGHPASS_BENCH " + json.dumps(res), flush=True)
        return
    K = band_matrix(g, len(lam)) if n_trial > 1 else None

    def way_a():
        M = dev.transit_expose(moments=False, model=True)[2]
        if np.isnan(M).any():
            raise RuntimeError("the bench's model holds NaN: the matrix form of (a) does not apply")
        Mf = obs.high_pass(M, g) if K is None else M - M @ K.T
        return host_moments(Mf, data, ivar)
    steps = {"a": way_a, "b": lambda: dev.transit_expose_highpass()[0], "c": lambda: dev.transit_expose()[0],
             "bd": lambda: dev.transit_expose_highpass(detrend=True)[0],
             "cd": lambda: dev.transit_expose_detrended()[0]}
    last = {}
    for w in WAYS:                                             # warm-up, untimed
        for _ in range(1 if (w == "a" and n_trial > 1) else 2):
            last[w] = steps[w]()
    per_round = {w: [] for w in WAYS}
    for _ in range(rounds):
        for w in WAYS:
            t = []
            for _ in range(EVALS[n_trial][w]):
                t0 = time.perf_counter()
                last[w] = steps[w]()     # ends in a stream synchronise (the copy back)
                t.append((time.perf_counter() - t0) * 1e3)
            per_round[w].append(statistics.median(t))
    res["ms"] = per_round
    res["chi2_sum"] = {w: float(np.sum(last[w][..., 6])) for w in WAYS}
    dev.transit_expose_highpass()
    res["k_highpass_ms"] = [dev.highpass_kernel_ms(10) for _ in range(rounds)]
    dev.transit_expose()
    res["k_expose_ms"] = dev.expose_kernel_ms(10)
    print("HIGHPASS_BENCH " + json.dumps(res), flush=True)


def run_child(n_trial, a, extra=()):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n_trial), "--config", a.config, "--rounds",
           str(a.rounds)] + list(extra)
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[n_trial])
    except subprocess.TimeoutExpired:
        sys.stderr.write("(%d trials) did not finish within its limit of %d s: no result\n" % (n_trial, LIMIT_S[n_trial]))
        return None                      # the child is killed; nothing more is started on the device
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("HIGHPASS_BENCH ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        return None                      # a failed child ends the session
    return json.loads(line[-1][len("HIGHPASS_BENCH "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "highpass_latency.txt"))
    ap.add_argument("--child", type=int, default=None)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "tools"))
    if a.child is not None:
        child(a.child, a.config, a.rounds, a.kernel_only)
        return 0
    if a.kernel_only:
        for n in TRIALS:
            x = run_child(n, a, ["--kernel-only"])
            if x is None:
                return 1
            print("%s %d trial(s): k_highpass %s ms (means of 10)" % (
                x["lib"] or "the package's library", n, " ".join("%.4f" % v for v in x["k_highpass_ms"])), flush=True)
        return 0
    a.rounds = max(4, a.rounds)
    runs = {}
    for n in TRIALS:
        runs[n] = run_child(n, a)
        if runs[n] is None:
            return 1
    x0 = runs[1]
    lines = ["Latency of one likelihood evaluation against high-pass filtered exposures, %s with the inputs resident and R "
             "in device memory" % a.config,
             "(tools/highpass_bench.py): %d pixels of 0.01 A about Na D at R = 140,000, %d exposures over the %d phases, "
             "%d sub-samples (%d taps)," % (x0["n_pix"], x0["n_exp"], x0["n_orb"], N_SUB, x0["n_tap"]),
             "a Gaussian high-pass of sigma = %g pixels cut at h = %d over one order, subtracting; a basis of %d "
             "components; %d wavelengths." % (SIGMA_PIX, x0["half_width"], x0["n_comp"], x0["n_wav"]),
             "Per round the median of the evaluations by the host clock (each ends in a stream synchronise); one process "
             "per trial count,",
             "in it the ways alternated %s ... for %d rounds; everything resident is set once, before the clock."
             % (" ".join(WAYS), a.rounds),
             "  (a)  transit_expose with the model brought back, the high-pass and the moments in numpy (1 trial: "
             "observation.high_pass;",
             "       1,024 trials: the matrix product M - M K^T, the fastest numpy form without NaN: high_pass' own "
             "loop was not run there)",
             "  (b)  transit_expose_highpass, moments only",
             "  (c)  transit_expose, moments only: no filter, the floor",
             "  (bd) transit_expose_highpass with detrend = 1        (cd) transit_expose_detrended", ""]
    for n in TRIALS:
        med, spread = {}, {}
        lines.append("%d trial(s):" % n)
        for w in WAYS:
            v = runs[n]["ms"][w]
            med[w], spread[w] = statistics.median(v), max(v) - min(v)
            lines.append("  (%-2s, %2d evaluations a round) ms per round: %s   median %.4f   spread (max - min) %.4f"
                         % (w, EVALS[n][w], " ".join("%.4f" % t for t in v), med[w], spread[w]))
        cost, sc = med["b"] - med["c"], max(spread["b"], spread["c"])
        costd, scd = med["bd"] - med["cd"], max(spread["bd"], spread["cd"])
        gain, sg = med["a"] - med["b"], max(spread["a"], spread["b"])
        kh = statistics.median(runs[n]["k_highpass_ms"])
        x = runs[n]
        need = 2 * x["model_bytes"] + 4 * x["n_pix"]
        lines += ["  the feature's cost (b) - (c) = %.4f ms against a spread of %.4f ms, (b) / (c) = %.3f" % (
                      cost, sc, med["b"] / med["c"]),
                  "  with the SYSREM filter (bd) - (cd) = %.4f ms against a spread of %.4f ms, (bd) / (cd) = %.3f" % (
                      costd, scd, med["bd"] / med["cd"]),
                  "  (a) - (b) = %.4f ms against a spread of %.4f ms, (a) / (b) = %.1f: (b) is %s" % (
                      gain, sg, med["a"] / med["b"], "faster than (a) by more than the spread" if gain > sg else
                      "NOT faster than (a) by more than the spread"),
                  "  (a) brings %.1f MB of model over the bus an evaluation, the others 64 bytes per (exposure, trial)"
                  % (x["model_bytes"] / 1e6),
                  "  sum of chi2 over the table: " + "  ".join("(%s) %.17g" % (w, x["chi2_sum"][w]) for w in WAYS),
                  "  k_highpass by device events, means of 10, one per round: %s ms, median %.4f ms"
                  % (" ".join("%.4f" % v for v in x["k_highpass_ms"]), kh),
                  "    the algorithm needs %.1f MB (the model read once and written once, perm once): %.3f TB/s if "
                  "that were the traffic" % (need / 1e6, need / (kh * 1e-3) / 1e12),
                  "    (a derived count, not an HBM figure: no counter was read)",
                  "    the window costs %d multiplies and %d additions per value: %.2f T operations a second"
                  % (2 * x["half_width"] + 1, 2 * x["half_width"] + 1,
                     2.0 * (2 * x["half_width"] + 1) * x["model_bytes"] / 8 / (kh * 1e-3) / 1e12),
                  "  k_expose (moments only, the floor's kernel, first batch) %.4f ms" % x["k_expose_ms"], ""]
    lines += ["Not measured: hardware counters (no rocprofv3 --pmc run), so neither the traffic that reaches HBM nor LDS "
              "bank conflicts; observation.high_pass", "itself at 1,024 trials; (a) with the SYSREM filter in numpy; "
              "several orders; mode 1; half widths other than %d." % x0["half_width"]]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
