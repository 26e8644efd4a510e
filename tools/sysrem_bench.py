#!/usr/bin/env python3
"""Latency of one injection with its cleaning, on the host and on the device (GPU box), on C3 with the inputs resident
(one transit_run, then R, the pixels, the exposure table, the high-pass and the raw exposures stay in device memory):
the instrument of tools/detrend_bench.py (pixels of 0.01 A at R = 140,000, 48 exposures over the 16 phases, three
sub-samples each, 32 x 32 trials), a Gaussian high-pass of sigma = 40 pixels cut at 4 sigma (h = 160) over one order,
dividing, and SYSREM with 6 components of 30 iterations; at 2,000 pixels about Na D and at the largest pixel count the
instrument offers, 0.01 A pixels over the whole C3 grid (320,000):

  (a)  today's route: transit_expose with the model of ONE trial brought back (a table of that trial alone), then the
       numpy injection, observation.high_pass and observation.sysrem
  (b)  transit_inject: the same on the device; U and the cleaned data come back

One child process per pixel count, under its own time limit; inside it the ways are alternated ROUNDS times
(a b a b ...), so drifts of the box show as the spread between rounds.  Also reported: the device durations of the
SYSREM loop, the injection and k_highpass (prom_sysrem_kernel_ms), with the bytes the algorithm needs.

  python tools/sysrem_bench.py [--config C3] [--rounds 4] [--out profiles/sysrem_latency.txt]
  python tools/sysrem_bench.py --kernel-only      (the device durations alone at both sizes, e.g. of a variant library
                                                   named by PROMETHEUS_AMD_LIB, built with another PROM_SY_VEC)
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
SIZES = (2000, 320000)
LIMIT_S = {2000: 300, 320000: 1100}
EVALS = {2000: dict(a=5, b=20), 320000: dict(a=1, b=5)}
N_COMP, N_ITER, SIGMA_PIX, TRIAL = 6, 30, 40.0, 500


def pixels(np, lc, tr, n_pix):
    if n_pix == SIZES[0]:
        return 0.5 * (lc.NA_D2 + lc.NA_D1) + 1e-10 * (np.arange(n_pix) - n_pix // 2)
    wav = np.asarray(tr.wavelength)
    return wav[0] + (wav[-1] - wav[0]) * (np.arange(n_pix) + 0.5) / n_pix


def child(n_pix, config, rounds, kernel_only=False):
    import numpy as np
    from prometheus_amd import _native, configs, setupfile
    from prometheus_amd import lightcurve as lc
    from prometheus_amd import observation as obs
    from detrend_bench import N_EXP, tables
    tr = setupfile.build_transit(configs.get(config))
    dev = _native.get_device(0)
    host = tr._host_inputs()
    wav = np.asarray(tr.wavelength)
    dev.transit_set(tr._problem(dev, host, 0, len(wav), 0.0))
    dev.transit_run()
    n_orb = len(host["orb"])
    lam = pixels(np, lc, tr, n_pix)
    sig = lam / (140000.0 * 2.3548200450309493)
    rng = np.random.default_rng(0)
    x = np.linspace(-1.0, 1.0, n_pix)
    raw = (1.0 + 0.2 * x)[None, :] * (1.0 + 0.05 * np.linspace(-1, 1, N_EXP)[:, None] * np.sin(40.0 * x)[None, :])
    raw = raw * (1.0 + 1e-3 * rng.normal(size=(N_EXP, n_pix)))
    err = np.full(raw.shape, 1e-3)
    ivar = 1.0 / (err * err)
    rows, a, F = tables(tr, 1024)
    F1 = np.ascontiguousarray(F[:, TRIAL:TRIAL + 1])
    g = obs.gaussian_taps(SIGMA_PIX)
    dev.observe_set(lam, sig, 5.0, n_orb)
    res = {"n_orb": n_orb, "n_wav": len(wav), "n_pix": n_pix, "n_exp": N_EXP, "n_tap": int(rows.shape[1]),
           "n_comp": N_COMP, "n_iter": N_ITER, "half_width": len(g) - 1, "lib": os.environ.get("PROMETHEUS_AMD_LIB", "")}

    def table(Fx):
        dev.expose_set(rows, a, Fx, raw, ivar)
        dev.highpass_set([0, n_pix], np.arange(n_pix), g, 1)
        dev.sysrem_set(raw)

    # (a) and (b) keep their own resident tables; setting them is outside the clock, as a user's loop would have it:
    # (a) needs the one-trial table, (b) the full one.  The table is set again whenever the way changes.
    def way_a():
        M = dev.transit_expose(moments=False, model=True)[2][:, 0]
        with np.errstate(invalid="ignore"):
            D = np.where(np.isnan(M), raw, raw * (1.0 + 1.0 * (M - 1.0)))
        flat = obs.high_pass(D, g, mode="divide")
        return obs.sysrem(flat, err, N_COMP, N_ITER)

    def way_b():
        U, cleaned, _ = dev.transit_inject(TRIAL, 1.0, N_COMP, N_ITER, highpass=True)
        return U, cleaned
    steps = {"a": (F1, way_a), "b": (F, way_b)}
    if kernel_only:
        table(F)
        way_b()
        res["kernel_ms"] = [dev.sysrem_kernel_ms(3) for _ in range(max(1, rounds))]
        print("SYSREM_BENCH " + json.dumps(res), flush=True)
        return
    last = {}
    for w in WAYS:                                             # warm-up, untimed
        table(steps[w][0])
        last[w] = steps[w][1]()
    per_round = {w: [] for w in WAYS}
    for _ in range(rounds):
        for w in WAYS:
            table(steps[w][0])
            t = []
            for _ in range(EVALS[n_pix][w]):
                t0 = time.perf_counter()
                last[w] = steps[w][1]()     # (b) ends in a stream synchronise (the copy back)
                t.append((time.perf_counter() - t0) * 1e3)
            per_round[w].append(statistics.median(t))
    res["ms"] = per_round
    live = np.isfinite(last["a"][1])
    res["max_abs_diff_cleaned"] = float(np.max(np.abs(last["a"][1][live] - last["b"][1][live])))
    res["max_abs_diff_U"] = float(np.max(np.abs(np.abs(last["a"][0]) - np.abs(last["b"][0]))))
    res["kernel_ms"] = [dev.sysrem_kernel_ms(3) for _ in range(rounds)]
    print("SYSREM_BENCH " + json.dumps(res), flush=True)


def run_child(n_pix, a, extra=()):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n_pix), "--config", a.config, "--rounds",
           str(a.rounds)] + list(extra)
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[n_pix])
    except subprocess.TimeoutExpired:
        sys.stderr.write("(%d pixels) did not finish within its limit of %d s: no result\n" % (n_pix, LIMIT_S[n_pix]))
        return None                      # the child is killed; nothing more is started on the device
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("SYSREM_BENCH ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        return None                      # a failed child ends the session
    return json.loads(line[-1][len("SYSREM_BENCH "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sysrem_latency.txt"))
    ap.add_argument("--child", type=int, default=None)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "tools"))
    if a.child is not None:
        child(a.child, a.config, a.rounds, a.kernel_only)
        return 0
    if a.kernel_only:
        for n in SIZES:
            x = run_child(n, a, ["--kernel-only"])
            if x is None:
                return 1
            print("%s %d pixels: (SYSREM loop, injection, k_highpass) ms, means of 3: %s" % (
                x["lib"] or "the package's library", n,
                "  ".join("%.4f %.4f %.4f" % tuple(k) for k in x["kernel_ms"])), flush=True)
        return 0
    a.rounds = max(4, a.rounds)
    runs = {}
    for n in SIZES:
        runs[n] = run_child(n, a)
        if runs[n] is None:
            return 1
    x0 = runs[SIZES[0]]
    lines = ["Latency of one injection with its cleaning, %s with the inputs resident and R in device memory" % a.config,
             "(tools/sysrem_bench.py): pixels of 0.01 A at R = 140,000, %d exposures over the %d phases (%d taps), trial %d "
             "of 1,024 at scale 1," % (x0["n_exp"], x0["n_orb"], x0["n_tap"], TRIAL),
             "a Gaussian high-pass of sigma = %g pixels cut at h = %d over one order, dividing; SYSREM with %d components "
             "of %d iterations; %d wavelengths." % (SIGMA_PIX, x0["half_width"], N_COMP, N_ITER, x0["n_wav"]),
             "Per round the median of the evaluations by the host clock; one process per pixel count, in it the ways "
             "alternated a b ... for %d rounds;" % a.rounds,
             "everything resident is set before the clock.",
             "  (a)  transit_expose of the one-trial table with the model brought back, then the numpy injection, "
             "observation.high_pass and observation.sysrem",
             "  (b)  transit_inject with the high-pass: U and the cleaned data come back", ""]
    for n in SIZES:
        x = runs[n]
        med, spread = {}, {}
        lines.append("%d pixels:" % n)
        for w in WAYS:
            v = x["ms"][w]
            med[w], spread[w] = statistics.median(v), max(v) - min(v)
            lines.append("  (%s, %2d evaluations a round) ms per round: %s   median %.3f   spread (max - min) %.3f"
                         % (w, EVALS[n][w], " ".join("%.3f" % t for t in v), med[w], spread[w]))
        gain, sg = med["a"] - med["b"], max(spread["a"], spread["b"])
        km = [statistics.median([k[i] for k in x["kernel_ms"]]) for i in range(3)]
        entries = x["n_exp"] * n
        passes = 2 * (N_ITER + 1) * N_COMP
        need = passes * 16 * entries + N_COMP * 8 * entries      # every walk reads r and w; the subtraction writes r
        lines += ["  (a) - (b) = %.3f ms against a spread of %.3f ms, (a) / (b) = %.1f: (b) is %s" % (
                      gain, sg, med["a"] / med["b"], "faster than (a) by more than the spread" if gain > sg else
                      "NOT faster than (a) by more than the spread"),
                  "  cleaned data of (a) and (b) differ by at most %.3g, |U| by at most %.3g (two float64 summation "
                  "orders)" % (x["max_abs_diff_cleaned"], x["max_abs_diff_U"]),
                  "  by device events, means of 3, the median of one per round: the SYSREM loop %.4f ms, the injection "
                  "%.4f ms, k_highpass %.4f ms" % tuple(km),
                  "    the loop's %d walks over [n_exp][n_pix] need %.1f MB (r and w read per walk, r written once per "
                  "component): %.3f TB/s if that were the traffic" % (passes, need / 1e6, need / (km[0] * 1e-3) / 1e12),
                  "    (a derived count, not an HBM figure: no counter was read; %d launches, so at 2,000 pixels the "
                  "loop's time is the launches')" % (N_COMP * (2 * N_ITER + 2) + 2), ""]
    lines += ["Not measured: hardware counters (no rocprofv3 --pmc run), so neither the traffic that reaches HBM nor how "
              "much of a step's second walk the caches serve;",
              "other numbers of pixels a lane owns than the build's (PROM_SY_VEC); several orders; n_comp and n_iter "
              "other than %d and %d." % (N_COMP, N_ITER)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
