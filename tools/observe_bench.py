#!/usr/bin/env python3
"""Latency of one likelihood evaluation with and without the observation on the device (GPU box), on C3 with the
inputs resident:

  (a) transit_run + transit_result into pinned memory: what a retrieval had to do before (R crosses the bus)
  (b) transit_run + transit_observe returning chi-square only: 2,000 pixels of 0.01 A about Na D at R = 140,000
  (c) transit_run + transit_observe returning num and den (M = num / den): ~320,000 pixels of 0.01 A over the range

Each measurement runs in a child process of its own under its own time limit; the three are alternated ROUNDS times
(a b c a b c ...), so drifts of the box show as the spread between rounds.  Also reported: k_observe's device
duration (prom_observe_kernel_ms) and the bytes it requests, counted by the host harness of its tile plan, against
the algorithmic bytes (R, wav and q once, the outputs).

  python tools/observe_bench.py [--config C3] [--rounds 4] [--evals 40] [--out profiles/observe_latency.txt]
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
LIMIT_S = {"a": 120, "b": 120, "c": 180}


def pixels(mode, wav):
    import numpy as np
    from prometheus_amd import lightcurve as lc
    if mode == "b":
        return 0.5 * (lc.NA_D2 + lc.NA_D1) + 1e-10 * (np.arange(2000) - 1000)
    return np.arange(wav[0], wav[-1], 1e-10)


def plan_bytes(wav, lam, sig, k, n_orb):
    """Bytes k_observe requests for a shared frame, from the walk of its launch by the host harness of obs_index.h
    (tests/helpers/observe_host.cpp: the kernel's own index functions): per workgroup the staged range (wav, q and
    the group's rows of R), per fallback pixel its support read from global memory."""
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from helpers import observe_plan as plan
    with tempfile.TemporaryDirectory() as d:
        lib = os.path.join(d, "libobserve_host.so")
        plan.compile_harness(lib)
        cnt, _ = plan.audit(plan.bind(lib), wav, lam, sig, k, None, n_orb, supports=False)
    for key in ("staged_oor", "global_oor", "stage_load_oor", "out_oor"):
        assert cnt[key] == 0, cnt
    out = 2 * n_orb * len(lam) * 8
    algorithmic = (n_orb + 2) * len(wav) * 8 + 2 * len(lam) * 8 + out
    return {"staged_bytes": 8 * cnt["stage_values"], "fallback_bytes": 8 * cnt["fallback_values"],
            "fallback_pixels": cnt["fallback_pix"], "output_bytes": out, "algorithmic_bytes": algorithmic,
            "support_points": cnt["points"]}


def child(mode, config, evals):
    import numpy as np
    from prometheus_amd import _native, configs, setupfile
    tr = setupfile.build_transit(configs.get(config))
    dev = _native.get_device(0)
    host = tr._host_inputs()
    wav = np.asarray(tr.wavelength)
    dev.transit_set(tr._problem(dev, host, 0, len(wav), 0.0))
    n_orb = len(host["orb"])
    res = {"mode": mode, "n_orb": n_orb, "n_wav": len(wav)}
    if mode == "a":
        out = _native.host_array((n_orb, len(wav)))
        assert out is not None, "no pinned memory"

        def step():
            dev.transit_run()
            dev.transit_result(out=out)
    else:
        lam = pixels(mode, wav)
        sig = lam / (140000.0 * 2.3548200450309493)
        rng = np.random.default_rng(0)
        data = 1.0 - 0.01 * rng.random((n_orb, len(lam)))
        dev.observe_set(lam, sig, 5.0, n_orb, None, data, np.full(data.shape, 1e6))
        res.update(n_pix=len(lam), **plan_bytes(wav, lam, sig, 5.0, n_orb))
        if mode == "b":
            def step():
                dev.transit_run()
                dev.transit_observe(partials=False, chi2=True)
        else:
            def step():
                dev.transit_run()
                dev.transit_observe(partials=True, chi2=False)
    for _ in range(5):
        step()
    t = []
    for _ in range(evals):
        t0 = time.perf_counter()
        step()            # ends in a stream synchronise (the copy back)
        t.append((time.perf_counter() - t0) * 1e3)
    res.update(ms_median=statistics.median(t), ms_mean=statistics.fmean(t), ms_min=min(t), ms_max=max(t), evals=evals)
    if mode != "a":
        res["k_observe_ms"] = dev.observe_kernel_ms(20)
    print("OBSERVE_BENCH " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--evals", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "observe_latency.txt"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.config, a.evals)
        return 0
    runs = {"a": [], "b": [], "c": []}
    for r in range(max(4, a.rounds)):
        for mode in "abc":
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--config", a.config,
                                    "--evals", str(a.evals)], capture_output=True, text=True, timeout=LIMIT_S[mode])
            except subprocess.TimeoutExpired:
                # the child is killed; nothing more is started on the device
                msg = "(%s) did not finish within its limit of %d s in round %d: no result\n" % (mode, LIMIT_S[mode], r)
                sys.stderr.write(msg)
                with open(a.out, "w") as f:
                    f.write(msg)
                return 1
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("OBSERVE_BENCH ")]
            if p.returncode != 0 or not line:
                # a failed child ends the session: nothing more is started on the device
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                return 1
            runs[mode].append(json.loads(line[-1][len("OBSERVE_BENCH "):]))
            print("round %d (%s): %.4f ms median" % (r, mode, runs[mode][-1]["ms_median"]), flush=True)
    lines = ["Latency of one evaluation, %s with the inputs resident (tools/observe_bench.py): per round the median of %d"
             % (a.config, a.evals),
             "evaluations by the host clock (each ends in a stream synchronise), the rounds alternated a b c a b c ...",
             "  (a) transit_run + transit_result into pinned memory (R: %d x %d doubles, %.1f MB)"
             % (runs["a"][0]["n_orb"], runs["a"][0]["n_wav"], runs["a"][0]["n_orb"] * runs["a"][0]["n_wav"] * 8e-6),
             "  (b) transit_run + transit_observe, chi-square only, %d pixels about Na D" % runs["b"][0]["n_pix"],
             "  (c) transit_run + transit_observe, num and den, %d pixels over the range" % runs["c"][0]["n_pix"], ""]
    med = {}
    for mode in "abc":
        v = [x["ms_median"] for x in runs[mode]]
        med[mode] = statistics.median(v)
        lines.append("(%s) ms per round: %s   median %.4f   spread (max - min) %.4f"
                     % (mode, " ".join("%.4f" % x for x in v), med[mode], max(v) - min(v)))
    spread = max(max(x["ms_median"] for x in runs[m]) - min(x["ms_median"] for x in runs[m]) for m in "ab")
    gain = med["a"] - med["b"]
    lines += ["", "(a) - (b) = %.4f ms against a spread of %.4f ms: (b) is %s" % (
        gain, spread, "faster than (a) by more than the spread" if gain > spread else
        "NOT faster than (a) by more than the spread")]
    for mode in "bc":
        x = runs[mode][0]
        km = statistics.median(y["k_observe_ms"] for y in runs[mode])
        req = x["staged_bytes"] + x["fallback_bytes"] + x["output_bytes"]
        lines += ["", "k_observe (%s): %.4f ms (device events, median of the rounds' means of 20); %d support points "
                  "over the phase groups"
                  % (mode, km, x["support_points"]),
                  "  bytes requested by its tile plan (counted on the host, not a hardware counter): staged %.2f MB, "
                  "fallback %.2f MB (%d pixels), outputs %.2f MB: %.2f MB" % (
                      x["staged_bytes"] / 1e6, x["fallback_bytes"] / 1e6, x["fallback_pixels"], x["output_bytes"] / 1e6,
                      req / 1e6),
                  "  algorithmic bytes (R, wav and q once, pixels, outputs): %.2f MB; requested / algorithmic %.2f"
                  % (x["algorithmic_bytes"] / 1e6, req / x["algorithmic_bytes"])]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
