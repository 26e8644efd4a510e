#!/usr/bin/env python3
"""Latency of one likelihood evaluation with and without the broadening stage (GPU box), on C3 with the inputs resident:
2,000 pixels of 0.01 A about Na D at R = 140,000, --exposures exposures over the phases (default 16, one per phase)
with --sub sub-samples each (default 1), one trial, and a 33-node ring at 3 km/s (observation.rotation_kernel) as the velocity kernel:

  (a) transit_run + transit_expose, moments only: no broadening
  (b) transit_run + transit_broaden + transit_expose: R_b formed on the device, nothing more crosses the bus
  (c) transit_run + transit_result: the copy of R a host-side broadening cannot avoid (the convolution and the copy
      back are not even counted)

Each measurement runs in a child process of its own under its own time limit; they are alternated ROUNDS times
(a b c a b c ...), so drifts of the box show as the spread between rounds.  Also reported: k_broaden's device duration
(prom_broaden_kernel_ms), the supports' minimum, mean and maximum, and the kernel's bytes floor (R read once, R_b
written once, wav and q) at the HBM rate bench.py's roofline uses.

  python tools/broaden_bench.py [--config C3] [--rounds 4] [--exposures 16] [--sub 1] [--out profiles/broaden_latency.txt]
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
MODES = ("a", "b", "c")
LIMIT_S = 240
EVALS = 20
HBM_PEAK_GBS = 8000.0            # bench.py's HBM_PEAK_GBS
V_EQ, NODES = 3e5, 33


def supports(wav, b0, s, n_k):
    """(min, mean, max) of the supports' sizes, from the real-number ends (a point or two off the float64 rule's)."""
    import numpy as np
    lo = np.searchsorted(wav, wav * (1.0 + b0), "left")
    hi = np.searchsorted(wav, wav * (1.0 + b0 + (n_k - 1) / s), "right")
    n = hi - lo
    return int(n.min()), float(n.mean()), int(n.max())


def child(mode, config, N_EXP, N_SUB):
    import numpy as np
    from prometheus_amd import _native, configs, setupfile
    from prometheus_amd import lightcurve as lc
    from prometheus_amd import observation as obs
    tr = setupfile.build_transit(configs.get(config))
    dev = _native.get_device(0)
    host = tr._host_inputs()
    wav = np.asarray(tr.wavelength)
    dev.transit_set(tr._problem(dev, host, 0, len(wav), 0.0))
    dev.transit_run()
    orb = tr.spatialGrid.constructOrbphaseAxis()
    n_orb = len(orb)
    res = {"mode": mode, "n_orb": n_orb, "n_wav": len(wav), "evals": EVALS}
    bk = obs.Broadening(*obs.rotation_kernel(V_EQ, n=NODES))
    if mode == "c":
        out = _native.host_array((n_orb, len(wav)))
        out = np.empty((n_orb, len(wav))) if out is None else out

        def step():
            dev.transit_run()
            dev.transit_result(out=out)
            return float(out[0, 0])
    else:
        lam = 0.5 * (lc.NA_D2 + lc.NA_D1) + 1e-10 * (np.arange(2000) - 1000)
        sig = lam / (140000.0 * 2.3548200450309493)
        rng = np.random.default_rng(0)
        data = 1.0 - 0.01 * rng.random((N_EXP, len(lam)))
        ivar = np.full(data.shape, 1e6)
        base = obs.planet_frame_shifts(tr.planet, orb)
        span = orb[-1] - orb[0]
        mid = orb[0] + span * (np.arange(N_EXP) + 0.5) / N_EXP
        rows, a, F = obs.exposure_taps(orb, base, mid, np.full(N_EXP, 0.9 * span / N_EXP), n_sub=N_SUB)
        dev.observe_set(lam, sig, 5.0, n_orb)
        dev.expose_set(rows, a, F, data, ivar)
        dev.broaden_set(bk.K, bk.b0, bk.s)
        res.update(n_pix=len(lam), n_exp=N_EXP, n_tap=int(rows.shape[1]))

        def step():
            dev.transit_run()
            if mode == "b":
                dev.transit_broaden()
            return float(dev.transit_expose()[0][..., 6].sum())
    for _ in range(3):
        last = step()
    t = []
    for _ in range(EVALS):
        t0 = time.perf_counter()
        last = step()            # ends in a stream synchronise (the copy back)
        t.append((time.perf_counter() - t0) * 1e3)
    res.update(ms_median=statistics.median(t), ms_min=min(t), ms_max=max(t), value=last)
    if mode == "b":
        res["k_broaden_ms"] = dev.broaden_kernel_ms(20)
        res["support"] = supports(wav, bk.b0, bk.s, NODES)
        res["floor_bytes"] = 8 * (2 * n_orb * len(wav) + 2 * len(wav))
    print("BROADEN_BENCH " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "broaden_latency.txt"))
    ap.add_argument("--exposures", type=int, default=16, help="exposures of the table (default: one per phase of C3)")
    ap.add_argument("--sub", type=int, default=1, help="sub-samples per exposure (2 taps each)")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.config, a.exposures, a.sub)
        return 0
    runs = {m: [] for m in MODES}
    for r in range(max(3, a.rounds)):
        for mode in MODES:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--config", a.config, "--exposures",
                   str(a.exposures), "--sub", str(a.sub)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S)
            except subprocess.TimeoutExpired:
                # the child is killed; nothing more is started on the device
                msg = "(%s) did not finish within its limit of %d s in round %d: no result\n" % (mode, LIMIT_S, r)
                sys.stderr.write(msg)
                return 1
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("BROADEN_BENCH ")]
            if p.returncode != 0 or not line:
                # a failed child ends the session: nothing more is started on the device
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                return 1
            runs[mode].append(json.loads(line[-1][len("BROADEN_BENCH "):]))
            print("round %d (%s): %.4f ms median" % (r, mode, runs[mode][-1]["ms_median"]), flush=True)
    xb = runs["b"][0]
    lines = ["Latency of one likelihood evaluation with the broadening stage, %s with the inputs resident "
             "(tools/broaden_bench.py):" % a.config,
             "%d phases x %d wavelengths, %d pixels of 0.01 A about Na D at R = 140,000, %d exposures of %d taps, one "
             "trial;" % (xb["n_orb"], xb["n_wav"], xb["n_pix"], xb["n_exp"], xb["n_tap"]),
             "the kernel is a %d-node ring at %.0f km/s (observation.rotation_kernel).  Per round the median of %d "
             "evaluations by the" % (NODES, V_EQ / 1e5, EVALS),
             "host clock (each ends in a stream synchronise), the rounds alternated a b c a b c ...",
             "  (a) transit_run + transit_expose (moments only)",
             "  (b) transit_run + transit_broaden + transit_expose",
             "  (c) transit_run + transit_result (R into page-locked memory): the copy a host-side broadening needs first",
             ""]
    med, spread = {}, {}
    for mode in MODES:
        v = [x["ms_median"] for x in runs[mode]]
        med[mode], spread[mode] = statistics.median(v), max(v) - min(v)
        lines.append("(%s) ms per round: %s   median %.4f   spread (max - min) %.4f"
                     % (mode, " ".join("%.4f" % x for x in v), med[mode], spread[mode]))
    worst_b, best_c = max(x["ms_median"] for x in runs["b"]), min(x["ms_median"] for x in runs["c"])
    lines += ["", "(b) - (a) = %.4f ms: what the stage adds to an evaluation" % (med["b"] - med["a"]),
              "(c) - (b) = %.4f ms (medians); the slowest round of (b) %.4f ms against the fastest of (c) %.4f ms: (b) %s"
              % (med["c"] - med["b"], worst_b, best_c,
                 "beats (c) in every round" if worst_b < best_c else
                 ("beats (c) by the medians, not in every round" if med["b"] < med["c"] else "does NOT beat (c)")),
              "  sum of chi2: (a) %.17g  (b) %.17g" % (runs["a"][0]["value"], runs["b"][0]["value"])]
    kb = statistics.median(x["k_broaden_ms"] for x in runs["b"])
    floor_ms = xb["floor_bytes"] / (HBM_PEAK_GBS * 1e9) * 1e3
    lines += ["", "k_broaden alone, device events, median of the rounds' means of 20: %.4f ms" % kb,
              "  supports (real-number ends): min %d, mean %.1f, max %d grid points" % tuple(xb["support"]),
              "  bytes floor: R read once, R_b written once, wav and q: %.2f MB at %.0f GB/s = %.4f ms; k_broaden takes "
              "%.1f x its floor" % (xb["floor_bytes"] / 1e6, HBM_PEAK_GBS, floor_ms, kb / floor_ms),
              "", "Not measured: hardware counters (no rocprofv3 --pmc run)."]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
