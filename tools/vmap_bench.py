#!/usr/bin/env python3
"""Latency of one velocity map with and without the map on the device (GPU box), on C3 with the inputs resident
(one transit_run, then R stays in device memory): 2,000 pixels of 0.01 A about Na D at R = 140,000, 16 phases, for
64 trials (1 km/s apart about the planet's frame) and 1,024 trials (a 32 x 32 (Kp, Vsys) grid):

  (a) the per-trial way: per trial one observe_set with that column as f plus transit_observe returning chi-square only
  (b) vmap_set once plus transit_vmap: seven moments and a count per (phase, trial)

Each measurement runs in a child process of its own under its own time limit; they are alternated ROUNDS times
(a64 b64 a1024 b1024 a64 ...), so drifts of the box show as the spread between rounds.  Also reported: k_vmap's device
duration (prom_vmap_kernel_ms) and the bytes it requests, counted by the host harness of its tile plan
(tests/helpers/vmap_host.cpp), against the algorithmic bytes.

  python tools/vmap_bench.py [--config C3] [--rounds 4] [--out profiles/vmap_latency.txt]
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
MODES = ("a64", "b64", "a1024", "b1024")
LIMIT_S = {"a64": 120, "b64": 180, "a1024": 240, "b1024": 400}
EVALS = {"a64": 10, "b64": 20, "a1024": 3, "b1024": 10}


def table(tr, n_orb, n_trial):
    import numpy as np
    from prometheus_amd import observation as obs
    orb = tr.spatialGrid.constructOrbphaseAxis()
    if n_trial == 64:
        return obs.trial_factors(obs.planet_frame_shifts(tr.planet, orb), 1e5 * (np.arange(64) - 32.0))
    return obs.kp_vsys_factors(orb, 1e5 * np.linspace(100.0, 255.0, 32), 1e5 * (np.arange(32) - 16.0))


def plan_bytes(wav, lam, sig, k, F):
    """Bytes k_vmap requests, from the walk of its launch by the host harness of vmap_index.h (the kernel's own index
    functions): per workgroup and tile the staged range (wav, q and one row of R), per support outside the stage its
    points read from global memory; plus data and ivar per (pixel, trial), the records and the outputs."""
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from helpers import vmap_plan as plan
    with tempfile.TemporaryDirectory() as d:
        lib = os.path.join(d, "libvmap_host.so")
        plan.compile_harness(lib)
        L = plan.bind(lib)
        cnt, _ = plan.audit(L, wav, lam, sig, k, F, supports=False)
        c = plan.constants(L)
    for key in plan.ERRORS:
        assert cnt[key] == 0, cnt
    n_orb, n_trial = F.shape
    n_chunks = -(-(-(-len(lam) // c["tile"])) // c["chunk"])
    records = 2 * n_orb * n_trial * n_chunks * 64                 # written by k_vmap, read by k_vmap_reduce
    out = n_orb * n_trial * 64
    pixel = (cnt["staged"] + cnt["fallback"] + cnt["empty"]) * (2 * 8 + 2 * 8)   # lam, sig, data, ivar per (pixel, trial)
    algorithmic = (n_orb + 2) * len(wav) * 8 + 2 * len(lam) * 8 + 2 * n_orb * len(lam) * 8 + F.size * 8 + out
    return {"staged_bytes": 8 * cnt["stage_values"], "fallback_bytes": 8 * cnt["fallback_values"],
            "fallback_supports": cnt["fallback"], "pixel_bytes": pixel, "record_bytes": records, "output_bytes": out,
            "algorithmic_bytes": algorithmic, "support_points": cnt["points"], "workgroups": cnt["workgroups"],
            "bracket_searches": cnt["bracket_searches"], "full_searches": cnt["full_searches"],
            "bracket_width_mean": cnt["bracket_width"] / max(1, cnt["bracket_searches"])}


def child(mode, config, with_plan):
    import numpy as np
    from prometheus_amd import _native, configs, setupfile
    from prometheus_amd import lightcurve as lc
    way, n_trial = mode[0], int(mode[1:])
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
    data = 1.0 - 0.01 * rng.random((n_orb, len(lam)))
    ivar = np.full(data.shape, 1e6)
    F = table(tr, n_orb, n_trial)
    res = {"mode": mode, "n_orb": n_orb, "n_wav": len(wav), "n_pix": len(lam), "n_trial": n_trial}
    if way == "a":
        def step():
            c2 = np.empty((n_orb, n_trial))
            for j in range(n_trial):
                dev.observe_set(lam, sig, 5.0, n_orb, F[:, j], data, ivar)
                c2[:, j] = dev.transit_observe(partials=False, chi2=True)[2]
            return c2
    else:
        dev.observe_set(lam, sig, 5.0, n_orb, None, data, ivar)

        def step():
            dev.vmap_set(F)
            return dev.transit_vmap()[0][..., 6]
    for _ in range(1 if way == "a" else 3):
        last = step()
    t = []
    for _ in range(EVALS[mode]):
        t0 = time.perf_counter()
        last = step()            # ends in a stream synchronise (the copy back)
        t.append((time.perf_counter() - t0) * 1e3)
    res.update(ms_median=statistics.median(t), ms_min=min(t), ms_max=max(t), evals=EVALS[mode],
               chi2_sum=float(np.sum(last)))
    if way == "b":
        res["k_vmap_ms"] = dev.vmap_kernel_ms(10)
        if with_plan:
            res.update(plan_bytes(wav, lam, sig, 5.0, F))
    print("VMAP_BENCH " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vmap_latency.txt"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--plan", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.config, a.plan)
        return 0
    runs = {m: [] for m in MODES}
    for r in range(max(4, a.rounds)):
        for mode in MODES:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--config", a.config]
            if r == 0 and mode[0] == "b":
                cmd.append("--plan")
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[mode])
            except subprocess.TimeoutExpired:
                # the child is killed; nothing more is started on the device
                msg = "(%s) did not finish within its limit of %d s in round %d: no result\n" % (mode, LIMIT_S[mode], r)
                sys.stderr.write(msg)
                with open(a.out, "w") as f:
                    f.write(msg)
                return 1
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("VMAP_BENCH ")]
            if p.returncode != 0 or not line:
                # a failed child ends the session: nothing more is started on the device
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                return 1
            runs[mode].append(json.loads(line[-1][len("VMAP_BENCH "):]))
            print("round %d (%s): %.4f ms median" % (r, mode, runs[mode][-1]["ms_median"]), flush=True)
    x0 = runs["b64"][0]
    lines = ["Latency of one velocity map, %s with the inputs resident and R in device memory (tools/vmap_bench.py):"
             % a.config,
             "%d pixels of 0.01 A about Na D at R = 140,000, %d phases, %d wavelengths; per round the median of the"
             % (x0["n_pix"], x0["n_orb"], x0["n_wav"]),
             "evaluations by the host clock (each ends in a stream synchronise), the rounds alternated %s ..."
             % " ".join(MODES),
             "  (a) per trial: observe_set with the column as f + transit_observe, chi-square only",
             "  (b) vmap_set + transit_vmap: seven moments and a count per (phase, trial)", ""]
    med, spread = {}, {}
    for mode in MODES:
        v = [x["ms_median"] for x in runs[mode]]
        med[mode], spread[mode] = statistics.median(v), max(v) - min(v)
        lines.append("(%s, %d evaluations a round) ms per round: %s   median %.4f   spread (max - min) %.4f"
                     % (mode, runs[mode][0]["evals"], " ".join("%.4f" % x for x in v), med[mode], spread[mode]))
    for n in ("64", "1024"):
        gain, s = med["a" + n] - med["b" + n], max(spread["a" + n], spread["b" + n])
        lines += ["", "%s trials: (a) - (b) = %.4f ms against a spread of %.4f ms, (a) / (b) = %.1f: (b) is %s" % (
            n, gain, s, med["a" + n] / med["b" + n], "faster than (a) by more than the spread" if gain > s else
            "NOT faster than (a) by more than the spread"),
            "  sum of chi2 over the map: (a) %.17g  (b) %.17g" % (runs["a" + n][0]["chi2_sum"], runs["b" + n][0]["chi2_sum"])]
    for n in ("64", "1024"):
        x = runs["b" + n][0]
        km = statistics.median(y["k_vmap_ms"] for y in runs["b" + n])
        req = x["staged_bytes"] + x["fallback_bytes"] + x["pixel_bytes"] + x["record_bytes"] + x["output_bytes"]
        lines += ["", "k_vmap (%s trials): %.4f ms (device events, median of the rounds' means of 10); %d workgroups, %d "
                  "support points, %.1f ns per 1,000 points" % (n, km, x["workgroups"], x["support_points"],
                                                              km * 1e9 / max(1, x["support_points"])),
                  "  searches inside a bracket %d (mean width %.0f points), over the whole grid %d"
                  % (x["bracket_searches"], x["bracket_width_mean"], x["full_searches"]),
                  "  bytes requested by its tile plan (counted on the host, not a hardware counter): staged %.2f MB, "
                  "global-read supports %.2f MB (%d supports), pixel tables %.2f MB, records %.2f MB, outputs %.2f MB: "
                  "%.2f MB" % (x["staged_bytes"] / 1e6, x["fallback_bytes"] / 1e6, x["fallback_supports"],
                               x["pixel_bytes"] / 1e6, x["record_bytes"] / 1e6, x["output_bytes"] / 1e6, req / 1e6),
                  "  algorithmic bytes (R, wav and q once, pixels, data, table, outputs): %.2f MB; requested / "
                  "algorithmic %.2f" % (x["algorithmic_bytes"] / 1e6, req / x["algorithmic_bytes"])]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
