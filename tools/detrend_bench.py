#!/usr/bin/env python3
"""Latency of one likelihood evaluation against detrended exposures with and without the filter on the device (GPU
box), on C3 with the inputs resident (one transit_run, then R, the pixels, the exposure table and the filter stay in
device memory): 2,000 pixels of 0.01 A about Na D at R = 140,000, 48 exposures over the 16 phases, three sub-samples
each (6 taps), a basis of 6 components, for one trial and for 1,024 trials (a 32 x 32 (Kp, Vsys) grid):

  (a) what a user has without it: transit_expose with the model brought back ([n_exp][n_trial][n_pix] doubles), then
      the filter m' = m - U (W_p m) and the seven moments in numpy
  (b) transit_expose_detrended, moments only
  (c) transit_expose, moments only: no filter at all, the floor

Each measurement runs in a child process of its own under its own time limit; they are alternated ROUNDS times
(a1 b1 c1 a1024 b1024 c1024 a1 ...), so drifts of the box show as the spread between rounds.  Also reported: the device
durations of k_detrend and k_model_moments (prom_detrend_kernel_ms) and the bytes they move over them.

  python tools/detrend_bench.py [--config C3] [--rounds 4] [--out profiles/detrend_latency.txt]
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
MODES = ("a1", "b1", "c1", "a1024", "b1024", "c1024")
LIMIT_S = {"a1": 120, "b1": 120, "c1": 120, "a1024": 400, "b1024": 240, "c1024": 240}
EVALS = {"a1": 20, "b1": 20, "c1": 20, "a1024": 2, "b1024": 10, "c1024": 10}
N_EXP, N_SUB, N_COMP = 48, 3, 6
HBM_NOMINAL_TBS, HBM_READ_PEAK_TBS = 8.0, 6.04     # the data sheet; profiles/r03_hbm_peak.json (measured read peak)


def tables(tr, n_trial):
    import numpy as np
    from prometheus_amd import observation as obs
    orb = tr.spatialGrid.constructOrbphaseAxis()
    base = obs.planet_frame_shifts(tr.planet, orb)
    span = orb[-1] - orb[0]
    mid = orb[0] + span * (np.arange(N_EXP) + 0.5) / N_EXP
    width = np.full(N_EXP, 0.9 * span / N_EXP)
    if n_trial == 1:
        return obs.exposure_taps(orb, base, mid, width, n_sub=N_SUB)
    return obs.exposure_taps(orb, base, mid, width, n_sub=N_SUB, Kp=1e5 * np.linspace(100.0, 255.0, 32),
                             Vsys=1e5 * (np.arange(32) - 16.0))


def basis():
    """An orthonormal basis of N_COMP smooth trends over the exposures (polynomials in the exposure's number)."""
    import numpy as np
    x = np.linspace(-1.0, 1.0, N_EXP)
    q, _ = np.linalg.qr(np.stack([x ** k for k in range(N_COMP)], axis=1))
    return np.ascontiguousarray(q)


def host_filter(M, U, W):
    import numpy as np
    c = np.einsum("kep,ejp->kjp", W, M, optimize=True)
    return M - np.einsum("ek,kjp->ejp", U, c, optimize=True)


def host_moments(M, data, ivar):
    import numpy as np
    iv, d = ivar[:, None, :], data[:, None, :]
    return np.stack([np.broadcast_to(iv, M.shape).sum(-1), (iv * M).sum(-1), np.broadcast_to(iv * d, M.shape).sum(-1),
                     (iv * M * M).sum(-1), (iv * M * d).sum(-1), np.broadcast_to(iv * d * d, M.shape).sum(-1),
                     (iv * (M - d) ** 2).sum(-1)], axis=-1)


def child(mode, config):
    import numpy as np
    from prometheus_amd import _native, configs, setupfile
    from prometheus_amd import lightcurve as lc
    from prometheus_amd import observation as obs
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
    data = 1e-4 * rng.normal(size=(N_EXP, len(lam)))          # cleaned data scatter about 0
    ivar = np.full(data.shape, 1e6)
    rows, a, F = tables(tr, n_trial)
    U = basis()
    W = obs.filter_weights(U, ivar)
    dev.observe_set(lam, sig, 5.0, n_orb)
    dev.expose_set(rows, a, F, data, ivar)
    dev.detrend_set(U, W)
    model_bytes = 8 * N_EXP * n_trial * len(lam)
    res = {"mode": mode, "n_orb": n_orb, "n_wav": len(wav), "n_pix": len(lam), "n_trial": n_trial, "n_exp": N_EXP,
           "n_tap": rows.shape[1], "n_comp": N_COMP, "model_bytes": model_bytes, "w_bytes": int(W.nbytes)}
    if way == "a":
        def step():
            M = dev.transit_expose(moments=False, model=True)[2]
            return host_moments(host_filter(M, U, W), data, ivar)
    elif way == "b":
        def step():
            return dev.transit_expose_detrended()[0]
    else:
        def step():
            return dev.transit_expose()[0]
    for _ in range(1 if mode == "a1024" else 3):
        last = step()
    t = []
    for _ in range(EVALS[mode]):
        t0 = time.perf_counter()
        last = step()            # ends in a stream synchronise (the copy back)
        t.append((time.perf_counter() - t0) * 1e3)
    res.update(ms_median=statistics.median(t), ms_min=min(t), ms_max=max(t), evals=EVALS[mode],
               chi2_sum=float(np.sum(last[..., 6])))
    if way == "b":
        res["k_detrend_ms"], res["k_model_moments_ms"] = dev.detrend_kernel_ms(10)
    if way == "c":
        res["k_expose_ms"] = dev.expose_kernel_ms(10)
    print("DETREND_BENCH " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "detrend_latency.txt"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.config)
        return 0
    runs = {m: [] for m in MODES}
    for r in range(max(4, a.rounds)):
        for mode in MODES:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--config", a.config]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[mode])
            except subprocess.TimeoutExpired:
                # the child is killed; nothing more is started on the device
                msg = "(%s) did not finish within its limit of %d s in round %d: no result\n" % (mode, LIMIT_S[mode], r)
                sys.stderr.write(msg)
                with open(a.out, "w") as f:
                    f.write(msg)
                return 1
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("DETREND_BENCH ")]
            if p.returncode != 0 or not line:
                # a failed child ends the session: nothing more is started on the device
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                return 1
            runs[mode].append(json.loads(line[-1][len("DETREND_BENCH "):]))
            print("round %d (%s): %.4f ms median" % (r, mode, runs[mode][-1]["ms_median"]), flush=True)
    x0 = runs["b1"][0]
    lines = ["Latency of one likelihood evaluation against detrended exposures, %s with the inputs resident and R in "
             "device memory" % a.config,
             "(tools/detrend_bench.py): %d pixels of 0.01 A about Na D at R = 140,000, %d exposures over the %d phases, "
             "%d sub-samples (%d taps)," % (x0["n_pix"], x0["n_exp"], x0["n_orb"], N_SUB, x0["n_tap"]),
             "a basis of %d components, %d wavelengths; per round the median of the evaluations by the host clock (each "
             "ends in a stream" % (x0["n_comp"], x0["n_wav"]),
             "synchronise), the rounds alternated %s ...; the table and the filter are set once, before the clock"
             % " ".join(MODES),
             "  (a) transit_expose with the model brought back, the filter and the moments in numpy",
             "  (b) transit_expose_detrended, moments only",
             "  (c) transit_expose, moments only: no filter, the floor", ""]
    med, spread = {}, {}
    for mode in MODES:
        v = [x["ms_median"] for x in runs[mode]]
        med[mode], spread[mode] = statistics.median(v), max(v) - min(v)
        lines.append("(%s, %d evaluations a round) ms per round: %s   median %.4f   spread (max - min) %.4f"
                     % (mode, runs[mode][0]["evals"], " ".join("%.4f" % x for x in v), med[mode], spread[mode]))
    for n in ("1", "1024"):
        gain, s = med["a" + n] - med["b" + n], max(spread["a" + n], spread["b" + n])
        cost, sc = med["b" + n] - med["c" + n], max(spread["b" + n], spread["c" + n])
        lines += ["", "%s trial(s): (a) - (b) = %.4f ms against a spread of %.4f ms, (a) / (b) = %.1f: (b) is %s" % (
            n, gain, s, med["a" + n] / med["b" + n], "faster than (a) by more than the spread" if gain > s else
            "NOT faster than (a) by more than the spread"),
            "  the feature's cost (b) - (c) = %.4f ms against a spread of %.4f ms, (b) / (c) = %.2f" % (
                cost, sc, med["b" + n] / med["c" + n]),
            "  (a) brings %.1f MB of model over the bus an evaluation, (b) and (c) 64 bytes per (exposure, trial)"
            % (runs["a" + n][0]["model_bytes"] / 1e6),
            "  sum of chi2 over the table: (a) %.17g  (b) %.17g  (c, unfiltered) %.17g"
            % (runs["a" + n][0]["chi2_sum"], runs["b" + n][0]["chi2_sum"], runs["c" + n][0]["chi2_sum"])]
    for n in ("1", "1024"):
        x = runs["b" + n][0]
        kd = statistics.median(y["k_detrend_ms"] for y in runs["b" + n])
        km = statistics.median(y["k_model_moments_ms"] for y in runs["b" + n])
        ke = statistics.median(y["k_expose_ms"] for y in runs["c" + n])
        bd = 3 * x["model_bytes"] + x["w_bytes"]           # the model read twice and written once, W once
        bm = x["model_bytes"]                              # the model read once more (flags, data and ivar are small)
        tbs = lambda b, ms: b / (ms * 1e-3) / 1e12
        both = tbs(bd + bm, kd + km)
        lines += ["", "%s trial(s), device events, median of the rounds' means of 10:" % n,
                  "  k_detrend        %.4f ms for %.1f MB (the model read twice and written once, W once): %.3f TB/s"
                  % (kd, bd / 1e6, tbs(bd, kd)),
                  "  k_model_moments  %.4f ms for %.1f MB (the model read once more): %.3f TB/s" % (km, bm / 1e6, tbs(bm, km)),
                  "  together %.4f ms for %.1f MB: %.3f TB/s = %.3f of the %.0f TB/s of the data sheet, %.3f of the "
                  "measured read peak of %.2f TB/s" % (kd + km, (bd + bm) / 1e6, both, both / HBM_NOMINAL_TBS,
                                                     HBM_NOMINAL_TBS, both / HBM_READ_PEAK_TBS, HBM_READ_PEAK_TBS),
                  "  (these are the bytes the algorithm needs, not counted traffic: what L2 and the 256 MB cache absorb "
                  "of the second read is not known)",
                  "  k_expose (moments only, the floor's kernel) %.4f ms" % ke]
    lines += ["", "Not measured: hardware counters (no rocprofv3 --pmc run), so neither the traffic that reaches HBM nor "
              "the hit rate of W in L1; a variant of k_detrend that stages W in LDS; n_comp other than %d." % N_COMP]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
