#!/usr/bin/env python3
"""Latency of one likelihood evaluation against exposures with and without the exposures on the device (GPU box), on
C3 with the inputs resident (one transit_run, then R stays in device memory): 2,000 pixels of 0.01 A about Na D at
R = 140,000, 48 exposures over the 16 phases, three sub-samples each (6 taps), for one trial and for 1,024 trials (a
32 x 32 (Kp, Vsys) grid):

  (a) what a user has without them: per distinct (row, factor) column a model spectrum from observe_set +
      transit_observe (num, den; one call serves one factor per row), the taps combined and the moments formed in numpy
  (b) expose_set + transit_expose, moments only

Each measurement runs in a child process of its own under its own time limit; they are alternated ROUNDS times
(a1 b1 a1024 b1024 a1 ...), so drifts of the box show as the spread between rounds.  Also reported: k_expose's device
duration (prom_expose_kernel_ms) per 1,000 support points beside k_vmap's (prom_vmap_kernel_ms) for a map with the
same number of (row, factor) columns, the support points estimated from a sample of the columns.

  python tools/expose_bench.py [--config C3] [--rounds 4] [--out profiles/expose_latency.txt]
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
MODES = ("a1", "b1", "a1024", "b1024")
LIMIT_S = {"a1": 120, "b1": 180, "a1024": 400, "b1024": 400}
EVALS = {"a1": 10, "b1": 20, "a1024": 2, "b1024": 10}
N_EXP, N_SUB = 48, 3


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


def mean_support(wav, lam, sig, k, factors, sample=256):
    """Mean number of grid points in a (pixel, column)'s support over a sample of the columns' factors."""
    import numpy as np
    f = np.unique(factors)
    f = f[:: max(1, len(f) // sample)]
    L, c = lam[None, :] * f[:, None], k * sig[None, :] * f[:, None]
    return float(np.mean(np.searchsorted(wav, L + c, "right") - np.searchsorted(wav, L - c, "left")))


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
    data = 1.0 - 0.01 * rng.random((N_EXP, len(lam)))
    ivar = np.full(data.shape, 1e6)
    rows, a, F = tables(tr, n_trial)
    n_tap = rows.shape[1]
    res = {"mode": mode, "n_orb": n_orb, "n_wav": len(wav), "n_pix": len(lam), "n_trial": n_trial, "n_exp": N_EXP,
           "n_tap": n_tap, "columns": int(F.size)}
    if way == "a":
        # per row the distinct factors its taps need; call c observes factor c of every row's list at once
        rr = np.broadcast_to(rows[:, None, :], F.shape)
        lists = [np.unique(F[rr == r]) for r in range(n_orb)]
        n_calls = max(len(x) for x in lists)
        f_calls = np.ones((n_calls, n_orb))
        for r, x in enumerate(lists):
            f_calls[:len(x), r] = x
        slot = np.empty(F.shape, dtype=np.int64)       # the call that holds a tap's column
        for r, x in enumerate(lists):
            m = rr == r
            slot[m] = np.searchsorted(x, F[m])
        res["observe_calls"] = n_calls
        # the taps a call serves, so that its model spectra are used and dropped (all columns at once would be 4.7 GB)
        e_of, j_of, i_of = (x.ravel() for x in np.indices(F.shape))
        r_of, s_of = rr.ravel(), slot.ravel()
        order = np.argsort(s_of, kind="stable")
        starts = np.searchsorted(s_of[order], np.arange(n_calls + 1))

        def step():
            Me = np.zeros((N_EXP, n_trial, len(lam)))
            for c in range(n_calls):
                dev.observe_set(lam, sig, 5.0, n_orb, f_calls[c])
                num, den, _, _ = dev.transit_observe()
                M = num / den
                sel = order[starts[c]:starts[c + 1]]
                np.add.at(Me, (e_of[sel], j_of[sel]), a[e_of[sel], i_of[sel]][:, None] * M[r_of[sel]])
            return host_moments(Me, data, ivar)
    else:
        dev.observe_set(lam, sig, 5.0, n_orb)

        def step():
            dev.expose_set(rows, a, F, data, ivar)
            return dev.transit_expose()[0]
    for _ in range(1 if way == "a" else 3):
        last = step()
    t = []
    for _ in range(EVALS[mode]):
        t0 = time.perf_counter()
        last = step()            # ends in a stream synchronise (the copy back)
        t.append((time.perf_counter() - t0) * 1e3)
    res.update(ms_median=statistics.median(t), ms_min=min(t), ms_max=max(t), evals=EVALS[mode],
               chi2_sum=float(np.sum(last[..., 6])))
    if way == "b":
        res["k_expose_ms"] = dev.expose_kernel_ms(10)
        res["mean_support"] = mean_support(wav, lam, sig, 5.0, F)
        # a map with as many (row, factor) columns: n_orb rows of columns / n_orb trials, the same factors
        n_cols = F.size // n_orb
        Fm = np.ascontiguousarray(F.reshape(-1)[:n_cols * n_orb].reshape(n_orb, n_cols))
        dev.observe_set(lam, sig, 5.0, n_orb, None, data[:n_orb], ivar[:n_orb])
        dev.vmap_set(Fm)
        dev.transit_vmap()
        res["k_vmap_ms"] = dev.vmap_kernel_ms(10)
        res["vmap_columns"] = int(Fm.size)
        res["vmap_mean_support"] = mean_support(wav, lam, sig, 5.0, Fm)
    print("EXPOSE_BENCH " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "expose_latency.txt"))
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
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("EXPOSE_BENCH ")]
            if p.returncode != 0 or not line:
                # a failed child ends the session: nothing more is started on the device
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                return 1
            runs[mode].append(json.loads(line[-1][len("EXPOSE_BENCH "):]))
            print("round %d (%s): %.4f ms median" % (r, mode, runs[mode][-1]["ms_median"]), flush=True)
    x0 = runs["b1"][0]
    lines = ["Latency of one likelihood evaluation against exposures, %s with the inputs resident and R in device memory"
             % a.config,
             "(tools/expose_bench.py): %d pixels of 0.01 A about Na D at R = 140,000, %d exposures over the %d phases, %d "
             "sub-samples (%d taps)," % (x0["n_pix"], x0["n_exp"], x0["n_orb"], N_SUB, x0["n_tap"]),
             "%d wavelengths; per round the median of the evaluations by the host clock (each ends in a stream "
             "synchronise)," % x0["n_wav"],
             "the rounds alternated %s ..." % " ".join(MODES),
             "  (a) per distinct (row, factor) column observe_set + transit_observe (num, den), one factor per row and "
             "call; taps and moments in numpy",
             "  (b) expose_set + transit_expose, moments only", ""]
    med, spread = {}, {}
    for mode in MODES:
        v = [x["ms_median"] for x in runs[mode]]
        med[mode], spread[mode] = statistics.median(v), max(v) - min(v)
        extra = "   %d observe calls an evaluation" % runs[mode][0]["observe_calls"] if mode[0] == "a" else ""
        lines.append("(%s, %d evaluations a round) ms per round: %s   median %.4f   spread (max - min) %.4f%s"
                     % (mode, runs[mode][0]["evals"], " ".join("%.4f" % x for x in v), med[mode], spread[mode], extra))
    for n in ("1", "1024"):
        gain, s = med["a" + n] - med["b" + n], max(spread["a" + n], spread["b" + n])
        lines += ["", "%s trial(s): (a) - (b) = %.4f ms against a spread of %.4f ms, (a) / (b) = %.1f: (b) is %s" % (
            n, gain, s, med["a" + n] / med["b" + n], "faster than (a) by more than the spread" if gain > s else
            "NOT faster than (a) by more than the spread"),
            "  sum of chi2 over the table: (a) %.17g  (b) %.17g" % (runs["a" + n][0]["chi2_sum"], runs["b" + n][0]["chi2_sum"])]
    for n in ("1", "1024"):
        x = runs["b" + n][0]
        ke = statistics.median(y["k_expose_ms"] for y in runs["b" + n])
        kv = statistics.median(y["k_vmap_ms"] for y in runs["b" + n])
        pe = x["columns"] * x["n_pix"] * x["mean_support"]
        pv = x["vmap_columns"] * x["n_pix"] * x["vmap_mean_support"]
        lines += ["", "%s trial(s), device events, median of the rounds' means of 10:" % n,
                  "  k_expose %.4f ms: %d (row, factor) columns, about %.3g support points (mean support %.1f, from a "
                  "sample of the columns): %.1f ns per 1,000 points" % (ke, x["columns"], pe, x["mean_support"],
                                                                        ke * 1e9 / max(1.0, pe)),
                  "  k_vmap   %.4f ms for a map over the same %d columns (%d phases x %d trials), about %.3g support "
                  "points: %.1f ns per 1,000 points" % (kv, x["vmap_columns"], x["n_orb"],
                                                        x["vmap_columns"] // x["n_orb"], pv, kv * 1e9 / max(1.0, pv))]
    lines += ["", "Not measured: hardware counters (no rocprofv3 --pmc run), a stage trace, the cost of the barriers per "
              "(tile, tap) beside the exp."]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
