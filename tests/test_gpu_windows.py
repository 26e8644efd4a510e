"""Target windows (k_sigma_tw, prometheus_amd/csrc/prom_tw.hip + prom_window.hip): the Doppler-shifted
cross-section lookups of the transmission-curve path grouped by target value instead of by wavelength block.

Every lookup evaluates fl(chi E_k) e^a of numpy's bracket k (gasProperties.py:941-954 via n_interp_log,
:34-51), whatever window, slice kind or pass it falls in, so R must be BITWISE the wavelength-block kernel's
(k_sigma_tc, PROM_TW=0) -- on the golden configs, at full size (C3, C4, C4x10), for wavelength shards and with
the host's window caps forced small (many windows, slices on the global-record and searched paths).  The windows
are the default (PROM_TW=0 switches them off); the tests set PROM_TW=1 explicitly.

Every test also asserts that k_sigma_tw took the PROM_TW=1 run (tau_kernel_variant // 10 == 9) and did not take the
PROM_TW=0 run: the debug line alone is printed whenever windows are built, whichever kernel then runs.  The
figures of that line (windows, slices by kind, windows with staged wavelengths) are compared with the plan the host
harness of the planner (tests/helpers/window_plan.py, tests/test_window_plan_cpu.py) makes from the oracle's grid,
table nodes and Doppler factors under the same caps, which also pins those inputs of the product to the
oracle's; each caps case asserts the slice kinds or staging it is there to reach.

Small shapes against the float64 oracle: fine low-end grids of C4 and C3 at 2 .. 8 phases, where the waves per row
or pair change (2-3 rows or pairs: two waves each; from 4: one), an odd row count leaves the last row without a
partner and the Doppler spread is many 64-wavelength chunks wide, so rows without wavelengths in a window sit
beside rows with some (the host audit of tests/test_window_plan_cpu.py checks every index of these plans).

Slices of kind 0 (targets outside the table) cannot be reached through a setup file: the tables span +-1 % of the
grid against a Doppler shift of 1e-4.  Kind 0 is covered on the planner's side only (the synthetic case of
tests/test_window_plan_cpu.py).
"""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R_TOL = 1e-10   # the project's parity tolerance against the oracle (tests/test_gpu_tcurve.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LINE = re.compile(r"target windows: (\d+) \(slices: (\d+) staged, (\d+) global, (\d+) staged unguessed, "
                   r"(\d+) outside the table; wavelengths staged in (\d+) windows")


def _transit(name, reduced=False):
    from prometheus_amd import configs, setupfile
    cfg = configs.get(name)
    if reduced:
        cfg = configs.reduced(cfg)
    return setupfile.build_transit(cfg)


def _windows_line(capfd):
    err = capfd.readouterr().err
    lines = [l for l in err.splitlines() if "target windows" in l]
    return lines[-1] if lines else None


def _counts(line):
    """(windows, slices staged, global, staged unguessed, outside the table, windows with staged wavelengths): the
    order of helpers.window_plan.debug_counts."""
    m = _LINE.search(line)
    assert m, line
    return tuple(int(v) for v in m.groups())


def _variants(tr):
    return [st["tau_kernel_variant"] // 10 for st in tr.last_stats]


def _run_on_off(tr, monkeypatch):
    """R over target windows and R of the wavelength-block kernel, each with the kernel that took the run asserted."""
    tr.collect_stats = True
    monkeypatch.setenv("PROM_TW", "1")   # (the default)
    R = tr.sumOverChords(devices=[0])
    assert _variants(tr) == [9], tr.last_stats
    monkeypatch.setenv("PROM_TW", "0")
    R0 = tr.sumOverChords(devices=[0])
    assert _variants(tr) and 9 not in _variants(tr), tr.last_stats
    return R, R0


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    from helpers.window_plan import Libs
    return Libs(tmp_path_factory.mktemp("tw"))


def _host_counts(libs, name, n, caps):
    from helpers import window_plan as WP
    return WP.debug_counts(WP.make_plan(libs, WP.inputs(name, n), caps))


@pytest.mark.parametrize("name", ["C3", "C4", "exomoon"])
def test_windows_bitwise_reduced(name, monkeypatch, capfd, libs):
    monkeypatch.setenv("PROM_DEBUG", "1")
    tr = _transit(name, reduced=True)
    R, R0 = _run_on_off(tr, monkeypatch)
    line = _windows_line(capfd)
    assert line is not None, "the target-window path did not build windows"
    print(name, line)
    assert np.array_equal(R, R0)
    if name == "C3":
        # the planner's inputs and plan are the host harness': default caps, searched slices among them
        from helpers.window_plan import Caps
        assert _counts(line) == _host_counts(libs, "C3r", None, Caps(R.shape[0]))
        assert _counts(line)[3] > 0


@pytest.mark.parametrize("name", ["C3", "C4", "C4x10"])
def test_windows_bitwise_full_size(name, monkeypatch, capfd):
    monkeypatch.setenv("PROM_DEBUG", "1")
    tr = _transit(name)
    R, R0 = _run_on_off(tr, monkeypatch)
    line = _windows_line(capfd)
    assert line is not None
    print(name, R.shape, line)
    assert np.array_equal(R, R0)


def test_windows_shards_bitwise(monkeypatch):
    """Wavelength shards build their own windows; R is bitwise the one-shard R."""
    monkeypatch.setenv("PROM_TW", "1")
    tr = _transit("C4x10")
    tr.collect_stats = True
    R1 = tr.sumOverChords(devices=[0])
    assert _variants(tr) == [9], tr.last_stats
    R3 = tr.sumOverChords(devices=[0, 0, 0])
    assert _variants(tr) == [9, 9, 9], tr.last_stats
    assert np.array_equal(R1, R3)
    monkeypatch.setenv("PROM_TW", "0")
    tr.sumOverChords(devices=[0])
    assert _variants(tr) and 9 not in _variants(tr), tr.last_stats


# one transit with target windows and without, in a process of its own (the knobs are read once per process): a JSON
# line with the bitwise comparison and the kernel variants of both runs
_ON_OFF = (
    "import numpy as np, json, os\n"
    "from prometheus_amd import configs, setupfile\n"
    "tr = setupfile.build_transit(%s)\n"
    "tr.collect_stats = True\n"
    "R = tr.sumOverChords(devices=[0])\n"
    "v1 = [s['tau_kernel_variant'] for s in tr.last_stats]\n"
    "os.environ['PROM_TW'] = '0'\n"
    "R0 = tr.sumOverChords(devices=[0])\n"
    "v0 = [s['tau_kernel_variant'] for s in tr.last_stats]\n"
    "print(json.dumps({'eq': bool(np.array_equal(R, R0)), 'shape': list(R.shape), 'v1': v1, 'v0': v0}))\n")


def _assert_variants(out):
    assert out["v1"] and all(v // 10 == 9 for v in out["v1"]), out
    assert out["v0"] and all(v // 10 != 9 for v in out["v0"]), out


@pytest.mark.parametrize("caps", [("8", "64", "2560"), ("4", "32", "96"), ("256", "8192", "16"),
                                  ("256", "8192", "2560", "0"), ("256", "8192", "2560", "1024", "1"),
                                  ("256", "8192", "2560", "0", "0", "0"),
                                  ("256", "8192", "2560", "1024", "0", "1", "0", "2"),
                                  ("100", "8192", "2560", "0", "0", "1", "64", "2")])
def test_windows_small_caps_bitwise(caps, libs):
    """Window caps (wavelengths per row, points per window, LDS doubles[, staged wavelengths, windows grown only while
    their wavelengths fit, exact-guess marks, lane alignment, row pairs]) in a fresh process each: tiny windows, slices
    over the LDS budget (global records, kind 2), a 16-double budget (almost every slice global), wavelengths never
    staged / always staged, the bracket test on every lookup, unaligned windows, two rows per wave with staged and with
    global wavelengths (rows of 100: ragged chunks).  The knobs are read once per process, so each case runs in a
    subprocess.  The debug line's figures are the host harness' for the same caps, and each case reaches what it is
    there for."""
    from helpers.window_plan import Caps
    env = dict(os.environ, PROM_TW_ROWCAP=caps[0], PROM_TW_PMAX=caps[1], PROM_TW_LDS=caps[2], PROM_DEBUG="1",
               PROM_TW="1")
    for k, v in zip(("PROM_TW_LAMCAP", "PROM_TW_LAMFIT", "PROM_TW_EXACT", "PROM_TW_ALIGN", "PROM_TW_RP"), caps[3:]):
        env[k] = v
    code = _ON_OFF % "configs.reduced(configs.get('C3'))"
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stderr.splitlines() if "target windows" in l]
    assert lines, p.stderr[-2000:]
    print(caps, lines[0])
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["eq"]
    _assert_variants(out)
    nw, staged, glob, unguessed, outside, lam_staged = got = _counts(lines[0])
    assert got == _host_counts(libs, "C3r", None, Caps(out["shape"][0], caps))
    if caps == ("256", "8192", "16"):
        assert glob > 0 and outside > 0      # (almost every slice global; unguessed ones that fit no pool: kind 0)
    if caps == ("4", "32", "96"):
        assert glob > 0 and unguessed > 0    # (global records and searched slices)
    if len(caps) > 3 and caps[3] == "0":
        assert lam_staged == 0               # (PROM_TW_LAMCAP=0: wavelengths never staged)
    if len(caps) > 4 and caps[4] == "1":
        assert lam_staged == nw              # (PROM_TW_LAMFIT=1: always)


@pytest.mark.parametrize("name", ["C4", "exomoon"])
def test_windows_row_pairs_one_species_bitwise(name):
    """Two rows per wave (PROM_TW_RP=2, read once per process: a subprocess) on one-species problems at their shipped
    sizes (C4 full size: 8 rows; the reduced exomoon golden config): R bitwise the wavelength-block kernel's."""
    env = dict(os.environ, PROM_TW_RP="2", PROM_TW="1", PROM_DEBUG="1")
    red = "configs.reduced(configs.get(%r))" % name if name == "exomoon" else "configs.get(%r)" % name
    p = subprocess.run([sys.executable, "-c", _ON_OFF % red], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert any("target windows" in l for l in p.stderr.splitlines()), p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(name, out)
    assert out["eq"]
    _assert_variants(out)


# ---- small shapes against the oracle ----
_SMALL = (
    "import numpy as np, json, os, sys\n"
    "from prometheus_amd import setupfile\n"
    "for case in json.load(open(sys.argv[1])):\n"
    "    os.environ['PROM_TW'] = '1'\n"
    "    tr = setupfile.build_transit(case['cfg'])\n"
    "    tr.collect_stats = True\n"
    "    R = tr.sumOverChords(devices=[0])\n"
    "    v1 = [s['tau_kernel_variant'] for s in tr.last_stats]\n"
    "    os.environ['PROM_TW'] = '0'\n"
    "    R0 = tr.sumOverChords(devices=[0])\n"
    "    v0 = [s['tau_kernel_variant'] for s in tr.last_stats]\n"
    "    Ro = np.load(case['oracle'])\n"
    "    err = float(np.max(np.abs(R - Ro) / np.abs(Ro))) if R.shape == Ro.shape else float('inf')\n"
    "    print(json.dumps({'n': case['n'], 'eq': bool(np.array_equal(R, R0)), 'shape': list(R.shape), 'v1': v1,\n"
    "                      'v0': v0, 'err': err, 'finite': bool(np.all(np.isfinite(R)))}), flush=True)\n")
_SMALL_STOP = []   # (a subprocess that ended with a non-zero return code: no further GPU work from this test)


@functools.lru_cache(maxsize=None)
def _oracle_R(name, n, d):
    """The float64 oracle's R of a fine config, computed once per (config, phase count) and passed by file."""
    from helpers import window_plan as WP
    from oracle import prom_oracle as O
    cfg = WP.c4fine_cfg(n) if name == "C4fine" else WP.c3fine_cfg(n)
    _, _, R = O.run_setup(cfg)
    path = os.path.join(d, "oracle_%s_%d.npy" % (name, n))
    np.save(path, R)
    return cfg, path


@pytest.fixture(scope="module")
def oracle_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("oracle"))


@pytest.mark.parametrize("name,phases,knobs", [
    ("C4fine", (2, 3, 5, 8), {}),
    ("C4fine", (2, 3, 5, 8), {"RP": "1"}),
    ("C4fine", (2, 3, 5, 8), {"RP": "2", "LAMCAP": "0"}),
    ("C4fine", (2, 3, 5, 8), {"ROWCAP": "100"}),
    ("C3fine", (3, 6), {}),
    ("C3fine", (3, 6), {"RP": "2"}),
], ids=["C4fine-default", "C4fine-RP1", "C4fine-RP2-LAMCAP0", "C4fine-ROWCAP100", "C3fine-default", "C3fine-RP2"])
def test_windows_small_shapes_against_oracle(name, phases, knobs, libs, oracle_dir, tmp_path):
    """k_sigma_tw at the row counts where its dispatch changes, on grids whose Doppler spread is many chunks wide
    (C4fine: 14,561 wavelengths, 14,561 % 64 = 33, one table, row pairs by default; C3fine: 12,001 wavelengths, three
    tables, single rows by default), per knob set in a process of its own: k_sigma_tw took the run, R is bitwise the
    wavelength-block kernel's and within 1e-10 of the float64 oracle's, and the windows built are the host harness'
    plan for the same inputs and caps."""
    from helpers.window_plan import Caps
    assert not _SMALL_STOP, "an earlier case's process ended with return code %s" % _SMALL_STOP[:1]
    cases = []
    for n in phases:
        cfg, path = _oracle_R(name, n, oracle_dir)
        cases.append({"n": n, "cfg": cfg, "oracle": path})
    job = tmp_path / "cases.json"
    job.write_text(json.dumps(cases))
    env = dict(os.environ, PROM_DEBUG="1")
    for k, v in knobs.items():
        env["PROM_TW_" + k] = v
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _SMALL, str(job)], env=env, cwd=ROOT,
                       capture_output=True, text=True)
    if p.returncode != 0:
        _SMALL_STOP.append(p.returncode)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = [l for l in p.stderr.splitlines() if "target windows" in l]
    outs = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]   # (setup warnings share stdout)
    assert len(outs) == len(phases) and len(lines) == len(phases), (p.stdout, p.stderr[-2000:])
    for n, out, line in zip(phases, outs, lines):
        print(name, knobs, out, line)
        assert out["n"] == n and out["shape"][0] == n and out["finite"]
        _assert_variants(out)
        assert out["eq"], "R over target windows is not bitwise the wavelength-block kernel's"
        assert out["err"] < R_TOL, out
        caps = Caps(n, **{k: v for k, v in knobs.items() if k != "RP"})
        assert _counts(line) == _host_counts(libs, name, n, caps)
        if knobs.get("LAMCAP") == "0":
            assert _counts(line)[5] == 0
