"""k_sigma_tw's staging prologue from the windows' stage records (prometheus_amd/csrc/tw_stage.h), its row-resident
curve scalars and its split by wavelength source, on the GPU: R over target windows (PROM_TW=1) is BITWISE the
wavelength-block kernel's (PROM_TW=0), and k_sigma_tw took the windowed run (tau_kernel_variant // 10 == 9) and not
the other, so a silent fallback cannot pass.

Shapes: the fine low-end grid of C3 (three merged species, 12,001 wavelengths) at 2, 3, 5 and 16 phases -- fewer rows
than waves, a row count that is no multiple of 4, C3's own 16 -- and of C4 (one species, row pairs) at 2 phases; at 3
phases also C3's setup without Mg I (two species) and with K I added (four).  Knob sets, one process each (the knobs
are read once per process), every shape in it:

  default      the shipped caps: ~100 windows, some with staged wavelengths, most with global ones (both instances
               of the first pass), searched slices at 2 and 16 phases
  tiny         ROWCAP=8 PMAX=64 LDS=2560: 1,600-3,000 windows whose slices are far shorter than 256 nodes, so one
               thread's pool entries and neighbouring threads straddle the species' boundaries; every window staged
  LDS=96       a 31-node pool: ~3,000 windows of a few nodes per species.  (On these grids every slice still fits the
               pool -- the planner shortens the windows instead -- so this set reaches no rare window; LDS=16 does)
  LDS=16       no slice fits the pool: global slices, rare windows, the second pass for almost every window
  LAMCAP=0     wavelengths never staged: the global instance after the split
  LAMFIT=1     windows grown only while their wavelengths fit: the staged instance (every window of the C3 shapes)
  EXACT=0      no exact marks: the bracket test on every lookup

The debug line's figures (windows, slices by kind, windows with staged wavelengths) are the host planner's for the
same inputs and caps (tests/helpers/window_plan.py), and each knob set asserts there what it is there to reach.
"""
import copy
import functools
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LINE = re.compile(r"target windows: (\d+) \(slices: (\d+) staged, (\d+) global, (\d+) staged unguessed, "
                   r"(\d+) outside the table; wavelengths staged in (\d+) windows")

# every shape of a job file with target windows and without, in one process: a JSON line per shape with the bitwise
# comparison and the kernel variants of both runs
_JOB = (
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
    "    print(json.dumps({'id': case['id'], 'eq': bool(np.array_equal(R, R0)), 'shape': list(R.shape), 'v1': v1,\n"
    "                      'v0': v0, 'finite': bool(np.all(np.isfinite(R)))}), flush=True)\n")
_STOP = []   # (a subprocess that ended with a non-zero return code: no further GPU work from this module)


def _cfg(name, n):
    from helpers import window_plan as WP
    if name == "C4fine":
        return WP.c4fine_cfg(n)
    cfg = copy.deepcopy(WP.c3fine_cfg(n))
    if name == "C3fine-2sp":
        del cfg["Species"]["powerLaw"]["MgI"]
    elif name == "C3fine-4sp":
        cfg["Species"]["powerLaw"]["KI"] = {"chi": 1e-06}
    return cfg


@functools.lru_cache(maxsize=None)
def _inputs(name, n):
    from helpers import window_plan as WP
    return WP.oracle_inputs(_cfg(name, n))


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    from helpers.window_plan import Libs
    return Libs(tmp_path_factory.mktemp("tw"))


SHAPES = [("C3fine", 2), ("C3fine", 3), ("C3fine", 5), ("C3fine", 16), ("C4fine", 2)]
OTHER_SPECIES = [("C3fine-2sp", 3), ("C3fine-4sp", 3)]
TINY = {"ROWCAP": "8", "PMAX": "64", "LDS": "2560"}


@pytest.mark.parametrize("knobs,shapes", [
    ({}, SHAPES + OTHER_SPECIES),
    (TINY, SHAPES + OTHER_SPECIES),
    ({"LDS": "96"}, SHAPES),
    ({"LDS": "16"}, SHAPES),
    ({"LAMCAP": "0"}, SHAPES),
    ({"LAMFIT": "1"}, SHAPES),
    ({"EXACT": "0"}, SHAPES),
], ids=["default", "tiny", "LDS96", "LDS16", "LAMCAP0", "LAMFIT1", "EXACT0"])
def test_tw_stage_bitwise(knobs, shapes, libs, tmp_path):
    from helpers import window_plan as WP
    assert not _STOP, "an earlier case's process ended with return code %s" % _STOP[:1]
    job = tmp_path / "cases.json"
    job.write_text(json.dumps([{"id": "%s-%d" % (name, n), "cfg": _cfg(name, n)} for name, n in shapes]))
    env = dict(os.environ, PROM_DEBUG="1")
    for k, v in knobs.items():
        env["PROM_TW_" + k] = v
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", _JOB, str(job)], env=env, cwd=ROOT,
                       capture_output=True, text=True)
    if p.returncode != 0:
        _STOP.append(p.returncode)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = [l for l in p.stderr.splitlines() if "target windows" in l]
    outs = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]   # (setup warnings share stdout)
    assert len(outs) == len(shapes) and len(lines) == len(shapes), (p.stdout, p.stderr[-2000:])
    for (name, n), out, line in zip(shapes, outs, lines):
        print(name, n, knobs, out, line)
        assert out["id"] == "%s-%d" % (name, n) and out["shape"][0] == n and out["finite"]
        assert out["v1"] and all(v // 10 == 9 for v in out["v1"]), out
        assert out["v0"] and all(v // 10 != 9 for v in out["v0"]), out
        assert out["eq"], "R over target windows is not bitwise the wavelength-block kernel's"
        m = _LINE.search(line)
        assert m, line
        got = tuple(int(v) for v in m.groups())
        caps = WP.Caps(n, **{k: v for k, v in knobs.items() if k != "EXACT"})
        nw, staged, glob, unguessed, outside, lam_staged = got
        assert got == WP.debug_counts(WP.make_plan(libs, _inputs(name, n), caps))
        c3 = name.startswith("C3fine")
        if not knobs or knobs == {"EXACT": "0"}:
            assert 0 < lam_staged < nw and glob == 0     # (both instances of the first pass)
        elif knobs == TINY:
            assert nw >= 1600 and glob == 0 and (lam_staged == nw or not c3)
        elif knobs == {"LDS": "96"}:
            assert nw >= 3000 and glob == 0
        elif knobs == {"LDS": "16"}:
            assert glob > 0                              # (rare windows: the second pass)
        elif knobs == {"LAMCAP": "0"}:
            assert lam_staged == 0
        elif knobs == {"LAMFIT": "1"}:
            assert lam_staged == nw if c3 else lam_staged > 0
    if not knobs:
        assert any(o[3] > 0 for o in [tuple(int(v) for v in _LINE.search(l).groups()) for l in lines])   # (searched slices)
