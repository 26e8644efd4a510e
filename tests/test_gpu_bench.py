"""bench.py on the GPU, one process: a plain run prints the headline line only and --dump-outputs writes the R of
its last timed step, the same array from run to run; --full adds the figures that take runs of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("roofline", "stage_ms_single_run", "single_run_ms", "chords", "end_to_end_s", "cpu_baseline",
             "strong_scaling_projection")


def _run(*args):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "C2", *args]
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dump"))
    res = _run("--steps", "5", "--warmup", "2", "--dump-outputs", out, "--dump-R", os.path.join(out, "dump_R"))
    return res, out


def test_plain_line_is_the_headline(plain):
    res, _ = plain
    for k in HEADLINE:
        assert k in res
    for k in FULL_ONLY:
        assert k not in res
    assert res["steps"] == 5 and res["warmup"] == 2 and res["dtype"] == "f64" and res["higher_is_better"] is True
    n_pts = res["config"]["global_wavelengths"] * res["config"]["orbital_phases"]
    assert res["ms_per_step"] > 0 and abs(res["value"] * res["ms_per_step"] * 1e-3 - n_pts) / n_pts < 1e-9


def test_dump_outputs_is_the_last_steps_R(plain):
    res, out = plain
    R = np.load(os.path.join(out, "R.npy"))
    assert R.dtype == np.float64
    assert R.shape == (res["config"]["orbital_phases"], res["config"]["global_wavelengths"])
    assert np.all(np.isfinite(R)) and R.min() < R.max()
    assert np.array_equal(R, np.load(os.path.join(out, "dump_R", "R_rank0.npy")))


def test_dump_outputs_repeats_and_full_adds_figures(plain, tmp_path):
    """A second process, other step counts, --full (no CPU legs or projection: their own time): the same R bit for
    bit, and the line carries the per-kernel figures."""
    _, out = plain
    res = _run("--steps", "9", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-projection",
               "--dump-outputs", str(tmp_path))
    assert res["steps"] == 9
    for k in HEADLINE + ("roofline", "stage_ms_single_run", "single_run_ms", "chords", "end_to_end_s"):
        assert k in res
    assert res["roofline"]["kernels"]
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "R.npy")), np.load(os.path.join(out, "R.npy")))
