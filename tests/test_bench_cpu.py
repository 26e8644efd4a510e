"""bench.py without a GPU: the options of a plain and a --full run, and what --dump-outputs writes."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, REPO)
    try:
        import bench as b
    finally:
        sys.path.remove(REPO)
    return b


def _parse(bench, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return bench.parse()


def test_plain_run_measures_the_headline_only(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert not a.full and a.steps == 7 and a.warmup == 2 and a.config == "C3"
    assert a.strong == "" and a.dump_outputs is None


def test_full_run_keeps_the_default_strong_legs(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--full")
    assert a.full and a.strong == "C4x10,C4x10p256"
    assert _parse(bench, monkeypatch, "--full", "--strong", "").strong == ""
    assert _parse(bench, monkeypatch, "--strong", "C4").strong == "C4"


def test_steps_must_be_positive(bench, monkeypatch):
    with pytest.raises(SystemExit):
        _parse(bench, monkeypatch, "--steps", "0")


def test_dump_outputs_whole(bench, tmp_path):
    R = np.random.default_rng(1).random((3, 41))
    bench.dump_outputs(str(tmp_path / "d"), R, 0, 1)
    assert sorted(os.listdir(tmp_path / "d")) == ["R.npy"]
    got = np.load(tmp_path / "d" / "R.npy")
    assert got.dtype == np.float64 and np.array_equal(got, R)
    bench.dump_outputs(str(tmp_path / "d2"), R, 1, 2)
    assert sorted(os.listdir(tmp_path / "d2")) == ["R_rank1.npy"]


def test_dump_outputs_sample_is_fixed_and_within_budget(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1600)
    R = np.random.default_rng(2).random((5, 401))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), R, 0, 1)
    va, ia = np.load(tmp_path / "a" / "R.npy"), np.load(tmp_path / "a" / "R_index.npy")
    vb, ib = np.load(tmp_path / "b" / "R.npy"), np.load(tmp_path / "b" / "R_index.npy")
    assert va.dtype == ia.dtype == np.float64 and va.shape == ia.shape == (100,)
    assert va.nbytes + ia.nbytes <= 1600
    assert np.array_equal(ia, ib) and np.array_equal(va, vb)
    idx = ia.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < R.size
    assert np.array_equal(va, R.reshape(-1)[idx])
