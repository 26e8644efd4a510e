"""The exposure families share one runner and the buffers ex.q, ex.model and ex.flag (prom_api_expose.hip): nothing of
one call may reach the next.  Eight calls of five families are interleaved on one context, each asking for every
output, and each call's outputs equal, byte for byte and NaNs included, those of the same call made alone on a fresh
context; after each call the family's *_kernel_ms aid runs once and the call is repeated with the same bytes.  The
same sequence runs on a context under a small PROM_VMAP_SCRATCH_MB, where the moments and the per-order records take
two batches.

The table is the smallest that has every stage and the batching: 3 exposures, kVmTrials + 1 trials (two trial groups),
130 pixels (two SYSREM tiles) in two orders of 127 and 3 pixels, a filter of 2 components, a high-pass of half width 2,
one entry with ivar = 0, and the raw exposures."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_sysrem as ts

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_EXP, N_TRIAL, N_PIX, N_COMP = 3, 8 + 1, 130, 2      # (8: kVmTrials = kOdTrials)
SHORT = np.array([5, 64, 129])                        # the short order's device pixels
RECOVER = dict(trial=4, scale=0.7, n_comp=N_COMP, n_iter=4, highpass=True, orders=True, model=True)


def design():
    d = ts.design(N_EXP, N_PIX, n_trial=N_TRIAL, seed=21, holes=False)
    d["ivar"][1, 40] = 0.0
    long_ = np.setdiff1d(np.arange(N_PIX), SHORT)
    d["seg"] = np.array([0, len(long_), N_PIX], dtype=np.int32)
    d["perm"] = np.concatenate([long_, SHORT]).astype(np.int32)
    d["g"] = np.array([1.0, 0.6, 0.2])
    d["U"] = np.random.default_rng(22).normal(size=(N_EXP, N_COMP))
    return d


def setup(dev, d):
    ts.upload(dev, d)
    dev.highpass_set(d["seg"], d["perm"], d["g"], 0)
    dev.orders_set(d["seg"], d["perm"])
    dev.detrend_build(d["U"])


# the eight calls in their order: (name, the call, the family's aids)
def _recover(dev, d):
    kw = dict(RECOVER)
    return dev.spectrum_recover(d["wav"], d["R"], kw.pop("trial"), kw.pop("scale"), kw.pop("n_comp"), **kw)


CALLS = [
    ("expose", lambda dev, d: dev.spectrum_expose(d["wav"], d["R"], model=True), ("expose_kernel_ms",)),
    ("orders 1 1", lambda dev, d: dev.spectrum_expose_orders(d["wav"], d["R"], highpass=True, detrend=True, model=True),
     ("orders_kernel_ms",)),
    ("highpass 0", lambda dev, d: dev.spectrum_expose_highpass(d["wav"], d["R"], detrend=False, model=True),
     ("highpass_kernel_ms",)),
    ("recover", _recover, ("filter_kernel_ms", "sysrem_kernel_ms")),
    ("detrended", lambda dev, d: dev.spectrum_expose_detrended(d["wav"], d["R"], model=True), ("detrend_kernel_ms",)),
    ("orders 0 0", lambda dev, d: dev.spectrum_expose_orders(d["wav"], d["R"], highpass=False, detrend=False, model=True),
     ("orders_kernel_ms",)),
    ("highpass 1", lambda dev, d: dev.spectrum_expose_highpass(d["wav"], d["R"], detrend=True, model=True),
     ("highpass_kernel_ms",)),
    ("expose", lambda dev, d: dev.spectrum_expose(d["wav"], d["R"], model=True), ("expose_kernel_ms",)),
]


def digest(out):
    """One sha256 per output over its raw bytes (equal digests: equal bytes, NaN payloads included)."""
    assert all(x is not None for x in out)
    return [hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() for x in out]


def alone(d):
    """Each distinct call on a context of its own: {name: digests}."""
    from prometheus_amd import _native
    want = {}
    for name, call, _ in CALLS:
        if name in want:
            continue
        dev = _native.Device(0)
        try:
            setup(dev, d)
            out = call(dev, d)
            assert np.isfinite(out[0]).any() and out[1].any(), name      # (the call has met pixels)
            want[name] = digest(out)
        finally:
            dev.close()
    return want


def sequence(d):
    """The eight calls on one fresh context, each followed by its aids and a repetition: [(name, digests, digests)]."""
    from prometheus_amd import _native
    dev = _native.Device(0)
    got = []
    try:
        setup(dev, d)
        for name, call, aids in CALLS:
            first = digest(call(dev, d))
            for aid in aids:
                assert np.all(np.asarray(getattr(dev, aid)(1)) > 0.0), (name, aid)
            got.append((name, first, digest(call(dev, d))))
    finally:
        dev.close()
    return got


@pytest.fixture(scope="module")
def want():
    return alone(design())


def check(got, want):
    assert [g[0] for g in got] == [c[0] for c in CALLS]
    for i, (name, first, again) in enumerate(got):
        assert first == want[name], ("call %d" % (i + 1), name)
        assert again == want[name], ("call %d after its aids" % (i + 1), name)


def test_interleaved_calls_equal_the_calls_alone_bytewise(want):
    assert len(set(map(tuple, want.values()))) == len(want)      # (the seven calls differ, so a leak would show)
    check(sequence(design()), want)


_BATCHED = """
import json, sys
sys.path.insert(0, %r)
from test_gpu_chain_entries import design, sequence
print(json.dumps(sequence(design())))
"""


def test_interleaved_calls_in_two_batches_bytewise(want):
    """PROM_VMAP_SCRATCH_MB is read at context creation, so the case runs in a process of its own: 0.0001 MB is below
    one trial group's partial records and one group's per-order records, so each of the two groups is a batch."""
    env = dict(os.environ, PROM_VMAP_SCRATCH_MB="0.0001", PROM_DEBUG="1")
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _BATCHED % os.path.join(REPO, "tests")],
                       env=env, cwd=REPO, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    for what in ("exposures:", "detrended moments:", "per-order moments:"):
        lines = [l for l in p.stderr.splitlines() if what in l]
        assert lines and all("2 groups, 2 batches of up to 1 groups" in l for l in lines), (what, p.stderr[-2000:])
    got = json.loads([l for l in p.stdout.splitlines() if l.startswith("[")][-1])
    check([tuple(g) for g in got], want)
