"""The injection side's counterpart of test_gpu_chain_entries.py: clean, inject, recover and their grids run through one
runner and share the buffers sy.D .. sy.U, sy.Fj, sy.model, sy.trial / sy.scale and rc.W (prom_api_inject.hip), between
calls whose layouts differ: [1] against [B] injections, the whole table against [n_seg] items n_max wide, with and
without W.  Nothing of one call may reach the next.  Nine calls are interleaved on one context, each asking for every
output, and each call's outputs equal, byte for byte and NaNs included, those of the same call made alone on a fresh
context.  After a single call prom_sysrem_kernel_ms runs once (after the recovery prom_filter_kernel_ms too), every
stage the call had takes time, and the call is repeated with the same bytes; after a grid call both aids refuse, and
entry b of every grid output is the matching single call made alone.  The same sequence runs under
PROM_GRID_SCRATCH_MB forced down so that the list of three runs as 2 + 1.

The design is test_gpu_chain_entries.py's: 3 exposures, 9 trials (two trial groups), 130 pixels (two SYSREM tiles) in
two orders of 127 and 3 pixels, one entry with ivar = 0, a high-pass of half width 2, and the raw exposures."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import grid_design as gd
import test_gpu_chain_entries as ce
import test_gpu_sysrem as ts
import test_gpu_sysrem_orders as tso

pytestmark = pytest.mark.gpu

REPO = ce.REPO
CAP = "PROM_GRID_SCRATCH_MB"                                  # read at every grid call
POINTS = [(4, 0.7), (0, 0.0), (8, -0.3)]                      # the list; its first entry is the single calls' injection
TRIALS, SCALES = [t for t, _ in POINTS], [s for _, s in POINTS]
KW = dict(n_comp=2, n_iter=4, highpass=True)
design = ce.design


def setup(dev, d):
    ts.upload(dev, d)
    dev.highpass_set(d["seg"], d["perm"], d["g"], 0)
    dev.orders_set(d["seg"], d["perm"])


def _inject(dev, d, t, s):
    return dev.spectrum_inject(d["wav"], d["R"], t, s, ones=True, injected=True, **KW)


def _inject_orders(dev, d, t, s):
    return dev.spectrum_inject_orders(d["wav"], d["R"], t, s, injected=True, **KW)


def _recover(dev, d, t, s):
    return dev.spectrum_recover(d["wav"], d["R"], t, s, orders=True, model=True, **KW)


# the single calls a grid's entries are compared with, and the outputs of theirs that the grid has
SINGLES = {"inject": (_inject, (0, 1, 2)), "inject orders": (_inject_orders, (0, 1, 2)),
           "recover": (_recover, (0, 1, 4, 6))}

# the nine calls in their order: (name, the call, the single call of its entries or None)
CALLS = [
    ("clean", lambda dev, d: dev.sysrem_clean(ones=True, injected=True, **KW), None),
    ("inject grid", lambda dev, d: dev.spectrum_inject_grid(d["wav"], d["R"], TRIALS, SCALES, ones=True, injected=True,
                                                            **KW), "inject"),
    ("inject orders", lambda dev, d: _inject_orders(dev, d, *POINTS[0]), None),
    ("recover", lambda dev, d: _recover(dev, d, *POINTS[0]), None),
    ("inject grid orders", lambda dev, d: dev.spectrum_inject_grid_orders(d["wav"], d["R"], TRIALS, SCALES, injected=True,
                                                                          **KW), "inject orders"),
    ("inject", lambda dev, d: _inject(dev, d, *POINTS[0]), None),
    ("recover grid", lambda dev, d: dev.spectrum_recover_grid(d["wav"], d["R"], TRIALS, SCALES, orders=True, **KW),
     "recover"),
    ("clean orders", lambda dev, d: dev.sysrem_clean_orders(ones=True, injected=True, **KW), None),
    ("inject", lambda dev, d: _inject(dev, d, *POINTS[0]), None),
]


def digest(out):
    """One sha256 per output over its raw bytes (equal digests: equal bytes, NaN payloads included)."""
    assert all(x is not None for x in out)
    return [hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() for x in out]


def cap_mb(d, name, nb=2):
    """Megabytes under which a sub-batch of the grid call ``name`` holds exactly nb injections of the design, as
    test_gpu_inject_grid.cap_for and test_gpu_sysrem_orders set them."""
    n_exp, n_pix = d["raw"].shape
    n_tap = d["F"].shape[2]
    if name == "inject grid orders":
        per = tso.order_bytes(n_exp, n_pix, len(d["seg"]) - 1, int(np.diff(d["seg"]).max()), 2, n_tap)
    else:
        per = gd.injection_bytes(n_exp, n_pix, 3 if name == "inject grid" else 2, n_tap, name == "recover grid")
    return repr((nb * per + per // 2) / 1048576.0)


def fresh(d, call):
    """The digests of call(dev, d) on a context of its own."""
    from prometheus_amd import _native
    dev = _native.Device(0)
    try:
        setup(dev, d)
        return digest(call(dev, d))
    finally:
        dev.close()


def alone(d):
    """Each distinct call, and each single call of each entry of the list, on a context of its own:
    ({name: digests}, {single: [digests of entry b]})."""
    want = {}
    for name, call, _ in CALLS:
        if name not in want:
            want[name] = fresh(d, call)
    entries = {single: [[fresh(d, lambda dev, d_: call(dev, d_, t, s))[i] for i in keep] for t, s in POINTS]
               for single, (call, keep) in SINGLES.items()}
    return want, entries


def sequence(d, capped):
    """The nine calls on one fresh context: [(name, digests, the repetition's digests or None, per entry digests or
    None)].  A single call is followed by its aids and repeated; after a grid call the aids refuse."""
    from prometheus_amd import _native
    dev = _native.Device(0)
    got = []
    try:
        setup(dev, d)
        for name, call, single in CALLS:
            if single is None:
                first = digest(call(dev, d))
                if name == "recover":                                       # (first: the other aid's run moves U)
                    assert dev.filter_kernel_ms(1) > 0.0
                ms = dev.sysrem_kernel_ms(1)                                # (the loop, the injection, the high-pass)
                assert ms[0] > 0.0 and ms[2] > 0.0, (name, ms)
                assert np.isnan(ms[1]) if name.startswith("clean") else ms[1] > 0.0, (name, ms)
                got.append((name, first, digest(call(dev, d)), None))
                continue
            if capped:                                                      # (a process of its own: see below)
                os.environ[CAP] = cap_mb(d, name)
            out = call(dev, d)
            for aid in (dev.sysrem_kernel_ms, dev.filter_kernel_ms):        # nothing of a grid call to repeat
                with pytest.raises(_native.NativeError, match="PROM_E_STATE"):
                    aid(1)
            got.append((name, digest(out), None, [digest([x[b] for x in out]) for b in range(len(POINTS))]))
    finally:
        dev.close()
    return got


@pytest.fixture(scope="module")
def want():
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv(CAP, raising=False)
        return alone(design())


def check(got, want):
    want, entries = want
    assert [g[0] for g in got] == [c[0] for c in CALLS]
    for i, ((name, first, again, per_entry), (_, _, single)) in enumerate(zip(got, CALLS)):
        assert first == want[name], ("call %d" % (i + 1), name)
        if single is None:
            assert again == want[name], ("call %d after its aids" % (i + 1), name)
        else:
            assert per_entry == entries[single], ("call %d, its entries against the single calls" % (i + 1), name)


def test_the_calls_differ_so_a_leak_would_show(want):
    want, entries = want
    assert len(set(map(tuple, want.values()))) == len(want) == 8
    for single, per_entry in entries.items():                              # ... and so do the entries of the list
        assert len(set(map(tuple, per_entry))) == len(POINTS), single
    assert entries["inject"][0] == want["inject"] and entries["inject orders"][0] == want["inject orders"]


def test_interleaved_calls_equal_the_calls_alone_bytewise(want, monkeypatch):
    monkeypatch.delenv(CAP, raising=False)
    check(sequence(design(), False), want)


_CAPPED = """
import json, sys
sys.path.insert(0, %r)
from test_gpu_inject_entries import design, sequence
print(json.dumps(sequence(design(), True)))
"""


def test_interleaved_calls_in_sub_batches_of_two_bytewise(want):
    """Every grid call under a cap that holds two injections, so the list of three runs as 2 + 1; PROM_DEBUG is read
    once per process, so the case runs in a process of its own."""
    env = dict(os.environ, PROM_DEBUG="1")
    env.pop(CAP, None)
    p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CAPPED % os.path.join(REPO, "tests")],
                       env=env, cwd=REPO, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = [l for l in p.stderr.splitlines() if "injection grid:" in l]
    assert len(lines) == 3 and all("3 injections in 2 sub-batches of up to 2," in l for l in lines), p.stderr[-2000:]
    got = json.loads([l for l in p.stdout.splitlines() if l.startswith("[")][-1])
    check([tuple(g) for g in got], want)
