"""Stalled cross-workgroup hand-offs fail loudly (ADVICE r1 / VERDICT r1 weak #6).

The stream-K Gram partials poll a flag a bounded number of times.  When a wait gives up, the kernel sets a bit in the call's status word (the head of its workspace, include/pt2q.h PT2Q_STATUS_BYTES) and the Python layer
raises Pt2qError instead of returning results computed from stale data.  The cap is a load-time
setting (PT2Q_DEBUG_SPIN_CAP; 0 makes every hand-off report a stall), so the forced-stall runs
happen in a child process.  The ATQ launch's S1/d hand-off does not fail: a row wave whose
wait gives up forms S1/d itself in the same order (atq.hip s1_local), so its results are the
same bits -- checked below with every hand-off forced to give up."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CHILD = r'''
import sys, torch
sys.path.insert(0, ROOT)
import pt2q_loader
pt2q = pt2q_loader.load()
X = pt2q.fill_synthetic((16384, 4096), 5, outliers=True).half()
W = pt2q.fill_synthetic((1024, 4096), 6, std=0.02)
def attempt(tag, fn):
    try:
        fn()
        torch.cuda.synchronize()
        print(tag, "NO-RAISE", flush=True)
    except pt2q._lib.Pt2qError as e:
        print(tag, "RAISED", e, flush=True)
attempt("gram", lambda: pt2q.gram(X))
attempt("layer", lambda: pt2q.quantize_layer(W, X))
g = pt2q.LayerGraph(W, X)
g.replay()
attempt("graph", g.spd)
'''


def run_child(cap):
    env = dict(os.environ)
    if cap is None:
        env.pop("PT2Q_DEBUG_SPIN_CAP", None)
    else:
        env["PT2Q_DEBUG_SPIN_CAP"] = str(cap)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_forced_stall_raises():
    """Spin cap 0: the Gram's continuing pieces report their hand-off as stalled, and every
    entry point that forms a Gram raises."""
    out = run_child(0)
    assert "gram RAISED" in out and "Gram partial-tile hand-off" in out, out
    assert "layer RAISED" in out, out
    assert "graph RAISED" in out, out


def test_default_cap_no_stall(pt2q):
    """The default cap never trips on a healthy run (same workload, in process)."""
    X = pt2q.fill_synthetic((16384, 4096), 5, outliers=True).half()
    W = pt2q.fill_synthetic((1024, 4096), 6, std=0.02)
    G = pt2q.gram(X)
    out = pt2q.quantize_layer(W, X)
    assert out.spd and int(out.status.item()) == 0
    assert G.shape == (4096, 4096)


CHILD_BLOCKS = r'''
import sys, hashlib, torch
sys.path.insert(0, ROOT)
import pt2q_loader
pt2q = pt2q_loader.load()
X = pt2q.fill_synthetic((4096, 1024), 15, outliers=True).half().float()
W = pt2q.fill_synthetic((768, 1024), 16, std=0.02)
G = X.T @ X  # test input only (no hand-off), the same G in both children
Hinv, spd = pt2q.hessian_inverse(G, X.shape[0])
out = pt2q.quantize_blocks(W, G, Hinv, 128, True)
torch.cuda.synchronize()
h = hashlib.sha256()
for t in (out.alpha, out.mu, out.T, out.perm, out.iters):
    h.update(t.cpu().numpy().tobytes())
print("BLOCKS", spd, h.hexdigest(), flush=True)
'''


def test_atq_s1_fallback_same_bits():
    """Every ATQ S1/d wait forced to give up (cap 0): the row waves form S1/d themselves and the
    whole SSR block loop returns exactly the default run's bits, with no stall raised."""
    outs = []
    for cap in (None, 0):
        env = dict(os.environ)
        env.pop("PT2Q_DEBUG_SPIN_CAP", None)
        if cap is not None:
            env["PT2Q_DEBUG_SPIN_CAP"] = str(cap)
        r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD_BLOCKS], env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=110)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append([l for l in r.stdout.splitlines() if l.startswith("BLOCKS")][0])
    assert outs[0] == outs[1], outs
