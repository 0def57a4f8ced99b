"""Every stream-taking entry of include/pt2q.h on a delayed, non-default stream.

pt2q.h promises that a call is stream-ordered and asynchronous (no host synchronisation, no
allocation) and retains nothing.  Per case of tests/stream_cases.py:

  1. reference: one call on the idle default stream, real inputs, fresh buffers (checked against
     the case's oracle outputs where it carries them; else the test named in `pinned` ties these
     bits to the oracle); its host time is t_host;
  2. a second buffer set holds the DECOY problem (same shapes, another seed) and has just run it,
     so outputs hold decoy results and the workspace is dirty with a real run of the same entry;
  3. a stream s sleeps for max(20 ms, 10 t_host); behind the sleep, on s: the real inputs are
     copied over the decoys, the entry runs, outputs and status words are cloned, the decoys are
     copied back and the decoy problem runs again;
     (all of 3 twice, on two streams: see the test);
  4. the entry must return while s still sleeps (it did not synchronise, and everything above was
     enqueued before any of it ran); host pointer arrays are then pointed at other buffers;
  5. the clones must equal the reference bit for bit.

Work issued on a stream that s does not order runs at enqueue time and meets decoys; side work not
joined before the call's last kernel is overtaken by the refill and the second decoy run; a
workspace word the call forgets to initialise on its own stream is left over from the decoy run.
Decoys are always valid values of their kind (never NaN fill or random bytes), so an ordering bug
shows as wrong bits, never as a wild access.  New entries: add a case to tests/stream_cases.py."""
import time

import numpy as np
import pytest
import torch

import stream_cases as sc
from test_gpu_parity import bits_equal

pytestmark = pytest.mark.gpu

DEV = "cuda"
MIN_DELAY_MS = 20.0


@pytest.fixture(scope="module")
def cycles_per_ms():
    """torch.cuda._sleep's cycle rate, from two events around a fixed sleep."""
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 2_000_000
    a.record()
    torch.cuda._sleep(n)
    b.record()
    torch.cuda.synchronize()
    rate = n / a.elapsed_time(b)
    print("stream-order: calibrated %.0f cycles per ms" % rate)
    return rate


def sleep_on(stream, ms, rate):
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * rate))


class Bufs:
    """One set of device buffers of a case: its inputs (from host tensors), zeroed outputs and
    zeroed workspaces."""

    def __init__(self, case, L, inputs):
        self.host = {k: v for k, v in inputs.items() if k.startswith("h_")}
        self.names = [k for k in inputs if not k.startswith("h_")]
        self.t = {k: inputs[k].to(DEV) for k in self.names}
        for k, (shape, dt) in case.out.items():
            self.t[k] = torch.zeros(shape, dtype=dt, device=DEV)
        for k, nbytes in case.ws.items():
            self.t[k] = torch.zeros(max(int(nbytes(L)), 256), dtype=torch.uint8, device=DEV)

    def fill(self, staged):
        for k in self.names:
            self.t[k].copy_(staged[k])


def run(case, pt2q, bufs, host, stream):
    """One call of the entry; -> (its Ctx, host seconds).  No synchronisation."""
    ctx = sc.Ctx(pt2q._lib.lib(), bufs.t, host, stream.cuda_stream)
    t0 = time.perf_counter()
    rcs = case.call(ctx)
    dt = time.perf_counter() - t0
    for rc in rcs if isinstance(rcs, list) else [rcs]:
        pt2q._lib.check(rc, case.entry)
    return ctx, dt


def snapshot(case, bufs):
    out = {k: bufs.t[k].clone() for k in case.outputs}
    out.update({"status:" + k: bufs.t[k][:4].view(torch.int32).clone() for k in case.status})
    return out


def same_bits(a, b):
    a, b = a.cpu(), b.cpu() if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b))
    if a.dtype in (torch.float16, torch.bfloat16):
        a, b = a.float(), b.float()
    if a.is_floating_point():
        return a.shape == b.shape and bits_equal(a.numpy(), b.numpy())
    return a.shape == b.shape and np.array_equal(a.numpy(), b.numpy())


def reference(case, pt2q, real):
    """Step 1 -> (buffer set, reference snapshot, t_host)."""
    A = Bufs(case, pt2q._lib.lib(), real)
    torch.cuda.synchronize()
    _, t_host = run(case, pt2q, A, A.host, torch.cuda.current_stream())
    torch.cuda.synchronize()
    ref = snapshot(case, A)
    for k in case.status:
        assert int(ref["status:" + k].item()) == 0, (case.id, k)
    if case.oracle is not None:
        for k, v in case.oracle(real).items():
            assert same_bits(ref[k], v), (case.id, k, "default stream vs oracle")
    return A, ref, t_host


def prepared(case, pt2q, decoy):
    """Step 2 -> a buffer set that holds the decoy problem and has just run it."""
    B = Bufs(case, pt2q._lib.lib(), decoy)
    run(case, pt2q, B, B.host, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return B


def enqueue(case, pt2q, B, real_dev, real_host, decoy_dev, decoy_host, s, others, woke=None):
    """Steps 4-6 on the current stream s -> (clones, whether the stream was awake at the return)."""
    B.fill(real_dev)
    ctx, _ = run(case, pt2q, B, real_host, s)
    awake = woke.query() if woke is not None else None
    for arr, names in ctx.arrays:  # "read during the call only": point them elsewhere at once
        for j, k in enumerate(names):
            arr[j] = others.t[k].data_ptr()
    got = snapshot(case, B)
    B.fill(decoy_dev)
    run(case, pt2q, B, decoy_host, s)
    return got, awake


@pytest.mark.parametrize("case", sc.CASES, ids=repr)
def test_entry_on_a_delayed_stream(pt2q, cycles_per_ms, case):
    real, decoy = case.make(sc.REAL_SEED), case.make(sc.DECOY_SEED)
    A, ref, t_host = reference(case, pt2q, real)
    B = prepared(case, pt2q, decoy)
    real_dev = {k: real[k].to(DEV) for k in B.names}
    decoy_dev = {k: decoy[k].to(DEV) for k in B.names}
    A.fill(decoy_dev)  # the other buffers the pointer arrays are pointed at: decoys too
    torch.cuda.synchronize()
    delay = max(MIN_DELAY_MS, 10e3 * t_host)
    print("stream-order: %-32s t_host %8.3f ms  delay %7.1f ms" % (case.id, 1e3 * t_host, delay))
    # Twice, on two streams taken one after the other from torch's pool: streams share hardware
    # queues (four by default), and a sleeping stream holds back every stream on its queue, so
    # work issued on the wrong stream -- stream 0, say -- is ordered by accident when that stream
    # shares s's queue.  It cannot share both.
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        # The caching allocator keeps one pool per stream: the clones taken behind the sleep would be
        # the first blocks of s's pool, i.e. device allocations (milliseconds each for the larger
        # outputs, and of no fixed cost) inside the timed window.  Take and drop them once before the
        # sleep, so that the window holds the enqueue alone.
        with torch.cuda.stream(s):
            snapshot(case, B)
        sleep_on(s, delay, cycles_per_ms)
        woke = torch.cuda.Event()
        woke.record(s)
        with torch.cuda.stream(s):
            t0 = time.perf_counter()
            got, awake = enqueue(case, pt2q, B, real_dev, A.host, decoy_dev, B.host, s, A, woke)
            t_enq = time.perf_counter() - t0
            covered = not woke.query()
        print("stream-order: %-32s enqueue %8.3f ms behind %7.1f ms" % (case.id, 1e3 * t_enq, delay))
        assert not awake, ("%s returned after its stream woke: the call synchronised with the device, or the "
                           "delay did not cover the enqueue (t_host %.3f ms, delay %.1f ms, enqueue up to the "
                           "return and after %.3f ms)" % (case.entry, 1e3 * t_host, delay, 1e3 * t_enq))
        assert covered, ("%s: the stream woke before the refill and the second decoy run were enqueued (%.3f ms "
                         "behind a delay of %.1f ms): a late reader could go unseen" % (case.id, 1e3 * t_enq, delay))
        s.synchronize()
        for k, v in ref.items():
            assert same_bits(got[k], v), (case.id, k)


def _ahead_case():
    return sc.BY_ID["cholesky-inverse-%d" % sc.CHOL_AHEAD_M]


def test_lookahead_inverse_twice_on_one_stream(pt2q, cycles_per_ms):
    """Two m = 6208 inverses back to back on one delayed stream, on different matrices with
    separate buffers and workspaces: both calls share the side stream of (device, s), so the first
    call's forked work must be joined before the second call zeroes its scratch."""
    case = _ahead_case()
    hosts = [case.make(sc.REAL_SEED), case.make(sc.DECOY_SEED)]
    refs, sets = [], []
    for h in hosts:
        A, ref, _ = reference(case, pt2q, h)
        refs.append(ref)
        del A
        sets.append(Bufs(case, pt2q._lib.lib(), h))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    sleep_on(s, MIN_DELAY_MS, cycles_per_ms)
    with torch.cuda.stream(s):
        for B in sets:
            run(case, pt2q, B, B.host, s)
        got = [snapshot(case, B) for B in sets]
    s.synchronize()
    for z in range(2):
        for k, v in refs[z].items():
            assert same_bits(got[z][k], v), (z, k)


def test_lookahead_inverse_on_two_streams(pt2q, cycles_per_ms):
    """The same m = 6208 inverse on two streams that start together (both wait on one event
    behind a single delay on a third stream): each (device, stream) has a side stream and events
    of its own, each call its own buffers and workspace."""
    case = _ahead_case()
    hosts = [case.make(sc.REAL_SEED), case.make(sc.DECOY_SEED)]
    refs, sets = [], []
    for h in hosts:
        A, ref, _ = reference(case, pt2q, h)
        refs.append(ref)
        del A
        sets.append(Bufs(case, pt2q._lib.lib(), h))
    torch.cuda.synchronize()
    gate, streams = torch.cuda.Stream(), [torch.cuda.Stream(), torch.cuda.Stream()]
    sleep_on(gate, MIN_DELAY_MS, cycles_per_ms)
    go = torch.cuda.Event()
    go.record(gate)
    got = []
    for s, B in zip(streams, sets):
        s.wait_event(go)
        with torch.cuda.stream(s):
            run(case, pt2q, B, B.host, s)
            got.append(snapshot(case, B))
    for s in streams:
        s.synchronize()
    for z in range(2):
        for k, v in refs[z].items():
            assert same_bits(got[z][k], v), (z, k)
