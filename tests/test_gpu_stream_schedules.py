"""Delay injection into the Python schedules: engine.UnitPipeline and sharding.GramsFirst.

The existing schedule tests compare bits with the sequential result on an idle GPU, where a
producer nearly always finishes before its consumer whether or not an event orders them.  Here each
schedule runs two steps on DIFFERENT inputs through the same persistent input buffers: step 1
undisturbed, so every slot, scratch buffer and lane workspace holds step-1 data, then step 2 with
one of the schedule's streams -- or the caller's -- put to sleep for 20 ms at the start of the step.
Step 2's inputs are written on the caller's stream inside the step.  A lost wait_stream /
wait_event edge lets a consumer run ahead of the sleeping producer and read step-1 data, which
differs from step-2 data: the results must equal quantize_unit on the step-2 inputs bit for bit
(computed beforehand on the default stream).  Every stream is delayed in turn, with step 1 run
again before each turn.  The schedules are driven through their public calls only, and no Gram is
started outside them while they run (a stream-K Gram needs the whole chip)."""
import importlib

import pytest
import torch

import synth
from test_gpu_parity import bits_equal, cuda, host
from test_gpu_stream_order import MIN_DELAY_MS, cycles_per_ms, sleep_on  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIELDS = ("alpha", "mu", "T", "perm", "iters")
# (m, row counts, N, dtype): mixed widths 512 / 768, a shared-input unit, one fp32 unit
UNITS = [(512, (384, 256), 1024, torch.float16), (768, (512,), 2048, torch.float16),
         (512, (640,), 1024, torch.float32), (512, (384,), 1024, torch.float16)]
# per-channel (block_size >= m > 512): two widths, so two S1 / d streams
PC_UNITS = [(1024, (640, 512), 4096, torch.bfloat16), (1024, (640,), 4096, torch.bfloat16),
            (768, (256,), 2048, torch.bfloat16)]
PC_BS = 1024


def delayed(stream, rate):
    """Enqueue the calibrated 20 ms delay on a torch stream."""
    sleep_on(stream, MIN_DELAY_MS, rate)


class Steps:
    """Two steps of inputs for a unit list, the persistent device buffers a step writes them into,
    and quantize_unit's results per step (default stream, computed once)."""

    def __init__(self, pt2q, specs, bs, tag):
        self.specs, self.bs = specs, bs
        self.stage = []
        for step in (0, 1):
            seed = 3000 + 1000 * step + tag
            self.stage.append([(cuda(synth.activations(seed + i, N, m)).to(dt),
                                [cuda(synth.weights(seed + 100 + 10 * i + k, n, m)).to(dt) for k, n in enumerate(ns)])
                               for i, (m, ns, N, dt) in enumerate(specs)])
        self.X = [torch.empty_like(X) for X, _ in self.stage[0]]
        self.W = [[torch.empty_like(W) for W in Ws] for _, Ws in self.stage[0]]
        self.want = [[pt2q.quantize_unit(Ws, X, block_size=bs, use_ssr=True) for X, Ws in st] for st in self.stage]
        # a unit's raw Gram, inverse and S1 / d per step, for the run() forms that take them
        self.G = [[pt2q.gram(X) for X, _ in st] for st in self.stage]
        self.Gbuf = [torch.empty_like(G) for G in self.G[0]]
        torch.cuda.synchronize()

    def write(self, step, i):
        """Unit i's inputs of `step` into the persistent buffers, on the current stream."""
        X, Ws = self.stage[step][i]
        self.X[i].copy_(X)
        for dst, src in zip(self.W[i], Ws):
            dst.copy_(src)
        return self.X[i], self.W[i]

    def check(self, step, i, outs):
        assert len(outs) == len(self.want[step][i])
        for k, (o, r) in enumerate(zip(outs, self.want[step][i])):
            for f in FIELDS:
                a = o[f] if isinstance(o, dict) else getattr(o, f)
                assert bits_equal(host(a), host(getattr(r, f))), (step, i, k, f)


@pytest.fixture(scope="module")
def steps(pt2q):
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = Steps(pt2q, *{"blocks": (UNITS, 128, 0), "pc": (PC_UNITS, PC_BS, 500)}[kind])
        return cache[kind]
    return get


# ------------------------------------------------------------------ UnitPipeline

def pipeline_step(pt2q, pipe, S, step, mode, extra, victim, rate, caller):
    """One step of every unit through pipe.run in the form `mode`; victim: a stream to delay at
    the start of the step (the caller's: before its inputs are written), or None."""
    with torch.cuda.stream(caller):
        if victim is not None:
            delayed(victim, rate)
        runs = []
        for i in range(len(S.specs)):
            X, Ws = S.write(step, i)
            if mode == "X":
                runs.append(pipe.run(Ws, X))
                continue
            S.Gbuf[i].copy_(S.G[step][i])
            N = S.specs[i][2]
            if mode == "G":
                runs.append(pipe.run(Ws, G=S.Gbuf[i], nsamples=N))
            elif mode == "Hinv":
                Hbuf, ibuf = extra["buf"][i]
                Hbuf.copy_(extra["Hinv"][step][i])
                ibuf.copy_(extra["info"][step][i])
                runs.append(pipe.run(Ws, G=S.Gbuf[i], nsamples=N, Hinv=Hbuf, info=ibuf))
            else:
                sbuf = extra["buf"][i]
                sbuf.copy_(extra["s1d"][step][i])
                runs.append(pipe.run(Ws, G=S.Gbuf[i], nsamples=N, s1d=sbuf))
        outs = [r.finish() for r in runs]
        got = [[{f: getattr(o, f).clone() for f in FIELDS} for o in uo] for uo in outs]  # on the caller's stream
    caller.synchronize()
    return got


@pytest.mark.parametrize("mode", ["X", "G", "Hinv", "s1d"])
@pytest.mark.parametrize("lanes", [2, 3])
def test_unit_pipeline_with_a_delayed_stream(pt2q, steps, cycles_per_ms, lanes, mode):  # noqa: F811
    """run(Ws, X), run(Ws, G=, nsamples=), run(..., Hinv=, info=) and run(..., s1d=) with each lane
    delayed in turn, then the caller."""
    S = steps("pc" if mode == "s1d" else "blocks")
    extra = None
    if mode == "Hinv":
        inv = [[pt2q.engine.hessian_inverse_batched(G[None].contiguous(), S.specs[i][2], 0.01)
                for i, G in enumerate(Gs)] for Gs in S.G]
        extra = {"Hinv": [[h[0] for h, _ in st] for st in inv], "info": [[f for _, f in st] for st in inv]}
        extra["buf"] = [(torch.empty_like(h), torch.empty_like(f)) for h, f in zip(extra["Hinv"][0], extra["info"][0])]
    elif mode == "s1d":
        extra = {"s1d": [[pt2q.engine.s1_from_gram_batched(G[None].contiguous())[0] for G in Gs] for Gs in S.G]}
        extra["buf"] = [torch.empty_like(v) for v in extra["s1d"][0]]
    torch.cuda.synchronize()
    pipe = pt2q.UnitPipeline(DEV, S.bs, True, lanes=lanes)
    caller = torch.cuda.Stream()
    for name, victim in [("lane %d" % j, ln.stream) for j, ln in enumerate(pipe.lanes)] + [("the caller", caller)]:
        got = pipeline_step(pt2q, pipe, S, 0, mode, extra, None, cycles_per_ms, caller)
        for i, outs in enumerate(got):
            S.check(0, i, outs)
        got = pipeline_step(pt2q, pipe, S, 1, mode, extra, victim, cycles_per_ms, caller)
        try:
            for i, outs in enumerate(got):
                S.check(1, i, outs)
        except AssertionError as e:
            raise AssertionError("with %s delayed: %s" % (name, str(e)[:300])) from None


# ------------------------------------------------------------------ GramsFirst

def sharded_step(sharding, gf, S, units, step, victim, rate, caller):
    """One quantize_units_sharded step whose provider writes the step's inputs on the caller's
    stream; victim as in pipeline_step."""
    def provider(u):
        i = int(u[0][1:])
        X, Ws = S.write(step, i)
        return X, {"p%d" % k: W for k, W in enumerate(Ws)}
    with torch.cuda.stream(caller):
        if victim is not None:
            delayed(victim, rate)
        res, _ = sharding.quantize_units_sharded(units, provider, block_size=S.bs, pack=False, grams_first=gf)
        got = {k: {f: v.clone() for f, v in r.items() if f in FIELDS} for k, r in res.items()}
    caller.synchronize()
    return got


def phased_step(gf, S, units, step, victim, rate, caller):
    """The same step through GramsFirst's own phase calls, in quantize_units_sharded's order, with
    the victim put to sleep AFTER begin(): begin() joins the S1 / d streams of the previous step
    into the caller's stream, so a delay placed on one of them before it only delays the caller
    and every later edge is met by arrival order."""
    with torch.cuda.stream(caller):
        data = [S.write(step, i) for i in range(len(units))]
        gf.begin([(i, u[1][0][2], u[2]) for i, u in enumerate(units)])
        delayed(victim, rate)
        for i, (X, _) in enumerate(data):
            gf.gram(i, X)
        gf.flush()
        gf.inverses()
        jobs = [(i, data[i][1], u[2]) for i, u in enumerate(units)]
        runs = gf.tails(jobs) if gf.grouped else [gf.tail(i, Ws, N) for i, Ws, N in jobs]
        outs = [r.finish() for r in runs]
        gf.check()
        got = {"%s.p%d" % (u[0], k): {f: getattr(o, f).clone() for f in FIELDS}
               for u, uo in zip(units, outs) for k, o in enumerate(uo)}
    caller.synchronize()
    return got


def check_sharded(S, units, step, got):
    for i, (name, lins, _) in enumerate(units):
        for k, ((p, _, _), r) in enumerate(zip(lins, S.want[step][i])):
            o = got["%s.%s" % (name, p)]
            for f in ("alpha", "mu", "T", "perm"):
                assert bits_equal(host(o[f]), host(getattr(r, f))), (step, name, p, f)


def grams_first_victims(gf, caller):
    side = [ln.stream for ln in gf.pipe.lanes] + ([gf.inv_stream] if gf.inv_stream is not None else [])
    return [("caller", caller)] + [("side%d" % j, s) for j, s in enumerate(side + gf._istreams + gf._s1_streams)]


def run_grams_first(pt2q, S, rate, shift=0, **kw):
    sharding = importlib.import_module("pt2q.sharding")
    units = [("u%d" % i, [("p%d" % k, n, m) for k, n in enumerate(ns)], N) for i, (m, ns, N, _) in enumerate(S.specs)]
    pipe = pt2q.UnitPipeline(DEV, S.bs, True, lanes=3)
    gf = sharding.GramsFirst(pipe, DEV, **kw)
    caller = torch.cuda.Stream()
    spare = [torch.cuda.Stream() for _ in range(shift)]  # noqa: F841 (see the per-channel test)
    check_sharded(S, units, 0, sharded_step(sharding, gf, S, units, 0, None, rate, caller))
    victims = grams_first_victims(gf, caller)  # every stream exists after step 1
    for j, (name, victim) in enumerate(victims):
        if j:  # refill every slot and workspace with step-1 data
            check_sharded(S, units, 0, sharded_step(sharding, gf, S, units, 0, None, rate, caller))
        got = sharded_step(sharding, gf, S, units, 1, victim, rate, caller)
        try:
            check_sharded(S, units, 1, got)
        except AssertionError as e:
            raise AssertionError("with %s delayed: %s" % (name, str(e)[:300])) from None
    for j, victim in enumerate(gf._s1_streams):
        check_sharded(S, units, 0, sharded_step(sharding, gf, S, units, 0, None, rate, caller))
        got = phased_step(gf, S, units, 1, victim, rate, caller)
        try:
            check_sharded(S, units, 1, got)
        except AssertionError as e:
            raise AssertionError("with S1 / d stream %d delayed after begin(): %s" % (j, str(e)[:300])) from None
    return gf, victims


@pytest.mark.parametrize("kw", [dict(batched=False), dict(batched=True, group=1), dict(batched=True, group=16),
                                dict(batched=True, inv_streams=3), dict(batched=True, overlap=True)],
                         ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_grams_first_with_a_delayed_stream(pt2q, steps, cycles_per_ms, kw):  # noqa: F811
    """quantize_units_sharded through GramsFirst with the caller, every lane, the inverse stream
    (overlap=True, bench.py --inverse-overlap) and every inverse-chunk stream delayed in turn."""
    gf, victims = run_grams_first(pt2q, steps("blocks"), cycles_per_ms, **kw)
    assert len(victims) == 4 + (kw.get("overlap", False)) + (min(3, len(gf._istreams)) if "inv_streams" in kw else 0)
    if "inv_streams" in kw:
        assert len(gf._istreams) >= 2
    if kw.get("overlap"):
        assert gf.inv_stream is not None and gf.inv_done


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("group", [16, 1])
def test_grams_first_per_channel_with_a_delayed_stream(pt2q, steps, cycles_per_ms, group, shift):  # noqa: F811
    """Per-channel steps (block_size >= m, bf16, two widths): the S1 / d streams and the s1_done
    events are in play; the caller, the lanes and each S1 / d stream delayed in turn, and each
    S1 / d stream once more after begin() (phased_step): only then does a lane's loop reach its
    s1_done wait while the S1 / d launch pair is still held back.

    shift: streams share hardware queues (four by default), and a sleeping stream holds back every
    stream on its queue, which orders a lane behind an S1 / d stream by accident.  The S1 / d
    streams are created in the first step; taking `shift` streams from torch's pool before it moves
    them against the lanes, so that over the four values no lane stays paired with the stream whose
    S1 / d it reads."""
    gf, victims = run_grams_first(pt2q, steps("pc"), cycles_per_ms, shift=shift, batched=True, group=group)
    assert len(gf._s1_streams) == 2 and len(gf.s1_done) == 2 and len(victims) == 6
