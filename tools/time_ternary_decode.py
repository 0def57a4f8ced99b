"""Time the fused ternary decode kernel against the MFMA path it can replace (dev tool):
python tools/time_ternary_decode.py [--out FILE] [--resources FILE] [n m ...]

For each n x m (default: the Llama-2-7B decode shapes 4096 x 4096, 11008 x 4096, 4096 x 11008 and
the 13B shape 5120 x 5120; block 128, random codes, a random permutation, bias), each token count
in 1, 2, 4, 8 and fp16 / bf16 it times
  mfma    TernaryLinear(decode="mfma")(x): pt2q_ternary_linear (gather, split-K MFMA, reduce)
  fused   TernaryLinear(decode="fused")(x): pt2q_ternary_decode (one launch)
in windows of CALLS back-to-back calls between one pair of HIP events (one call is below an
event's resolution), WINDOWS windows per series after a warm-up.  The series alternate in the same
process as mfma(A), fused, mfma(B): the two mfma series are repeats of the same thing, and their
difference is the spread a margin has to beat.  Two kinds of window:
  graph   the CALLS calls captured once into a hipGraph and the graph replayed: device time, what
          a captured decode step pays; the verdict column rests on this one
  eager   the same calls issued from Python (module forward, ctypes): host-bound at these sizes,
          reported for what an uncaptured caller sees
Per call, median and minimum over the windows, in µs.  GB/s counts the bytes the layer needs once
(2-bit codes + fp32 scales + bias + x + y) over the fused graph median, beside the 8 TB/s HBM peak
of MI355X_MICROARCH.md (6.3 TB/s measured by a copy).  The calls of a window walk a ring of layers
with their own packed buffers, 320 MiB in all, so the codes come from HBM as in a decoder step, not
from the Infinity Cache.  Before timing, the two paths' outputs
are compared at the tolerances of tests/test_gpu_ternary.py.  verdict: `ok` when the fused median
is below both mfma medians by more than their spread."""
import copy
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pt2q_loader  # noqa: E402

pt2q = pt2q_loader.load()
L = pt2q._lib
DEV = torch.device("cuda", 0)
HBM_PEAK_TBS = 8.0
CALLS = 1000
RING_BYTES = 320 << 20  # packed layers walked in turn: more than the Infinity Cache holds
WINDOWS = 7
TOKENS = (1, 2, 4, 8)


def window_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def series(fns):
    """{name: (median, min) µs per call}: WINDOWS rounds, each timing every fn once, in order."""
    ts = {k: [] for k, _ in fns}
    for _ in range(WINDOWS):
        for k, fn in fns:
            ts[k].append(window_ms(fn) * 1e3 / CALLS)
    return {k: (statistics.median(v), min(v)) for k, v in ts.items()}


def captured(ring, x):
    """A hipGraph of CALLS forwards on x, taking the layers of `ring` in turn (one stream, a
    plain chain), and the same calls as a Python function."""
    def calls():
        for i in range(CALLS):
            ring[i % len(ring)](x)
    ring[0](x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        calls()
    return g, calls


def make_layers(n, m, dt):
    g = torch.Generator(device=DEV).manual_seed(n + m)
    B = -(-m // 128)
    T = torch.randint(-1, 2, (n, m), device=DEV, generator=g, dtype=torch.int8)
    alpha = torch.rand((n, B), device=DEV, generator=g) * 0.05 + 0.005
    mu = torch.randn((n, B), device=DEV, generator=g) * 0.002
    perm = torch.randperm(m, device=DEV, generator=g)
    bias = torch.randn(n, device=DEV, generator=g) * 0.1
    layers = {}
    for mode in ("mfma", "fused"):
        lay = pt2q.TernaryLinear(m, n, 128, bias=True, dtype=dt, decode=mode)
        lay.set_quantized_params(alpha, mu, T, perm, bias)
        lay._prepare()
        layers[mode] = lay
    # a ring of layers with their own copies of the packed buffers, RING_BYTES in all: a decoder
    # step walks through ~1.7 GB of distinct layers, so no call finds its codes in the 256 MiB
    # Infinity Cache; the ring is walked the same way by both paths
    per = sum(t.numel() * t.element_size() for t in layers["mfma"]._packed)
    packs = [tuple(t.clone() for t in layers["mfma"]._packed) for _ in range(-(-RING_BYTES // per))]
    rings = {}
    for mode in ("mfma", "fused"):
        rings[mode] = []
        for pk in packs:
            lay = copy.copy(layers[mode])
            lay._packed = pk
            rings[mode].append(lay)
    return layers, rings, g


def run(n, m, say):
    say(f"{n} x {m} (n x m):")
    say(f"  {'dtype':<5} {'tok':>3} | {'graph: mfma(A)':>16} {'fused':>14} {'mfma(B)':>14} | {'margin':>7} {'spread':>7} "
        f"{'verdict':<7} | {'eager: mfma(A)':>16} {'fused':>14} {'mfma(B)':>14} | {'fused GB/s':>10}")
    ok_all = {}
    for dt in (torch.float16, torch.bfloat16):
        layers, rings, g = make_layers(n, m, dt)
        for tokens in TOKENS:
            x = torch.randn((tokens, m), device=DEV, generator=g).to(dt)
            ym, yf = layers["mfma"](x).float(), layers["fused"](x).float()
            rtol, atol = (2e-3, 2e-3 * max(1.0, (m / 512) ** 0.5)) if dt == torch.float16 else (1.6e-2, 1e-2)
            bad = (yf - ym).abs() > atol + rtol * ym.abs()
            if bool(bad.any()):
                raise SystemExit(f"outputs differ: {n} x {m}, {tokens} tokens, {dt}: {int(bad.sum())} elements, "
                                 f"max |diff| {float((yf - ym).abs().max()):.3e}")
            gm, cm = captured(rings["mfma"], x)
            gf, cf = captured(rings["fused"], x)
            for _ in range(2):  # warm-up of every timed path
                gm.replay(), gf.replay(), cm(), cf()
            tg = series([("a", gm.replay), ("f", gf.replay), ("b", gm.replay)])
            te = series([("a", cm), ("f", cf), ("b", cm)])
            margin = min(tg["a"][0], tg["b"][0]) - tg["f"][0]
            spread = abs(tg["a"][0] - tg["b"][0])
            ok = margin > spread and margin > 0
            ok_all[(dt, tokens)] = ok
            P = -(-m // 128) * 128
            nbytes = n * P // 4 + 2 * n * (-(-m // 128)) * 4 + n * 4 + tokens * m * 2 + tokens * n * 2
            cell = lambda t: f"{t[0]:7.2f}/{t[1]:6.2f}"  # noqa: E731
            say(f"  {'fp16' if dt == torch.float16 else 'bf16':<5} {tokens:>3} | {cell(tg['a']):>16} {cell(tg['f']):>14} "
                f"{cell(tg['b']):>14} | {margin:7.2f} {spread:7.2f} {'ok' if ok else 'NOT ok':<7} | {cell(te['a']):>16} "
                f"{cell(te['f']):>14} {cell(te['b']):>14} | {nbytes / (tg['f'][0] * 1e-6) / 1e9:10.0f}")
    return ok_all


def main(argv):
    out = res = None
    while argv[:1] and argv[0] in ("--out", "--resources"):
        if argv[0] == "--out":
            out = argv[1]
        else:
            res = argv[1]
        argv = argv[2:]
    shapes = [(int(argv[i]), int(argv[i + 1])) for i in range(0, len(argv), 2)] or \
        [(4096, 4096), (11008, 4096), (4096, 11008), (5120, 5120)]
    lines = []
    shipped = pt2q.ternary.decode_max_tokens
    pt2q.ternary.decode_max_tokens = L.lib().pt2q_ternary_decode_max_tokens()  # measure up to the cap

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if res:  # the compiler's kernel-resource-usage figures, kept by whoever built the library
        for ln in open(res).read().splitlines():
            say(ln)
    say(f"{L.version()} on {torch.cuda.get_device_name(0)}; µs per call as median/min of {WINDOWS} windows of {CALLS} "
        f"calls between one pair of HIP events; HBM peak {HBM_PEAK_TBS:.1f} TB/s = {HBM_PEAK_TBS * 1e3:.0f} GB/s; "
        f"fused modules measured up to the library cap of {L.lib().pt2q_ternary_decode_max_tokens()} tokens "
        f"(shipped ternary.decode_max_tokens = {shipped})")
    ok = {}
    for n, m in shapes:
        for k, v in run(n, m, say).items():
            ok[k[1]] = ok.get(k[1], True) and v
    holds = [t for t in TOKENS if all(ok.get(u, False) for u in TOKENS if u <= t)]
    say(f"fused below mfma by more than the spread at every shape and dtype for tokens in {holds or 'none'}; "
        f"largest such count: {max(holds) if holds else 0}")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
