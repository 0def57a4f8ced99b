"""Time the 2-64 token ternary kernel against the MFMA path it can replace (dev tool):
python tools/time_ternary_skinny.py [--out FILE] [--resources FILE] [n m ...]

For each n x m (default: the Llama-2-7B shapes 4096 x 4096, 11008 x 4096, 4096 x 11008 and the 13B
shape 5120 x 5120; block 128, random codes, a random permutation, bias), each token count in
2, 4, 8, 16, 32, 64 and fp16 / bf16 it times
  mfma    TernaryLinear(decode="mfma")(x): pt2q_ternary_linear (gather, split-K MFMA, reduce)
  skinny  TernaryLinear(decode="skinny")(x) with the crossovers set so that the call reaches
          pt2q_ternary_skinny (gather, GEMM with the split reduced inside)
  fused   up to 8 tokens, TernaryLinear(decode="fused")(x) -> pt2q_ternary_decode, for comparison
by the method of tools/time_ternary_decode.py: CALLS calls captured once into a hipGraph, the graph
replayed between one pair of HIP events, WINDOWS windows per series after a warm-up, the calls of a
window walking a ring of layers with their own packed buffers (320 MiB in all, so codes come from
HBM).  The series alternate in one process as mfma(A), skinny(A), mfma(B), skinny(B) [, fused]: A
and B are repeats of the same thing, and the larger of their two differences is the spread a
margin has to beat.  Per call, median/minimum over the windows, in µs.  margin = the smaller mfma
median - the larger skinny median; verdict `ok` when it is positive and above the spread.  Before
timing, the two paths' outputs are compared at the tolerances of tests/test_gpu_ternary.py."""
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
CALLS = 1000
RING_BYTES = 320 << 20  # packed layers walked in turn: more than the Infinity Cache holds
WINDOWS = 7
TOKENS = (2, 4, 8, 16, 32, 64)
FUSED_CAP = int(L.lib().pt2q_ternary_decode_max_tokens())
MODES = ("mfma", "skinny", "fused")


def window_us(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / CALLS


def series(graphs):
    """{name: (median, min) µs per call}: WINDOWS rounds, each timing every graph once, in order."""
    ts = {k: [] for k, _ in graphs}
    for _ in range(WINDOWS):
        for k, g in graphs:
            ts[k].append(window_us(g))
    return {k: (statistics.median(v), min(v)) for k, v in ts.items()}


def route(mode):
    """Module crossovers under which a forward of `mode` layers reaches that mode's kernel."""
    pt2q.ternary.decode_max_tokens = FUSED_CAP if mode == "fused" else 0
    pt2q.ternary.skinny_max_tokens = int(L.lib().pt2q_ternary_skinny_max_tokens())


def captured(mode, ring, x):
    """A hipGraph of CALLS forwards on x, taking the layers of `ring` in turn (one stream, a chain)."""
    route(mode)
    ring[0](x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(CALLS):
            ring[i % len(ring)](x)
    return g


def make_layers(n, m, dt):
    g = torch.Generator(device=DEV).manual_seed(n + m)
    B = -(-m // 128)
    T = torch.randint(-1, 2, (n, m), device=DEV, generator=g, dtype=torch.int8)
    alpha = torch.rand((n, B), device=DEV, generator=g) * 0.05 + 0.005
    mu = torch.randn((n, B), device=DEV, generator=g) * 0.002
    perm = torch.randperm(m, device=DEV, generator=g)
    bias = torch.randn(n, device=DEV, generator=g) * 0.1
    layers = {}
    for mode in MODES:
        lay = pt2q.TernaryLinear(m, n, 128, bias=True, dtype=dt, decode=mode)
        lay.set_quantized_params(alpha, mu, T, perm, bias)
        lay._prepare()
        layers[mode] = lay
    per = sum(t.numel() * t.element_size() for t in layers["mfma"]._packed)
    packs = [tuple(t.clone() for t in layers["mfma"]._packed) for _ in range(-(-RING_BYTES // per))]
    rings = {}
    for mode in MODES:
        rings[mode] = []
        for pk in packs:
            lay = copy.copy(layers[mode])
            lay._packed = pk
            rings[mode].append(lay)
    return layers, rings, g


def run(n, m, say):
    say(f"{n} x {m} (n x m):")
    say(f"  {'dtype':<5} {'tok':>3} | {'mfma(A)':>14} {'skinny(A)':>14} {'mfma(B)':>14} {'skinny(B)':>14} {'fused':>14} | "
        f"{'margin':>7} {'spread':>7} {'verdict':<7}")
    ok_all = {}
    for dt in (torch.float16, torch.bfloat16):
        layers, rings, g = make_layers(n, m, dt)
        for tokens in TOKENS:
            x = torch.randn((tokens, m), device=DEV, generator=g).to(dt)
            route("mfma")
            ym = layers["mfma"](x).float()
            route("skinny")
            ys = layers["skinny"](x).float()
            rtol, atol = (2e-3, 2e-3 * max(1.0, (m / 512) ** 0.5)) if dt == torch.float16 else (1.6e-2, 1e-2)
            bad = (ys - ym).abs() > atol + rtol * ym.abs()
            if bool(bad.any()):
                raise SystemExit(f"outputs differ: {n} x {m}, {tokens} tokens, {dt}: {int(bad.sum())} elements, "
                                 f"max |diff| {float((ys - ym).abs().max()):.3e}")
            gm, gs = captured("mfma", rings["mfma"], x), captured("skinny", rings["skinny"], x)
            graphs = [("a", gm), ("s", gs), ("b", gm), ("s2", gs)]
            if tokens <= FUSED_CAP:
                graphs.append(("f", captured("fused", rings["fused"], x)))
            for _, gr in graphs[1:]:  # warm-up of every timed graph
                gr.replay()
            t = series(graphs)
            margin = min(t["a"][0], t["b"][0]) - max(t["s"][0], t["s2"][0])
            spread = max(abs(t["a"][0] - t["b"][0]), abs(t["s"][0] - t["s2"][0]))
            ok = ok_all[(dt, tokens)] = margin > spread and margin > 0
            cell = lambda k: f"{t[k][0]:7.2f}/{t[k][1]:6.2f}" if k in t else "-"  # noqa: E731
            say(f"  {'fp16' if dt == torch.float16 else 'bf16':<5} {tokens:>3} | {cell('a'):>14} {cell('s'):>14} "
                f"{cell('b'):>14} {cell('s2'):>14} {cell('f'):>14} | {margin:7.2f} {spread:7.2f} {'ok' if ok else 'NOT ok':<7}")
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
    shipped = pt2q.ternary.skinny_max_tokens

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if res:  # the compiler's kernel-resource-usage figures, kept by whoever built the library
        for ln in open(res).read().splitlines():
            say(ln)
    say(f"{L.version()} on {torch.cuda.get_device_name(0)}; µs per call as median/min of {WINDOWS} windows of {CALLS} "
        f"calls captured into one hipGraph, between one pair of HIP events; skinny measured up to the library cap of "
        f"{L.lib().pt2q_ternary_skinny_max_tokens()} tokens (shipped ternary.skinny_max_tokens = {shipped})")
    ok = {}
    for n, m in shapes:
        for k, v in run(n, m, say).items():
            ok[k[1]] = ok.get(k[1], True) and v
    holds = [t for t in TOKENS if ok.get(t, False)]
    say(f"skinny below mfma by more than the spread at every shape and dtype for tokens in {holds or 'none'}; "
        f"largest such count: {max(holds) if holds else 0}")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
