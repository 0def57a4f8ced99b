"""Time the fused gated MLP and the grouped q/k/v call against the per-projection decode calls they
replace (dev tool): python tools/time_ternary_mlp.py [--out FILE] [--resources FILE] [hidden inter ...]

For each hidden / intermediate size (default: Llama-2-7B 4096 / 11008 and 13B 5120 / 13824; block
128, random codes, random permutations, bias), fp16 / bf16 and each token count in 1, 2, 4, 8:
  MLP    parent   down(silu(gate(x)) * up(x)) over three TernaryLinear(decode="fused") with
                  decode_max_tokens at the library cap: three pt2q_ternary_decode launches and the
                  torch silu and mul kernels -- what a decode="fused" model ran before
         fused    TernaryGatedMLP: pt2q_ternary_decode_group (SWIGLU) and pt2q_ternary_decode
  q/k/v  parent   three pt2q_ternary_decode calls on hidden x hidden layers
         group    one pt2q_ternary_decode_group (PLAIN) of the three
Windows of CALLS back-to-back calls captured once into a hipGraph (one stream, a plain chain) and
replayed between one pair of HIP events: device time, what a captured decode step pays.  The series
alternate in one process as parent(A), new, parent(B); the two parent series repeat the same
thing, and their difference is the spread a margin has to beat.  Per call, median/minimum over
WINDOWS windows, in µs.  The calls of a window walk a ring of layers with their own packed buffers,
RING_BYTES in all, so the codes come from HBM as in a decoder step, not from the Infinity Cache.
Before timing the outputs are compared: q/k/v bit for bit, the MLP at the tolerances of
tests/test_gpu_ternary.py (the two differ where SWIGLU16 and torch's SiLU round differently).
verdict: `ok` when the new median is below both parent medians by more than their spread."""
import copy
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pt2q_loader  # noqa: E402

pt2q = pt2q_loader.load()
L = pt2q._lib
DEV = torch.device("cuda", 0)
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
    """A hipGraph of CALLS calls on x, taking the callables of `ring` in turn."""
    ring[0](x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(CALLS):
            ring[i % len(ring)](x)
    return g


def make_linear(n, m, dt, g):
    B = -(-m // 128)
    lay = pt2q.TernaryLinear(m, n, 128, bias=True, dtype=dt, decode="fused")
    lay.set_quantized_params(torch.rand((n, B), device=DEV, generator=g) * 0.05 + 0.005,
                             torch.randn((n, B), device=DEV, generator=g) * 0.002,
                             torch.randint(-1, 2, (n, m), device=DEV, generator=g, dtype=torch.int8),
                             torch.randperm(m, device=DEV, generator=g), torch.randn(n, device=DEV, generator=g) * 0.1)
    lay._prepare()
    return lay


def ring_of(layers):
    """Copies of the tuple `layers` with their own packed buffers, RING_BYTES in all."""
    per = sum(t.numel() * t.element_size() for lay in layers for t in lay._packed)
    out = []
    for _ in range(-(-RING_BYTES // per)):
        cs = []
        for lay in layers:
            c = copy.copy(lay)
            c._packed = tuple(t.clone() for t in lay._packed)
            cs.append(c)
        out.append(tuple(cs))
    return out


def abba(parent, new, x):
    gp, gn = captured(parent, x), captured(new, x)
    for _ in range(2):  # warm-up of every timed path
        gp.replay(), gn.replay()
    t = series([("a", gp.replay), ("n", gn.replay), ("b", gp.replay)])
    margin = min(t["a"][0], t["b"][0]) - t["n"][0]
    spread = abs(t["a"][0] - t["b"][0])
    return t, margin, spread, margin > spread and margin > 0


def run(hidden, inter, say):
    say(f"hidden {hidden}, intermediate {inter}:")
    say(f"  {'dtype':<5} {'tok':>3} | {'MLP: parent(A)':>16} {'fused':>14} {'parent(B)':>14} | {'margin':>7} {'spread':>7} "
        f"{'verdict':<7} | {'q/k/v: parent(A)':>16} {'group':>14} {'parent(B)':>14} | {'margin':>7} {'spread':>7} {'verdict':<7}")
    ok_mlp, ok_qkv = {}, {}
    for dt in (torch.float16, torch.bfloat16):
        g = torch.Generator(device=DEV).manual_seed(hidden + inter)
        mlps = ring_of((make_linear(inter, hidden, dt, g), make_linear(inter, hidden, dt, g),
                        make_linear(hidden, inter, dt, g)))
        qkvs = ring_of(tuple(make_linear(hidden, hidden, dt, g) for _ in range(3)))
        mlp_parent = [lambda x, c=c: c[2](F.silu(c[0](x)) * c[1](x)) for c in mlps]
        mlp_fused = [pt2q.TernaryGatedMLP(*c) for c in mlps]
        qkv_parent = [lambda x, c=c: (c[0](x), c[1](x), c[2](x)) for c in qkvs]
        qkv_group = [lambda x, c=c: pt2q.ternary_decode_group(x, list(c)) for c in qkvs]
        for tokens in TOKENS:
            x = torch.randn((tokens, hidden), device=DEV, generator=g).to(dt)
            yp, yf = mlp_parent[0](x).float(), mlp_fused[0](x).float()
            rtol, atol = (2e-3, 2e-3) if dt == torch.float16 else (1.6e-2, 1e-2)
            bad = (yf - yp).abs() > atol + rtol * yp.abs()
            if bool(bad.any()):
                raise SystemExit(f"MLP outputs differ: {hidden} / {inter}, {tokens} tokens, {dt}: {int(bad.sum())} "
                                 f"elements, max |diff| {float((yf - yp).abs().max()):.3e}")
            if not all(torch.equal(a, b) for a, b in zip(qkv_parent[0](x), qkv_group[0](x))):
                raise SystemExit(f"q/k/v outputs differ: {hidden}, {tokens} tokens, {dt}")
            tm, mm, sm, okm = abba(mlp_parent, mlp_fused, x)
            tq, mq, sq, okq = abba(qkv_parent, qkv_group, x)
            ok_mlp[(dt, tokens)], ok_qkv[(dt, tokens)] = okm, okq
            cell = lambda t: f"{t[0]:7.2f}/{t[1]:6.2f}"  # noqa: E731
            say(f"  {'fp16' if dt == torch.float16 else 'bf16':<5} {tokens:>3} | {cell(tm['a']):>16} {cell(tm['n']):>14} "
                f"{cell(tm['b']):>14} | {mm:7.2f} {sm:7.2f} {'ok' if okm else 'NOT ok':<7} | {cell(tq['a']):>16} "
                f"{cell(tq['n']):>14} {cell(tq['b']):>14} | {mq:7.2f} {sq:7.2f} {'ok' if okq else 'NOT ok':<7}")
        del mlps, qkvs, mlp_parent, mlp_fused, qkv_parent, qkv_group
        torch.cuda.empty_cache()
    return ok_mlp, ok_qkv


def main(argv):
    out = res = None
    while argv[:1] and argv[0] in ("--out", "--resources"):
        if argv[0] == "--out":
            out = argv[1]
        else:
            res = argv[1]
        argv = argv[2:]
    shapes = [(int(argv[i]), int(argv[i + 1])) for i in range(0, len(argv), 2)] or [(4096, 11008), (5120, 13824)]
    lines = []
    cap = int(L.lib().pt2q_ternary_decode_max_tokens())
    shipped = pt2q.ternary.mlp_decode_max_tokens
    pt2q.ternary.decode_max_tokens = pt2q.ternary.mlp_decode_max_tokens = cap  # measure up to the cap

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if res:  # the compiler's kernel-resource-usage figures, kept by whoever built the library
        for ln in open(res).read().splitlines():
            say(ln)
    say(f"{L.version()} on {torch.cuda.get_device_name(0)}; µs per call (one MLP forward, one q/k/v set) as median/min "
        f"of {WINDOWS} hipGraph windows of {CALLS} calls between one pair of HIP events; ring of {RING_BYTES >> 20} MiB "
        f"of packed layers; modules measured up to the library cap of {cap} tokens (shipped "
        f"ternary.mlp_decode_max_tokens = {shipped}); eager (uncaptured) calls not measured")
    ok_mlp, ok_qkv = {}, {}
    for hidden, inter in shapes:
        a, b = run(hidden, inter, say)
        for acc, part in ((ok_mlp, a), (ok_qkv, b)):
            for k, v in part.items():
                acc[k[1]] = acc.get(k[1], True) and v
    for name, ok in (("fused MLP", ok_mlp), ("grouped q/k/v", ok_qkv)):
        holds = [t for t in TOKENS if all(ok.get(u, False) for u in TOKENS if u <= t)]
        say(f"{name} below the parent path by more than the spread at every shape and dtype for tokens in "
            f"{holds or 'none'}; largest such count: {max(holds) if holds else 0}")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
