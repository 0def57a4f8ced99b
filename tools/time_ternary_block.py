"""Time the decode kernel's RMSNorm prologue and residual epilogue against the launches they
replace (dev tool): python tools/time_ternary_block.py [--out FILE] [--resources FILE] [hidden inter ...]

For each hidden / intermediate size (default: Llama-2-7B 4096 / 11008 and 13B 5120 / 13824; block
128, random codes, random permutations, bias), fp16 / bf16 and each token count in 1, 2, 4, 8:
  block  4-launch  h + mlp(rms_norm(h)): pt2q_rmsnorm, TernaryGatedMLP (SWIGLU, down_proj) and torch's add
         fused     TernaryMLPBlock: SWIGLU with the norm prologue, down_proj with the residual epilogue
         hf-norm   the 4-launch form with the norm written as the torch ops of a Llama RMSNorm
                   (float, pow, mean, add, rsqrt, mul, to, mul) -- what an unmodified host runs
  q/k/v  2-launch  pt2q_rmsnorm, then pt2q_ternary_decode_group (PLAIN) of three hidden x hidden layers
         fused     the group with the norm prologue
Windows of CALLS back-to-back calls captured once into a hipGraph (one stream, a plain chain) and
replayed between one pair of HIP events: device time, what a captured decode step pays.  The series
alternate in one process as unfused(A), fused, unfused(B) (and hf-norm); the two unfused series
repeat the same thing, and their difference is the spread a margin has to beat.  Per call,
median/minimum over WINDOWS windows, in µs.  The calls of a window walk a ring of layers with their
own packed buffers, RING_BYTES in all, so the codes come from HBM as in a decoder step, not from
the Infinity Cache.  Before timing the fused outputs are compared with the unfused ones bit for
bit (contracts RMSNORM16 and RESADD16 make them equal).
verdict: `ok` when the fused median is below both unfused medians by more than their spread."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_ternary_mlp import CALLS, DEV, RING_BYTES, TOKENS, WINDOWS, L, captured, make_linear, pt2q, ring_of, series  # noqa: E402

EPS = 1e-5


def hf_norm(x, w, eps):
    v = x.float()
    return w * (v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype)


def abba(unfused, fused, x, extra=None):
    gu = captured(unfused, x)
    graphs = [("a", gu), ("n", captured(fused, x)), ("b", gu)]
    if extra is not None:
        graphs.append(("h", captured(extra, x)))
    for _ in range(2):  # warm-up of every timed path
        for _, g in graphs:
            g.replay()
    t = series([(k, g.replay) for k, g in graphs])
    margin = min(t["a"][0], t["b"][0]) - t["n"][0]
    spread = abs(t["a"][0] - t["b"][0])
    return t, margin, spread, margin > spread and margin > 0


def run(hidden, inter, say):
    say(f"hidden {hidden}, intermediate {inter}:")
    say(f"  {'dtype':<5} {'tok':>3} | {'block: 4-launch(A)':>18} {'fused':>14} {'4-launch(B)':>14} {'hf-norm':>14} | {'margin':>7} "
        f"{'spread':>7} {'verdict':<7} | {'q/k/v: 2-launch(A)':>18} {'fused':>14} {'2-launch(B)':>14} | {'margin':>7} {'spread':>7} "
        f"{'verdict':<7}")
    ok_blk, ok_qkv = {}, {}
    for dt in (torch.float16, torch.bfloat16):
        g = torch.Generator(device=DEV).manual_seed(hidden + inter)
        w = (1.0 + (torch.rand(hidden, device=DEV, generator=g) - 0.5)).to(dt)
        mlps = [pt2q.TernaryGatedMLP(*c) for c in ring_of((make_linear(inter, hidden, dt, g), make_linear(inter, hidden, dt, g),
                                                           make_linear(hidden, inter, dt, g)))]
        qkvs = ring_of(tuple(make_linear(hidden, hidden, dt, g) for _ in range(3)))
        blk_unfused = [lambda h, c=c: h + c(pt2q.rms_norm(h, w, EPS)) for c in mlps]
        blk_hf = [lambda h, c=c: h + c(hf_norm(h, w, EPS)) for c in mlps]
        blk_fused = [pt2q.TernaryMLPBlock(w, EPS, c) for c in mlps]
        qkv_unfused = [lambda x, c=c: pt2q.ternary_decode_group(pt2q.rms_norm(x, w, EPS), list(c)) for c in qkvs]
        qkv_fused = [lambda x, c=c: pt2q.ternary_decode_group(x, list(c), norm=(w, EPS)) for c in qkvs]
        for tokens in TOKENS:
            x = torch.randn((tokens, hidden), device=DEV, generator=g).to(dt)
            if not torch.equal(blk_unfused[0](x), blk_fused[0](x)):
                raise SystemExit(f"block outputs differ: {hidden} / {inter}, {tokens} tokens, {dt}")
            if not all(torch.equal(a, b) for a, b in zip(qkv_unfused[0](x), qkv_fused[0](x))):
                raise SystemExit(f"q/k/v outputs differ: {hidden}, {tokens} tokens, {dt}")
            tb, mb, sb, okb = abba(blk_unfused, blk_fused, x, blk_hf)
            tq, mq, sq, okq = abba(qkv_unfused, qkv_fused, x)
            ok_blk[(dt, tokens)], ok_qkv[(dt, tokens)] = okb, okq
            cell = lambda t: f"{t[0]:7.2f}/{t[1]:6.2f}"  # noqa: E731
            say(f"  {'fp16' if dt == torch.float16 else 'bf16':<5} {tokens:>3} | {cell(tb['a']):>18} {cell(tb['n']):>14} "
                f"{cell(tb['b']):>14} {cell(tb['h']):>14} | {mb:7.2f} {sb:7.2f} {'ok' if okb else 'NOT ok':<7} | {cell(tq['a']):>18} "
                f"{cell(tq['n']):>14} {cell(tq['b']):>14} | {mq:7.2f} {sq:7.2f} {'ok' if okq else 'NOT ok':<7}")
        del mlps, qkvs, blk_unfused, blk_hf, blk_fused, qkv_unfused, qkv_fused
        torch.cuda.empty_cache()
    return ok_blk, ok_qkv


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
    shipped = pt2q.ternary.block_decode_max_tokens
    # measure up to the cap, the unfused forms at their best (the two-launch MLP)
    pt2q.ternary.decode_max_tokens = pt2q.ternary.mlp_decode_max_tokens = pt2q.ternary.block_decode_max_tokens = cap

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if res:  # the compiler's kernel-resource-usage figures, kept by whoever built the library
        for ln in open(res).read().splitlines():
            say(ln)
    say(f"{L.version()} on {torch.cuda.get_device_name(0)}; µs per call (one h + mlp(norm(h)), one norm + q/k/v set) as "
        f"median/min of {WINDOWS} hipGraph windows of {CALLS} calls between one pair of HIP events; ring of "
        f"{RING_BYTES >> 20} MiB of packed layers; measured up to the library cap of {cap} tokens (shipped "
        f"ternary.block_decode_max_tokens = {shipped}); eager (uncaptured) calls not measured")
    ok_blk, ok_qkv = {}, {}
    for hidden, inter in shapes:
        a, b = run(hidden, inter, say)
        for acc, part in ((ok_blk, a), (ok_qkv, b)):
            for k, v in part.items():
                acc[k[1]] = acc.get(k[1], True) and v
    for name, ok in (("fused block below the 4-launch form", ok_blk), ("q/k/v with the norm prologue below rms_norm + group", ok_qkv)):
        holds = [t for t in TOKENS if all(ok.get(u, False) for u in TOKENS if u <= t)]
        say(f"{name} by more than the spread at every shape and dtype for tokens in {holds or 'none'}; largest such count: "
            f"{max(holds) if holds else 0}")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
