"""Time the skinny calls with the RMSNorm prologue and the residual epilogue (pt2q_ternary_skinny_fused)
against the unfused forms they replace, 2-64 tokens (dev tool):
python tools/time_ternary_skinny_block.py [--out FILE] [--resources FILE] [--parts block,qkv,oproj] [hidden inter ...]

For each hidden / intermediate size (default: Llama-2-7B 4096 / 11008 and 13B 5120 / 13824; block
128, random codes, random permutations, bias), fp16 / bf16 and each token count in 2, 4, 8, 16, 32, 64:
  block  parent   h + mlp(rms_norm(h)) with mlp a TernaryGatedMLP over decode="skinny" children, what a
                  TernaryMLPBlock over such children ran before: pt2q_rmsnorm, pt2q_ternary_skinny_group
                  (SWIGLU), pt2q_ternary_skinny and torch's add (six launches)
         two      TernaryMLPBlock with skinny_block_max_tokens at the library cap: ternary_skinny_swiglu
                  with norm=, ternary_skinny with residual= (four launches)
  qkv    parent   rms_norm, then ternary_skinny_group on three hidden x hidden layers (three launches)
         fused    ternary_skinny_group(norm=) (two launches)
  oproj  parent   h + ternary_skinny on a hidden x hidden layer (three launches)
         fused    ternary_skinny(residual=h) (two launches)
by the method and with the helpers of tools/time_ternary_mlp.py and tools/time_ternary_skinny_group.py
(hipGraph windows of CALLS calls over a ring of RING_BYTES of packed layers, median/minimum over
WINDOWS windows, µs per call; series parent(A), new(A), parent(B), new(B); margin = the smaller parent
median - the larger new median, `ok` when it is positive and above the spread of the repeats).  Before
timing the two forms' outputs are compared bit for bit."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_ternary_skinny_group as grp  # noqa: E402

base = grp.base
pt2q, L, DEV = base.pt2q, base.L, base.DEV
TOKENS = grp.TOKENS
EPS = 1e-5
PARTS = ("block", "qkv", "oproj")
TITLE = {"block": "block, two calls", "qkv": "norm + q/k/v", "oproj": "o_proj + residual"}


def forms(part, ring, w):
    """(parent callables, new callables) over the ring's layer tuples."""
    if part == "block":
        mlps = [pt2q.TernaryGatedMLP(*c) for c in ring]
        return ([lambda h, m=m: h + m(pt2q.rms_norm(h, w, EPS)) for m in mlps],
                [pt2q.TernaryMLPBlock(w, EPS, m) for m in mlps])
    if part == "qkv":
        return ([lambda h, c=c: pt2q.ternary_skinny_group(pt2q.rms_norm(h, w, EPS), list(c)) for c in ring],
                [lambda h, c=c: pt2q.ternary_skinny_group(h, list(c), norm=(w, EPS)) for c in ring])
    one = lambda c, h, **kw: pt2q.ternary_skinny(h, *c[0]._packed[:4], c[0].block_size, c[0]._packed[4], **kw)  # noqa: E731
    return ([lambda h, c=c: h + one(c, h) for c in ring], [lambda h, c=c: one(c, h, residual=h) for c in ring])


def same(a, b):
    a, b = (list(t) if isinstance(t, (list, tuple)) else [t] for t in (a, b))
    return all(torch.equal(u, v) for u, v in zip(a, b))


def run(hidden, inter, parts, say):
    say(f"hidden {hidden}, intermediate {inter}:")
    head = f"{'parent(A)':>14} {'new(A)':>14} {'parent(B)':>14} {'new(B)':>14} | {'margin':>7} {'spread':>7} {'verdict':<7}"
    say(f"  {'dtype':<5} {'tok':>3} | " + " | ".join(f"{TITLE[p]}: {head}" for p in parts))
    ok = {p: {} for p in parts}
    for dt in (torch.float16, torch.bfloat16):
        g = torch.Generator(device=DEV).manual_seed(hidden + inter)
        w = (1.0 + (torch.rand(hidden, device=DEV, generator=g) - 0.5)).to(dt)
        lin = lambda n, m: grp.skinny_linear(n, m, dt, g)  # noqa: E731
        rings = {"block": lambda: base.ring_of((lin(inter, hidden), lin(inter, hidden), lin(hidden, inter))),
                 "qkv": lambda: base.ring_of(tuple(lin(hidden, hidden) for _ in range(3))),
                 "oproj": lambda: base.ring_of((lin(hidden, hidden),))}
        fs = {p: forms(p, rings[p](), w) for p in parts}
        for tokens in TOKENS:
            h = torch.randn((tokens, hidden), device=DEV, generator=g).to(dt)
            cells = []
            for p in parts:
                parent, new = fs[p]
                if not same(parent[0](h), new[0](h)):
                    raise SystemExit(f"{p}: outputs differ: {hidden} / {inter}, {tokens} tokens, {dt}")
                r = grp.abab(parent, new, h)
                ok[p][(dt, tokens)] = r[3]
                cells.append(f"{TITLE[p]}: " + " ".join(f"{r[0][k][0]:7.2f}/{r[0][k][1]:6.2f}" for k in ("a", "n", "b", "n2")) +
                             f" | {r[1]:7.2f} {r[2]:7.2f} {'ok' if r[3] else 'NOT ok':<7}")
            say(f"  {'fp16' if dt == torch.float16 else 'bf16':<5} {tokens:>3} | " + " | ".join(cells))
        del fs
        torch.cuda.empty_cache()
    return ok


def main(argv):
    out = res = None
    parts = PARTS
    while argv[:1] and argv[0] in ("--out", "--resources", "--parts"):
        if argv[0] == "--out":
            out = argv[1]
        elif argv[0] == "--resources":
            res = argv[1]
        else:
            parts = tuple(argv[1].split(","))
        argv = argv[2:]
    shapes = [(int(argv[i]), int(argv[i + 1])) for i in range(0, len(argv), 2)] or [(4096, 11008), (5120, 13824)]
    lines = []
    cap = int(L.lib().pt2q_ternary_skinny_max_tokens())
    shipped = pt2q.ternary.skinny_block_max_tokens
    # every call of 2 .. 64 tokens on the skinny kernels, the module routing on up to the cap
    pt2q.ternary.decode_max_tokens = pt2q.ternary.mlp_decode_max_tokens = pt2q.ternary.block_decode_max_tokens = 0
    pt2q.ternary.skinny_max_tokens = pt2q.ternary.skinny_mlp_max_tokens = pt2q.ternary.skinny_block_max_tokens = cap

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if res:  # the compiler's kernel-resource-usage figures, kept by whoever built the library
        for ln in open(res).read().splitlines():
            say(ln)
    say(f"{L.version()} on {torch.cuda.get_device_name(0)}; µs per call (one block forward, one norm + q/k/v set, one "
        f"o_proj + residual) as median/min of {base.WINDOWS} hipGraph windows of {base.CALLS} calls between one pair of "
        f"HIP events; ring of {base.RING_BYTES >> 20} MiB of packed layers; modules measured up to the library cap of "
        f"{cap} tokens (shipped ternary.skinny_block_max_tokens = {shipped}); eager (uncaptured) calls not measured")
    ok = {p: {} for p in parts}
    for hidden, inter in shapes:
        for p, part in run(hidden, inter, parts, say).items():
            for k, v in part.items():
                ok[p][k[1]] = ok[p].get(k[1], True) and v
    for p in parts:
        holds = [t for t in TOKENS if all(ok[p].get(u, False) for u in TOKENS if u <= t)]
        say(f"{TITLE[p]} below the parent path by more than the spread at every shape and dtype for tokens in "
            f"{holds or 'none'}; largest such count: {max(holds) if holds else 0}")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
