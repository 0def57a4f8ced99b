"""Time the grouped skinny calls against the separate skinny calls they replace, 2-64 tokens (dev tool):
python tools/time_ternary_skinny_group.py [--out FILE] [--resources FILE] [hidden inter ...]

For each hidden / intermediate size (default: Llama-2-7B 4096 / 11008 and 13B 5120 / 13824; block
128, random codes, random permutations, bias), fp16 / bf16 and each token count in 2, 4, 8, 16, 32, 64:
  MLP    parent   down(silu(gate(x)) * up(x)) over three TernaryLinear(decode="skinny"): three
                  pt2q_ternary_skinny calls (six launches) and the torch silu and mul kernels
         two      TernaryGatedMLP over the same children with skinny_mlp_max_tokens at the library
                  cap: pt2q_ternary_skinny_group (SWIGLU) and pt2q_ternary_skinny (four launches)
  q/k/v  parent   three pt2q_ternary_skinny calls on hidden x hidden layers
         group    one pt2q_ternary_skinny_group (PLAIN) of the three
by the method and with the helpers of tools/time_ternary_mlp.py (hipGraph windows of CALLS calls
over a ring of RING_BYTES of packed layers, median/minimum over WINDOWS windows, µs per call).  The
series alternate in one process as parent(A), new(A), parent(B), new(B); A and B repeat the same
thing, and the larger of their two differences is the spread a margin has to beat.  margin = the
smaller parent median - the larger new median; verdict `ok` when it is positive and above the
spread.  Before timing the outputs are compared: q/k/v bit for bit, the MLP at the tolerances of
tests/test_gpu_ternary.py (the two differ where SWIGLU16 and torch's SiLU round differently)."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_ternary_mlp as base  # noqa: E402

pt2q, L, DEV = base.pt2q, base.L, base.DEV
TOKENS = (2, 4, 8, 16, 32, 64)


def abab(parent, new, x):
    gp, gn = base.captured(parent, x), base.captured(new, x)
    for _ in range(2):  # warm-up of every timed path
        gp.replay(), gn.replay()
    t = base.series([("a", gp.replay), ("n", gn.replay), ("b", gp.replay), ("n2", gn.replay)])
    margin = min(t["a"][0], t["b"][0]) - max(t["n"][0], t["n2"][0])
    spread = max(abs(t["a"][0] - t["b"][0]), abs(t["n"][0] - t["n2"][0]))
    return t, margin, spread, margin > spread and margin > 0


def skinny_linear(n, m, dt, g):
    lay = base.make_linear(n, m, dt, g)
    lay.decode = "skinny"
    return lay


def run(hidden, inter, say):
    say(f"hidden {hidden}, intermediate {inter}:")
    head = f"{'parent(A)':>14} {'new(A)':>14} {'parent(B)':>14} {'new(B)':>14} | {'margin':>7} {'spread':>7} {'verdict':<7}"
    say(f"  {'dtype':<5} {'tok':>3} | MLP, two calls: {head} | q/k/v, one group: {head}")
    ok_mlp, ok_qkv = {}, {}
    for dt in (torch.float16, torch.bfloat16):
        g = torch.Generator(device=DEV).manual_seed(hidden + inter)
        mlps = base.ring_of((skinny_linear(inter, hidden, dt, g), skinny_linear(inter, hidden, dt, g),
                             skinny_linear(hidden, inter, dt, g)))
        qkvs = base.ring_of(tuple(skinny_linear(hidden, hidden, dt, g) for _ in range(3)))
        mlp_parent = [lambda x, c=c: c[2](F.silu(c[0](x)) * c[1](x)) for c in mlps]
        mlp_two = [pt2q.TernaryGatedMLP(*c) for c in mlps]
        qkv_parent = [lambda x, c=c: (c[0](x), c[1](x), c[2](x)) for c in qkvs]
        qkv_group = [lambda x, c=c: pt2q.ternary_skinny_group(x, list(c)) for c in qkvs]
        for tokens in TOKENS:
            x = torch.randn((tokens, hidden), device=DEV, generator=g).to(dt)
            yp, yt = mlp_parent[0](x).float(), mlp_two[0](x).float()
            rtol, atol = (2e-3, 2e-3) if dt == torch.float16 else (1.6e-2, 1e-2)
            bad = (yt - yp).abs() > atol + rtol * yp.abs()
            if bool(bad.any()):
                raise SystemExit(f"MLP outputs differ: {hidden} / {inter}, {tokens} tokens, {dt}: {int(bad.sum())} "
                                 f"elements, max |diff| {float((yt - yp).abs().max()):.3e}")
            if not all(torch.equal(a, b) for a, b in zip(qkv_parent[0](x), qkv_group[0](x))):
                raise SystemExit(f"q/k/v outputs differ: {hidden}, {tokens} tokens, {dt}")
            rm, rq = abab(mlp_parent, mlp_two, x), abab(qkv_parent, qkv_group, x)
            ok_mlp[(dt, tokens)], ok_qkv[(dt, tokens)] = rm[3], rq[3]
            cells = lambda r: " ".join(f"{r[0][k][0]:7.2f}/{r[0][k][1]:6.2f}" for k in ("a", "n", "b", "n2")) + \
                f" | {r[1]:7.2f} {r[2]:7.2f} {'ok' if r[3] else 'NOT ok':<7}"  # noqa: E731
            say(f"  {'fp16' if dt == torch.float16 else 'bf16':<5} {tokens:>3} | MLP, two calls: {cells(rm)} | "
                f"q/k/v, one group: {cells(rq)}")
        del mlps, qkvs, mlp_parent, mlp_two, qkv_parent, qkv_group
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
    cap = int(L.lib().pt2q_ternary_skinny_max_tokens())
    shipped = pt2q.ternary.skinny_mlp_max_tokens
    # every call of 2 .. 64 tokens on the skinny kernels, the module routing on up to the cap
    pt2q.ternary.decode_max_tokens, pt2q.ternary.mlp_decode_max_tokens = 0, 0
    pt2q.ternary.skinny_max_tokens = pt2q.ternary.skinny_mlp_max_tokens = cap

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if res:  # the compiler's kernel-resource-usage figures, kept by whoever built the library
        for ln in open(res).read().splitlines():
            say(ln)
    say(f"{L.version()} on {torch.cuda.get_device_name(0)}; µs per call (one MLP forward, one q/k/v set) as median/min "
        f"of {base.WINDOWS} hipGraph windows of {base.CALLS} calls between one pair of HIP events; ring of "
        f"{base.RING_BYTES >> 20} MiB of packed layers; modules measured up to the library cap of {cap} tokens (shipped "
        f"ternary.skinny_mlp_max_tokens = {shipped}); eager (uncaptured) calls not measured")
    ok_mlp, ok_qkv = {}, {}
    for hidden, inter in shapes:
        a, b = run(hidden, inter, say)
        for acc, part in ((ok_mlp, a), (ok_qkv, b)):
            for k, v in part.items():
                acc[k[1]] = acc.get(k[1], True) and v
    for name, ok in (("two-call MLP", ok_mlp), ("grouped q/k/v", ok_qkv)):
        holds = [t for t in TOKENS if all(ok.get(u, False) for u in TOKENS if u <= t)]
        say(f"{name} below the parent path by more than the spread at every shape and dtype for tokens in "
            f"{holds or 'none'}; largest such count: {max(holds) if holds else 0}")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
