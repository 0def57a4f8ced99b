"""Time the grouped prefill calls against what they replace (dev tool):
python tools/time_ternary_prefill.py [--out FILE] [--resources FILE] [--parent-lib libpt2q.so] [hidden inter ...]
python tools/time_ternary_prefill.py --lone LIB          (the child process of comparison (c))

For each hidden / inter (default: 4096 / 11008 and 5120 / 13824; block 128, random codes, random
permutations, bias), fp16 / bf16 and 128, 256, 512, 1024, 2048, 4096 tokens:
  (a) mlp   down(ternary_prefill_swiglu(x, gate, up))  against  down(F.silu(gate(x)) * up(x)), same children
  (b) qkv   ternary_prefill_group(x, [q, k, v]) on three hidden x hidden members  against  q(x), k(x), v(x)
  (c) lone  pt2q_ternary_linear on inter x hidden at 256 .. 4096 tokens in this tree's library against the
            same call in --parent-lib (a library built from the parent commit), each in a process of its
            own that binds the C entry by ctypes, the processes alternating parent, this, parent, this
by the method of tools/time_ternary_skinny.py: the calls of a window captured once into a hipGraph and
replayed between one pair of HIP events, WINDOWS windows per series after a warm-up, the series
alternating A, B, A, B in one process.  A window's call count is sized from one eager call so that a
window lasts about WINDOW_MS.  Per call, median/minimum over the windows, in µs.  margin = the smaller
old-form median - the larger new-form median; spread = the larger difference between the two repeats of
the same series; verdict `ok` when the margin is positive and above the spread.  (c) is `level` when
|difference of the medians' means| is within the spread."""
import ctypes
import json
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
WINDOWS = 7
WINDOW_MS = 30.0
TOKENS = (128, 256, 512, 1024, 2048, 4096)
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def window_us(g, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def captured(fn):
    """(hipGraph of `calls` calls of fn, calls): calls sized so that a replay lasts about WINDOW_MS."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    calls = max(4, min(1000, int(WINDOW_MS / max(e0.elapsed_time(e1), 1e-3))))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    g.replay()  # warm-up
    return g, calls


def series(graphs):
    """{name: (median, min) µs per call}: WINDOWS rounds, each timing every graph once, in order."""
    ts = {k: [] for k, _ in graphs}
    for _ in range(WINDOWS):
        for k, (g, calls) in graphs:
            ts[k].append(window_us(g, calls))
    return {k: (statistics.median(v), min(v)) for k, v in ts.items()}


def ab(old, new):
    """old(A), new(A), old(B), new(B) -> the four cells, margin, spread."""
    go, gn = captured(old), captured(new)
    t = series([("a", go), ("n", gn), ("b", go), ("n2", gn)])
    margin = min(t["a"][0], t["b"][0]) - max(t["n"][0], t["n2"][0])
    spread = max(abs(t["a"][0] - t["b"][0]), abs(t["n"][0] - t["n2"][0]))
    return t, margin, spread


def params(n, m, g):
    B = -(-m // 128)
    return (torch.rand((n, B), device=DEV, generator=g) * 0.05 + 0.005, torch.randn((n, B), device=DEV, generator=g) * 0.002,
            torch.randint(-1, 2, (n, m), device=DEV, generator=g, dtype=torch.int8), torch.randperm(m, device=DEV, generator=g),
            torch.randn(n, device=DEV, generator=g) * 0.1)


def lone_child(so):
    """Comparison (c), one library: JSON {"dtype tokens": median µs} of pt2q_ternary_linear, bound by ctypes."""
    h = ctypes.CDLL(so)
    P_, I_, L_, Z_ = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    h.pt2q_ternary_linear_positions.restype = Z_
    h.pt2q_ternary_linear_workspace_bytes.restype = Z_
    h.pt2q_ternary_pack.argtypes = [P_, L_, I_, I_, P_, I_, P_, P_, P_]
    h.pt2q_ternary_linear.argtypes = [P_, I_, I_, L_, I_, I_, P_, P_, P_, P_, I_, I_, P_, P_, I_, L_, P_, Z_, P_]
    n, m = 11008, 4096
    g = torch.Generator(device=DEV).manual_seed(n + m)
    alpha, mu, T, perm, bias = params(n, m, g)
    P = int(h.pt2q_ternary_linear_positions(m))
    codes = torch.empty((n, P // 4), dtype=torch.uint8, device=DEV)
    gather = torch.empty(P, dtype=torch.int32, device=DEV)
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)  # noqa: E731
    assert h.pt2q_ternary_pack(T.data_ptr(), m, n, m, perm.data_ptr(), 0, codes.data_ptr(), gather.data_ptr(), st()) == 0
    out = {}
    for name, dt in DT.items():
        a32, m32 = alpha.to(dt).float().contiguous(), mu.to(dt).float().contiguous()
        for tokens in TOKENS[1:]:
            x = torch.randn((tokens, m), device=DEV, generator=g).to(dt)
            y = torch.empty((tokens, n), dtype=dt, device=DEV)
            ws = torch.empty(int(h.pt2q_ternary_linear_workspace_bytes(tokens, n, m)), dtype=torch.uint8, device=DEV)

            def call():
                rc = h.pt2q_ternary_linear(x.data_ptr(), 1 if dt == torch.float16 else 2, tokens, m, n, m, codes.data_ptr(),
                                           gather.data_ptr(), a32.data_ptr(), m32.data_ptr(), a32.shape[1], 128,
                                           bias.data_ptr(), y.data_ptr(), 1 if dt == torch.float16 else 2, n, ws.data_ptr(),
                                           ws.numel(), st())
                assert rc == 0, rc
            gr = captured(call)
            out[f"{name} {tokens}"] = series([("t", gr)])["t"][0]
    print(json.dumps(out))


def lone_table(parent, say):
    mine = os.path.join(ROOT, "snlp---tenary-post-train-quantization_amd", "libpt2q.so")
    runs = [json.loads(subprocess.check_output([sys.executable, os.path.abspath(__file__), "--lone", so], text=True)
                       .strip().splitlines()[-1]) for so in (parent, mine, parent, mine)]
    say("(c) lone pt2q_ternary_linear, 11008 x 4096 (n x m): median µs per call, one process per column")
    say(f"  {'dtype':<5} {'tok':>4} | {'parent(A)':>10} {'this(A)':>10} {'parent(B)':>10} {'this(B)':>10} | {'diff':>7} {'spread':>7} verdict")
    level = True
    for k in runs[0]:
        p0, t0, p1, t1 = (r[k] for r in runs)
        diff, spread = (t0 + t1) / 2 - (p0 + p1) / 2, max(abs(p0 - p1), abs(t0 - t1))
        ok = abs(diff) <= spread
        level = level and ok
        name, tok = k.split()
        say(f"  {name:<5} {tok:>4} | {p0:10.2f} {t0:10.2f} {p1:10.2f} {t1:10.2f} | {diff:7.2f} {spread:7.2f} {'level' if ok else 'NOT level'}")
    say(f"lone path level with the parent at every row: {level}")


def main(argv):
    if argv[:1] == ["--lone"]:
        return lone_child(argv[1])
    opt = {}
    while argv[:1] and argv[0] in ("--out", "--resources", "--parent-lib"):
        opt[argv[0]] = argv[1]
        argv = argv[2:]
    shapes = [(int(argv[i]), int(argv[i + 1])) for i in range(0, len(argv), 2)] or [(4096, 11008), (5120, 13824)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if "--resources" in opt:  # the compiler's kernel-resource-usage figures, kept by whoever built the library
        for ln in open(opt["--resources"]).read().splitlines():
            say(ln)
    if "--parent-lib" in opt:  # before this process opens the GPU
        lone_table(opt["--parent-lib"], say)
    sys.path.insert(0, ROOT)
    import pt2q_loader
    pt2q = pt2q_loader.load()
    say(f"{pt2q._lib.version()} on {torch.cuda.get_device_name(0)}; µs per call as median/min of {WINDOWS} windows of "
        f"about {WINDOW_MS:.0f} ms, captured into one hipGraph, between one pair of HIP events")
    wins = {}
    for hid, inter in shapes:
        for name, dt in DT.items():
            g = torch.Generator(device=DEV).manual_seed(hid + inter)

            def layer(n, m):
                lay = pt2q.TernaryLinear(m, n, 128, bias=True, dtype=dt, decode="mfma")
                lay.set_quantized_params(*params(n, m, g))
                lay._prepare()
                return lay
            gate, up, down = layer(inter, hid), layer(inter, hid), layer(hid, inter)
            qkv = [layer(hid, hid) for _ in range(3)]
            say(f"hidden {hid} / inter {inter}, {name}: old(A) new(A) old(B) new(B) as median/min")
            for tokens in TOKENS:
                x = torch.randn((tokens, hid), device=DEV, generator=g).to(dt)
                want, got = down(F.silu(gate(x)) * up(x)).float(), down(pt2q.ternary_prefill_swiglu(x, gate, up)).float()
                bad = (got - want).abs() > 2e-2 * (1 + want.abs())
                if bool(bad.any()):
                    raise SystemExit(f"outputs differ: {hid} / {inter}, {tokens} tokens, {name}: {int(bad.sum())} elements")
                for tag, old, new in (
                        ("mlp", lambda: down(F.silu(gate(x)) * up(x)), lambda: down(pt2q.ternary_prefill_swiglu(x, gate, up))),
                        ("qkv", lambda: [l(x) for l in qkv], lambda: pt2q.ternary_prefill_group(x, qkv))):
                    t, margin, spread = ab(old, new)
                    ok = margin > spread and margin > 0
                    if tag == "mlp":
                        wins[tokens] = wins.get(tokens, True) and ok
                    cell = lambda k: f"{t[k][0]:8.1f}/{t[k][1]:8.1f}"  # noqa: E731
                    say(f"  {tag} {tokens:>4} | {cell('a')} {cell('n')} {cell('b')} {cell('n2')} | margin {margin:8.1f} "
                        f"spread {spread:6.1f} {'ok' if ok else 'NOT ok'}")
    cross = None
    for tokens in reversed(TOKENS):  # the smallest count from which every larger measured count wins too
        if not wins.get(tokens, False):
            break
        cross = tokens
    say(f"(a) below the children form by more than the spread at every shape and dtype from {cross} tokens "
        f"(None: at no measured count)")
    if "--out" in opt:
        os.makedirs(os.path.dirname(os.path.abspath(opt["--out"])), exist_ok=True)
        with open(opt["--out"], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
