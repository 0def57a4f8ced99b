"""Time the layer report (dev tool): python tools/time_layer_report.py [--out FILE] [n m ...]

For each n x m (default 4096 x 4096, 11008 x 4096 and 4096 x 11008; fp32 synthetic W, random
ternary codes and grids, G the Gram of 2048 synthetic activation rows) it reports, from HIP events
around each call after a warm-up, the median and minimum of 7 runs of
  report      pt2q_layer_report without PT2Q_REPORT_REF  (ew, ex: n rows through the fused kernel)
  report+ref  pt2q_layer_report with PT2Q_REPORT_REF     (ew, ex, ey: 2n rows in one launch)
  torch       ((D @ G) * D).sum(1) in fp32 on the same device, D given (rocBLAS; the n x m product
              goes through memory), and the same with W stacked under D for the +ref quantity
TF/s counts the chain GEMM alone, 2 rows m^2 flops, over the whole call (residual, transposes and
the finishing kernels included), beside the 157 TF f32 MFMA peak DESIGN.md uses.  The two results
are compared (relative difference of the totals; the orders of summation differ)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pt2q_loader  # noqa: E402

pt2q = pt2q_loader.load()
L = pt2q._lib
DEV = torch.device("cuda", 0)
PEAK_TF = 157.0
RUNS = 7


def timed(fn):
    """(median, min) ms of RUNS single calls, each between its own pair of events."""
    ts = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts)


def run(n, m, say):
    lib = L.lib()
    b = 128
    B = -(-m // b)
    W = pt2q.fill_synthetic((n, m), 77 + n + m, outliers=True)
    X = pt2q.fill_synthetic((2048, m), 78 + m, outliers=True)
    G = pt2q.gram(X)
    del X
    g = torch.Generator(device=DEV).manual_seed(n + m)
    T = torch.randint(-1, 2, (n, m), device=DEV, generator=g, dtype=torch.int8)
    alpha = W.abs().mean() * (0.5 + torch.rand((n, B), device=DEV, generator=g))
    mu = 0.01 * torch.randn((n, B), device=DEV, generator=g)
    perm = torch.randperm(m, device=DEV, generator=g)
    out = torch.empty((3, n), dtype=torch.float32, device=DEV)
    totals = torch.empty((2, 3), dtype=torch.float32, device=DEV)
    st = L.stream_of(DEV)
    ws = L.workspace(lib.pt2q_layer_report_workspace_bytes(n, m, 1), DEV)

    def report(flags):
        L.check(lib.pt2q_layer_report(L.ptr(W), L.F32, m, n, m, b, L.ptr(alpha), L.ptr(mu), L.ptr(T), L.I8, m,
                                      L.ptr(perm), L.ptr(G), m, flags, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]),
                                      L.ptr(totals[flags]), L.ptr(ws), ws.numel(), st), "pt2q_layer_report")

    D = W - pt2q.dequantize(alpha, mu, T, perm, b)
    DW = torch.cat([D, W])
    res = {}

    def torch_expr(A, key):
        res[key] = ((A @ G) * A).sum(1)

    for f in (lambda: report(0), lambda: report(1), lambda: torch_expr(D, "d"), lambda: torch_expr(DW, "dw")):
        f()
        f()  # warm-up: code objects, rocBLAS solution selection, allocator
    t = {"report": timed(lambda: report(0)), "report+ref": timed(lambda: report(1)),
         "torch": timed(lambda: torch_expr(D, "d")), "torch+ref": timed(lambda: torch_expr(DW, "dw"))}
    tot = totals.cpu()
    rel = abs(tot[1, 1].item() - res["d"].double().sum().item()) / abs(res["d"].double().sum().item())
    say(f"{n} x {m}:")
    for key, rows in (("report", n), ("report+ref", 2 * n), ("torch", n), ("torch+ref", 2 * n)):
        med, mn = t[key]
        tf = 2.0 * rows * m * m / (med * 1e-3) / 1e12
        say(f"  {key:<11} median {med:8.3f} ms  min {mn:8.3f} ms  {tf:6.1f} TF/s ({100 * tf / PEAK_TF:4.1f} % of "
            f"{PEAK_TF:.0f})")
    say(f"  report / torch {t['report'][0] / t['torch'][0]:.2f}x   report+ref / torch+ref "
        f"{t['report+ref'][0] / t['torch+ref'][0]:.2f}x   (time ratios, medians; > 1: the fused call is slower)   "
        f"output_error vs torch {rel:.2e} relative   relative_output_error {tot[1, 1].item() / tot[1, 2].item():.4f}")


def main(argv):
    out = None
    if argv[:1] == ["--out"]:
        out, argv = argv[1], argv[2:]
    shapes = [(int(argv[i]), int(argv[i + 1])) for i in range(0, len(argv), 2)] or \
        [(4096, 4096), (11008, 4096), (4096, 11008)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"{L.version()} on {torch.cuda.get_device_name(0)}; HIP events per call, warmed up, {RUNS} runs; "
        f"fp32 W, block 128, random codes")
    for n, m in shapes:
        run(n, m, say)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
