"""Time the static SSR reorder (dev tool): python tools/time_static_reorder.py [--out FILE] [n m ...]

For each n x m (default 4096 x 4096 and 4096 x 11008, fp32 synthetic weights with outlier columns)
it reports, from HIP events after a warm-up, separately:
  cosine    pt2q_cosine_similarity (norms, normalisation, f32 Gram)
  order     pt2q_ssr_static_order (sequential row sums + the one-workgroup greedy kernel)
  baseline  the same running-sum greedy written with torch device ops on the same S: per step one
            row add, one masked fill and one argmax, m steps, no host synchronisation inside
The baseline is not the reference's O(m^3) loop.  Its order is compared with the kernel's (torch's
row sums and argmax ties are its own, so a difference is reported, not asserted)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pt2q_loader  # noqa: E402

pt2q = pt2q_loader.load()
L = pt2q._lib
DEV = torch.device("cuda", 0)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_greedy(S, steps=None):
    m = S.shape[0]
    steps = m if steps is None else steps
    perm = torch.empty(m, dtype=torch.int64, device=S.device)
    sel = torch.zeros(m, dtype=torch.bool, device=S.device)
    acc = torch.zeros(m, dtype=torch.float32, device=S.device)
    p = S.sum(dim=1).argmax().view(1)
    for t in range(steps):
        perm[t:t + 1] = p
        sel.index_fill_(0, p, True)
        acc += S.index_select(0, p)[0]
        p = acc.masked_fill(sel, float("-inf")).argmax().view(1)
    return perm


def run(n, m, say):
    lib = L.lib()
    W = pt2q.fill_synthetic((n, m), 1234 + m, outliers=True)
    S = torch.empty((m, m), dtype=torch.float32, device=DEV)
    perm = torch.empty(m, dtype=torch.int64, device=DEV)
    inv = torch.empty(m, dtype=torch.int64, device=DEV)
    wc = L.workspace(lib.pt2q_cosine_similarity_workspace_bytes(n, m), DEV)
    wo = L.workspace(lib.pt2q_ssr_static_order_workspace_bytes(m), DEV)
    st = L.stream_of(DEV)

    def cosine():
        L.check(lib.pt2q_cosine_similarity(L.ptr(W), L.F32, m, n, m, L.ptr(S), m, L.ptr(wc), wc.numel(), st),
                "pt2q_cosine_similarity")

    def order():
        L.check(lib.pt2q_ssr_static_order(L.ptr(S), m, m, L.ptr(perm), L.ptr(inv), L.ptr(wo), wo.numel(), st),
                "pt2q_ssr_static_order")

    cosine(); order(); torch_greedy(S, steps=64)  # warm-up: code objects, allocator
    t_cos = timed(cosine, 5)
    t_ord = timed(order, 3)
    base = []
    t_base = timed(lambda: base.append(torch_greedy(S)), 1)
    same = bool(torch.equal(base[0], perm))
    ok = bool(torch.equal(torch.sort(perm).values, torch.arange(m, device=DEV)))
    say(f"{n} x {m}: cosine {t_cos:8.2f} ms   order {t_ord:8.2f} ms ({1e3 * t_ord / m:.2f} us/step)   "
        f"torch baseline {t_base:9.2f} ms ({1e3 * t_base / m:.2f} us/step)   "
        f"order/baseline {t_base / t_ord:.1f}x   permutation {ok}   baseline order identical {same}")


def main(argv):
    out = None
    if argv[:1] == ["--out"]:
        out, argv = argv[1], argv[2:]
    shapes = [(int(argv[i]), int(argv[i + 1])) for i in range(0, len(argv), 2)] or [(4096, 4096), (4096, 11008)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"{L.version()} on {torch.cuda.get_device_name(0)}; HIP events, warmed up; fp32 W, outlier columns")
    for n, m in shapes:
        run(n, m, say)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
