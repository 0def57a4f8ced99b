"""Generate the static-reorder fixtures (static_reorder_*.npz) from the REFERENCE implementation.

Run here (the reference is importable only in the build container):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_static_reorder.py

It imports /root/reference/reorder.py and runs compute_cosine_similarity_matrix,
get_initial_reorder_indices and compute_block_variance on the CPU (one thread).  Only data is
stored: W itself, the reference's S, perm and block variances, and the float64 margins below.

The reference's argmax over near-ties depends on its BLAS, so a fixture is kept only when no fp32
evaluation order can change its order.  In a float64 replay of reorder.py:81-104 both must hold:
  * at every step the best and second-best unselected cluster means differ by at least
    eps = 2 (n + m + 4) 2^-24, and
  * the two largest row sums differ by at least m eps.
|S_ij| <= 1 and sum_k |a_k b_k| <= 1 for normalised columns, so an fp32 S entry is within
(n + 4) 2^-24 of the exact one however it is summed, a mean of up to m of them adds at most
m 2^-24 more, and two competing scores together move by less than eps (row sums: m entries, so
m eps).  The generator searches seeds until both hold and asserts that the reference's order then
equals the float64 replay.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(1)
import reorder as rr  # noqa: E402

BLOCK = 32
CASES = [(100, 130, "gauss"), (64, 97, "outliers"), (260, 64, "gauss"), (48, 192, "outliers")]


def eps_of(n, m):
    return 2.0 * (n + m + 4) * 2.0 ** -24


def make_w(n, m, variant, seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(n, m, generator=g)
    if variant == "outliers":
        W[:, ::17] *= 20.0
        W = W + 0.3 * torch.randn(n, 1, generator=g)
    return W.contiguous()


def replay64(W):
    """reorder.py:15-33 and :81-104 in float64: (perm, smallest top-two gap of the cluster means
    over the steps, top-two gap of the row sums)."""
    W = W.double()
    Wn = W / W.norm(dim=0, keepdim=True).clamp(min=1e-8)
    S = (Wn.T @ Wn).numpy()
    m = S.shape[0]
    rs = S.sum(axis=1)
    top = np.sort(rs)[::-1]
    rs_gap = float(top[0] - top[1]) if m > 1 else float("inf")
    perm = [int(rs.argmax())]
    sel = np.zeros(m, bool)
    sel[perm[0]] = True
    acc = np.zeros(m)
    gap = float("inf")
    while len(perm) < m:
        acc = acc + S[:, perm[-1]]
        mean = acc / len(perm)
        mean[sel] = -np.inf
        p = int(mean.argmax())
        if m - len(perm) > 1:
            second = np.partition(mean, -2)[-2]
            gap = min(gap, float(mean[p] - second))
        perm.append(p)
        sel[p] = True
    return np.array(perm, np.int64), gap, rs_gap


def main():
    for n, m, variant in CASES:
        eps = eps_of(n, m)
        for seed in range(1000):
            W = make_w(n, m, variant, seed)
            perm64, gap, rs_gap = replay64(W)
            if gap >= eps and rs_gap >= m * eps:
                break
        else:
            raise SystemExit(f"no qualifying seed for {n}x{m} {variant}")
        S = rr.compute_cosine_similarity_matrix(W)
        perm = rr.get_initial_reorder_indices(W, BLOCK).numpy().astype(np.int64)
        assert np.array_equal(perm, perm64), (n, m, variant, seed)
        var = np.array(rr.compute_block_variance(W, BLOCK), np.float64)
        name = f"static_reorder_{n}x{m}_{variant}"
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, W=W.numpy(), S=S.numpy(), perm=perm, block_var=var, block=BLOCK,
                            mean_gap=gap, rowsum_gap=rs_gap, seed=seed)
        print(f"  {name}.npz seed {seed} mean gap {gap:.3e} (eps {eps:.3e}) row-sum gap {rs_gap:.3e} "
              f"(m eps {m * eps:.3e}) {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
