"""SSR on MI355X — the whole surface of the reference's reorder.py.

Dynamic block selection (reorder.py:36-61 and :107-143): one call = the similarity of every
remaining column to the remaining-column mean plus the ordered top-k (ssr.hip).  Ties (equal
similarity) resolve to the lower position in `remaining_indices`; torch.topk leaves that order
unspecified.

Static reorder (reorder.py:15-33 and :64-104): the cosine-similarity matrix and the greedy column
order built from it (reorder_static.hip).  The order keeps a running sum where the reference
recomputes a mean, and equal scores resolve to the lowest column index; argmax leaves that
unspecified.

CPU inputs (the reference's call shape) are computed on the current HIP device and returned on the
CPU.  SSRReorderer and the permutation helpers (reorder.py:146-221) are gathers on the tensor's
own device.
"""
from typing import List, Tuple

import torch

from . import _lib


def _ssr_call(W, remaining_indices, block_size, want_sim):
    dev = _lib.compute_device(W, remaining_indices)  # CPU callers: computed on the GPU
    Wf = W.to(dev).contiguous().float()
    n, m = Wf.shape
    rem = remaining_indices.to(device=dev, dtype=torch.int64).contiguous()
    r = rem.numel()
    bs = min(block_size, r)
    blk = torch.empty(max(bs, 1), dtype=torch.int64, device=dev)
    newrem = torch.empty(max(r - bs, 1), dtype=torch.int64, device=dev)
    sim = torch.empty(r, dtype=torch.float32, device=dev) if want_sim else None
    ws = _lib.workspace(_lib.lib().pt2q_ssr_workspace_bytes(n, m), dev)
    rc = _lib.lib().pt2q_ssr_select(_lib.ptr(Wf), m, n, m, _lib.ptr(rem), r, int(block_size),
                                    _lib.ptr(blk), _lib.ptr(newrem), _lib.ptr(sim), _lib.ptr(ws),
                                    ws.numel(), _lib.stream_of(dev))
    _lib.check(rc, "pt2q_ssr_select")
    return blk[:bs], newrem[: r - bs], sim


def compute_column_similarity_to_mean(W: torch.Tensor, indices: torch.Tensor) -> torch.Tensor:
    """reorder.py:36-61: cosine similarity of each W[:, indices] column to their mean."""
    _, _, sim = _ssr_call(W, indices, 1, True)
    return sim.to(W.device, W.dtype)


def select_next_block_ssr(W: torch.Tensor, remaining_indices: torch.Tensor,
                          block_size: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """reorder.py:107-143: (block_indices in similarity order, new_remaining ascending)."""
    if len(remaining_indices) <= block_size:
        return remaining_indices, torch.tensor([], dtype=remaining_indices.dtype,
                                               device=remaining_indices.device)
    blk, newrem, _ = _ssr_call(W, remaining_indices, block_size, False)
    dt, dv = remaining_indices.dtype, remaining_indices.device
    return blk.to(dv, dt), newrem.to(dv, dt)


# ---------------------------------------------------------------- static reorder

_NATIVE = (torch.float32, torch.float16, torch.bfloat16)


def _cosine_on_device(W, dev):
    """S (m x m fp32 on dev) of a 2-D W: fp32 / fp16 / bf16 go to the kernel as they are."""
    Wd = W.to(dev)
    if Wd.dtype not in _NATIVE:
        Wd = Wd.float()
    Wd = Wd.contiguous()
    n, m = Wd.shape
    S = torch.empty((m, m), dtype=torch.float32, device=dev)
    ws = _lib.workspace(_lib.lib().pt2q_cosine_similarity_workspace_bytes(n, m), dev)
    rc = _lib.lib().pt2q_cosine_similarity(_lib.ptr(Wd), _lib.dtype_code(Wd), m, n, m, _lib.ptr(S), m,
                                           _lib.ptr(ws), ws.numel(), _lib.stream_of(dev))
    _lib.check(rc, "pt2q_cosine_similarity")
    return S


def _static_order_on_device(S, want_inv=False):
    """(perm, inv_perm or None), int64 on S.device, of a symmetric fp32 S on a HIP device."""
    m = S.shape[0]
    dev = S.device
    perm = torch.empty(m, dtype=torch.int64, device=dev)
    inv = torch.empty(m, dtype=torch.int64, device=dev) if want_inv else None
    ws = _lib.workspace(_lib.lib().pt2q_ssr_static_order_workspace_bytes(m), dev)
    rc = _lib.lib().pt2q_ssr_static_order(_lib.ptr(S), S.stride(0), m, _lib.ptr(perm), _lib.ptr(inv),
                                          _lib.ptr(ws), ws.numel(), _lib.stream_of(dev))
    _lib.check(rc, "pt2q_ssr_static_order")
    return perm, inv


def compute_cosine_similarity_matrix(W: torch.Tensor) -> torch.Tensor:
    """reorder.py:15-33 (Eq. 15): S_ij = cosine similarity of columns i and j of W (n x m)."""
    dev = _lib.compute_device(W)
    return _cosine_on_device(W, dev).to(W.device, W.dtype)


def get_initial_reorder_indices(W: torch.Tensor, block_size: int) -> torch.Tensor:
    """reorder.py:64-104: the greedy column order, int64 on W.device (block_size is unused, as in
    the reference)."""
    dev = _lib.compute_device(W)
    perm, _ = _static_order_on_device(_cosine_on_device(W, dev))
    return perm.to(W.device)


class SSRReorderer:
    """reorder.py:146-189: the full initial reordering (use_dynamic=False) or the identity that the
    dynamic block selection starts from."""

    def __init__(self, W: torch.Tensor, block_size: int = 128, use_dynamic: bool = True):
        self.block_size = block_size
        self.use_dynamic = use_dynamic
        self.n, self.m = W.shape
        if not use_dynamic:
            dev = _lib.compute_device(W)
            perm, inv = _static_order_on_device(_cosine_on_device(W, dev), want_inv=True)
            self.perm, self.inv_perm = perm.to(W.device), inv.to(W.device)  # inv == argsort(perm)
        else:
            self.perm = torch.arange(self.m, device=W.device)
            self.inv_perm = self.perm.clone()

    def get_permutation(self) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.perm, self.inv_perm

    def reorder_weights(self, W: torch.Tensor) -> torch.Tensor:
        return W[:, self.perm]

    def reorder_activations(self, X: torch.Tensor) -> torch.Tensor:
        return X[..., self.perm]

    def restore_order(self, W: torch.Tensor) -> torch.Tensor:
        return W[:, self.inv_perm]


def apply_permutation(W: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    """reorder.py:192-194: W' = WP."""
    return W[:, perm]


def apply_permutation_to_input(X: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    """reorder.py:197-204: X' = XP on the feature dimension of a 2-D or 3-D input."""
    if X.dim() == 2:
        return X[:, perm]
    elif X.dim() == 3:
        return X[:, :, perm]
    else:
        raise ValueError(f"Unexpected input dimension: {X.dim()}")


def compute_block_variance(W: torch.Tensor, block_size: int) -> List[float]:
    """reorder.py:207-221: the variance of each block of block_size columns (analysis only)."""
    n, m = W.shape
    return [W[:, i:min(i + block_size, m)].var().item() for i in range(0, m, block_size)]
