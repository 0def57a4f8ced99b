"""The static SSR reorder without a GPU: the two C entries reject bad arguments before any device
work, the permutation helpers of reorder.py:146-221 are plain gathers on the tensor's own device,
and the reference fixtures carry the margins that make their order independent of the fp32
evaluation order (tests/golden/gen_static_reorder.py)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden

E_ARG, E_UNSUPPORTED, E_WORKSPACE = 1, 3, 5
F32, F16, BF16, I8 = 0, 1, 2, 3
P = ctypes.c_void_p(4096)  # a fake non-null pointer: never touched
BIG = 1 << 30


def test_cosine_similarity_argument_errors(pt2q):
    lib = pt2q._lib.lib()

    def cos(W=P, dt=F32, ldw=64, n=16, m=64, S=P, lds=64, ws=P, wsb=BIG):
        return lib.pt2q_cosine_similarity(W, dt, ldw, n, m, S, lds, ws, wsb, None)
    assert cos(W=None) == E_ARG
    assert cos(S=None) == E_ARG
    assert cos(n=0) == E_ARG and cos(n=-1) == E_ARG
    assert cos(m=0) == E_ARG and cos(m=-1) == E_ARG
    assert cos(ldw=63) == E_ARG
    assert cos(lds=63) == E_ARG
    assert cos(dt=I8) == E_ARG
    need = lib.pt2q_cosine_similarity_workspace_bytes(16, 64)
    assert cos(ws=None, wsb=0) == E_WORKSPACE
    assert cos(wsb=need - 1) == E_WORKSPACE
    assert cos(wsb=0) == E_WORKSPACE


def test_static_order_argument_errors(pt2q):
    lib = pt2q._lib.lib()

    def order(S=P, lds=64, m=64, perm=P, inv=P, ws=P, wsb=BIG):
        return lib.pt2q_ssr_static_order(S, lds, m, perm, inv, ws, wsb, None)
    assert order(S=None) == E_ARG
    assert order(perm=None) == E_ARG
    assert order(m=0) == E_ARG and order(m=-5) == E_ARG
    assert order(lds=63) == E_ARG
    need = lib.pt2q_ssr_static_order_workspace_bytes(64)
    assert order(ws=None, wsb=0) == E_WORKSPACE
    assert order(wsb=need - 1) == E_WORKSPACE
    # the one-workgroup kernel holds at most 16 columns per thread
    assert order(m=16385, lds=16385) == E_UNSUPPORTED
    assert order(m=16385, lds=16385, inv=None, wsb=0) == E_UNSUPPORTED  # before the workspace check
    assert order(m=16385, lds=16384) == E_ARG


def test_workspace_sizes_positive_and_monotone(pt2q):
    lib = pt2q._lib.lib()
    st = pt2q._lib.STATUS_BYTES
    cos, order = lib.pt2q_cosine_similarity_workspace_bytes, lib.pt2q_ssr_static_order_workspace_bytes
    assert cos(0, 64) == 0 and cos(64, 0) == 0 and order(0) == 0
    sizes = [1, 2, 3, 63, 64, 65, 1000, 1024, 4096, 11008, 16384]
    for n in sizes:
        for m in sizes:
            assert cos(n, m) >= st + 4 * m + 4 * n * m  # status word, norms, Wn
    for a, b in zip(sizes, sizes[1:]):
        assert 0 < cos(a, 77) <= cos(b, 77)
        assert 0 < cos(77, a) <= cos(77, b)
        assert 0 < order(a) <= order(b)
    assert order(16384) >= st + 4 * 16384


def test_helpers_match_their_definitions(pt2q):
    g = torch.Generator().manual_seed(3)
    W = torch.randn(6, 10, generator=g)
    X2 = torch.randn(4, 10, generator=g)
    X3 = torch.randn(2, 4, 10, generator=g)
    perm = torch.randperm(10, generator=g)
    assert torch.equal(pt2q.apply_permutation(W, perm), W[:, perm])
    assert torch.equal(pt2q.apply_permutation_to_input(X2, perm), X2[:, perm])
    assert torch.equal(pt2q.apply_permutation_to_input(X3, perm), X3[:, :, perm])
    with pytest.raises(ValueError, match="Unexpected input dimension: 4"):
        pt2q.apply_permutation_to_input(torch.zeros(1, 2, 3, 10), perm)
    with pytest.raises(ValueError):
        pt2q.apply_permutation_to_input(torch.zeros(10), perm)
    var = pt2q.compute_block_variance(W, 4)
    assert isinstance(var, list) and len(var) == 3 and all(isinstance(v, float) for v in var)
    assert var == [W[:, 0:4].var().item(), W[:, 4:8].var().item(), W[:, 8:10].var().item()]


def test_dynamic_reorderer_is_the_identity_without_a_gpu(pt2q):
    W = torch.arange(24, dtype=torch.float32).reshape(3, 8)
    r = pt2q.SSRReorderer(W)  # use_dynamic defaults to True, as in the reference
    assert r.use_dynamic and r.block_size == 128 and (r.n, r.m) == (3, 8)
    perm, inv = r.get_permutation()
    assert perm.dtype == torch.int64 and torch.equal(perm, torch.arange(8)) and torch.equal(inv, perm)
    assert perm is not inv
    assert torch.equal(r.reorder_weights(W), W) and torch.equal(r.restore_order(W), W)
    X = torch.arange(32, dtype=torch.float32).reshape(2, 2, 8)
    assert torch.equal(r.reorder_activations(X), X)
    # a given order: the gathers and their inverse
    r.perm = torch.tensor([3, 0, 7, 1, 2, 6, 5, 4])
    r.inv_perm = torch.argsort(r.perm)
    assert torch.equal(r.reorder_weights(W), W[:, r.perm])
    assert torch.equal(r.reorder_activations(X), X[..., r.perm])
    assert torch.equal(r.restore_order(r.reorder_weights(W)), W)


def test_static_surface_fails_loudly_without_gpu(pt2q):
    if torch.cuda.is_available():
        return  # with a device these compute (tests/test_gpu_static_reorder.py)
    W = torch.zeros(4, 8)
    for call in (lambda: pt2q.compute_cosine_similarity_matrix(W),
                 lambda: pt2q.get_initial_reorder_indices(W, 4),
                 lambda: pt2q.SSRReorderer(W, use_dynamic=False)):
        with pytest.raises(pt2q._lib.Pt2qError):
            call()


def test_fixtures_carry_their_margins():
    names = golden_names("static_reorder_")
    shapes = sorted(load_golden(k)["W"].shape for k in names)
    assert shapes == [(48, 192), (64, 97), (100, 130), (260, 64)]
    for k in names:
        g = load_golden(k)
        n, m = g["W"].shape
        eps = 2.0 * (n + m + 4) * 2.0 ** -24
        assert float(g["mean_gap"]) >= eps, k
        assert float(g["rowsum_gap"]) >= m * eps, k
        assert g["W"].dtype == np.float32 and g["S"].shape == (m, m) and g["S"].dtype == np.float32
        assert g["perm"].dtype == np.int64 and np.array_equal(np.sort(g["perm"]), np.arange(m))
        b = int(g["block"])
        assert b == 32 and g["block_var"].shape == ((m + b - 1) // b,)
