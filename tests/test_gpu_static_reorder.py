"""The static SSR reorder on the GPU (reorder_static.hip; reference reorder.py:15-33, :64-104).

Bit-exact against a CPU restatement of the contract (DESIGN.md §3 "Static reorder") built from
the oracle's Gram and sequential row sums plus numpy float32 operations, against the reference's
own results on fixtures whose order no fp32 evaluation order can change
(tests/golden/gen_static_reorder.py), and once inside the workflow it is meant for."""
import ctypes

import numpy as np
import pytest
import torch

import synth
from conftest import golden_names, load_golden
from oracle import oracle as orc
from test_gpu_parity import bits_equal
from test_gpu_strides import Pad, ins_ok, outs_ok

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32


# ---------------------------------------------------------------- the CPU restatement

def restate_cosine(W32):
    """Contract items 1-3 on the exact fp32 upcast of W."""
    W32 = np.ascontiguousarray(W32, dtype=F32)
    with np.errstate(all="ignore"):
        q = np.diag(orc.gram(W32)).astype(F32)          # k-ascending fmaf(w, w, q) chains from +0
        nrm = np.sqrt(q)
        nrm = np.where(nrm < F32(1e-8), F32(1e-8), nrm)  # clamp; NaN propagates
        Wn = (W32 / nrm[None, :]).astype(F32)            # one correctly rounded division
    return orc.gram(Wn)


def restate_order(S):
    """Contract items 4-5 on a symmetric fp32 S: (perm, inv_perm)."""
    S = np.ascontiguousarray(S, dtype=F32)
    m = S.shape[0]
    rs = orc.rowsum_seq(S)
    p = int(np.argmax(rs))  # first maximum
    perm = [p]
    left = np.ones(m, bool)
    left[p] = False
    acc = np.zeros(m, F32)
    while len(perm) < m:
        acc = acc + S[p]  # one fp32 add per step, in selection order
        idx = np.flatnonzero(left)
        p = int(idx[np.argmax(acc[idx])])  # largest sum, lowest index among equals
        perm.append(p)
        left[p] = False
    perm = np.array(perm, np.int64)
    inv = np.empty(m, np.int64)
    inv[perm] = np.arange(m)
    return perm, inv


# ---------------------------------------------------------------- direct C entries

def c_cosine(pt2q, Wt):
    """pt2q_cosine_similarity on a contiguous device W (fp32 / fp16 / bf16)."""
    lib = pt2q._lib.lib()
    n, m = Wt.shape
    S = torch.empty((m, m), dtype=torch.float32, device=DEV)
    ws = pt2q._lib.workspace(lib.pt2q_cosine_similarity_workspace_bytes(n, m), DEV)
    rc = lib.pt2q_cosine_similarity(pt2q._lib.ptr(Wt), pt2q._lib.dtype_code(Wt), m, n, m, pt2q._lib.ptr(S), m,
                                    pt2q._lib.ptr(ws), ws.numel(), None)
    assert rc == 0
    return S


def c_order(pt2q, S, want_inv=True):
    lib = pt2q._lib.lib()
    m = S.shape[0]
    perm = torch.full((m,), -7, dtype=torch.int64, device=DEV)
    inv = torch.full((m,), -7, dtype=torch.int64, device=DEV) if want_inv else None
    ws = pt2q._lib.workspace(lib.pt2q_ssr_static_order_workspace_bytes(m), DEV)
    rc = lib.pt2q_ssr_static_order(pt2q._lib.ptr(S), m, m, pt2q._lib.ptr(perm), pt2q._lib.ptr(inv),
                                   pt2q._lib.ptr(ws), ws.numel(), None)
    assert rc == 0
    return perm, inv


# ---------------------------------------------------------------- inputs

def int_row(seed, m, signed):
    """One row of small integers (squares, roots and quotients exact): every cosine is +-1."""
    v = (synth.centered24(seed, m) > 0).astype(F32) * 2 + 1  # 1 or 3
    if signed:
        v = v * np.where(synth.centered24(seed + 1, m) > 0, F32(1), F32(-1))
    return v.reshape(1, m).astype(F32)


def make_w(kind, n, m, seed):
    if kind == "ones":
        return int_row(seed, m, signed=False)
    if kind == "signs":
        return int_row(seed, m, signed=True)
    W = synth.weights(seed, n, m)
    if kind == "dup":  # two pairs of bit-identical columns: their scores tie at every step
        W[:, m - 3] = W[:, 5]
        W[:, 2] = W[:, m // 2]
    elif kind == "zero":
        W[:, m // 3] = 0.0
    return np.ascontiguousarray(W)


# (kind, n, m): the smallest shapes that reach each path -- one to three columns per thread of
# the order kernel with ragged ends, every row-sum kernel (m <= 128, <= 512, wider, 16-byte rows or
# not), 64 x 64 and 128 x 128 Gram tiles, the unrolled and the tail part of the norm chain
CASES = [
    ("rand", 7, 1), ("rand", 7, 2), ("rand", 7, 63), ("rand", 19, 64), ("rand", 7, 65),
    ("rand", 5, 1023), ("rand", 5, 1024), ("rand", 5, 1025), ("rand", 5, 2050),
    ("ones", 1, 200), ("signs", 1, 1500), ("rand", 3, 130), ("rand", 64, 130), ("rand", 257, 96),
    ("dup", 33, 300), ("dup", 6, 1100), ("zero", 20, 140),
]


@pytest.mark.parametrize("kind,n,m", CASES, ids=[f"{k}-{n}x{m}" for k, n, m in CASES])
def test_bit_exact_against_restatement(pt2q, kind, n, m):
    W = make_w(kind, n, m, 900 + 7 * n + m)
    S_ref = restate_cosine(W)
    perm_ref, inv_ref = restate_order(S_ref)
    if kind == "ones":  # S is all ones: every score ties at every step
        assert np.array_equal(S_ref, np.ones((m, m), F32)) and np.array_equal(perm_ref, np.arange(m))
    if kind == "signs":
        assert np.array_equal(np.abs(S_ref), np.ones((m, m), F32))
    Wt = torch.from_numpy(W).to(DEV)
    # the C entries
    S = c_cosine(pt2q, Wt)
    assert np.array_equal(S.cpu().numpy(), S_ref) and bits_equal(S.cpu().numpy(), S_ref)
    perm, inv = c_order(pt2q, S)
    assert np.array_equal(perm.cpu().numpy(), perm_ref)
    assert np.array_equal(inv.cpu().numpy(), inv_ref)
    perm2, none = c_order(pt2q, S, want_inv=False)
    assert none is None and torch.equal(perm2, perm)
    # the Python surface, device and CPU callers
    Sp = pt2q.compute_cosine_similarity_matrix(Wt)
    assert Sp.device == Wt.device and Sp.dtype == torch.float32 and torch.equal(Sp, S)
    pp = pt2q.get_initial_reorder_indices(Wt, 128)
    assert pp.device == Wt.device and pp.dtype == torch.int64 and torch.equal(pp, perm)
    Wc = torch.from_numpy(W)
    Sc = pt2q.compute_cosine_similarity_matrix(Wc)
    pc = pt2q.get_initial_reorder_indices(Wc, 128)
    assert Sc.device.type == "cpu" and pc.device.type == "cpu" and pc.dtype == torch.int64
    assert np.array_equal(Sc.numpy(), S_ref) and np.array_equal(pc.numpy(), perm_ref)
    r = pt2q.SSRReorderer(Wt, block_size=64, use_dynamic=False)
    assert torch.equal(r.perm, perm) and torch.equal(r.inv_perm, inv)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_16bit_weights_upcast_exactly(pt2q, dtype):
    n, m = 40, 200
    W16 = torch.from_numpy(synth.weights(77, n, m)).to(dtype)
    S_ref = restate_cosine(W16.float().numpy())
    perm_ref, inv_ref = restate_order(S_ref)
    Wt = W16.to(DEV)
    S = c_cosine(pt2q, Wt)
    assert np.array_equal(S.cpu().numpy(), S_ref)
    perm, inv = c_order(pt2q, S)
    assert np.array_equal(perm.cpu().numpy(), perm_ref) and np.array_equal(inv.cpu().numpy(), inv_ref)
    Sp = pt2q.compute_cosine_similarity_matrix(Wt)  # S comes back in W's dtype
    assert Sp.dtype == dtype and torch.equal(Sp, S.to(dtype))
    assert torch.equal(pt2q.get_initial_reorder_indices(Wt, 128), perm)


@pytest.mark.parametrize("n,m,padw,pads,lead", [(9, 70, 2, 6, 0), (9, 70, 3, 5, 1), (6, 1100, 4, 4, 1),
                                                (6, 1100, 1, 3, 0)],
                         ids=["aligned", "odd-lead1", "wide-lead1", "wide-odd"])
def test_padded_leading_dimensions(pt2q, n, m, padw, pads, lead):
    """ldw and lds above the row length, bases offset by `lead` elements, sentinel-filled pads
    (NaN in the inputs): the windows are the contiguous results, every pad keeps its sentinel."""
    lib = pt2q._lib.lib()
    W = synth.weights(31 + m, n, m)
    S_ref = restate_cosine(W)
    perm_ref, inv_ref = restate_order(S_ref)
    Wp = Pad((n, m), m + padw, torch.float32, data=W, lead=lead)
    Sp = Pad((m, m), m + pads, torch.float32, lead=lead, out=True)
    ws = pt2q._lib.workspace(lib.pt2q_cosine_similarity_workspace_bytes(n, m), DEV)
    assert lib.pt2q_cosine_similarity(Wp.p, 0, m + padw, n, m, Sp.p, m + pads, pt2q._lib.ptr(ws), ws.numel(),
                                      None) == 0
    assert np.array_equal(Sp.win(), S_ref)
    assert outs_ok(Sp) and ins_ok(Wp)
    # the order reads S in place from a padded, NaN-padded buffer
    Sin = Pad((m, m), m + pads, torch.float32, data=S_ref, lead=lead)
    perm = Pad((1, m), m, torch.int64, lead=lead, out=True)
    inv = Pad((1, m), m, torch.int64, lead=lead, out=True)
    ws2 = pt2q._lib.workspace(lib.pt2q_ssr_static_order_workspace_bytes(m), DEV)
    assert lib.pt2q_ssr_static_order(Sin.p, m + pads, m, perm.p, inv.p, pt2q._lib.ptr(ws2), ws2.numel(),
                                     None) == 0
    assert np.array_equal(perm.win()[0], perm_ref) and np.array_equal(inv.win()[0], inv_ref)
    assert outs_ok(perm, inv) and ins_ok(Sin)


@pytest.fixture(scope="module")
def fixtures():
    return {k: load_golden(k) for k in golden_names("static_reorder_")}


def test_reference_fixtures(pt2q, fixtures):
    assert len(fixtures) == 4
    for k, g in fixtures.items():
        W = torch.from_numpy(g["W"])
        n, m = W.shape
        Wt = W.to(DEV)
        S = pt2q.compute_cosine_similarity_matrix(Wt).cpu().numpy()
        err = float(np.abs(S.astype(np.float64) - g["S"].astype(np.float64)).max())
        bound = 2.0 * (n + 4) * 2.0 ** -24
        print(f"{k}: max |S - S_ref| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound, k
        perm = pt2q.get_initial_reorder_indices(Wt, int(g["block"]))
        assert np.array_equal(perm.cpu().numpy(), g["perm"]), k
        r = pt2q.SSRReorderer(Wt, block_size=int(g["block"]), use_dynamic=False)
        p, inv = r.get_permutation()
        assert np.array_equal(p.cpu().numpy(), g["perm"]), k
        assert torch.equal(inv, torch.argsort(p)), k
        assert torch.equal(r.restore_order(r.reorder_weights(Wt)), Wt), k
        # a reference-style CPU caller
        assert np.array_equal(pt2q.get_initial_reorder_indices(W, int(g["block"])).numpy(), g["perm"]), k
        var = pt2q.compute_block_variance(W, int(g["block"]))
        np.testing.assert_allclose(np.array(var, np.float64), g["block_var"], rtol=1e-5)


def test_nan_column_still_gives_a_permutation(pt2q):
    n, m = 12, 1300
    W = synth.weights(5, n, m)
    W[:, 17] = np.nan
    perm = pt2q.get_initial_reorder_indices(torch.from_numpy(W).to(DEV), 128)
    assert np.array_equal(np.sort(perm.cpu().numpy()), np.arange(m))


def test_static_order_feeds_the_layer_quantizer(pt2q):
    """The intended workflow: order the columns once, permute weights and activations, quantise
    in that order (sequential blocks).  No new kernel runs beyond the order."""
    n, m, N = 64, 256, 512
    W = synth.weights(41, n, m)
    X = synth.activations(42, N, m)
    Wt, Xt = torch.from_numpy(W).to(DEV), torch.from_numpy(X).to(DEV)
    r = pt2q.SSRReorderer(Wt, block_size=128, use_dynamic=False)
    perm = r.perm.cpu().numpy()
    assert np.array_equal(perm, restate_order(restate_cosine(W))[0])
    Wp, Xp = r.reorder_weights(Wt).contiguous(), r.reorder_activations(Xt).contiguous()
    assert np.array_equal(Wp.cpu().numpy(), W[:, perm]) and np.array_equal(Xp.cpu().numpy(), X[:, perm])
    out = pt2q.quantize_layer(Wp, Xp, use_ssr=False)
    torch.cuda.synchronize()
    ref = orc.quantize_layer_m(np.ascontiguousarray(W[:, perm]), np.ascontiguousarray(X[:, perm]), use_ssr=False)
    assert np.array_equal(out.perm.cpu().numpy(), ref["perm"])
    assert np.array_equal(out.T.cpu().numpy(), ref["T"])
    assert bits_equal(out.alpha.cpu().numpy(), ref["alpha"])
    assert bits_equal(out.mu.cpu().numpy(), ref["mu"])
