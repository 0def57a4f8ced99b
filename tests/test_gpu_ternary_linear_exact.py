"""The MFMA ternary linear path (pt2q_ternary_linear: tl_gemm_kernel<BF16, NT> + tl_reduce_kernel,
tl_prefill_kernel) pinned bit for bit.  No assertion here carries a tolerance.

  a. exact GEMM     exactly summable data (tests/ternary_linear_ref.py): any summation order, K split
                    and 16-bit type must give the integer reference's bits
  b. weight readout one-hot activations read the dequantised weight out of each kernel element by
                    element, with realistic scales that do need the TX rounding
  c. guards         alpha, mu and bias inside NaN-filled buffers: nothing past an array may reach y
  d. stale pack     the packed copy must follow load_state_dict, dtype casts and device moves

Which kernel a shape reaches (ternary_linear_ref.launch_path restates the launcher):
  prefill   tokens >= 256 and (bs >= m or bs % 128 == 0)
  K split   otherwise, NT = 1 for tokens < 128, 2 for tokens < 512, else 4; splits from tl_plan"""
import numpy as np
import pytest
import torch

import ternary_linear_ref as ref
from test_gpu_parity import cuda

pytestmark = pytest.mark.gpu

TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _layer(pt2q, c, dtype, compat, bias=True):
    lay = pt2q.TernaryLinear(c["m"], c["n"], c["bs"], bias=bias, dtype=TDT[dtype], compat=compat, decode="mfma")
    lay.set_quantized_params(cuda(c["alpha"]), cuda(c["mu"]), cuda(c["T"]), cuda(c["perm"]),
                             cuda(c["bias"]) if bias else None)
    return lay


def _call(pt2q, lay, x, ydt, bias):
    """pt2q_ternary_linear on the layer's packed operands, with an fp32 or 16-bit y and with or
    without the bias (the module itself always writes x's type and passes its bias)."""
    L = pt2q._lib
    lib = L.lib()
    if lay._packed is None:
        lay._prepare()
    codes, gather, a32, m32, b32 = lay._packed
    tokens, m = x.shape
    n = lay.out_features
    y = torch.empty((tokens, n), dtype=ydt, device=x.device)
    ws = L.workspace(lib.pt2q_ternary_linear_workspace_bytes(tokens, n, m), x.device)
    L.check(lib.pt2q_ternary_linear(L.ptr(x), L.dtype_code(x), tokens, m, n, m, L.ptr(codes), L.ptr(gather),
                                    L.ptr(a32), L.ptr(m32), a32.shape[1], lay.block_size,
                                    L.ptr(b32) if bias else None, L.ptr(y), L.dtype_code(y), n, L.ptr(ws),
                                    ws.numel(), L.stream_of(x.device)), "pt2q_ternary_linear")
    return y


def _same(y, want):
    """y (device tensor) holds exactly the float32 values `want` (numpy)."""
    got = y.float().cpu()
    return torch.equal(got, torch.from_numpy(want)) and bool(torch.isfinite(got).all())


# ------------------------------------------------------------------ a. exact GEMM

@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("n,m,bs,tokens,compat16", ref.GEMM_SHAPES)
def test_exact_gemm(pt2q, n, m, bs, tokens, compat16, dtype):
    """Every shape of ternary_linear_ref.GEMM_SHAPES (the path of each is noted there) in fp16 with
    the listed semantics and in bf16 with the other one; y in x's type and in fp32, with and
    without bias.  The module's own forward gives the (x's type, bias) output."""
    compat = compat16 if dtype == "fp16" else not compat16
    c = ref.exact_case(n, m, bs, tokens, ref.case_seed(n, m, bs, tokens))
    lay = _layer(pt2q, c, dtype, compat)
    x = cuda(c["x"]).to(TDT[dtype])
    path = ref.launch_path(n, m, bs, tokens)
    assert _same(lay(x), ref.exact_reference(c, compat, True, dtype)), path
    assert _same(_call(pt2q, lay, x, TDT[dtype], False), ref.exact_reference(c, compat, False, dtype)), path
    for bias in (True, False):
        assert _same(_call(pt2q, lay, x, torch.float32, bias), ref.exact_reference(c, compat, bias)), (path, bias)


# ------------------------------------------------------------------ b. weight readout

# (n, m, bs, [token slices]): x is one-hot, token t = value * e_t, so tokens = the slice's length
READOUT = [
    # 300 tokens: prefill (two 256-feature workgroups, three token tiles); slices of 100: K split
    # NT = 1; slices of 200: NT = 2
    (260, 300, 128, [(0, 300), (0, 100), (100, 200), (200, 300), (0, 200), (100, 300)]),
    (130, 600, 64, [(0, 600)]),   # K split, NT = 4, two tables per 128-position block
    (130, 200, 48, [(0, 200)]),   # K split, NT = 2, tables that switch inside a block
    (130, 130, 130, [(0, 130)]),  # per-channel, K split, NT = 2
]


@pytest.mark.parametrize("compat", [False, True])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("n,m,bs,slices", READOUT)
def test_weight_readout(pt2q, n, m, bs, slices, dtype, compat):
    """Scales in the range of real layers (alpha +- mu needs the TX rounding).  Every output is one
    exact product value * Wd[i][t], so y must be value * weight_tx(...)ᵀ bit for bit, in fp32 and
    in x's type: codes, table, block index, gather and both permutation conventions."""
    rng = np.random.default_rng(17 * n + m + bs)
    B = ref.nblocks(m, bs)
    c = {"n": n, "m": m, "bs": bs, "T": rng.integers(-1, 2, size=(n, m)).astype(np.int8),
         "alpha": ref.round16(rng.random((n, B)) * 0.05 + 0.005, dtype),
         "mu": ref.round16(rng.standard_normal((n, B)) * 0.002, dtype),
         "perm": rng.permutation(m).astype(np.int64)}
    W = ref.weight_tx(c["alpha"], c["mu"], c["T"], c["perm"], bs, compat, dtype)
    assert not np.array_equal(W, ref.weight_tx(c["alpha"], c["mu"], c["T"], c["perm"], bs, compat,
                                               "bf16" if dtype == "fp16" else "fp16"))  # the rounding matters
    lay = _layer(pt2q, c, dtype, compat, bias=False)
    eye = torch.eye(m, dtype=TDT[dtype], device="cuda")
    for value in (1.0, -2.0):
        want = np.ascontiguousarray((np.float32(value) * W).T)
        for s, e in slices:
            x = (eye[s:e] * value).contiguous()
            path = ref.launch_path(n, m, bs, e - s)
            assert _same(_call(pt2q, lay, x, torch.float32, False), want[s:e]), (path, value, s, e)
            assert _same(lay(x), want[s:e]), (path, value, s, e)


# ------------------------------------------------------------------ c. scale arrays with a guard

GUARD = 64  # fp32 elements of NaN before and after each array (the arrays stay 256-byte aligned)


def _guarded(t):
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=torch.float32, device=t.device)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("n,m,bs,tokens", ref.GUARD_SHAPES)
def test_scale_arrays_with_nan_guards(pt2q, n, m, bs, tokens, dtype):
    """K-split kernel, NT = 1 (5 tokens) and NT = 2 (130).  ceil(P / bs) > B: the padding positions
    of the last 128-position block have p / bs = B, one past the row's scales (for the last feature,
    past the array).  Their codes are 0 and they multiply a gathered 0, so whatever lies there --
    here a NaN -- must not be read into a weight: the scale block is clamped to B - 1.
    Before that clamp (tl_gemm_kernel read arow[p / bs]) this test gave NaN in feature n - 1 of
    every token, in all eight cases, and every other output was already exact."""
    c = ref.exact_case(n, m, bs, tokens, ref.case_seed(n, m, bs, tokens))
    lay = _layer(pt2q, c, dtype, compat=False)
    lay._prepare()
    codes, gather, a32, m32, b32 = lay._packed
    (abuf, a32), (mbuf, m32), (bbuf, b32) = _guarded(a32), _guarded(m32), _guarded(b32)
    lay._packed = (codes, gather, a32, m32, b32)
    snaps = [b.clone().view(torch.int32) for b in (abuf, mbuf, bbuf)]
    x = cuda(c["x"]).to(TDT[dtype])
    y16 = lay(x)
    y32 = _call(pt2q, lay, x, torch.float32, False)
    bad = torch.isnan(y16.float()).nonzero().cpu().tolist()
    assert _same(y16, ref.exact_reference(c, False, True, dtype)), f"NaN at (token, feature) {bad[:8]}"
    assert _same(y32, ref.exact_reference(c, False, False))
    for b, s in zip((abuf, mbuf, bbuf), snaps):
        assert torch.equal(b.view(torch.int32), s)


# ------------------------------------------------------------------ d. stale pack

def _stale_cases():
    n, m, bs, tokens = ref.STALE_SHAPE
    seed = ref.case_seed(n, m, bs, tokens)
    return ref.exact_case(n, m, bs, tokens, seed), ref.exact_case(n, m, bs, tokens, seed + 1)


def test_pack_follows_load_state_dict(pt2q):
    """forward (packs A), load_state_dict of layer B, on the module and through a parent: the next
    forward is layer B's, bit for bit."""
    A, Bc = _stale_cases()
    layB = _layer(pt2q, Bc, "fp16", False)
    x = cuda(A["x"]).half()
    wantA = ref.exact_reference(A, False, True, "fp16")
    yB = layB(x)
    lay = _layer(pt2q, A, "fp16", False)
    assert _same(lay(x), wantA)
    assert not torch.equal(lay(x), yB)
    lay.load_state_dict(layB.state_dict())
    assert torch.equal(lay(x), yB)
    seq = torch.nn.Sequential(_layer(pt2q, A, "fp16", False))
    assert _same(seq(x), wantA)
    seq.load_state_dict(torch.nn.Sequential(layB).state_dict())
    assert torch.equal(seq(x), yB)
    assert _same(layB(cuda(Bc["x"]).half()), ref.exact_reference(Bc, False, True, "fp16"))


def _fresh_bf16(pt2q, lay16):
    n, m = lay16.out_features, lay16.in_features
    fresh = pt2q.TernaryLinear(m, n, lay16.block_size, bias=True, dtype=torch.bfloat16, decode="mfma")
    fresh.load_state_dict(lay16.state_dict())
    return fresh


def test_pack_follows_dtype_cast_and_move(pt2q):
    """After a forward, .bfloat16() on the module (and on a parent) must give the output of a fresh
    bf16 layer loaded from the same state dict, and .to("cuda:0") still computes.  Exact data first
    (the issue's case; its scales survive the cast unchanged), then scales in the range of real
    layers, whose bf16 rounding a stale fp16 pack would miss."""
    A, _ = _stale_cases()
    rng = np.random.default_rng(5)
    R = dict(A, alpha=(rng.random(A["alpha"].shape) * 0.05 + 0.005).astype(np.float32),
             mu=(rng.standard_normal(A["mu"].shape) * 0.002).astype(np.float32))
    x = cuda(A["x"])
    for c, exact in ((A, True), (R, False)):
        lay = _layer(pt2q, c, "fp16", False)
        y16 = lay(x.half())
        fresh = _fresh_bf16(pt2q, lay)
        want = fresh(x.bfloat16())
        if exact:
            assert _same(y16, ref.exact_reference(A, False, True, "fp16"))
            assert _same(want, ref.exact_reference(A, False, True, "bf16"))
        else:  # the cast changes the scales, so a pack made before it computes something else
            assert not torch.equal(lay.alpha.bfloat16().float(), lay.alpha.float())
        lay.bfloat16()
        got = lay(x.bfloat16())
        assert got.dtype == torch.bfloat16 and torch.equal(got, want)
        lay.to("cuda:0")
        assert torch.equal(lay(x.bfloat16()), want)
        seq = torch.nn.Sequential(_layer(pt2q, c, "fp16", False))
        seq(x.half())
        seq.bfloat16()
        assert torch.equal(seq(x.bfloat16()), want)
