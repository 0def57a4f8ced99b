"""The fused decode kernel (pt2q_ternary_decode, csrc/ternary_decode.hip) against the numpy
restatement of its arithmetic contract DOT64P (tests/ternary_decode_ref.py):
bit for bit, since every product is exact in fp32 and the summation order is fixed.  The module
path (TernaryLinear(decode="fused")) is also compared with the reference's recorded outputs at the
tolerances of tests/test_gpu_ternary.py."""
import numpy as np
import pytest
import torch

import ternary_decode_ref as ref
from conftest import load_golden
from test_gpu_parity import cuda, host

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-3, 2e-3
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
_CASES = {}


def device_case(pt2q, n, m, bs, tokens, dtype, compat=False):
    """A ref.make_case case with its device tensors: x (16-bit), the packed codes and gather of
    pt2q_ternary_pack, fp32 alpha / mu / bias.  Built once per shape."""
    key = (n, m, bs, tokens, dtype, compat)
    if key not in _CASES:
        c = ref.make_case(n, m, bs, tokens, dtype)
        lay = pt2q.TernaryLinear(m, n, bs, bias=True, dtype=TDT[dtype], compat=compat, decode="fused")
        lay.set_quantized_params(cuda(c["alpha"]), cuda(c["mu"]), cuda(c["T"]), cuda(c["perm"]), cuda(c["bias"]))
        lay._prepare()
        codes, gather, a32, m32, b32 = lay._packed
        d = {"x": cuda(c["x"]).to(TDT[dtype]), "codes": codes, "gather": gather, "alpha": a32, "mu": m32,
             "bias": b32, "layer": lay}
        # the scales reach the kernel exactly as the restatement takes them
        assert np.array_equal(host(a32), c["alpha"]) and np.array_equal(host(m32), c["mu"])
        assert np.array_equal(host(b32), c["bias"]) and np.array_equal(host(d["x"].float()), c["x"])
        _CASES[key] = (c, d)
    return _CASES[key]


def run(pt2q, d, bs, x=None, bias=True, out_dtype=None, out=None):
    return pt2q.ternary_decode(d["x"] if x is None else x, d["codes"], d["gather"], d["alpha"], d["mu"], bs,
                               d["bias"] if bias else None, out_dtype=out_dtype, out=out)


@pytest.mark.parametrize("f32out", [False, True], ids=["tx", "f32"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("n,m,bs,tokens,dtype", ref.SHAPES)
def test_bit_exact_vs_restatement(pt2q, n, m, bs, tokens, dtype, bias, f32out):
    c, d = device_case(pt2q, n, m, bs, tokens, dtype)
    y = run(pt2q, d, bs, bias=bias, out_dtype=torch.float32 if f32out else None)
    assert y.dtype == (torch.float32 if f32out else TDT[dtype]) and tuple(y.shape) == (tokens, n)
    want = ref.reference(c, bias=bias, out_dtype="fp32" if f32out else None)
    assert np.array_equal(host(y.float()), want)


# n = 5 rows, 3 tokens: a single workgroup whose waves 5-7 own no row, and a token count that is no
# multiple of the 4 tokens a workgroup takes -- unless ref.SHAPES already has such a case
FEW_ROWS = [] if any(s[0] < 8 for s in ref.SHAPES) else [(5, 100, 16, 3, "bf16")]


@pytest.mark.parametrize("n,m,bs,tokens,dtype", FEW_ROWS)
def test_fewer_rows_than_waves(pt2q, n, m, bs, tokens, dtype):
    c, d = device_case(pt2q, n, m, bs, tokens, dtype)
    assert np.array_equal(host(run(pt2q, d, bs).float()), ref.reference(c))


def test_single_entry_argument_errors_launch_nothing(pt2q):
    """The C entry pt2q_ternary_decode itself, by status: a valid call, then every refusal, after
    which y still holds its sentinel."""
    L = pt2q._lib
    E_ARG, E_UNSUPPORTED = 1, 3
    n, m, bs, tokens, dtype = ref.SHAPES[0]
    assert (n, m, bs, tokens, dtype) == (33, 100, 16, 2, "fp16")
    c, d = device_case(pt2q, n, m, bs, tokens, dtype)
    x = d["x"]
    B = d["alpha"].shape[1]

    def call(ntok=tokens, mm=m, Bv=B, bsv=bs, ldx=None, ldy=n, ydtype=torch.float16, null=None):
        y = torch.full((tokens, n), -77.0, dtype=torch.float16, device=x.device)
        p = {k: None if k == null else L.ptr(t) for k, t in (("codes", d["codes"]), ("gather", d["gather"]), ("y", y))}
        rc = L.lib().pt2q_ternary_decode(L.ptr(x), L.dtype_code(x), ntok, mm if ldx is None else ldx, n, mm,
                                         p["codes"], p["gather"], L.ptr(d["alpha"]), L.ptr(d["mu"]), Bv, bsv,
                                         L.ptr(d["bias"]), p["y"], L._DT[ydtype], ldy, L.stream_of(x.device))
        torch.cuda.synchronize()
        if rc == 0:
            assert np.array_equal(host(y.float()), ref.reference(c))
        else:
            assert bool((y == -77.0).all())
        return rc

    assert call() == 0  # the harness itself is a valid call
    assert call(null="codes") == E_ARG and call(null="gather") == E_ARG and call(null="y") == E_ARG
    assert call(ldx=m - 1) == E_ARG and call(ldy=n - 1) == E_ARG
    assert call(Bv=B - 1) == E_ARG
    assert call(ntok=0) == E_ARG
    assert call(ydtype=torch.bfloat16) == E_ARG
    assert call(ntok=9) == E_UNSUPPORTED
    assert call(bsv=24) == E_UNSUPPORTED  # below m, not a multiple of 16
    assert call(mm=32769, Bv=-(-32769 // bs)) == E_UNSUPPORTED


@pytest.mark.parametrize("n,m,bs,tokens,dtype", ref.SHAPES[:3])
def test_pack_matches_restated_layout(pt2q, n, m, bs, tokens, dtype):
    """The buffers the kernel consumes are the ones the restatement builds its positions from."""
    c, d = device_case(pt2q, n, m, bs, tokens, dtype)
    codes, gather = ref.pack(c["T"], c["perm"], compat=False)
    assert np.array_equal(host(d["codes"]), ref.packed_bytes(codes))
    assert np.array_equal(host(d["gather"]), gather)


@pytest.mark.parametrize("n,m,bs,dtype", [(96, 1100, 128, "fp16"), (130, 8320, 128, "fp16")])
def test_token_invariance(pt2q, n, m, bs, dtype):
    """Row t of a T-token call equals the 1-token call on that row, whatever T (and so whatever
    token grouping the launcher picks)."""
    c, d = device_case(pt2q, n, m, bs, 8, dtype)
    single = torch.cat([run(pt2q, d, bs, x=d["x"][t:t + 1]) for t in range(8)])
    assert np.array_equal(host(single.float()), ref.reference(c))
    for T in (1, 2, 3, 5, 8):
        assert torch.equal(run(pt2q, d, bs, x=d["x"][:T]), single[:T]), T
        assert torch.equal(run(pt2q, d, bs, x=d["x"][8 - T:]), single[8 - T:]), T


@pytest.mark.parametrize("n,m,bs,tokens,dtype", [(33, 100, 16, 2, "fp16"), (40, 1030, 64, 8, "bf16"),
                                                 (130, 8320, 128, 8, "fp16")])
@pytest.mark.parametrize("f32out", [False, True], ids=["tx", "f32"])
def test_strides_and_alignment(pt2q, n, m, bs, tokens, dtype, f32out):
    """x a column slice (ldx > m, base 2 bytes off 16-byte alignment), y with ldy > n whose padding
    keeps its sentinel."""
    c, d = device_case(pt2q, n, m, bs, tokens, dtype)
    buf = torch.zeros((tokens, m + 11), dtype=TDT[dtype], device=d["x"].device)
    buf[:, 1:1 + m] = d["x"]
    xv = buf[:, 1:1 + m]
    assert xv.data_ptr() % 16 == 2 and xv.stride(0) > m
    odt = torch.float32 if f32out else TDT[dtype]
    ybuf = torch.full((tokens, n + 5), -77.0, dtype=odt, device=d["x"].device)
    run(pt2q, d, bs, x=xv, out_dtype=odt, out=ybuf[:, :n])
    want = ref.reference(c, out_dtype="fp32" if f32out else None)
    assert np.array_equal(host(ybuf[:, :n].float()), want)
    assert bool((ybuf[:, n:] == -77.0).all())
    # a gather index 4 bytes off 16-byte alignment (the kernel then reads it element by element)
    gbuf = torch.empty(d["gather"].numel() + 1, dtype=torch.int32, device=d["x"].device)
    gbuf[1:] = d["gather"]
    assert gbuf[1:].data_ptr() % 16 == 4
    y = pt2q.ternary_decode(xv, d["codes"], gbuf[1:], d["alpha"], d["mu"], bs, d["bias"], out_dtype=odt)
    assert np.array_equal(host(y.float()), want)


@pytest.mark.parametrize("tokens,dtype", [(1, "fp16"), (3, "bf16")])
def test_wide_layer(pt2q, tokens, dtype):
    """m = 28672 (seven rounds of pieces): one token's activations need more than 64 KiB of LDS, and
    three tokens go one per workgroup."""
    n, m, bs = 24, 28672, 128
    c, d = device_case(pt2q, n, m, bs, tokens, dtype)
    assert np.array_equal(host(run(pt2q, d, bs).float()), ref.reference(c))


def test_subnormal_activations(pt2q):
    """fp16 x whose only non-zero entries are f16 subnormals, fp32 output: an input flushed to zero
    on its way into the multiply would show as a changed (or zero) sum."""
    n, m, bs = 96, 1100, 128
    c, d = device_case(pt2q, n, m, bs, 3, "fp16")
    rng = np.random.default_rng(5)
    x = np.zeros((3, m), np.float16)
    idx = rng.random((3, m)) < 0.3
    sub = (rng.integers(1, 1024, size=(3, m)).astype(np.uint16) | (rng.integers(0, 2, size=(3, m)).astype(np.uint16) << 15))
    x.view(np.uint16)[idx] = sub[idx]
    assert (np.abs(x[idx].astype(np.float32)) < 6.2e-5).all() and idx.sum() > 100
    want = ref.decode(x.astype(np.float32), c["alpha"], c["mu"], c["T"], c["perm"], None, bs, "fp16", out_dtype="fp32")
    assert np.count_nonzero(want) > 0.99 * want.size
    y = run(pt2q, d, bs, x=cuda(x), bias=False, out_dtype=torch.float32)
    assert np.array_equal(host(y), want)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_zero_activations_and_zero_codes(pt2q, dtype):
    """All-zero x with negative mu: +bias, or +0 (never -0) without bias.  A row of all-zero codes:
    every weight is RN(mu)."""
    n, m, bs = 40, 1030, 64
    c = ref.make_case(n, m, bs, 2, dtype, seed=11)
    c["mu"] = ref.round16(-np.abs(c["mu"]) - np.float32(2.0 ** -7), dtype)
    c["T"][3] = 0
    lay = pt2q.TernaryLinear(m, n, bs, bias=True, dtype=TDT[dtype], decode="fused")
    lay.set_quantized_params(cuda(c["alpha"]), cuda(c["mu"]), cuda(c["T"]), cuda(c["perm"]), cuda(c["bias"]))
    lay._prepare()
    codes, gather, a32, m32, b32 = lay._packed
    z = torch.zeros((2, m), dtype=TDT[dtype], device=codes.device)
    y0 = host(pt2q.ternary_decode(z, codes, gather, a32, m32, bs, None, out_dtype=torch.float32))
    assert not y0.any() and not np.signbit(y0).any()
    yb = host(pt2q.ternary_decode(z, codes, gather, a32, m32, bs, b32, out_dtype=torch.float32))
    assert np.array_equal(yb, np.broadcast_to(c["bias"], (2, n))) and \
        np.array_equal(np.signbit(yb), np.broadcast_to(np.signbit(c["bias"]), (2, n)))
    y = host(pt2q.ternary_decode(cuda(c["x"]).to(TDT[dtype]), codes, gather, a32, m32, bs, b32).float())
    want = ref.decode(c["x"], c["alpha"], c["mu"], c["T"], c["perm"], c["bias"], bs, dtype)
    assert np.array_equal(y, want)


@pytest.fixture
def cap8(pt2q, monkeypatch):
    """Fused modules take every token count the library does (the shipped decode_max_tokens is the
    measured crossover, which is lower)."""
    monkeypatch.setattr(pt2q.ternary, "decode_max_tokens", pt2q._lib.lib().pt2q_ternary_decode_max_tokens())
    assert pt2q.ternary.decode_max_tokens == 8


def _golden_layer(pt2q, g, compat, decode):
    n, m = int(g["n"]), int(g["m"])
    lay = pt2q.TernaryLinear(m, n, int(g["block_size"]), bias=True, dtype=torch.float16, compat=compat, decode=decode)
    lay.set_quantized_params(cuda(g["alpha"]), cuda(g["mu"]), cuda(g["T"]), cuda(g["perm"]),
                             cuda(g["bias"].astype(np.float32)))
    return lay


@pytest.mark.parametrize("compat", [True, False], ids=["compat", "correct"])
@pytest.mark.parametrize("name", ["ternary_linear_384x512", "ternary_linear_200x1000_pc"])
def test_module_fused_on_golden(pt2q, cap8, name, compat):
    from oracle import oracle as orc
    g = load_golden(name)
    lay = _golden_layer(pt2q, g, compat, "fused")
    x = cuda(g["x"][:8])
    y = lay(x)
    if compat:
        np.testing.assert_allclose(host(y.float()), g["out"][:8].astype(np.float32), rtol=RTOL, atol=ATOL)
    yo = orc.ternary_linear(g["x"][:8], g["alpha"], g["mu"], g["T"], g["perm"], g["bias"], int(g["block_size"]),
                            compat=compat).astype(np.float32)
    np.testing.assert_allclose(host(y.float()), yo, rtol=RTOL, atol=ATOL)
    codes, gather, a32, m32, b32 = lay._packed
    assert torch.equal(y, pt2q.ternary_decode(x, codes, gather, a32, m32, int(g["block_size"]), b32))
    want = ref.decode(g["x"][:8].astype(np.float32), ref.round16(g["alpha"], "fp16"), ref.round16(g["mu"], "fp16"),
                      g["T"], g["perm"], g["bias"].astype(np.float32), int(g["block_size"]), "fp16", compat=compat)
    assert np.array_equal(host(y.float()), want)
    # a leading batch dimension flattens into tokens
    assert torch.equal(lay(x[:4].reshape(2, 2, -1)), y[:4].reshape(2, 2, -1))


def test_module_falls_back_to_mfma_path_exactly(pt2q, cap8):
    """More tokens than decode_max_tokens through a fused module, and any call through the default
    module, give exactly what decode="mfma" gives."""
    g = load_golden("ternary_linear_384x512")
    fused, mfma = _golden_layer(pt2q, g, False, "fused"), _golden_layer(pt2q, g, False, "mfma")
    n, m = int(g["n"]), int(g["m"])
    default = pt2q.TernaryLinear(m, n, int(g["block_size"]), bias=True, dtype=torch.float16)
    default.set_quantized_params(cuda(g["alpha"]), cuda(g["mu"]), cuda(g["T"]), cuda(g["perm"]),
                                 cuda(g["bias"].astype(np.float32)))
    assert default.decode == "mfma" and pt2q.ternary.decode_max_tokens <= 8
    x9 = cuda(g["x"][:9])
    assert torch.equal(fused(x9), mfma(x9))
    for T in (1, 3, 9):
        assert torch.equal(default(x9[:T]), mfma(x9[:T]))
    with pytest.raises(ValueError):
        pt2q.TernaryLinear(m, n, decode="eager")


def test_module_at_the_shipped_crossover(pt2q):
    """With decode_max_tokens as shipped: up to that many tokens take the fused kernel (bit-equal to
    the functional call), one more takes the MFMA path exactly."""
    g = load_golden("ternary_linear_384x512")
    fused, mfma = _golden_layer(pt2q, g, False, "fused"), _golden_layer(pt2q, g, False, "mfma")
    k = pt2q.ternary.decode_max_tokens
    assert 1 <= k <= 8
    x = cuda(g["x"][:k + 1])
    codes, gather, a32, m32, b32 = (fused(x[:1]), fused._packed)[1]
    assert torch.equal(fused(x[:k]), pt2q.ternary_decode(x[:k], codes, gather, a32, m32, 128, b32))
    assert torch.equal(fused(x), mfma(x))


def test_set_decode_on_sequential(pt2q, cap8):
    ga, gb = load_golden("ternary_linear_384x512"), load_golden("ternary_linear_200x1000_pc")
    # 512 -> 384, then a 384 -> 200 layer cut from the second fixture's first 384 columns
    l0 = _golden_layer(pt2q, ga, False, "mfma")
    l1 = pt2q.TernaryLinear(384, 200, 128, bias=True, dtype=torch.float16)
    l1.set_quantized_params(cuda(np.repeat(gb["alpha"], 3, axis=1)), cuda(np.repeat(gb["mu"], 3, axis=1)),
                            cuda(np.ascontiguousarray(gb["T"][:, :384])), torch.randperm(384, device="cuda"),
                            cuda(gb["bias"].astype(np.float32)))
    model = torch.nn.Sequential(l0, l1)
    x = cuda(ga["x"][:4])
    y_mfma = model(x)
    assert pt2q.set_decode(model, "fused") is model and [l.decode for l in model] == ["fused", "fused"]
    y_fused = model(x)
    h = pt2q.ternary_decode(x, *l0._packed[:4], 128, l0._packed[4])
    assert torch.equal(y_fused, pt2q.ternary_decode(h, *l1._packed[:4], 128, l1._packed[4]))
    np.testing.assert_allclose(host(y_fused.float()), host(y_mfma.float()), rtol=1e-2, atol=2e-2)
    pt2q.set_decode(model, "mfma")
    assert torch.equal(model(x), y_mfma)
    with pytest.raises(ValueError):
        pt2q.set_decode(model, "eager")


def test_replace_linear_passes_decode(pt2q, cap8):
    g = load_golden("ternary_linear_384x512")
    n, m = int(g["n"]), int(g["m"])
    model = torch.nn.Sequential(torch.nn.Linear(m, n, bias=True)).cuda().half()
    model[0].bias.data = cuda(g["bias"]).half()
    params = {"0": {"alpha": cuda(g["alpha"]).half(), "mu": cuda(g["mu"]).half(), "T": cuda(g["T"]),
                    "perm": cuda(g["perm"])}}
    pt2q.replace_linear_with_ternary(model, params, block_size=128, compat=True, decode="fused")
    assert model[0].decode == "fused"
    y = model(cuda(g["x"][:2]))
    np.testing.assert_allclose(host(y.float()), g["out"][:2].astype(np.float32), rtol=RTOL, atol=ATOL)


def test_graph_capture_replays_eager_bits(pt2q):
    """Two fused decode calls on one stream (no parallel branches), captured the way
    engine.LayerGraph captures a layer; the replay gives the eager bits."""
    c, d = device_case(pt2q, 96, 1100, 128, 3, "fp16")
    _, d2 = device_case(pt2q, 33, 100, 16, 2, "fp16")
    y1 = torch.empty((3, 96), dtype=torch.float16, device=d["x"].device)
    y2 = torch.empty((2, 33), dtype=torch.float32, device=d["x"].device)

    def both():
        run(pt2q, d, 128, out=y1)
        run(pt2q, d2, 16, out_dtype=torch.float32, out=y2)
    both()  # eager warm-up: loads the kernels before capture
    torch.cuda.synchronize()
    e1, e2 = y1.clone(), y2.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    y1.zero_()
    y2.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y1, e1) and torch.equal(y2, e2)
    assert np.array_equal(host(y1.float()), ref.reference(c))
