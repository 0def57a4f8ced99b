"""DOT64P, the fused decode kernel's arithmetic contract, on the CPU: the numpy
restatement (tests/ternary_decode_ref.py) against the float64 product of the same rounded operands
and the reference's recorded outputs, its own invariants, and the C entry's argument checks
(no device needed)."""
import ctypes

import numpy as np
import pytest
import torch

import ternary_decode_ref as ref
from conftest import load_golden
from oracle import oracle as orc

RTOL, ATOL = 2e-3, 2e-3  # tests/test_gpu_ternary.py


def _f64_bf16(c):
    """tests/test_gpu_ternary.py's bf16 check value: float64 product of the bf16-rounded operands."""
    n, m, bs = c["n"], c["m"], c["bs"]
    W = np.zeros((n, m), np.float32)
    for k in range(c["alpha"].shape[1]):
        cols = c["perm"][k * bs:(k + 1) * bs]
        W[:, cols] = ref.round16(c["alpha"][:, k:k + 1] * c["T"][:, cols].astype(np.float32)
                                 + c["mu"][:, k:k + 1], "bf16")
    y = c["x"].astype(np.float64) @ W.astype(np.float64).T + c["bias"].astype(np.float64)
    return ref.round16(y.astype(np.float32), "bf16")


@pytest.mark.parametrize("n,m,bs,tokens,dtype", ref.SHAPES)
def test_restatement_vs_float64(n, m, bs, tokens, dtype):
    c = ref.make_case(n, m, bs, tokens, dtype)
    y = ref.reference(c)
    if dtype == "fp16":
        yo = orc.ternary_linear(c["x"], c["alpha"], c["mu"], c["T"], c["perm"], c["bias"], bs,
                                compat=False).astype(np.float32)
        rtol, atol = RTOL, ATOL * max(1.0, np.sqrt(m / 512))
    else:
        yo, rtol, atol = _f64_bf16(c), 1.6e-2, 1e-2
    np.testing.assert_allclose(y, yo, rtol=rtol, atol=atol)


@pytest.mark.parametrize("name", ["ternary_linear_384x512", "ternary_linear_200x1000_pc"])
def test_restatement_vs_reference_outputs(name):
    """Compat semantics against the reference's own fp16 outputs (first 8 rows of x)."""
    g = load_golden(name)
    x = g["x"][:8].astype(np.float32)
    y = ref.decode(x, ref.round16(g["alpha"], "fp16"), ref.round16(g["mu"], "fp16"), g["T"], g["perm"],
                   g["bias"].astype(np.float32), int(g["block_size"]), "fp16", compat=True)
    np.testing.assert_allclose(y, g["out"][:8].astype(np.float32), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("n,m,bs,tokens,dtype", ref.SHAPES[:5])
def test_products_are_exact(n, m, bs, tokens, dtype):
    c = ref.make_case(n, m, bs, tokens, dtype)
    y = ref.decode(c["x"], c["alpha"], c["mu"], c["T"], c["perm"], c["bias"], bs, dtype, check_exact=True)
    assert np.array_equal(y, ref.reference(c))


def test_products_are_exact_at_the_dtype_extremes():
    """16-bit x 16-bit significands (11 or 8 bits each) fit fp32's 24: exact wherever the exponent
    stays in range, which fp16 always does (2^-48 .. 2^32)."""
    for dt, vals in ((np.float16, [6.0e-8, 65504.0, 1.0009765625, 0.333251953125]),):
        v = np.array(vals, dt).astype(np.float32)
        p32 = v[:, None] * v[None, :]
        assert np.array_equal(p32.astype(np.float64), v[:, None].astype(np.float64) * v[None, :].astype(np.float64))


@pytest.mark.parametrize("n,m,bs,dtype", [(96, 1100, 128, "fp16"), (130, 8320, 128, "fp16"), (40, 1030, 64, "bf16")])
def test_token_invariance_of_the_restatement(n, m, bs, dtype):
    c = ref.make_case(n, m, bs, 8, dtype)
    y8 = ref.reference(c)
    for t in (0, 5):
        y1 = ref.decode(c["x"][t:t + 1], c["alpha"], c["mu"], c["T"], c["perm"], c["bias"], bs, dtype)
        assert np.array_equal(y8[t:t + 1], y1)


def test_packed_bytes_roundtrip():
    """packed_bytes restates tl_pack_kernel's layout: position p's code + 1 sits at byte
    32 kb + 16 h + 2 g + j / 4, bits 2 (j % 4)."""
    c = ref.make_case(5, 300, 128, 1, "fp16")
    codes, gather = ref.pack(c["T"], c["perm"], compat=False)
    by = ref.packed_bytes(codes)
    P = ref.positions(300)
    assert by.shape == (5, P // 4) and gather.shape == (P,) and (gather[300:] == -1).all()
    for p in (0, 7, 8, 15, 16, 127, 128, 299, 300, P - 1):
        kb, g, h, j = p // 128, (p % 128) // 16, (p % 16) // 8, p % 8
        got = (by[:, 32 * kb + 16 * h + 2 * g + j // 4] >> (2 * (j % 4))) & 3
        assert np.array_equal(got.astype(np.int8) - 1, codes[:, p])
    assert np.array_equal(codes[:, :300], c["T"][:, c["perm"]])


def test_argument_errors_without_device(pt2q):
    lib = pt2q._lib.lib()
    E_ARG, E_UNSUPPORTED = 1, 3  # include/pt2q.h
    p = ctypes.c_void_p(4096)
    F32, F16, BF16 = 0, 1, 2

    def call(x=p, xdt=F16, tokens=4, ldx=128, n=16, m=128, codes=p, gather=p, alpha=p, mu=p, B=1, bs=128,
             y=p, ydt=F16, ldy=16):
        return lib.pt2q_ternary_decode(x, xdt, tokens, ldx, n, m, codes, gather, alpha, mu, B, bs, None, y, ydt,
                                       ldy, None)
    assert lib.pt2q_ternary_decode_max_tokens() == 8
    assert pt2q.ternary.decode_max_tokens <= 8
    assert call(tokens=9) == E_UNSUPPORTED
    for kw in ("x", "codes", "gather", "alpha", "mu", "y"):
        assert call(**{kw: None}) == E_ARG, kw
    assert call(ldx=127) == E_ARG and call(ldy=15) == E_ARG
    assert call(tokens=0) == E_ARG and call(n=0) == E_ARG and call(m=0) == E_ARG
    assert call(m=300, ldx=300, bs=128, B=2) == E_ARG          # too few scale blocks
    assert call(ydt=BF16) == E_ARG                             # ydtype neither xdtype nor F32
    assert call(xdt=F32, ydt=F32) == E_UNSUPPORTED             # non-16-bit x
    assert call(m=300, ldx=300, bs=24, B=13) == E_UNSUPPORTED  # bs < m, bs % 16 != 0
    assert call(m=40000, ldx=40000, B=313) == E_UNSUPPORTED    # a token's activations past the LDS budget


def test_python_surface(pt2q):
    assert pt2q.ternary.decode_max_tokens >= 1
    assert callable(pt2q.ternary_decode) and callable(pt2q.set_decode)
    with pytest.raises(ValueError):
        pt2q.ternary._check_mode("eager")
    with pytest.raises(pt2q._lib.Pt2qError):  # no CPU path
        pt2q.ternary_decode(torch.zeros(1, 128, dtype=torch.float16), torch.zeros(4, 32, dtype=torch.uint8),
                            torch.zeros(128, dtype=torch.int32), torch.ones(4, 1), torch.zeros(4, 1), 128)
