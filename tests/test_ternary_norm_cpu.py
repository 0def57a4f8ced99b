"""Contracts RMSNORM16 and RESADD16 as restated in tests/ternary_norm_ref.py, without
a GPU: the restatement against a float64 evaluation of x w / sqrt(mean(x²) + eps) within two
roundings to TX, its own structure (float32 throughout, ragged chains, signed zeros), and RESADD16
against torch's 16-bit add on the CPU."""
import numpy as np
import pytest
import torch

import ternary_decode_ref as ref
import ternary_norm_ref as nref

F = np.float32
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
PREC = {"fp16": 11, "bf16": 8}
EPS = 1e-5


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("m", [100, 1030, 4096, 8320])
def test_restatement_within_two_roundings_of_float64(m, dtype):
    """|out - ref| <= (2^-(p-1) + 2^-20) |ref|: xn and out are each one rounding to TX (2^-p
    relative each, 2^-(p-1) together to first order), and r carries the fp32 error of a sum of m
    squares, a division, a square root and a reciprocal, far inside 2^-20.  fp16 results below the
    normal range (2^-14), where a rounding is absolute, are excluded."""
    p = PREC[dtype]
    bound = 2.0 ** -(p - 1) + 2.0 ** -20
    worst = 0.0
    for k, sx in enumerate((1.0, 0.05, 3.0, 20.0)):
        x, w = nref.make_inputs(3, m, dtype, seed=m + k, scale_x=sx)
        out = nref.rmsnorm(x, w, EPS, dtype)
        assert out.dtype == F and out.shape == x.shape
        want = nref.rmsnorm64(x, w, EPS)
        keep = np.abs(want) >= 2.0 ** -14 if dtype == "fp16" else want != 0
        rel = np.abs(out.astype(np.float64) - want)[keep] / np.abs(want)[keep]
        worst = max(worst, float(rel.max()))
        assert keep.sum() > 0.9 * keep.size
    print(f"m {m} {dtype}: max relative error {worst:.5f}, bound {bound:.5f}")
    assert worst <= bound


def _slow(x, w, eps, dtype):
    """RMSNORM16 for one row by scalar loops, written from the contract's text alone."""
    m = x.size
    part = []
    for j in range(512):
        acc = F(0)
        for i in range(j, m, 512):
            acc = F(np.float64(x[i]) * np.float64(x[i]) + np.float64(acc))  # exact product and sum, one rounding
        part.append(acc)
    sums = []
    for k in range(8):
        v = np.array(part[64 * k:64 * k + 64], F)
        for s in (32, 16, 8, 4, 2, 1):
            v = v + v[np.arange(64) ^ s]
        sums.append(v[0])
    ss = sums[0]
    for k in range(1, 8):
        ss = F(ss + sums[k])
    r = F(1) / np.sqrt(F(F(ss / F(m)) + F(eps)))
    return ref.round16(ref.round16(x * r, dtype) * w, dtype)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("m", [5, 63, 100, 520, 1030])
def test_ragged_partials(m, dtype):
    """m < 64 (one wave holds every element, seven wave sums are +0) and m not a multiple of 512
    (the last element of some chains is missing): the vectorised restatement is the scalar one.
    The float64 sum in _slow is exact here (a 22-bit product beside a 24-bit accumulator of nearby
    exponent), so its single rounding is fmaf's."""
    x, w = nref.make_inputs(2, m, dtype, seed=900 + m)
    out = nref.rmsnorm(x, w, EPS, dtype)
    for t in range(2):
        assert np.array_equal(out[t], _slow(x[t], w, EPS, dtype))
    p = nref.partials(x)
    assert p.shape == (2, 512) and bool((p[:, min(m, 512):] == 0).all()) and bool((p[:, :min(m, 512)] > 0).all())


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_zero_row_keeps_the_signs(dtype):
    rng = np.random.default_rng(3)
    m = 200
    x = np.where(rng.random((1, m)) < 0.5, F(0.0), F(-0.0)).astype(F)
    w = ref.round16(rng.standard_normal(m), dtype)
    out = nref.rmsnorm(x, w, EPS, dtype)
    assert bool((out == 0).all())
    assert np.array_equal(np.signbit(out), np.signbit(x) ^ np.signbit(w)[None, :])


def test_every_intermediate_is_float32():
    x, w = nref.make_inputs(2, 700, "bf16", seed=1)
    assert nref.partials(x).dtype == F and nref.sum_of_squares(x).dtype == F and nref.scale(x, EPS).dtype == F
    assert nref.rmsnorm(x, w, EPS, "bf16").dtype == F  # and the asserts inside each of them
    assert nref.resadd(x, x, "bf16").dtype == F


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_resadd_is_torchs_16bit_add(dtype):
    """Random 16-bit patterns (every exponent, both signs, subnormals), pairs that cancel and pairs
    that overflow: torch's CPU res + y, bit for bit."""
    rng = np.random.default_rng(16)
    bits = rng.integers(0, 1 << 16, size=(2, 200000)).astype(np.uint16)
    t = torch.from_numpy(bits.view(np.int16)).view(TDT[dtype])
    y0, res = t[0], t[1]
    near = (res.float() * -1.0009765625).to(TDT[dtype])  # y0 close to -res: cancellation
    for a, b in ((y0, res), (near, res)):
        fin = torch.isfinite(a) & torch.isfinite(b)
        a, b = a[fin], b[fin]
        want = (b + a).float().numpy()
        got = nref.resadd(a.float().numpy(), b.float().numpy(), dtype)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
