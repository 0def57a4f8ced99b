"""CPU restatement of contracts RMSNORM16 and RESADD16, the norm prologue and the
residual epilogue of the decode kernel and the stand-alone pt2q_rmsnorm (csrc/ternary_decode.hip),
in numpy float32 -- a plain helper for the norm tests, not a conftest.

  RMSNORM16, per token row x[0..m) of dtype TX, weight w[0..m) of TX, fp32 eps
    partial j in [0, 512):  acc = fmaf(xf, xf, acc) from +0 over i = j, j + 512, ... ascending
    wave sum k in [0, 8):   partials 64 k .. 64 k + 63 folded by v = v + v[lane ^ s], s = 32 .. 1
    ss = ((s0 + s1) + s2) + ... + s7
    mean = ss / (float)m;  v = mean + eps;  r = 1 / sqrt(v)     (each correctly rounded fp32)
    xn = RN_TX(xf * r);  out = RN_TX(xn * wf)
  RESADD16
    y = RN_TY(f32(y0) + f32(res)) for y0 = RN_TY(v + bias), what the call without a residual stores

Every operation is one fp32 operation rounded to nearest even; none is fused except the fmaf of
the chains, whose product must be exact in fp32 for this restatement (it always is for fp16; for
bf16 it is while x² neither overflows nor falls below 2^-126: rmsnorm asserts it)."""
import numpy as np

import ternary_decode_ref as ref

F = np.float32
CHAINS, WAVE = 512, 64


def partials(x):
    """(tokens x 512) chain sums of squares; a chain with no element stays +0."""
    x = np.asarray(x, F)
    tokens, m = x.shape
    acc = np.zeros((tokens, CHAINS), F)
    for i0 in range(0, m, CHAINS):
        seg = x[:, i0:i0 + CHAINS]
        prod = seg * seg
        assert np.array_equal(prod.astype(np.float64), seg.astype(np.float64) ** 2), "x² is not exact in fp32"
        acc[:, :seg.shape[1]] = acc[:, :seg.shape[1]] + prod  # fp32 add of the exact product: fmaf
    assert acc.dtype == F
    return acc


def sum_of_squares(x):
    """ss (tokens,): the butterfly per 64 chains, then the eight wave sums in order."""
    p = partials(x).reshape(-1, CHAINS // WAVE, WAVE)
    lanes = np.arange(WAVE)
    for s in (32, 16, 8, 4, 2, 1):
        p = p + p[:, :, lanes ^ s]
    ss = p[:, 0, 0]
    for k in range(1, CHAINS // WAVE):
        ss = ss + p[:, k, 0]
    assert p.dtype == F and ss.dtype == F
    return ss


def scale(x, eps):
    """r (tokens,) = 1 / sqrt(ss / m + eps)."""
    x = np.asarray(x, F)
    ss = sum_of_squares(x)
    with np.errstate(divide="ignore"):  # an all-zero row with eps = 0 is outside the contract
        mean = ss / F(x.shape[1])
        v = mean + F(eps)
        r = F(1) / np.sqrt(v)
    assert all(a.dtype == F for a in (mean, v, r))
    return r


def rmsnorm(x, w, eps, dtype):
    """out (tokens x m, float32 holding dtype values) for x, w already rounded to dtype."""
    x = np.atleast_2d(np.asarray(x, F))
    w = np.asarray(w, F)
    assert np.array_equal(ref.round16(x, dtype), x) and np.array_equal(ref.round16(w, dtype), w)
    r = scale(x, eps)
    with np.errstate(over="ignore", invalid="ignore"):
        p1 = x * r[:, None]
        xn = ref.round16(p1, dtype)
        p2 = xn * w[None, :]
        out = ref.round16(p2, dtype)
    assert all(a.dtype == F for a in (p1, xn, p2, out))
    return out


def resadd(y0, res, dtype):
    """RN_TY(y0 + res) for y0, res holding dtype values."""
    with np.errstate(over="ignore"):  # a sum past the top of TY (bf16: of fp32) is inf, as on the device
        s = np.asarray(y0, F) + np.asarray(res, F)
        assert s.dtype == F
        return ref.round16(s, dtype)


def rmsnorm64(x, w, eps):
    """x w / sqrt(mean(x²) + eps) in float64."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    return x * np.asarray(w, np.float64)[None, :] / np.sqrt((x * x).mean(axis=1, keepdims=True) + float(F(eps)))


def make_inputs(tokens, m, dtype, seed, scale_x=1.0):
    """x ~ N(0, 1) scale_x and w = 1 +- 0.5, both rounded to dtype."""
    rng = np.random.default_rng(seed)
    x = ref.round16(rng.standard_normal((tokens, m)) * scale_x, dtype)
    w = ref.round16(1.0 + rng.uniform(-0.5, 0.5, size=m), dtype)
    return x, w
