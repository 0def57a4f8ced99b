"""CPU restatement of contract SWIGLU16, the SWIGLU epilogue of the decode kernel
(csrc/ternary_decode.hip), in numpy float32 -- a plain helper for the group tests, not a
conftest.  g and u come from DOT64P (tests/ternary_decode_ref.py: fold, finish, round16).

  g = RN_TY(v_gate + bias_gate),  u = RN_TY(v_up + bias_up)
  a = |g|;  t = a * (-LOG2E)
  if t < -125:  e = 0
  else: n = rint(t);  r = (-a) - n*LN2_HI;  r = r - n*LN2_LO
        p = c6; for k = 5..0: p = p*r; p = p + c_k
        e = ldexp(p, n)
  q = (g >= 0 ? 1 : e) / (1 + e);   s = RN_TY(g * q);   h = RN_TY(s * u)

Every operation is one fp32 operation rounded to nearest even; none is fused."""
import numpy as np

import ternary_decode_ref as ref

F = np.float32


def _f(bits):
    return np.array(bits, np.uint32).view(F)


LOG2E = _f(0x3FB8AA3B)
LN2_HI = _f(0x3F317200)  # 15 significant bits: n * LN2_HI is exact for |n| <= 125
LN2_LO = _f(0x35BFBE8E)
C = _f([0x3F800000, 0x3F800000, 0x3F000000, 0x3E2AA9FB, 0x3D2AAA2D, 0x3C093B5E, 0x3AB6D7B4])


def silu32(g):
    """g * q in fp32, before the rounding to TY (g: float32 array of finite values)."""
    g = np.asarray(g, F)
    a = np.abs(g)
    with np.errstate(over="ignore"):  # |g| near the top of bf16: t = -inf, which is below -125
        t = a * (-LOG2E)
    small = t < F(-125)
    n = np.rint(np.where(small, F(0), t)).astype(F)
    r = (-a) - n * LN2_HI
    r = r - n * LN2_LO
    r = np.where(small, F(0), r)
    p = np.full(g.shape, C[6], F)
    for k in range(5, -1, -1):
        p = p * r
        p = p + C[k]
    e = np.where(small, F(0), np.ldexp(p, n.astype(np.int32))).astype(F)
    q = np.where(g >= 0, F(1), e) / (F(1) + e)
    out = g * q
    assert all(v.dtype == F for v in (a, t, n, r, p, e, q, out))
    return out


def swiglu(g, u, dtype):
    """h = RN_TY(RN_TY(silu32(g)) * u) for g, u already rounded to dtype ("fp16" | "bf16")."""
    with np.errstate(over="ignore"):  # a product past the top of TY is inf, as on the device
        s = ref.round16(silu32(g), dtype)
        return ref.round16(s * np.asarray(u, F), dtype)


def silu64(g):
    """SiLU in float64, overflow-free: g / (1 + exp(-g)) for g >= 0, g exp(g) / (1 + exp(g)) below."""
    g = np.asarray(g, np.float64)
    e = np.exp(-np.abs(g))
    return g * np.where(g >= 0, 1.0, e) / (1.0 + e)


def finite16(dtype):
    """Every finite value of dtype, as float32."""
    b = np.arange(1 << 16, dtype=np.uint32)
    if dtype == "fp16":
        v = b.astype(np.uint16).view(np.float16).astype(F)
    else:
        v = (b << 16).view(F)
    return v[np.isfinite(v)]


def round16_from64(v, dtype):
    """float64 -> dtype with ONE rounding to nearest even, returned as float32.  bf16 goes through
    float32 rounded to odd (truncate, then set the last bit when inexact), which makes the second
    rounding safe: float32 keeps 16 bits more than bf16 at every exponent, subnormals included."""
    v = np.asarray(v, np.float64)
    if dtype == "fp16":
        return v.astype(np.float16).astype(F)
    f = v.astype(F)
    over = np.abs(f.astype(np.float64)) > np.abs(v)
    f = np.where(over, np.nextafter(f, F(0)), f).astype(F)  # truncated toward zero
    inexact = f.astype(np.float64) != v
    f = (f.view(np.uint32) | inexact.astype(np.uint32)).view(F)
    return ref.round16(f, "bf16")
