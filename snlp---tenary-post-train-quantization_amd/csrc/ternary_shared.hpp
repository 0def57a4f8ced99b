// What the ternary decode kernel (ternary_decode.hip) and the skinny kernels (ternary_skinny.hip)
// share: the exact 16-bit <-> fp32 conversions, the arithmetic of contracts SWIGLU16 and RMSNORM16
// (DESIGN.md §3), and the select that reads one member's entry of a by-value group argument.
// One definition, so the two files' SwiGLU epilogues and norm prologues cannot drift apart.
#pragma once
#include "common.hpp"

namespace {

template <bool BF16>
PT2Q_DEV uint32_t td_bits(float v) {  // RN to the activation dtype, as to_bits of ternary_linear.hip
  uint16_t u;
  if constexpr (BF16) {
    __bf16 h = (__bf16)v;
    __builtin_memcpy(&u, &h, 2);
  } else {
    _Float16 h = (_Float16)v;
    __builtin_memcpy(&u, &h, 2);
  }
  return u;
}

// the low / high 16-bit element of a register, widened exactly to fp32
template <bool BF16>
PT2Q_DEV float td_lo(uint32_t u) {
  if constexpr (BF16) {
    return __uint_as_float(u << 16);
  } else {
    const uint16_t s = (uint16_t)(u & 0xffffu);
    _Float16 h;
    __builtin_memcpy(&h, &s, 2);
    return (float)h;
  }
}
template <bool BF16>
PT2Q_DEV float td_hi(uint32_t u) {
  if constexpr (BF16) {
    return __uint_as_float(u & 0xffff0000u);
  } else {
    const uint16_t s = (uint16_t)(u >> 16);
    _Float16 h;
    __builtin_memcpy(&h, &s, 2);
    return (float)h;
  }
}

static_assert(PT2Q_DECODE_GROUP_MAX == 4, "td_pick and the member searches name four entries");

// a[z] by selects: the argument arrays stay in the kernarg segment, nothing is indexed in memory
template <class T>
PT2Q_DEV T td_pick(const T (&a)[4], int z) {
  T r = a[0];
  if (z == 1) r = a[1];
  if (z == 2) r = a[2];
  if (z == 3) r = a[3];
  return r;
}

template <bool BF16>
PT2Q_DEV float td_round(float v) {  // RN_TY(v), widened back
  return td_lo<BF16>(td_bits<BF16>(v));
}

// An fp32 product as a value of its own.  Without it the compiler folds RN_f16(g * q) into one
// v_fma_mixlo_f16 with a +0 addend: a single rounding of the exact product where SWIGLU16 has two,
// and +0 where the product is -0.
PT2Q_DEV float td_rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// q of contract SWIGLU16: sigmoid(g) = (g >= 0 ? 1 : e) / (1 + e), e = exp(-|g|) by a degree-6
// polynomial on the reduced argument.  fp32, every operation rounded on its own (-ffp-contract=off).
PT2Q_DEV float td_sigmoid(float g) {
  const float LOG2E = __uint_as_float(0x3FB8AA3Bu);
  const float LN2_HI = __uint_as_float(0x3F317200u), LN2_LO = __uint_as_float(0x35BFBE8Eu);
  const float C[7] = {__uint_as_float(0x3F800000u), __uint_as_float(0x3F800000u), __uint_as_float(0x3F000000u),
                      __uint_as_float(0x3E2AA9FBu), __uint_as_float(0x3D2AAA2Du), __uint_as_float(0x3C093B5Eu),
                      __uint_as_float(0x3AB6D7B4u)};
  const float a = fabsf(g);
  const float t = a * (-LOG2E);
  float e = 0.0f;
  if (!(t < -125.0f)) {
    const float n = rintf(t);
    float r = (-a) - n * LN2_HI;  // n * LN2_HI is exact: 7 bits by 15
    r = r - n * LN2_LO;
    float p = C[6];
#pragma unroll
    for (int k = 5; k >= 0; --k) {
      p = p * r;
      p = p + C[k];
    }
    e = ldexpf(p, (int)n);  // exact: n >= -125, p in [0.7, 1.42]
  }
  return (g >= 0.0f ? 1.0f : e) / (1.0f + e);
}

// h of contract SWIGLU16 from g = RN_TY(v_gate + bias_gate), u = RN_TY(v_up + bias_up), both widened
// back to fp32: RN_TY(RN_TY(g * sigmoid(g)) * u) before its last rounding, which the store's
// conversion to TY performs.
template <bool BF16>
PT2Q_DEV float td_swiglu(float g, float u) {
  const float s = td_round<BF16>(td_rounded(g * td_sigmoid(g)));
  return td_rounded(s * u);
}

// r of contract RMSNORM16 from the eight wave sums of a row's squares: the sums
// added in order, then a division, an add, a square root and a division, each the correctly
// rounded fp32 operation (hipcc's default for / and sqrtf; no fast-math, no contraction).
constexpr int TD_NORM_SUMS = 8;  // 512 chains in waves of 64
PT2Q_DEV float td_norm_r(const float* sums, int m, float eps) {
  float ss = sums[0];
#pragma unroll
  for (int k = 1; k < TD_NORM_SUMS; ++k) ss = ss + sums[k];
  const float mean = ss / (float)m;
  return 1.0f / sqrtf(mean + eps);
}
// RN_TX(RN_TX(xf * r) * wf): both products fp32 values of their own (td_rounded)
template <bool BF16>
PT2Q_DEV uint16_t td_normed(uint32_t xu, uint32_t wu, float r) {
  const float xn = td_round<BF16>(td_rounded(td_lo<BF16>(xu) * r));
  return (uint16_t)td_bits<BF16>(td_rounded(xn * td_lo<BF16>(wu)));
}
constexpr int TD_NORM_PREFETCH = 16;  // elements a thread loads ahead of the sums' barrier: all of them for m <= 8192

}  // namespace
