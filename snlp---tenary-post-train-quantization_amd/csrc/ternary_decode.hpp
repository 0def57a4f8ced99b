// What the fused decode kernels share (csrc/ternary_decode.hip: one linear per launch,
// csrc/ternary_decode_group.hip: up to four linears on one x, or gate/up with the SwiGLU
// epilogue): the constants of the LDS image, the 16-bit operand helpers and td_piece, the chain
// of contract DOT64P over one 16-byte piece of a packed row.
#pragma once
#include "common.hpp"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int TD_MAX_TOKENS = 8;
constexpr int TD_WAVES = 8;                  // rows in flight per workgroup
constexpr int TD_DEPTH = 4;                  // (row, round) items a wave keeps in flight
constexpr int TD_THREADS = TD_WAVES * 64;
constexpr int TD_ROUND_BYTES = 64 * 128;     // LDS per (round of 64 pieces, token)
constexpr int TD_LDS_PLAIN = 64 * 1024;      // dynamic LDS a launch gets without asking
constexpr int TD_LDS_MAX = 128 * 1024;       // what one token of the widest supported layer needs
constexpr int TD_MAX_ROUNDS = 8;             // P <= 32768 positions: 64 KiB gathered + 64 KiB staged

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

// acc = fmaf((float)lo(w), (float)lo(x), acc) and the same for the high halves.  fp16 takes the
// mixed-precision FMA, which widens both 16-bit operands inside the instruction (subnormals
// included: the kernel runs with denormals on) -- the same bits as converting first, no conversion
// instructions; bf16 widens by a shift or a mask.
template <bool BF16>
PT2Q_DEV float td_fma_lo(uint32_t w, uint32_t x, float acc) {
  if constexpr (BF16) {
    return fmaf(td_lo<true>(w), td_lo<true>(x), acc);
  } else {
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel_hi:[1,1,0]" : "+v"(acc) : "v"(w), "v"(x));
    return acc;
  }
}
template <bool BF16>
PT2Q_DEV float td_fma_hi(uint32_t w, uint32_t x, float acc) {
  if constexpr (BF16) {
    return fmaf(td_hi<true>(w), td_hi<true>(x), acc);
  } else {
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "+v"(acc) : "v"(w), "v"(x));
    return acc;
  }
}

struct TdItem {  // what a lane needs of one (row, round): its piece's codes, scales and the row's bias
  u32x4 cw;
  float a, mm, bv;
};

// acc[t] of piece q of one row, continued over the piece's 64 positions (g then j ascending) for
// the TG tokens of the workgroup.  xk: the lane's first chunk of the piece's round in the gathered
// image [token][group g][lane]; it: the piece's codes and, with one scale block per piece
// (perpiece), its scales; arow / mrow: the row's alpha and mu, read per 16-position group otherwise.
template <bool BF16, int TG>
PT2Q_DEV void td_piece(const u32x4* xk, const TdItem& it, bool perpiece, int q, int bse, int B, const float* arow,
                       const float* mrow, float (&acc)[TG]) {
  // groups per unrolled step: eight LDS reads in flight whatever TG is (more would cost the
  // registers that let two workgroups share a CU)
  constexpr int GU = 8 / TG;
  uint32_t tab0 = 0, tab1 = 0;
  if (perpiece) {
    tab0 = td_bits<BF16>(it.mm - it.a) | (td_bits<BF16>(it.mm) << 16);
    tab1 = td_bits<BF16>(it.mm + it.a);
  }
  u32x4 cr = it.cw;  // cr[0], cr[1], ...: the codes of groups go, go + 1, ...
#pragma unroll 1
  for (int go = 0; go < 8; go += GU) {
#pragma unroll
    for (int gi = 0; gi < GU; ++gi) {
      const int g = go + gi;
      if (!perpiece) {  // bse % 16 == 0: the group's 16 positions share a block (clamped to B - 1)
        const int blk = min((128 * (q >> 1) + 16 * g) / bse, B - 1);
        const float ag = arow[blk], mg = mrow[blk];
        tab0 = td_bits<BF16>(mg - ag) | (td_bits<BF16>(mg) << 16);
        tab1 = td_bits<BF16>(mg + ag);
      }
      const uint32_t cb = (cr[gi >> 1] >> (16 * (gi & 1))) & 0xffffu;  // 8 codes, 2 bits each
      uint32_t w2[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const uint32_t sel = ((cb >> (4 * jj)) & 3u) | (((cb >> (4 * jj + 2)) & 3u) << 16);
        w2[jj] = __builtin_amdgcn_perm(tab1, tab0, sel * 0x202u + 0x01000100u);
      }
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        const u32x4 xv = xk[(t * 8 + g) * 64];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          acc[t] = td_fma_lo<BF16>(w2[jj], xv[jj], acc[t]);
          acc[t] = td_fma_hi<BF16>(w2[jj], xv[jj], acc[t]);
        }
      }
    }
    if constexpr (GU == 2) cr = u32x4{cr[1], cr[2], cr[3], cr[0]};
    if constexpr (GU == 4) cr = u32x4{cr[2], cr[3], cr[0], cr[1]};
  }
}

inline int td_cus() {
  static const int cus = [] {
    int dev = 0, c = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev);
    return c > 0 ? c : 256;
  }();
  return cus;
}

}  // namespace
