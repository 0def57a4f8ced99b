// The operand staging and the MFMA chain of the f32 chain-GEMM tile (gemmx.hip), shared with the
// fused quadratic-form kernel (layer_report.hip): a 128 x 128 tile per workgroup (4 waves 2 x 2,
// each 64 x 64 = 2 x 2 MFMA tiles of 32 x 32), K-major operand panels staged global -> LDS by
// LDS-DMA into a ring of XNS stages of XK k-rows, XOR-swizzled 16-byte chunks, hand-counted LDS
// read waits.  See gemmx.hip's header comment for the layout and the arithmetic.  Everything is
// internal to the including translation unit (anonymous namespace, its own zero-chunk source).
#pragma once
#include "common.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int XT = 128;              // tile side
constexpr int XROW = XT * 4;         // 512 B per k row of a panel

// ring geometry: XNS stages of XK k rows (64 KiB of LDS: two workgroups per CU; three stages of
// 32 rows or four / five of 16 measured slower)
constexpr int XNS = 2, XK = 32;
constexpr int XPANEL = XK * XROW;        // one operand's rows of a stage
constexpr int XSTG = 2 * XPANEL;         // A + B panels
constexpr int XDMA = XPANEL / 1024 / 4;  // DMA wave-instructions per wave per panel

__device__ uint4 gxz_zero16[4];      // the source of out-of-range chunks (zero-initialised)

// One panel of one stage: rows [k0, k0 + XK) (valid below kend) x columns [d0, d0 + 128) (valid
// below DMAX) of a K-major operand, into panel memory `pan` (swizzled).  Lane l of the wave's
// q-th instruction fills LDS chunk L = (wave * DMA + q) * 64 + l: row L / 32, position L % 32,
// which holds global chunk (L % 32) ^ ((row & 1) << 3).
PT2Q_DEV void x_panel_dma(const float* base, long ld, int d0, int DMAX, int k0, int kend, uint8_t* pan) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  typedef __attribute__((address_space(3))) void* lptr;
#pragma unroll
  for (int q = 0; q < XDMA; ++q) {
    const int L = (wave * XDMA + q) * 64 + lane;
    const int kr = L >> 5, p = L & 31;
    const int c = p ^ ((kr & 1) << 3);
    const int k = k0 + kr, d = d0 + 4 * c;
    const bool ok = k < kend && d < DMAX;
    const void* src = ok ? (const void*)(base + (long)k * ld + d) : (const void*)gxz_zero16;
    __builtin_amdgcn_global_load_lds(src, (lptr)(pan + (wave * XDMA + q) * 1024), 16, 0, 0);
  }
}

// Fast staging of a whole in-range panel (rows [k0, k0 + XK) below kend, columns [d0, d0 + 128)
// below DMAX): this lane's byte offsets from the panel's first element, fixed for the launch, and a
// scalar base -- s_mov m0 + one global_load_lds per chunk instead of per-lane address math.
PT2Q_DEV void x_panel_voff(long ld, uint32_t (&vo)[XDMA]) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
  for (int q = 0; q < XDMA; ++q) {
    const int L = (wave * XDMA + q) * 64 + lane;
    const int kr = L >> 5, c = (L & 31) ^ ((kr & 1) << 3);
    vo[q] = (uint32_t)(((long)kr * ld + 4 * c) * 4);
  }
}

PT2Q_DEV void x_panel_dma_fast(const float* base, long ld, int d0, int k0, const uint32_t (&vo)[XDMA],
                               uint32_t pan) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const char* sb = (const char*)(base + (long)k0 * ld + d0);
#pragma unroll
  for (int q = 0; q < XDMA; ++q)
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(vo[q]), "s"(sb),
                 "s"(pan + (uint32_t)((wave * XDMA + q) * 1024))
                 : "memory");
}

template <int OFF>
PT2Q_DEV float x_ld(uint32_t addr) {
  float r;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "i"(OFF));
  return r;
}

struct XOps {
  float v[4][4];  // ring of 4 k-pair sets: a0, a1, b0, b1
};

// k-pair S (rows 2S, 2S+1 of the stage): its 4 operands were read into set S % 4; the reads of
// pair S+2 go into set (S+2) % 4 before pair S's MFMAs, so their latency hides under them.
template <int S>
PT2Q_DEV void x_read(XOps& o, uint32_t aA0, uint32_t aA1, uint32_t aB0, uint32_t aB1) {
  constexpr int c = S % 4, off = S * 2 * XROW;
  o.v[c][0] = x_ld<off>(aA0);
  o.v[c][1] = x_ld<off>(aA1);
  o.v[c][2] = x_ld<off>(aB0);
  o.v[c][3] = x_ld<off>(aB1);
}

// the next stage's fast DMAs, one A and one B chunk after the first MFMA of k-pair q (q < DMA), so
// their issue sits in MFMA shadows instead of in front of the stage (on = false: nothing)
struct XStageIO {
  const char* sbA;
  const char* sbB;
  const uint32_t (&voA)[XDMA];
  const uint32_t (&voB)[XDMA];
  uint32_t mA, mB;
  bool on;
  template <int S>
  PT2Q_DEV void at() {
    if constexpr (S < XDMA) {
      if (on) {
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voA[S]), "s"(sbA),
                     "s"(mA + S * 1024)
                     : "memory");
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voB[S]), "s"(sbB),
                     "s"(mB + S * 1024)
                     : "memory");
      }
    }
  }
};

template <int S, int NP, class IO>
PT2Q_DEV void x_chain(f32x16 (&acc)[2][2], XOps& o, uint32_t aA0, uint32_t aA1, uint32_t aB0, uint32_t aB1, IO& io) {
  if constexpr (S == 0) {
    x_read<0>(o, aA0, aA1, aB0, aB1);
    x_read<1>(o, aA0, aA1, aB0, aB1);
    asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(o.v[0][0]), "+v"(o.v[0][1]), "+v"(o.v[0][2]), "+v"(o.v[0][3]));
  }
  if constexpr (S < NP) {
    constexpr int c = S % 4;
    if constexpr (S + 2 < NP) x_read<S + 2>(o, aA0, aA1, aB0, aB1);
    if constexpr (S > 0) {  // pair S-1's registers stay allocated until these reads are issued
      constexpr int p = (S + 3) % 4;
      asm volatile("" ::"v"(o.v[p][0]), "v"(o.v[p][1]), "v"(o.v[p][2]), "v"(o.v[p][3]));
    }
    __builtin_amdgcn_sched_barrier(0);
    // transposed tile: lane <-> C row (16-byte epilogue)
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.v[c][2], o.v[c][0], acc[0][0], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    io.template at<S>();
    __builtin_amdgcn_sched_barrier(0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.v[c][3], o.v[c][0], acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.v[c][2], o.v[c][1], acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.v[c][3], o.v[c][1], acc[1][1], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (S + 1 < NP) {  // pair S+1 landed (pair S+2 may stay in flight)
      constexpr int c1 = (S + 1) % 4;
      if constexpr (S + 2 < NP)
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(o.v[c1][0]), "+v"(o.v[c1][1]), "+v"(o.v[c1][2]), "+v"(o.v[c1][3]));
      else
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(o.v[c1][0]), "+v"(o.v[c1][1]), "+v"(o.v[c1][2]), "+v"(o.v[c1][3]));
    }
    x_chain<S + 1, NP>(acc, o, aA0, aA1, aB0, aB1, io);
  }
}

}  // namespace
