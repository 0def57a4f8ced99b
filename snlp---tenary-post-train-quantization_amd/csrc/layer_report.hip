// Per-layer quantization error report from the Gram (the Gram form of compute_quantization_error
// and compute_output_error, quantizer.py:296-306): for the residual D = W - W_hat of an n x m
// layer and the raw Gram G = XᵀX,
//
//   ew[i] = Σ_j d_ij²          ex[i] = d_i G d_iᵀ = ‖d_i Xᵀ‖²          ey[i] = w_i G w_iᵀ
//
// with no activations at hand.  Arithmetic: DESIGN.md §3 "Layer report" (ROWTREE).
//
//   report_blockof_kernel   blockof[c] = position of column c in perm, / b
//   report_residual_kernel  D (and / or W) feature-major (K-major A operand, zero padded rows) and
//                           the 32-column chunk partials of ew
//   quadform_rows_kernel    P = A G on the f32 MFMA, never stored: each 32 x 32 accumulator tile
//                           is multiplied by the matching A values and reduced along the row to
//                           one chunk partial per row
//   rowtree_finish_kernel   chunk partials added in ascending chunk order
//   rowtree_totals_kernel   ROWTREE of the per-row vectors
//
// The GEMM part is gemmx.hip's tile (gemmx_stage.hpp): 128 x 128 per workgroup, LDS-DMA ring, k
// ascending over all m, so every P_ij is the contract's fmaf chain.
#include "common.hpp"
#include "internal.hpp"
#include "gemmx_stage.hpp"

namespace {

template <typename T>
PT2Q_DEV float ld_f32(const T* p);
template <>
PT2Q_DEV float ld_f32<float>(const float* p) { return *p; }
template <>
PT2Q_DEV float ld_f32<_Float16>(const _Float16* p) { return (float)*p; }
template <>
PT2Q_DEV float ld_f32<uint16_t>(const uint16_t* p) { return __uint_as_float(((uint32_t)*p) << 16); }
template <>
PT2Q_DEV float ld_f32<int8_t>(const int8_t* p) { return (float)*p; }

// The halving tree 32 -> 16 -> ... -> 1 of a chunk (v[:h] + v[h:2h]).
PT2Q_DEV float tree32(float (&v)[32]) {
#pragma unroll
  for (int h = 16; h >= 1; h >>= 1)
#pragma unroll
    for (int j = 0; j < h; ++j) v[j] = v[j] + v[j + h];
  return v[0];
}

// blockof[c] = p / bb for the position p with perm[p] = c (perm NULL: p = c).  blockof is zeroed
// before the launch, so an entry no position names stays defined; an index outside [0, m) is not
// a column and is dropped.
__global__ void report_blockof_kernel(const int64_t* perm, int m, int bb, int* blockof) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const int64_t c = perm ? perm[p] : (int64_t)p;
  if (c >= 0 && c < m) blockof[c] = p / bb;
}

struct ResArgs {
  const void* W;  // n x m row-major
  long ldw;
  int n, m;
  const void* T;  // codes, original column order
  long ldt;
  const float* alpha;  // n x B
  const float* mu;
  int B;
  const int* blockof;
  float* Dt;    // m x ldd feature-major: rows [0, n) of a column slab, zero up to the slab's end
  long ldd;
  long woff;    // RES_BOTH: W goes to row offset woff of the same matrix
  float* partw;  // ew chunk partials, partw[chunk * ldp + row]
  long ldp;
};

enum { RES_D = 0, RES_BOTH = 1, RES_W = 2 };

// One 64 x 64 tile of W -> the residual D_ic = RN(W_ic - RN(RN(alpha_ik t_ic) + mu_ik)) (MODE
// RES_D / RES_BOTH) or W itself (RES_W), transposed through LDS into the feature-major operand
// (16-byte stores, four rows of one column), as misc.hip's transpose16_kernel does.  The loads are
// scalar and coalesced along the row (any element-aligned base and leading dimension).  Threads
// 0..127 then reduce the two 32-column chunks of each tile row of D² with the halving tree.
// grid.y covers the padded rows: rows >= n are written as zero.
template <typename TW, typename TT, int MODE>
__global__ __launch_bounds__(256) void report_residual_kernel(ResArgs a) {
  __shared__ float tD[64][65];
  __shared__ float tW[MODE == RES_BOTH ? 64 : 1][65];
  const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64, tid = threadIdx.x;
  {
    const int c = tid & 63, col = c0 + c;
    const int k = (MODE != RES_W && col < a.m) ? a.blockof[col] : 0;
#pragma unroll 4
    for (int p = 0; p < 16; ++p) {
      const int r = (tid >> 6) + 4 * p, row = r0 + r;
      const bool in = row < a.n && col < a.m;
      const float w = in ? ld_f32<TW>((const TW*)a.W + (long)row * a.ldw + col) : 0.0f;
      if constexpr (MODE == RES_W) {
        tD[r][c] = w;
      } else {
        const float t = in ? ld_f32<TT>((const TT*)a.T + (long)row * a.ldt + col) : 0.0f;
        const float al = in ? a.alpha[(long)row * a.B + k] : 0.0f;
        const float mu = in ? a.mu[(long)row * a.B + k] : 0.0f;
        const float wh = al * t + mu;  // two roundings (pt2q_dequantize)
        tD[r][c] = w - wh;
        if constexpr (MODE == RES_BOTH) tW[r][c] = w;
      }
    }
  }
  __syncthreads();
  if constexpr (MODE != RES_W) {
    if (tid < 128) {
      const int r = tid & 63, h = tid >> 6, chunk = c0 / 32 + h;
      if (chunk * 32 < a.m) {
        float v[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) {
          const float d = tD[r][h * 32 + j];
          v[j] = d * d;
        }
        a.partw[(long)chunk * a.ldp + r0 + r] = tree32(v);
      }
    }
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int idx = p * 256 + tid, c = idx / 16, r = (idx % 16) * 4;
    if (c0 + c < a.m) {
      float* dst = a.Dt + (long)(c0 + c) * a.ldd + r0 + r;
      *(f32x4*)dst = f32x4{tD[r][c], tD[r + 1][c], tD[r + 2][c], tD[r + 3][c]};
      if constexpr (MODE == RES_BOTH)
        *(f32x4*)(dst + a.woff) = f32x4{tW[r][c], tW[r + 1][c], tW[r + 2][c], tW[r + 3][c]};
    }
  }
}

// ---- the fused quadratic form

struct QfArgs {
  const float* At;  // K-major A: m x lda, R rows used (R % 128 == 0, lda % 4 == 0, 16-byte aligned,
  long lda;         // rows past the data zero)
  int R, m;
  const float* G;   // m x m, ld ldg, read as stored
  long ldg;
  float* part;      // part[chunk * ldp + row], chunk < ceil(m / 32), row < R
  long ldp;
  int tiles_n;
  int g16;          // G 16-byte aligned, ldg % 4 == 0 and m % 4 == 0: 16-byte DMA chunks
};

// x_panel_dma for an operand of any element alignment, leading dimension and width: 4-byte DMA
// elements.  A wave instruction fills 256 B = half a k-row (16 chunk positions); lane l is element
// l % 4 of chunk position half * 16 + l / 4, which holds global chunk position ^ ((row & 1) << 3)
// (the same swizzled image as the 16-byte path).  Out-of-range elements come from the zero source.
PT2Q_DEV void q_panel_dma4(const float* base, long ld, int d0, int DMAX, int k0, int kend, uint8_t* pan) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  typedef __attribute__((address_space(3))) void* lptr;
  constexpr int NI = XPANEL / 256 / 4;  // instructions per wave per panel
#pragma unroll
  for (int q = 0; q < NI; ++q) {
    const int I = wave * NI + q;
    const int kr = I >> 1, p = (I & 1) * 16 + (lane >> 2), e = lane & 3;
    const int c = p ^ ((kr & 1) << 3);
    const int k = k0 + kr, d = d0 + 4 * c + e;
    const bool ok = k < kend && d < DMAX;
    const void* src = ok ? (const void*)(base + (long)k * ld + d) : (const void*)gxz_zero16;
    __builtin_amdgcn_global_load_lds(src, (lptr)(pan + I * 256), 4, 0, 0);
  }
}

// One 128 x 128 tile of P = A G (rows i0.., columns j0..), K over all m, then the epilogue: lane
// <-> row, the 16 accumulator registers of a 32 x 32 tile are columns 8q + 4lk + e (q, e < 4, lk
// the half-wave).  R = RN(P * A) per element, then the halving tree of the 32-column chunk as a
// butterfly over the column bits in the tree's order: 16 and 8 (registers q), 4 (the other
// half-wave), 2 and 1 (registers e).  Additions commute, so both half-waves hold the chunk's
// partial; lk = 0 stores it.
__global__ __launch_bounds__(256) void quadform_rows_kernel(QfArgs X) {
  __shared__ __attribute__((aligned(1024))) uint8_t smem[XNS * XSTG];
  const int bid = blockIdx.x;
  const int ti = bid / X.tiles_n, tj = bid % X.tiles_n;
  const int i0 = ti * XT, j0 = tj * XT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1, li = lane & 31, lk = lane >> 5;
  const int kend = X.m;
  const int nst = (kend + XK - 1) / XK;
  uint32_t voA[XDMA], voB[XDMA];
  x_panel_voff(X.lda, voA);
  x_panel_voff(X.ldg, voB);
  const uint32_t ldsb = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem;
  // whole stages with a whole, 16-byte addressable G panel take the fast DMA (A's columns are
  // always whole: R % 128 == 0)
  const int nfull = (X.g16 && j0 + XT <= X.m) ? kend / XK : 0;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  auto stage = [&](int p) {
    uint8_t* sp = smem + (p % XNS) * XSTG;
    if (p < nfull) {
      x_panel_dma_fast(X.At, X.lda, i0, p * XK, voA, ldsb + (uint32_t)((p % XNS) * XSTG));
      x_panel_dma_fast(X.G, X.ldg, j0, p * XK, voB, ldsb + (uint32_t)((p % XNS) * XSTG + XPANEL));
    } else {
      x_panel_dma(X.At, X.lda, i0, X.R, p * XK, kend, sp);
      if (X.g16)
        x_panel_dma(X.G, X.ldg, j0, X.m, p * XK, kend, sp + XPANEL);
      else
        q_panel_dma4(X.G, X.ldg, j0, X.m, p * XK, kend, sp + XPANEL);
    }
  };
  stage(0);
  f32x16 acc[2][2];
#pragma unroll
  for (int rm = 0; rm < 2; ++rm)
#pragma unroll
    for (int rn = 0; rn < 2; ++rn)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[rm][rn][e] = 0.0f;
  auto opaddr = [&](int panel, int d) -> uint32_t {  // element (k = lk, column d) of a panel
    const int cch = (d >> 2) ^ (lk << 3);
    return (uint32_t)(panel + lk * XROW + cch * 16 + (d & 3) * 4);
  };
  const uint32_t oA0 = opaddr(0, wr * 64 + li), oA1 = opaddr(0, wr * 64 + 32 + li);
  const uint32_t oB0 = opaddr(XPANEL, wc * 64 + li), oB1 = opaddr(XPANEL, wc * 64 + 32 + li);
  XOps o;
  for (int t = 0; t < nst; ++t) {
    // stage t landed, then a raw barrier (it also retires every wave's reads of the slot the
    // next DMA reuses)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
    const int tn = t + 1;
    const bool fastn = tn < nfull;
    if (tn < nst && !fastn) stage(tn);
    XStageIO sio{(const char*)(X.At + (long)(tn * XK) * X.lda + i0),
                 (const char*)(X.G + (long)(tn * XK) * X.ldg + j0), voA, voB,
                 ldsb + (uint32_t)((tn % XNS) * XSTG + wv * XDMA * 1024),
                 ldsb + (uint32_t)((tn % XNS) * XSTG + XPANEL + wv * XDMA * 1024), tn < nst && fastn};
    const uint32_t sb = ldsb + (uint32_t)((t % XNS) * XSTG);
    x_chain<0, XK / 2>(acc, o, sb + oA0, sb + oA1, sb + oB0, sb + oB1, sio);
  }
#pragma unroll
  for (int rm = 0; rm < 2; ++rm)
#pragma unroll
    for (int rn = 0; rn < 2; ++rn) {
      const int row = i0 + wr * 64 + rm * 32 + li;
      const int cb = j0 + wc * 64 + rn * 32;
      if (cb >= X.m) continue;  // no such chunk (wave-uniform)
      float s2[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int col = cb + 8 * q + 4 * lk + e;
          const float a = col < X.m ? X.At[(long)col * X.lda + row] : 0.0f;  // +0 past m
          r[q] = acc[rm][rn][4 * q + e] * a;
        }
        s2[e] = (r[0] + r[2]) + (r[1] + r[3]);  // column bits 16, then 8
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) s2[e] = s2[e] + __shfl_xor(s2[e], 32);  // bit 4
      const float s = (s2[0] + s2[2]) + (s2[1] + s2[3]);                    // bits 2, then 1
      if (lk == 0) X.part[(long)(cb / 32) * X.ldp + row] = s;
    }
}

// out[i] = the chunk partials of row row0 + i added in ascending chunk order from +0.  One wave
// per workgroup (the rows spread over the CUs); the adds are sequential by contract, eight
// chunks of coalesced loads are in flight ahead of them.
__global__ __launch_bounds__(64) void rowtree_finish_kernel(const float* part, long ldp, int nchunks, long row0,
                                                            int n, float* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const float* p = part + row0 + i;
  float s = 0.0f;
  int c = 0;
  for (; c + 8 <= nchunks; c += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(long)(c + u) * ldp];
#pragma unroll
    for (int u = 0; u < 8; ++u) s = s + v[u];
  }
  for (; c < nchunks; ++c) s = s + p[(long)c * ldp];
  out[i] = s;
}

// totals[v] = ROWTREE of the length-n vector vec[v] (chunks of 32, +0 past n; NULL: +0), one
// workgroup per vector: chunk partials into scratch (ceil(n / 32) floats each), then one thread
// adds them in ascending order.
struct TotArgs {
  const float* vec[3];
  int n;
  float* scratch;
  float* totals;
};
__global__ __launch_bounds__(256) void rowtree_totals_kernel(TotArgs a) {
  const float* v = a.vec[blockIdx.x];
  const int nch = (a.n + 31) / 32;
  float* sc = a.scratch + (long)blockIdx.x * nch;
  if (!v) {
    if (threadIdx.x == 0) a.totals[blockIdx.x] = 0.0f;
    return;
  }
  for (int c = threadIdx.x; c < nch; c += blockDim.x) {
    float x[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) x[j] = (c * 32 + j < a.n) ? v[c * 32 + j] : 0.0f;
    sc[c] = tree32(x);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.0f;
    for (int c = 0; c < nch; ++c) s = s + sc[c];
    a.totals[blockIdx.x] = s;
  }
}

template <typename TW, int MODE>
int launch_residual_t(const ResArgs& a, int tdtype, dim3 grid, hipStream_t st) {
  if constexpr (MODE == RES_W) {  // no codes: one instantiation per W type
    hipLaunchKernelGGL((report_residual_kernel<TW, int8_t, MODE>), grid, dim3(256), 0, st, a);
  } else {
    if (tdtype == PT2Q_I8)
      hipLaunchKernelGGL((report_residual_kernel<TW, int8_t, MODE>), grid, dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL((report_residual_kernel<TW, float, MODE>), grid, dim3(256), 0, st, a);
  }
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}

template <int MODE>
int launch_residual_m(const ResArgs& a, int wdtype, int tdtype, dim3 grid, hipStream_t st) {
  switch (wdtype) {
    case PT2Q_F32: return launch_residual_t<float, MODE>(a, tdtype, grid, st);
    case PT2Q_F16: return launch_residual_t<_Float16, MODE>(a, tdtype, grid, st);
    case PT2Q_BF16: return launch_residual_t<uint16_t, MODE>(a, tdtype, grid, st);
  }
  return PT2Q_E_ARG;
}

}  // namespace

int pt2q_launch_report_blockof(const int64_t* perm, int m, int bb, int* blockof, hipStream_t st) {
  if (m <= 0 || bb <= 0 || !blockof) return PT2Q_E_ARG;
  if (hipMemsetAsync(blockof, 0, sizeof(int) * (size_t)m, st) != hipSuccess) return PT2Q_E_HIP;
  hipLaunchKernelGGL(report_blockof_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, perm, m, bb, blockof);
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}

int pt2q_launch_report_residual(int mode, const void* W, int wdtype, long ldw, int n, int m, const void* T,
                                int tdtype, long ldt, const float* alpha, const float* mu, int B,
                                const int* blockof, float* Dt, long ldd, long rows, long woff, float* partw,
                                long ldp, hipStream_t st) {
  if (!W || !Dt || n <= 0 || m <= 0 || rows < n || rows % 64 || ldd % 4 || (uintptr_t)Dt % 16) return PT2Q_E_ARG;
  if (mode != RES_W && (!T || !alpha || !mu || !blockof || !partw || (tdtype != PT2Q_I8 && tdtype != PT2Q_F32)))
    return PT2Q_E_ARG;
  if (rows / 64 > 65535) return PT2Q_E_UNSUPPORTED;
  ResArgs a{W, ldw, n, m, T, ldt, alpha, mu, B, blockof, Dt, ldd, woff, partw, ldp};
  const dim3 grid((unsigned)ceil_div(m, 64), (unsigned)(rows / 64));
  switch (mode) {
    case RES_D: return launch_residual_m<RES_D>(a, wdtype, tdtype, grid, st);
    case RES_BOTH: return launch_residual_m<RES_BOTH>(a, wdtype, tdtype, grid, st);
    case RES_W: return launch_residual_m<RES_W>(a, wdtype, tdtype, grid, st);
  }
  return PT2Q_E_ARG;
}

int pt2q_launch_quadform_rows(const float* At, long lda, long R, int m, const float* G, long ldg, float* part,
                              long ldp, hipStream_t st) {
  if (!At || !G || !part || R <= 0 || m <= 0 || R % XT || lda < R || lda % 4 || (uintptr_t)At % 16 || ldg < m ||
      ldp < R)
    return PT2Q_E_ARG;
  // the DMA's 32-bit lane offsets span 32 rows of an operand; one grid dimension of tiles
  const long tiles = (R / XT) * (long)ceil_div(m, XT);
  if (lda >= (1l << 24) || ldg >= (1l << 24) || tiles > 0x7fffffffl) return PT2Q_E_UNSUPPORTED;
  QfArgs X{At, lda, (int)R, m, G, ldg, part, ldp, ceil_div(m, XT),
           ((uintptr_t)G % 16 == 0 && ldg % 4 == 0 && m % 4 == 0) ? 1 : 0};
  hipLaunchKernelGGL(quadform_rows_kernel, dim3((unsigned)tiles), dim3(256), 0, st, X);
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}

int pt2q_launch_rowtree_finish(const float* part, long ldp, int m, long row0, int n, float* out, hipStream_t st) {
  if (!part || !out || n <= 0 || m <= 0) return PT2Q_E_ARG;
  hipLaunchKernelGGL(rowtree_finish_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, st, part, ldp, ceil_div(m, 32),
                     row0, n, out);
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}

int pt2q_launch_rowtree_totals(const float* v0, const float* v1, const float* v2, int count, int n, float* scratch,
                               float* totals, hipStream_t st) {
  if (count < 1 || count > 3 || n <= 0 || !scratch || !totals) return PT2Q_E_ARG;
  TotArgs a{{v0, v1, v2}, n, scratch, totals};
  hipLaunchKernelGGL(rowtree_totals_kernel, dim3((unsigned)count), dim3(256), 0, st, a);
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}
