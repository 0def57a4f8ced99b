// Fused decode kernel of the ternary linear layer: 1..8 tokens in ONE launch, no workspace
// (model.py:75-95; the buffers are those of pt2q_ternary_pack, csrc/ternary_linear.hip).
//
// Arithmetic contract DOT64P.  A piece q = 2 kb + h is the 64 positions of one
// 16-byte load of a packed row (p = 128 kb + 16 g + 8 h + j, g then j ascending).  Lane l of the
// row's wave owns the pieces q ≡ l (mod 64) in ascending q and forms
//   acc = fmaf((float)w, (float)xs, acc)   from +0, pieces then positions in that order
// (the 16-bit x 16-bit product is exact in fp32), the 64 partials are folded by bfly64 and
// y = RN_TY(v + bias).  Nothing else -- tokens per call, token grouping, grid, rows per wave --
// enters the order, so a token's bits do not depend on its neighbours.
//
// Structure: VALU, one wave per output row, 8 waves per workgroup, two workgroups per CU
// striding over rows.  The workgroup stages its tokens' rows of x in LDS and gathers them through
// `gather` once, LDS to LDS, into 16-byte chunks [round k][token][group g][lane], so that at every
// row a lane reads the 8 chunks of its piece with conflict-free ds_read_b128 (consecutive lanes,
// consecutive chunks).
// The codes of a wave's next four (row, piece) items are loaded straight into registers, the
// first four before the gather's barrier (at the decode shapes that is all a wave has, so HBM
// latency is paid once); the v_perm_b32 table of tl_gemm_kernel turns a code pair into two
// 16-bit weights.  A workgroup serves TG <= 4 tokens (blockIdx.y: token group), TG chosen so
// that the gathered activations and the staged rows of x fit 64 KiB of LDS.
#include "common.hpp"
#include "internal.hpp"
#include "ternary_decode.hpp"

namespace {

template <bool BF16, int TG>
__global__ __launch_bounds__(TD_THREADS, 4) void tl_decode_kernel(
    const uint16_t* x, long ldx, int tokens, int n, int m, int P, const uint8_t* codes, const int* gather,
    const float* alpha, const float* mu, int B, int bse, const float* bias, void* y, long ldy, int yf32) {
  extern __shared__ __attribute__((aligned(16))) uint8_t td_smem[];
  u32x4* xs = (u32x4*)td_smem;  // chunk ((k * TG + t) * 8 + g) * 64 + lane
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int npieces = P / 64, nround = (npieces + 63) / 64;
  const int t0 = blockIdx.y * TG;
  const int rstride = gridDim.x * TD_WAVES;
  const bool perpiece = bse % 128 == 0;  // one scale block per piece, else one per 16-position group
  const long rowbytes = P / 4;
  // codes (and, per piece, the scales; at a row's first piece its bias) of piece 64 k + lane of
  // `row`; nothing past a row's end
  auto fetch = [&](int row, int k, TdItem& it) {
    const int q = 64 * k + lane;
    it.cw = u32x4{0u, 0u, 0u, 0u};
    it.a = it.mm = it.bv = 0.0f;
    if (row < n && q < npieces) {
      it.cw = *(const u32x4*)(codes + (long)row * rowbytes + 16 * q);
      if (perpiece) {
        const int blk = min((q >> 1) * 128 / bse, B - 1);
        it.a = alpha[(long)row * B + blk];
        it.mm = mu[(long)row * B + blk];
      }
      if (k == 0 && bias) it.bv = bias[row];
    }
  };
  auto step = [&](int& r, int& kk) {  // the (row, round) after (r, kk) in this wave's sequence
    if (++kk == nround) {
      kk = 0;
      r += rstride;
    }
  };

  // the wave's first TD_DEPTH (row, round) items are in flight across the gather below; from
  // then on each item's slot is refilled as soon as it has been used
  int row = blockIdx.x * TD_WAVES + wv, k = 0;
  int frow = row, fk = 0;
  TdItem ring[TD_DEPTH];
#pragma unroll
  for (int s = 0; s < TD_DEPTH; ++s) {
    fetch(frow, fk, ring[s]);
    step(frow, fk);
  }

  // xs[t][p] = x[t0 + t][gather[p]] (+0 for padding positions and tokens past the end).  A token's
  // row is staged in LDS by coalesced loads and gathered from there: 64 lanes reading 64
  // scattered 2-byte elements from global memory cost the L1 a cache line each, per workgroup.
  // All TG rows are staged before one barrier, and a thread's first eight gather indices are
  // loaded ahead of it, so the prologue pays each global latency once, not once per token.
  uint16_t* raw = (uint16_t*)(td_smem + (size_t)nround * TG * TD_ROUND_BYTES);
  const int rawstride = (m + 7) / 8 * 8;  // elements between staged rows
  const bool galigned = ((uintptr_t)gather & 15) == 0;
  auto load_gi = [&](int o, int (&gi)[8]) {  // gather[8 o .. 8 o + 7], nothing past P
    if (o >= P / 8) return;
    if (galigned) {
      const int4 g0 = *(const int4*)(gather + 8 * o), g1 = *(const int4*)(gather + 8 * o + 4);
      gi[0] = g0.x, gi[1] = g0.y, gi[2] = g0.z, gi[3] = g0.w;
      gi[4] = g1.x, gi[5] = g1.y, gi[6] = g1.z, gi[7] = g1.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) gi[j] = gather[8 * o + j];
    }
  };
  int gn[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  load_gi(threadIdx.x, gn);
#pragma unroll
  for (int t = 0; t < TG; ++t) {
    if (t0 + t < tokens) {
      const uint16_t* xr = x + (long)(t0 + t) * ldx;
      for (int i = threadIdx.x; i < m; i += TD_THREADS) raw[t * rawstride + i] = xr[i];
    }
  }
  __syncthreads();
  for (int o = threadIdx.x; o < P / 8; o += TD_THREADS) {  // positions 8 o .. 8 o + 7
    const int q = 2 * (o >> 4) + (o & 1), g = (o >> 1) & 7;
    int gi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) gi[j] = gn[j];
    load_gi(o + TD_THREADS, gn);
#pragma unroll
    for (int t = 0; t < TG; ++t) {
      const bool tok = t0 + t < tokens;
      uint32_t e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = (tok && gi[j] >= 0) ? (uint32_t)raw[t * rawstride + gi[j]] : 0u;
      u32x4 v;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) v[jj] = e[2 * jj] | (e[2 * jj + 1] << 16);
      xs[(((q >> 6) * TG + t) * 8 + g) * 64 + (q & 63)] = v;
    }
  }
  __syncthreads();

  float acc[TG];
#pragma unroll
  for (int t = 0; t < TG; ++t) acc[t] = 0.0f;
  float bv = 0.0f;
  // one (row, round) item out of its ring slot, the slot refilled at once; false past the last row
  auto item = [&](TdItem& slot) __attribute__((always_inline)) -> bool {
    if (row >= n) return false;
    const TdItem it = slot;
    fetch(frow, fk, slot);
    step(frow, fk);
    if (k == 0) bv = it.bv;
    const int q = 64 * k + lane;
    if (q < npieces) {
      td_piece<BF16, TG>(xs + (long)k * TG * 512 + lane, it, perpiece, q, bse, B, alpha + (long)row * B,
                         mu + (long)row * B, acc);
    }
    const int r0 = row;
    step(row, k);
    if (k == 0) {  // that was the row's last round: fold, add the bias, store
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        float v = bfly64(acc[t]);
        if (bias) v = v + bv;
        if (lane == 0 && t0 + t < tokens) {
          const long o = (long)(t0 + t) * ldy + r0;
          if (yf32)
            ((float*)y)[o] = v;
          else if constexpr (BF16)
            ((__bf16*)y)[o] = (__bf16)v;
          else
            ((_Float16*)y)[o] = (_Float16)v;
        }
        acc[t] = 0.0f;
      }
    }
    return true;
  };
  static_assert(TD_DEPTH == 4, "the ring is walked by four explicit calls");
  while (item(ring[0]) && item(ring[1]) && item(ring[2]) && item(ring[3])) {
  }
}

}  // namespace

extern "C" int pt2q_ternary_decode_max_tokens(void) { return TD_MAX_TOKENS; }

extern "C" int pt2q_ternary_decode(const void* x, int xdtype, int tokens, int64_t ldx, int n, int m,
                                   const uint8_t* codes, const int* gather, const float* alpha,
                                   const float* mu, int B, int bs, const float* bias, void* y,
                                   int ydtype, int64_t ldy, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!x || !codes || !gather || !alpha || !mu || !y || tokens <= 0 || n <= 0 || m <= 0 ||
      ldx < m || ldy < n || B <= 0 || bs <= 0)
    return PT2Q_E_ARG;
  if (xdtype != PT2Q_F16 && xdtype != PT2Q_BF16) return PT2Q_E_UNSUPPORTED;
  if (ydtype != xdtype && ydtype != PT2Q_F32) return PT2Q_E_ARG;
  if (bs < m && bs % 16 != 0) return PT2Q_E_UNSUPPORTED;  // alpha constant within a 16-group
  if ((long)ceil_div(m, bs < m ? bs : m) > B) return PT2Q_E_ARG;
  if (tokens > TD_MAX_TOKENS) return PT2Q_E_UNSUPPORTED;
  const int P = (int)pt2q_ternary_linear_positions(m);
  const int bse = bs < m ? bs : P;  // per-channel: one scale for every position
  const int nround = ceil_div(P / 64, 64);
  if (nround > TD_MAX_ROUNDS) return PT2Q_E_UNSUPPORTED;  // one token's activations past TD_LDS_MAX
  // LDS: the gathered activations of TG tokens and their staged rows of x.  Tokens per workgroup: as
  // many (1, 2, 4) as TD_LDS_PLAIN holds, no more than the call has; one token of a wide layer
  // may need more than that (up to 128 KiB at m = 32768), which the kernel is then allowed once
  const size_t rawbytes = ((size_t)m * 2 + 15) / 16 * 16;
  auto lds_of = [&](int tg) { return ((size_t)nround * TD_ROUND_BYTES + rawbytes) * tg; };
  int TG = 1;
  while (TG < 4 && TG < tokens && lds_of(2 * TG) <= TD_LDS_PLAIN) TG *= 2;
  const size_t lds = lds_of(TG);
  // two workgroups per CU in all (one per token group when the call has several groups)
  const int groups = ceil_div(tokens, TG);
  const dim3 grid(min(ceil_div(n, TD_WAVES), td_cus() * (groups > 1 ? 1 : 2)), groups);
  bool attr_failed = false;
  auto launch = [&](auto kern) {
    if (lds > TD_LDS_PLAIN) {
      static bool allowed = false;  // per kernel instantiation (the lambda's, one per `kern` type)
      if (!allowed) {
        if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, TD_LDS_MAX) !=
            hipSuccess) {
          attr_failed = true;
          return;
        }
        allowed = true;
      }
    }
    hipLaunchKernelGGL(kern, grid, dim3(TD_THREADS), lds, st, (const uint16_t*)x, (long)ldx, tokens, n, m, P, codes,
                       gather, alpha, mu, B, bse, bias, y, (long)ldy, ydtype == PT2Q_F32 ? 1 : 0);
  };
  if (xdtype == PT2Q_BF16)
    TG == 4 ? launch(tl_decode_kernel<true, 4>) : TG == 2 ? launch(tl_decode_kernel<true, 2>)
                                                          : launch(tl_decode_kernel<true, 1>);
  else
    TG == 4 ? launch(tl_decode_kernel<false, 4>) : TG == 2 ? launch(tl_decode_kernel<false, 2>)
                                                           : launch(tl_decode_kernel<false, 1>);
  if (attr_failed) {
    (void)hipGetLastError();
    return PT2Q_E_UNSUPPORTED;
  }
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}
