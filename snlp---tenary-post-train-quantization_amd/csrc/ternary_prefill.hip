// The grouped forms of the ternary linear layer's prefill kernel (ternary_linear.hip has the formula,
// the packing and tl_prefill_kernel, which pt2q_ternary_linear launches for tokens >= 256 and
// bse % 128 == 0).  One device body, tp_body -- tl_prefill_kernel's loop, instruction for instruction in
// the source -- and the two kernels that instantiate it.  tl_prefill_kernel itself keeps its own text:
// instantiated from tp_body it compiled to another schedule of the same instructions and measured
// 0.4 .. 1.2 % slower than the parent's (profiles/ternary_prefill_group_timing.txt), so the lone path is
// byte for byte what it was, and tests/test_gpu_ternary_prefill_group.py holds the two texts to the
// same bits.
//
//   tp_group_kernel     1 .. 4 layers that read the same x (q/k/v), PLAIN: blockIdx.x walks the
//                       members' 256-feature tiles one member after the other
//   tp_swiglu_kernel    gate and up of a gated MLP, 512 threads: waves 0-3 run the body on the gate,
//                       waves 4-7 on the up projection, for the same 256 features x 128 tokens; the
//                       two halves then trade one 32-feature tile each way through LDS and every wave
//                       finishes contract SWIGLU16 on its half.  g and u never reach memory.
//
// tp_body: one team of 4 waves = 256 features x 128 tokens, each wave 64 features x 128 tokens (2 x 4
// MFMA tiles, D[token][feature]: lane <-> feature, so the epilogue stores 32 consecutive features per
// half-wave).  The gathered activations go global -> LDS by LDS-DMA in stages of 64 positions x 128
// tokens (16 KiB, ring of 3; 16-byte chunks XOR-swizzled by (token >> 1) & 7, so the 16 lanes a
// ds_read_b128 serves per clock hit 16 distinct 4-bank groups) and are shared by the team's 4 waves;
// every wave dequantises its own 64 features per k-step from the 2-bit codes through the v_perm_b32
// tables of tl_gemm_kernel.  Codes and scales of the next 128-position block come one block ahead by
// LDS-DMA as well (plain loads would make the compiler wait vmcnt(0) -- every DMA in flight -- before
// their first use); the hand-counted vmcnt waits below cover them.  Needs bs % 128 == 0 (a table per
// 128-position block); y (+ bias) is written directly, no split partials.
//
// What fixes an output element's bits: it is ONE chain of 32x32x16 MFMAs over the 128-position blocks
// in ascending order, position 128 kb + 16 g + 8 h + j in k-slot (h, j) of step g.  tp_body keeps the
// lone kernel's mapping and order, so a member's bits are those of the lone kernel, at any token count.
//
// The pair kernel's LDS is 2 x (48 KiB ring + 20 KiB block slots) = 136 KiB of the CU's 160 KiB: one
// workgroup of eight waves per CU, the wave count of two resident lone workgroups.  Each team issues
// only its own DMAs (TP_DMA and TP_FETCH per thread are unchanged, so every wave's vmcnt arithmetic is
// the lone kernel's) and reads only its own ring (4 ds_read_b128 per 8 MFMAs, as alone); the one
// s_barrier per stage spans all eight waves.
#include "common.hpp"
#include "internal.hpp"
#include "ternary_shared.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int TP_F = 256, TP_T = 128, TP_KS = 64;
constexpr int TP_ROW = TP_KS * 2;            // 128 B per token row of a stage
constexpr int TP_STG = TP_T * TP_ROW;        // 16 KiB
constexpr int TP_NS = 3;
constexpr int TP_DMA = TP_STG / (256 * 16);  // DMA instructions per thread per stage (4)
constexpr int TP_CB = TP_F * 32;             // codes of one 128-position block: 32 B per feature
constexpr int TP_BLK = TP_CB + 2 * TP_F * 4; // + alpha and mu per feature (10 KiB)
constexpr int TP_FETCH = 4;                  // DMA instructions per thread per block (2 codes, alpha, mu)
constexpr int TP_LDS = TP_NS * TP_STG + 2 * TP_BLK;  // one team's ring and block slots (68 KiB)
constexpr int TP_XCH = 64 * 64 * 2;          // a wave's exchange tile: 32 features x 128 tokens, 16-bit (8 KiB)
static_assert(4 * TP_XCH <= TP_NS * TP_STG, "the four exchange tiles of a team reuse its ring");
static_assert(2 * TP_LDS <= 160 * 1024, "the pair kernel's two teams fit one CU");

__device__ uint4 tp_zero16;  // DMA source past the data (zero-initialised)

template <int OFF>
PT2Q_DEV u32x4 tp_ld(uint32_t addr) {
  u32x4 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "i"(OFF));
  return r;
}

PT2Q_DEV float tp_ldf(uint32_t addr) {
  float r;
  asm volatile("ds_read_b32 %0, %1" : "=v"(r) : "v"(addr));
  return r;
}

template <bool BF16>
PT2Q_DEV void tp_table(float a, float mm, uint32_t& t0, uint32_t& t1) {
  t0 = td_bits<BF16>(mm - a) | (td_bits<BF16>(mm) << 16);
  t1 = td_bits<BF16>(mm + a);
}

// 8 weights (one 16-position group of a lane's half) from 8 packed codes
PT2Q_DEV void tp_decode(uint32_t cb, uint32_t t0, uint32_t t1, uint32_t (&wv)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t q = ((cb >> (4 * j)) & 3u) | (((cb >> (4 * j + 2)) & 3u) << 16);
    wv[j] = __builtin_amdgcn_perm(t1, t0, q * 0x202u + 0x01000100u);
  }
}

// One team's work on one layer: smem is the team's TP_LDS bytes, wv its wave (0 .. 3, uniform), fb and
// t0 the tile's first feature and token.  PAIR: the SwiGLU epilogue of tp_swiglu_kernel -- `up` says
// which team this is, xmine / xpeer are the wave's exchange tile and that of the wave of the other team
// which holds the same (feature, token) elements in the same lanes and registers; y is h.
template <bool BF16, typename TY, bool PAIR>
PT2Q_DEV void tp_body(uint8_t* smem, int wv, int up, uint8_t* xmine, const uint8_t* xpeer, const uint8_t* codes, int P,
                      const float* alpha, const float* mu, int B, int bs, const uint16_t* xs, int tokens, int n,
                      const float* bias, TY* y, long ldy, int fb, int t0) {
  typedef __attribute__((address_space(3))) void* lptr;
  const int lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  const int nst = P / TP_KS;  // P is a multiple of 128: an even number of stages
  // activations of stage st: thread's q-th chunk = LDS slot L = (w * TP_DMA + q) * 64 + lane,
  // token row L / 8, holding global chunk (L % 8) ^ ((row >> 1) & 7)
  auto dma = [&](int st) {
    uint8_t* slot = smem + (st % TP_NS) * TP_STG;
#pragma unroll
    for (int q = 0; q < TP_DMA; ++q) {
      const int L = (wv * TP_DMA + q) * 64 + lane;
      const int row = L >> 3, c = (L & 7) ^ ((row >> 1) & 7);
      const int t = t0 + row;
      const void* src = t < tokens ? (const void*)(xs + (long)t * P + st * TP_KS + 8 * c) : (const void*)&tp_zero16;
      __builtin_amdgcn_global_load_lds(src, (lptr)(slot + (wv * TP_DMA + q) * 1024), 16, 0, 0);
    }
  };
  // codes (feature fl at fl * 32 + 16 half) and scales (alpha[fl], mu[fl]) of block kb, by
  // LDS-DMA into block slot kb % 2: TP_FETCH instructions per thread, issued in this order
  auto fetch = [&](int kb) {
    uint8_t* bsl = smem + TP_NS * TP_STG + (kb & 1) * TP_BLK;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int L = (wv * 2 + q) * 64 + lane;
      const int f = fb + (L >> 1);
      const void* src = f < n ? (const void*)(codes + (long)f * (P / 4) + 32 * kb + 16 * (L & 1))
                              : (const void*)&tp_zero16;
      __builtin_amdgcn_global_load_lds(src, (lptr)(bsl + (wv * 2 + q) * 1024), 16, 0, 0);
    }
    // blk <= B - 1 without a clamp: kb * 128 <= P - 128, and for bs % 128 == 0 the multiple of 128
    // ceil(m / bs) * bs >= m is at least P, so blk < ceil(m / bs) <= B; per-channel has bs = P, blk = 0
    const int f = fb + wv * 64 + lane, blk = (kb * 128) / bs;
    const void* sa = f < n ? (const void*)(alpha + (long)f * B + blk) : (const void*)&tp_zero16;
    const void* sm = f < n ? (const void*)(mu + (long)f * B + blk) : (const void*)&tp_zero16;
    __builtin_amdgcn_global_load_lds(sa, (lptr)(bsl + TP_CB + wv * 256), 4, 0, 0);
    __builtin_amdgcn_global_load_lds(sm, (lptr)(bsl + TP_CB + TP_F * 4 + wv * 256), 4, 0, 0);
  };
  float bvs[2];  // bias of the lane's two features (waited for before any DMA is in flight)
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int f = fb + wv * 64 + 32 * a + r;
    bvs[a] = (bias && f < n) ? bias[f] : 0.0f;
  }
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(bvs[0]), "+v"(bvs[1])::"memory");
  fetch(0);
  dma(0);
  if (nst > 1) dma(1);
  f32x16 acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][u][e] = 0.0f;
  // lane's LDS byte offset of k-step s inside a stage (token row r of token tile 0)
  uint32_t offs[4];
#pragma unroll
  for (int s2 = 0; s2 < 4; ++s2) offs[s2] = r * TP_ROW + (((2 * s2 + h) ^ ((r >> 1) & 7)) * 16);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem;
  const uint32_t blk0 = lds0 + TP_NS * TP_STG;
  u32x4 cw[2];
  uint32_t tab0[2], tab1[2];
  for (int st = 0; st < nst; ++st) {
    const bool blk_start = (st & 1) == 0;
    // stage st landed.  Issue order: at an even stage e [block fetch for e/2 + 1][DMA e+2], at
    // an odd one [DMA e+2].  Younger than stage st's DMA: at an even st, stage st+1's DMA; at
    // an odd st, the block fetch and stage st+1's DMA, both issued at st-1.  At an even st the
    // fetch of this block (issued at st-2, before stage st's DMA) has landed too.
    if (st + 1 >= nst)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (blk_start)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TP_DMA) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TP_DMA + TP_FETCH) : "memory");
    asm volatile("s_barrier" ::: "memory");
    if (blk_start) {  // this block's codes and tables from LDS, then fetch the next block
      const uint32_t bsl = blk0 + ((st >> 1) & 1) * TP_BLK;
      float av[2], mv[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int fl = wv * 64 + 32 * a + r;
        cw[a] = tp_ld<0>(bsl + fl * 32 + 16 * h);
        av[a] = tp_ldf(bsl + TP_CB + fl * 4);
        mv[a] = tp_ldf(bsl + TP_CB + TP_F * 4 + fl * 4);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(cw[0]), "+v"(cw[1]), "+v"(av[0]), "+v"(av[1]), "+v"(mv[0]),
                   "+v"(mv[1])::"memory");
#pragma unroll
      for (int a = 0; a < 2; ++a) tp_table<BF16>(av[a], mv[a], tab0[a], tab1[a]);
      if (st + 2 < nst) fetch(st / 2 + 1);
    }
    if (st + 2 < nst) dma(st + 2);
    const uint32_t sb = lds0 + (uint32_t)((st % TP_NS) * TP_STG);
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
      const uint32_t ad = sb + offs[s2];
      u32x4 xv[4];
      xv[0] = tp_ld<0>(ad);
      xv[1] = tp_ld<32 * TP_ROW>(ad);
      xv[2] = tp_ld<64 * TP_ROW>(ad);
      xv[3] = tp_ld<96 * TP_ROW>(ad);
      const int g = (st & 1) * 4 + s2;  // 16-position group inside the 128-position block
      uint32_t wq[2][4];
#pragma unroll
      for (int a = 0; a < 2; ++a) tp_decode((cw[a][g >> 1] >> (16 * (g & 1))) & 0xffffu, tab0[a], tab1[a], wq[a]);
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xv[0]), "+v"(xv[1]), "+v"(xv[2]), "+v"(xv[3]));
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if constexpr (BF16) {
            bf16x8 Wb, Xb;
            __builtin_memcpy(&Wb, wq[a], 16);
            __builtin_memcpy(&Xb, &xv[u], 16);
            acc[a][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Xb, Wb, acc[a][u], 0, 0, 0);
          } else {
            f16x8 Wb, Xb;
            __builtin_memcpy(&Wb, wq[a], 16);
            __builtin_memcpy(&Xb, &xv[u], 16);
            acc[a][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Xb, Wb, acc[a][u], 0, 0, 0);
          }
        }
    }
  }
  // D[token][feature]: feature = lane & 31 (+ 32 a), token = (e & 3) + 8 (e >> 2) + 4 h (+ 32 u)
  if constexpr (!PAIR) {
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int f = fb + wv * 64 + 32 * a + r;
      if (f >= n) continue;
      const float bv = bvs[a];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int t = t0 + 32 * u + (e & 3) + 8 * (e >> 2) + 4 * h;
          if (t < tokens) y[(long)t * ldy + f] = (TY)(bias ? acc[a][u][e] + bv : acc[a][u][e]);
        }
    }
  } else {
    // The gate team finishes feature tile a = 0 of every wave, the up team tile a = 1.  A wave rounds
    // all its values to TY after the bias add (the lone call's 16-bit outputs), writes the tile it does
    // not finish into its exchange tile -- lane-private: 8 x 16 bytes per lane, chunk k of lane l at
    // (k * 64 + l) * 16, so a wave's ds_write_b128 / ds_read_b128 are conflict-free -- and reads the
    // other team's values for the tile it keeps from the same place in that team's ring.
    auto fin = [&](int a, int u, int e) {  // 16-bit value of element (a, u, e)
      return td_bits<BF16>(bias ? acc[a][u][e] + bvs[a] : acc[a][u][e]);
    };
    __syncthreads();  // every wave is past its last read of the rings
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      u32x4 pk;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int u = k >> 1, e = 8 * (k & 1) + 2 * j;
        const uint32_t g0 = fin(0, u, e) | (fin(0, u, e + 1) << 16), g1 = fin(1, u, e) | (fin(1, u, e + 1) << 16);
        pk[j] = up ? g0 : g1;  // the tile the other team finishes
      }
      *(u32x4*)(xmine + (k * 64 + lane) * 16) = pk;
    }
    __syncthreads();
    const int f = fb + wv * 64 + 32 * up + r;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const u32x4 pk = *(const u32x4*)(xpeer + (k * 64 + lane) * 16);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int u = k >> 1, e = 8 * (k & 1) + 2 * j;
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const float own = td_lo<BF16>(up ? fin(1, u, e + d) : fin(0, u, e + d));
          const float peer = d ? td_hi<BF16>(pk[j]) : td_lo<BF16>(pk[j]);
          const float hv = td_swiglu<BF16>(up ? peer : own, up ? own : peer);
          const int t = t0 + 32 * u + ((e + d) & 3) + 8 * ((e + d) >> 2) + 4 * h;
          if (f < n && t < tokens) y[(long)t * ldy + f] = (TY)hv;
        }
      }
    }
  }
}

// ---- The grouped call: 1 .. 4 layers that read the same x.  The members' device pointers travel by
// value in the kernel arguments (TsGroup's way, ternary_skinny.hip); entries past the call's count
// repeat the last tile_end and own no workgroup.
struct TpGroup {
  const uint8_t* codes[PT2Q_DECODE_GROUP_MAX];
  const float* alpha[PT2Q_DECODE_GROUP_MAX];
  const float* mu[PT2Q_DECODE_GROUP_MAX];
  const float* bias[PT2Q_DECODE_GROUP_MAX];
  void* y[PT2Q_DECODE_GROUP_MAX];
  long ldy[PT2Q_DECODE_GROUP_MAX];
  int n[PT2Q_DECODE_GROUP_MAX];
  int B[PT2Q_DECODE_GROUP_MAX];
  int tile_end[PT2Q_DECODE_GROUP_MAX];  // member z owns blockIdx.x in [tile_end[z - 1], tile_end[z])
};
struct TpGatherGroup {
  const int* g[PT2Q_DECODE_GROUP_MAX];
};

// x_sel[z][t][p] = x[t][g_z[p]] (0 at padding positions) for member z = blockIdx.y: every linear has
// its own order of the columns, so every member has its own x_sel.  A thread gathers 8 consecutive
// positions and writes them with one 16-byte store (P % 128 == 0; x_sel images start 256-byte aligned).
__global__ void tp_gather_group_kernel(const uint16_t* x, long ldx, int tokens, TpGatherGroup G, int P, uint16_t* xs,
                                       long xs_stride) {
  const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int chunks = P / 8;
  if (q >= (long)tokens * chunks) return;
  const int t = (int)(q / chunks), p = (int)(q % chunks) * 8;
  const int* g = td_pick(G.g, (int)blockIdx.y) + p;
  const uint16_t* xr = x + (long)t * ldx;
  uint32_t v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c0 = g[2 * j], c1 = g[2 * j + 1];
    const uint32_t lo = c0 >= 0 ? xr[c0] : 0u, hi = c1 >= 0 ? xr[c1] : 0u;
    v[j] = lo | (hi << 16);
  }
  *(uint4*)(xs + blockIdx.y * xs_stride + (long)t * P + p) = make_uint4(v[0], v[1], v[2], v[3]);
}

// PLAIN: the lone kernel's workgroup, on the member whose tile blockIdx.x is
template <bool BF16, typename TY>
__global__ __launch_bounds__(256, 2) void tp_group_kernel(int P, int bs, const uint16_t* xs, long xs_stride, int tokens,
                                                          TpGroup G) {
  __shared__ __attribute__((aligned(1024))) uint8_t smem[TP_LDS];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile = blockIdx.x;
  int z = 0, first = 0;
  if (tile >= G.tile_end[0]) z = 1, first = G.tile_end[0];
  if (tile >= G.tile_end[1]) z = 2, first = G.tile_end[1];
  if (tile >= G.tile_end[2]) z = 3, first = G.tile_end[2];
  tp_body<BF16, TY, false>(smem, wv, 0, nullptr, nullptr, td_pick(G.codes, z), P, td_pick(G.alpha, z), td_pick(G.mu, z),
                           td_pick(G.B, z), bs, xs + z * xs_stride, tokens, td_pick(G.n, z), td_pick(G.bias, z),
                           (TY*)td_pick(G.y, z), td_pick(G.ldy, z), (tile - first) * TP_F, blockIdx.y * TP_T);
}

// SWIGLU: team 0 (waves 0-3) on member 0, the gate, team 1 (waves 4-7) on member 1, the up projection
template <bool BF16, typename TY>
__global__ __launch_bounds__(512) void tp_swiglu_kernel(int P, int bs, const uint16_t* xs, long xs_stride, int tokens,
                                                        TpGroup G) {
  __shared__ __attribute__((aligned(1024))) uint8_t smem[2 * TP_LDS];
  const int w8 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int up = w8 >> 2, wv = w8 & 3;
  uint8_t* mine = smem + up * TP_LDS;
  const uint8_t* peer = smem + (up ^ 1) * TP_LDS;
  tp_body<BF16, TY, true>(mine, wv, up, mine + wv * TP_XCH, peer + wv * TP_XCH, up ? G.codes[1] : G.codes[0], P,
                          up ? G.alpha[1] : G.alpha[0], up ? G.mu[1] : G.mu[0], up ? G.B[1] : G.B[0], bs,
                          xs + up * xs_stride, tokens, G.n[0], up ? G.bias[1] : G.bias[0], (TY*)G.y[0], G.ldy[0],
                          blockIdx.x * TP_F, blockIdx.y * TP_T);
}

size_t tp_xs_bytes(int tokens, int P) { return ((size_t)tokens * P * 2 + 255) / 256 * 256; }

}  // namespace

extern "C" size_t pt2q_ternary_prefill_group_workspace_bytes(int tokens, int m, int count) {
  if (tokens <= 0 || m <= 0 || count < 1 || count > PT2Q_DECODE_GROUP_MAX) return 0;
  // one gathered x_sel (tokens x P 16-bit) per member
  return (size_t)count * tp_xs_bytes(tokens, (int)pt2q_ternary_linear_positions(m)) + 256;
}

extern "C" int pt2q_ternary_prefill_group(const void* x, int xdtype, int tokens, int64_t ldx, int m, int count,
                                          const int* n, const uint8_t* const* codes, const int* const* gather,
                                          const float* const* alpha, const float* const* mu, const int* B, int bs,
                                          const float* const* bias, void* const* y, int ydtype, const int64_t* ldy,
                                          int epilogue, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!x || !n || !codes || !gather || !alpha || !mu || !B || !y || !ldy || tokens <= 0 || m <= 0 || ldx < m ||
      bs <= 0 || count < 1 || count > PT2Q_DECODE_GROUP_MAX)
    return PT2Q_E_ARG;
  const bool swiglu = epilogue == PT2Q_DECODE_SWIGLU;
  if (!swiglu && epilogue != PT2Q_DECODE_PLAIN) return PT2Q_E_ARG;
  if (swiglu && (count != 2 || n[0] != n[1] || ydtype == PT2Q_F32)) return PT2Q_E_ARG;
  const int nout = swiglu ? 1 : count;  // outputs the call writes
  for (int z = 0; z < count; ++z) {
    if (!codes[z] || !gather[z] || !alpha[z] || !mu[z] || n[z] <= 0 || B[z] <= 0) return PT2Q_E_ARG;
    if (z < nout && (!y[z] || ldy[z] < n[z])) return PT2Q_E_ARG;
  }
  if (xdtype != PT2Q_F16 && xdtype != PT2Q_BF16) return PT2Q_E_UNSUPPORTED;
  if (ydtype != xdtype && ydtype != PT2Q_F32) return PT2Q_E_ARG;
  if (bs < m && bs % 128 != 0) return PT2Q_E_UNSUPPORTED;  // a weight table per 128-position block
  for (int z = 0; z < count; ++z)
    if ((long)ceil_div(m, bs < m ? bs : m) > B[z]) return PT2Q_E_ARG;
  for (int z = 0; z < count; ++z)
    if ((uintptr_t)codes[z] % 16 != 0) return PT2Q_E_UNSUPPORTED;  // the 16-byte code DMAs
  if (!workspace || (uintptr_t)workspace % 256 != 0) return PT2Q_E_UNSUPPORTED;
  if (workspace_bytes < pt2q_ternary_prefill_group_workspace_bytes(tokens, m, count)) return PT2Q_E_WORKSPACE;
  const int P = (int)pt2q_ternary_linear_positions(m);
  const int bse = bs < m ? bs : P;  // per-channel: one scale for every position
  uint16_t* xs = (uint16_t*)workspace;
  const long xs_stride = (long)(tp_xs_bytes(tokens, P) / 2);
  TpGroup G{};
  TpGatherGroup GG{};
  int tile_end = 0;
  for (int z = 0; z < PT2Q_DECODE_GROUP_MAX; ++z) {
    const int s = z < count ? z : 0;  // entries past count repeat member 0 and own no workgroup
    if (z < count) tile_end += ceil_div(n[z], TP_F);
    G.codes[z] = codes[s], G.alpha[z] = alpha[s], G.mu[z] = mu[s], G.bias[z] = bias ? bias[s] : nullptr;
    G.n[z] = n[s], G.B[z] = B[s], G.tile_end[z] = tile_end;
    G.y[z] = s < nout ? y[s] : nullptr, G.ldy[z] = s < nout ? (long)ldy[s] : 0;
    GG.g[z] = gather[s];
  }
  hipLaunchKernelGGL(tp_gather_group_kernel, dim3(ceil_div((long)tokens * (P / 8), 256), count), dim3(256), 0, st,
                     (const uint16_t*)x, (long)ldx, tokens, GG, P, xs, xs_stride);
  PT2Q_LAUNCH_CHECK();
  const bool bf16 = xdtype == PT2Q_BF16;
  const int ttiles = ceil_div(tokens, TP_T);
  auto go = [&](auto kern, int tiles, int threads) {
    hipLaunchKernelGGL(kern, dim3(tiles, ttiles), dim3(threads), 0, st, P, bse, (const uint16_t*)xs, xs_stride, tokens, G);
  };
  if (swiglu)
    bf16 ? go(tp_swiglu_kernel<true, __bf16>, ceil_div(n[0], TP_F), 512)
         : go(tp_swiglu_kernel<false, _Float16>, ceil_div(n[0], TP_F), 512);
  else if (ydtype == PT2Q_F32)
    bf16 ? go(tp_group_kernel<true, float>, tile_end, 256) : go(tp_group_kernel<false, float>, tile_end, 256);
  else
    bf16 ? go(tp_group_kernel<true, __bf16>, tile_end, 256) : go(tp_group_kernel<false, _Float16>, tile_end, 256);
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}
