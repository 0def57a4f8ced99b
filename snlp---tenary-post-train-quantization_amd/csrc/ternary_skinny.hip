// Ternary linear layer for 2..64 tokens (batched decode, speculative decoding, short prompts):
// the contract of ternary_linear.hip's header comment,
//
//   y[t][i] = Σ_p Wd[i][p] · x[t][g[p]] + bias[i],   Wd[i][p] = TX(α[i][blk]·c[i][p] + μ[i][blk]),
//   blk = min(pg / bs, B - 1) per 16-position group pg (per-channel layers: bs = P),
//
// on the operands pt2q_ternary_pack already writes, in two launches: the gather of x into position
// order (x_sel, which also zeroes the tile counters) and ts_kernel, which does the GEMM, the K-split
// reduction and the conversion to y.
//
// MFMA shape.  v_mfma_f32_16x16x32_{f16,bf16} (lane layout: tools/mfma16x16_probe.hip): features
// on A's 16 rows, tokens on B's 16 columns, so a call of up to 16 tokens fills its one token tile.
// Lane l has r = l & 15 (A row / B column) and kq = l >> 4, split as h = kq & 1, gq = kq >> 1.  The 8
// bytes at crow + 32 kb + 16 h + 8 gq of the packed row hold the four 16-bit code groups
// g = 4 gq + s, s = 0..3; MFMA s of block kb contracts positions 128 kb + 16 g + 8 h + j, j = 0..7,
// with A dequantised from code group s (the v_perm_b32 three-entry table) and B the 16 contiguous
// bytes x_sel[t = r][128 kb + 16 g + 8 h ..].  One 8-byte code load per lane feeds four MFMAs, and
// one dequantised A operand is reused over NT = ceil(tokens / 16) <= 4 token tiles (4 NT
// accumulator VGPRs).  D holds 4 consecutive features (4 kq + q) of token r per lane, so partials
// and y go out as 16-byte stores.
//
// Work split.  A workgroup is 4 waves x 16 features (TS_F = 64) times one K slice of whole
// 128-position blocks; slice z of `splits` takes blocks [z nkb / splits, (z + 1) nkb / splits).
// ts_plan, shared by the workspace query and the launcher, picks
//   splits = clamp(ceil(512 / tiles), 1, min(16, nkb / 2)),   tiles = ceil(n / 64):
// about two workgroups on each of the 256 CUs (the codes are read once whatever the split, so
// the split only buys parallelism for the HBM stream, and two resident workgroups per CU keep a
// block's loads in flight under the other's MFMAs); at least 2 blocks per slice where P allows, so
// the one-block-ahead prefetch has something to hide behind; at most 16 partials to re-read.
// 64 against 128 features per workgroup (PT2Q_TS_FT = 2: half the x traffic from L2, but half the
// tiles, so half the workgroups or twice the partials) was decided by measurement: 128 is slower at
// every shape and token count, 18.6 against 14.0 us at 4096^2 fp16 for 2 tokens, 43.9 against 23.5
// for 64 (profiles/ternary_skinny_timing.txt).  The macro stays as the way to
// repeat that measurement (make EXTRA_HIPFLAGS=-DPT2Q_TS_FT=2; the tests pass with it).
//
// x through LDS.  The workgroup stages its K slice of x_sel in stages of 128 positions x 16 NT
// tokens (4 NT KiB), a ring of 3 loaded by LDS-DMA two stages ahead and shared by the four waves.
// A token row is 256 B = 16 chunks of 16 B; chunk c of row t sits at chunk c ^ (t & 15), so the
// 16 lanes a ds_read_b128 serves per clock (one chunk index, 16 token rows) hit 16 distinct
// 4-bank groups.  Token rows >= tokens read a zero source.  Codes and scales go straight to
// registers one block ahead (plain loads, issued with the DMA of stage j + 2).  The hand-counted
// vmcnt(NT) at the top of an iteration is what stage j's correctness rests on; it would leave stage
// j + 1's DMA in flight, but the compiler then places its own vmcnt(0) before the first use of the
// block's codes and scales, which were issued in the same iteration as that DMA.  As compiled, every
// iteration therefore drains all loads: the ring buys one whole iteration of lead for x, not two,
// and the loop's latency chain is the code load issued one block earlier.
// One s_barrier per block: it publishes stage j and frees stage j - 1's slot for stage j + 2.
// LDS: 12 NT KiB <= 48 KiB; no scratch.
//
// Split reduction in the same launch.  Every workgroup writes its fp32 partial tile to the
// workspace ([split][token][feature], rows padded to 64 features) with agent-scope write-through
// (sc1) stores (the XCDs' L2s are not coherent for plain stores), drains them, and takes a ticket
// with atomicAdd on its tile's counter.  The workgroup that draws ticket splits - 1 reads all
// partials from memory with sc1 loads and sums them as tl_reduce_kernel does,
// ((p0 + p1) + ...) + bias -- the order is fixed
// whichever workgroup is last, so the result is identical run to run -- converts and stores y.
// Nobody waits for anybody: no spin, no grid sync.  The gather launch zeroes the counters, so
// nothing depends on what an earlier call left in the workspace.  splits = 1 stores y directly.
//
// Grouped variant (pt2q_ternary_skinny_group; kernels and their comments below ts_kernel).  Up to
// four layers that read the same x -- q/k/v, or a gated MLP's gate and up -- in ONE gather launch
// (grid.y = member: each member has its own column order, so its own x_sel) and ONE GEMM launch whose
// blockIdx.x walks the members' feature tiles one member after the other (at most three compares
// against the tile prefix sums find the member).  Each member keeps the split count ts_plan gives it
// alone, and the per-lane design above is untouched (ts_body is the one body of both kernels), so a
// member's partial tiles and their sum are the lone call's, bit for bit.  SWIGLU reduces the gate
// and the up tile of the same features under one shared ticket and applies contract SWIGLU16
// (ternary_shared.hpp, the decode kernel's arithmetic) where the partials are summed anyway: the
// fp32-to-16-bit stores of g and u, their re-reads and two elementwise launches disappear.
//
// Norm prologue and residual epilogue (pt2q_ternary_skinny_fused), still two launches.  The gather
// already reads every element of x, so contract RMSNORM16 runs there: ts_norm_gather_kernel, one
// 512-thread workgroup per (token, member), normalises the row into a 2 m-byte LDS image and gathers
// x_sel from LDS (its comment has the steps; m <= 32768).  The residual belongs where y is converted:
// ts_body's RES flag adds contract RESADD16 to finish(), on the direct path and in the last-ticket
// workgroup, whose lanes ask for the residual of exactly the elements they will store (so it may be y
// itself) before they walk the partial slices.  The flag is off in ts_kernel and ts_group_kernel, whose
// instructions are what they were; ts_group_res_kernel is the PLAIN grouped kernel with it on and the
// residual pointers as one more by-value argument.  Both contracts' arithmetic is the decode kernel's
// (ternary_shared.hpp), so the bits are those of pt2q_rmsnorm, the plain call and a 16-bit add.
#include <cfloat>

#include "common.hpp"
#include "internal.hpp"
#include "ternary_shared.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

#ifndef PT2Q_TS_FT
#define PT2Q_TS_FT 1
#endif
constexpr int TS_PB = 128;          // positions per packed block
constexpr int TS_MAX_TOKENS = 64;
constexpr int TS_FT = PT2Q_TS_FT;   // 16-feature MFMA tiles per wave
constexpr int TS_F = 64 * TS_FT;    // features per workgroup
constexpr int TS_ROW = TS_PB * 2;   // 256 B per token row of a stage
constexpr int TS_STG = 16 * TS_ROW; // 4 KiB per token tile of a stage
constexpr int TS_NS = 3;            // ring
constexpr int TS_WGS = 512;         // workgroups the plan aims at: two per CU

__device__ uint4 ts_zero16;  // DMA source of token rows past the call's (zero-initialised)

// x_sel[t][p] = x[t][g[p]] (0 for padding), 16-bit elements; tile counters to 0
__global__ void ts_gather_kernel(const uint16_t* x, long ldx, int tokens, const int* g, int P, uint16_t* xs,
                                 int* cnt, int tiles) {
  const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long c = q; c < tiles; c += (long)gridDim.x * blockDim.x) cnt[c] = 0;
  if (q >= (long)tokens * P) return;
  const int t = (int)(q / P), p = (int)(q % P);
  const int c = g[p];
  xs[q] = (c >= 0) ? x[(long)t * ldx + c] : (uint16_t)0;
}

template <bool BF16>
PT2Q_DEV uint32_t to_bits(float v) {
  if constexpr (BF16) {
    __bf16 h = (__bf16)v;
    uint16_t u;
    __builtin_memcpy(&u, &h, 2);
    return u;
  } else {
    _Float16 h = (_Float16)v;
    uint16_t u;
    __builtin_memcpy(&u, &h, 2);
    return u;
  }
}

// the three possible weights TX(mu - alpha), TX(mu), TX(mu + alpha) as an 8-byte table
template <bool BF16>
PT2Q_DEV void ts_table(float a, float mm, uint32_t& t0, uint32_t& t1) {
  t0 = to_bits<BF16>(mm - a) | (to_bits<BF16>(mm) << 16);
  t1 = to_bits<BF16>(mm + a);
}

// 8 weights from the 8 packed codes of one 16-bit code group
PT2Q_DEV void ts_decode(uint32_t cb, uint32_t t0, uint32_t t1, uint32_t (&wv)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t q = ((cb >> (4 * j)) & 3u) | (((cb >> (4 * j + 2)) & 3u) << 16);
    wv[j] = __builtin_amdgcn_perm(t1, t0, q * 0x202u + 0x01000100u);
  }
}

template <int OFF>
PT2Q_DEV u32x4 ts_ld(uint32_t addr) {
  u32x4 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "i"(OFF));
  return r;
}

// four consecutive features i0..i0+3 of token t: one 16-byte (fp32) or 8-byte (16-bit) store
// where y allows it (vec: base and ldy aligned to four elements), element stores at a ragged edge
template <typename TY>
PT2Q_DEV void ts_store4(TY* y, long ldy, int t, int i0, int n, bool vec, const float (&v)[4]) {
  TY* p = y + (long)t * ldy + i0;
  if (vec && i0 + 3 < n) {
    if constexpr (sizeof(TY) == 4) {
      f32x4 o = {v[0], v[1], v[2], v[3]};
      *(f32x4*)p = o;
    } else {
      TY o[4] = {(TY)v[0], (TY)v[1], (TY)v[2], (TY)v[3]};
      u32x2 w;
      __builtin_memcpy(&w, o, 8);
      *(u32x2*)p = w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (i0 + q < n) p[q] = (TY)v[q];
  }
}

// The residual of the four elements ts_store4 will store for this lane, two per register, +0 where it
// stores nothing: one 8-byte load where res allows it (vec: base and ldr aligned to four elements),
// element loads at a ragged edge.  A lane reads what it will write and nothing else: res may be y.
PT2Q_DEV u32x2 ts_res4(const uint16_t* res, long ldr, int t, int i0, int n, bool vec) {
  const uint16_t* p = res + (long)t * ldr + i0;
  u32x2 w = {0u, 0u};
  if (vec && i0 + 3 < n) {
    w = *(const u32x2*)p;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (i0 + q < n) w[q >> 1] |= (uint32_t)p[q] << (16 * (q & 1));
  }
  return w;
}

// What the SWIGLU epilogue needs of the two members, gate then up (the grouped kernel's TsGroup entries)
struct TsPair {
  float* part[2];
  const float* bias[2];
  int splits[2];
};

// One workgroup's work, the body of the lone and of the grouped kernel: features fb .. fb + TS_F - 1
// of one layer (n features, partial rows of nP floats, K slice z of `splits`, ticket counter *ticket).
// SWIGLU (grouped kernel only): the layer is the gate or the up projection of `pair`, y is h.
// RES (pt2q_ternary_skinny_fused, PLAIN, 16-bit y): contract RESADD16 where y is converted, on the
// direct path and in the last-ticket workgroup, y = RN_TY(f32(RN_TY(v + bias)) + f32(res)); res NULL
// for a member without a residual.  With RES off res, ldr and rvec are not looked at.
template <bool BF16, int NT, typename TY, bool SWIGLU, bool RES>
PT2Q_DEV void ts_body(const uint8_t* codes, int P, const float* alpha, const float* mu, int B, int bse,
                      const uint16_t* xs, int tokens, int n, int nP, int splits, float* part, int* ticket,
                      const float* bias, TY* y, long ldy, int yvec, int fb, int z, const TsPair& pair,
                      const uint16_t* res, long ldr, int rvec) {
  static_assert(!RES || (!SWIGLU && sizeof(TY) == 2), "RESADD16 is 16-bit and h has no residual");
  __shared__ __attribute__((aligned(1024))) uint8_t smem[TS_NS * TS_STG * NT];
  __shared__ int s_last;
  typedef __attribute__((address_space(3))) void* lptr;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, kq = lane >> 4, h = kq & 1, gq = kq >> 1;
  const int nkb = P / TS_PB;  // slice z: blocks [kb0, kb1)
  const int kb0 = z * nkb / splits, kb1 = (z + 1) * nkb / splits;  // splits <= 16, nkb < 2^24
  const int nb = kb1 - kb0;
  // stage j (block kb0 + j) into ring slot j % TS_NS: 16-byte LDS slot S = (wv NT + q) 64 + lane is
  // chunk S & 15 of token row S >> 4 and holds that row's global chunk (S & 15) ^ (row & 15)
  auto dma = [&](int j) {
    uint8_t* slot = smem + (j % TS_NS) * (TS_STG * NT);
    const uint16_t* src0 = xs + (long)(kb0 + j) * TS_PB;
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int S = (wv * NT + q) * 64 + lane;
      const int row = S >> 4, c = (S & 15) ^ (row & 15);
      const void* src = row < tokens ? (const void*)(src0 + (long)row * P + 8 * c) : (const void*)&ts_zero16;
      __builtin_amdgcn_global_load_lds(src, (lptr)(slot + (wv * NT + q) * 1024), 16, 0, 0);
    }
  };
  // the lane's A rows: feature fb + (wv TS_FT + f) 16 + r; rows past n read row 0 and store nothing
  const uint8_t* crow[TS_FT];
  const float *arow[TS_FT], *mrow[TS_FT];
#pragma unroll
  for (int f = 0; f < TS_FT; ++f) {
    const int i = fb + (wv * TS_FT + f) * 16 + r;
    const long row = i < n ? i : 0;
    crow[f] = codes + row * (P / 4) + 16 * h + 8 * gq;
    arow[f] = alpha + row * B;
    mrow[f] = mu + row * B;
  }
  // scale block of the lane's first 16-position group in block kb (padding positions can have
  // pg / bse = B, one past the row's scales: clamped as in ternary_linear.hip)
  auto blk_of = [&](int kb, int s) { return min((TS_PB * kb + 16 * (4 * gq + s)) / bse, B - 1); };
  u32x2 cwn[TS_FT];
  float an[TS_FT], mn[TS_FT];
  auto fetch = [&](int kb) {  // codes and first scales of block kb
    const int blk = blk_of(kb, 0);
#pragma unroll
    for (int f = 0; f < TS_FT; ++f) {
      cwn[f] = *(const u32x2*)(crow[f] + 32 * kb);
      an[f] = arow[f][blk];
      mn[f] = mrow[f][blk];
    }
  };
  fetch(kb0);
  dma(0);
  if (nb > 1) dma(1);
  f32x4 acc[TS_FT][NT];
#pragma unroll
  for (int f = 0; f < TS_FT; ++f)
#pragma unroll
    for (int u = 0; u < NT; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[f][u][e] = 0.0f;
  // lane's LDS byte offset of MFMA s inside a stage (token row r of token tile 0): chunk 8 gq + 2 s + h
  uint32_t offs[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) offs[s] = r * TS_ROW + (((8 * gq + 2 * s + h) ^ r) * 16);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem;
  for (int j = 0; j < nb; ++j) {
    // Issue order: [fetch(kb0)][DMA 0][DMA 1], then per iteration j [fetch(j + 1)][DMA j + 2].
    // Younger than stage j's DMA and this block's fetch is only stage j + 1's DMA (NT per thread), so
    // vmcnt(NT) makes stage j safe to read.  (The compiler's vmcnt(0) for cwn / an / mn below then
    // drains stage j + 1 as well: an over-wait, see the header comment.)
    if (j + 1 < nb)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NT) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
    const int kb = kb0 + j;
    u32x2 cw[TS_FT];
    uint32_t tab0[TS_FT], tab1[TS_FT];
    int tblk = blk_of(kb, 0);
#pragma unroll
    for (int f = 0; f < TS_FT; ++f) {
      cw[f] = cwn[f];
      ts_table<BF16>(an[f], mn[f], tab0[f], tab1[f]);
    }
    if (j + 1 < nb) fetch(kb + 1);
    if (j + 2 < nb) dma(j + 2);
    const uint32_t sb = lds0 + (uint32_t)((j % TS_NS) * (TS_STG * NT));
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int blk = blk_of(kb, s);
      if (blk != tblk) {  // bs below 64 or not a multiple of it: the table switches inside the lane's groups
        tblk = blk;
#pragma unroll
        for (int f = 0; f < TS_FT; ++f) ts_table<BF16>(arow[f][blk], mrow[f][blk], tab0[f], tab1[f]);
      }
      const uint32_t ad = sb + offs[s];
      u32x4 xv[NT];
      xv[0] = ts_ld<0>(ad);
      if constexpr (NT > 1) xv[1] = ts_ld<TS_STG>(ad);
      if constexpr (NT > 2) xv[2] = ts_ld<2 * TS_STG>(ad);
      if constexpr (NT > 3) xv[3] = ts_ld<3 * TS_STG>(ad);
      uint32_t wq[TS_FT][4];
#pragma unroll
      for (int f = 0; f < TS_FT; ++f) ts_decode((cw[f][s >> 1] >> (16 * (s & 1))) & 0xffffu, tab0[f], tab1[f], wq[f]);
      if constexpr (NT == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xv[0]));
      if constexpr (NT == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xv[0]), "+v"(xv[1]));
      if constexpr (NT == 3) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xv[0]), "+v"(xv[1]), "+v"(xv[2]));
      if constexpr (NT == 4) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xv[0]), "+v"(xv[1]), "+v"(xv[2]), "+v"(xv[3]));
#pragma unroll
      for (int f = 0; f < TS_FT; ++f)
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          if constexpr (BF16) {
            bf16x8 Wb, Xb;
            __builtin_memcpy(&Wb, wq[f], 16);
            __builtin_memcpy(&Xb, &xv[u], 16);
            acc[f][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Wb, Xb, acc[f][u], 0, 0, 0);
          } else {
            f16x8 Wb, Xb;
            __builtin_memcpy(&Wb, wq[f], 16);
            __builtin_memcpy(&Xb, &xv[u], 16);
            acc[f][u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Wb, Xb, acc[f][u], 0, 0, 0);
          }
        }
    }
  }
  // D[feature 4 kq + q][token r]: the lane holds features i0 .. i0 + 3 of token 16 u + r
  // RES: the residual of what the lane will store, asked for ahead of the sums it is added to
  u32x2 rr[TS_FT][NT];
  auto load_res = [&]() {
    if constexpr (RES) {
#pragma unroll
      for (int f = 0; f < TS_FT; ++f)
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          rr[f][u] = u32x2{0u, 0u};
          if (res && 16 * u + r < tokens)
            rr[f][u] = ts_res4(res, ldr, 16 * u + r, fb + (wv * TS_FT + f) * 16 + 4 * kq, n, rvec != 0);
        }
    }
  };
  auto finish = [&](int f, int u, float (&v)[4]) {  // + bias, (+ residual,) convert, store
    const int i0 = fb + (wv * TS_FT + f) * 16 + 4 * kq;
    if (bias) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (i0 + q < n) v[q] = v[q] + bias[i0 + q];
    }
    if constexpr (RES) {
      if (res) {
        const u32x2 w = rr[f][u];
        const float rf[4] = {td_lo<BF16>(w[0]), td_hi<BF16>(w[0]), td_lo<BF16>(w[1]), td_hi<BF16>(w[1])};
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = td_rounded(td_round<BF16>(v[q]) + rf[q]);
      }
    }
    ts_store4(y, ldy, 16 * u + r, i0, n, yvec != 0, v);
  };
  if (!SWIGLU && splits == 1) {
    load_res();
#pragma unroll
    for (int f = 0; f < TS_FT; ++f)
#pragma unroll
      for (int u = 0; u < NT; ++u) {
        if (16 * u + r >= tokens) continue;
        float v[4] = {acc[f][u][0], acc[f][u][1], acc[f][u][2], acc[f][u][3]};
        finish(f, u, v);
      }
    return;
  }
  // partial tile: part[z][t][i], rows of nP = tiles * TS_F floats, so every 16-byte store is inside
  // (the launchers keep splits * zs below 2^31).  Agent-scope hand-off as in
  // ssr.hip: write-through (sc1) stores, drained by every wave before the barrier that precedes
  // the ticket, and sc1 loads in the last workgroup -- they pass this XCD's L2 by, and no fence
  // writes back or invalidates a whole L2 under the other workgroups' x_sel and code lines.
  const int zs = tokens * nP * 4;
  const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(part, 0, splits * zs, 0x00020000);
#pragma unroll
  for (int f = 0; f < TS_FT; ++f)
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int t = 16 * u + r;
      if (t < tokens)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[f][u]), rp,
                                               z * zs + (t * nP + fb + (wv * TS_FT + f) * 16 + 4 * kq) * 4, 0, 16);  // sc1
    }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // SWIGLU: the gate and the up tile of these features share the counter, and both always get here
  const int target = SWIGLU ? pair.splits[0] + pair.splits[1] : splits;
  if (threadIdx.x == 0) s_last = atomicAdd(ticket, 1) == target - 1;
  __syncthreads();
  if (!s_last) return;
  load_res();  // in flight under the sc1 loads of the partial slices
  // v = (p0 + p1) + ... over the `ns` slices of a fragment in rs, in slice order
  auto sum = [&](const __amdgpu_buffer_rsrc_t rs, int ns, int off, float (&v)[4]) {
    const f32x4 s4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16));
    v[0] = s4[0], v[1] = s4[1], v[2] = s4[2], v[3] = s4[3];
    for (int zz = 1; zz < ns; ++zz) {
      const f32x4 p4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, zz * zs + off, 0, 16));
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = v[q] + p4[q];
    }
  };
#pragma unroll
  for (int f = 0; f < TS_FT; ++f)
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int t = 16 * u + r;
      if (t >= tokens) continue;
      const int off = (t * nP + fb + (wv * TS_FT + f) * 16 + 4 * kq) * 4;
      if constexpr (!SWIGLU) {
        float v[4];
        sum(rp, splits, off, v);
        finish(f, u, v);
      } else {
        // g and u as the two lone calls round them, then contract SWIGLU16 (td_swiglu leaves its last
        // rounding to the store's conversion to TY)
        const int i0 = fb + (wv * TS_FT + f) * 16 + 4 * kq;
        float gv[4], uv[4];
        sum(__builtin_amdgcn_make_buffer_rsrc(pair.part[0], 0, pair.splits[0] * zs, 0x00020000), pair.splits[0], off, gv);
        sum(__builtin_amdgcn_make_buffer_rsrc(pair.part[1], 0, pair.splits[1] * zs, 0x00020000), pair.splits[1], off, uv);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (i0 + q < n) {
            if (pair.bias[0]) gv[q] = gv[q] + pair.bias[0][i0 + q];
            if (pair.bias[1]) uv[q] = uv[q] + pair.bias[1][i0 + q];
          }
          gv[q] = td_swiglu<BF16>(td_round<BF16>(gv[q]), td_round<BF16>(uv[q]));
        }
        ts_store4(y, ldy, t, i0, n, yvec != 0, gv);
      }
    }
}

template <bool BF16, int NT, typename TY>
__global__ __launch_bounds__(256) void ts_kernel(const uint8_t* codes, int P, const float* alpha, const float* mu,
                                                 int B, int bse, const uint16_t* xs, int tokens, int n, int nP,
                                                 int splits, float* part, int* cnt, const float* bias, TY* y,
                                                 long ldy, int yvec) {
  // blockIdx.x: the workgroup's 64-feature tile; blockIdx.y: its K slice
  ts_body<BF16, NT, TY, false, false>(codes, P, alpha, mu, B, bse, xs, tokens, n, nP, splits, part, cnt + blockIdx.x,
                                      bias, y, ldy, yvec, blockIdx.x * TS_F, blockIdx.y, TsPair{}, nullptr, 0, 0);
}

// ---- The grouped variant: 1 .. 4 layers that read the same x in one gather and one GEMM launch.
// The members' device pointers travel by value in the kernel arguments (TdGroup's way,
// ternary_decode.hip); entries past the call's count repeat the last tile_end and own no workgroup.
struct TsGroup {
  const uint8_t* codes[PT2Q_DECODE_GROUP_MAX];
  const float* alpha[PT2Q_DECODE_GROUP_MAX];
  const float* mu[PT2Q_DECODE_GROUP_MAX];
  const float* bias[PT2Q_DECODE_GROUP_MAX];
  void* y[PT2Q_DECODE_GROUP_MAX];
  long ldy[PT2Q_DECODE_GROUP_MAX];
  float* part[PT2Q_DECODE_GROUP_MAX];  // the member's partial tiles
  int n[PT2Q_DECODE_GROUP_MAX];
  int B[PT2Q_DECODE_GROUP_MAX];
  int splits[PT2Q_DECODE_GROUP_MAX];    // ts_plan's for the member alone
  int yvec[PT2Q_DECODE_GROUP_MAX];
  int tile_end[PT2Q_DECODE_GROUP_MAX];  // member z owns blockIdx.x in [tile_end[z - 1], tile_end[z])
};
struct TsGatherGroup {
  const int* g[PT2Q_DECODE_GROUP_MAX];
};

// x_sel[z][t][p] = x[t][g_z[p]] for member z = blockIdx.y (every linear has its own order of the
// columns, so the members cannot share one x_sel); the call's ncnt ticket counters to 0
__global__ void ts_gather_group_kernel(const uint16_t* x, long ldx, int tokens, TsGatherGroup G, int P, uint16_t* xs,
                                       long xs_stride, int* cnt, int ncnt) {
  const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.y == 0)
    for (long c = q; c < ncnt; c += (long)gridDim.x * blockDim.x) cnt[c] = 0;
  if (q >= (long)tokens * P) return;
  const int t = (int)(q / P), p = (int)(q % P);
  const int c = td_pick(G.g, (int)blockIdx.y)[p];
  xs[blockIdx.y * xs_stride + q] = (c >= 0) ? x[(long)t * ldx + c] : (uint16_t)0;
}

// The grouped gather with contract RMSNORM16 in front of it, for
// pt2q_ternary_skinny_fused with a norm weight: x_sel[z][t][p] = rmsnorm(x)[t][g_z[p]], the bits
// pt2q_rmsnorm would have written, and x itself is never written.  One workgroup of 512 threads serves
// token t = blockIdx.x for the members z = blockIdx.y, blockIdx.y + gridDim.y, ...:
//   1. thread j runs the fmaf chain of squares over the elements i ≡ j (mod 512), ascending from +0
//      (partial j of RMSNORM16), keeping its first TD_NORM_PREFETCH elements of x and of the weight in
//      registers (16-bit loads: x has any 2-byte-aligned base and any ldx); bfly64 per wave, the eight
//      wave sums through the head of the LDS image, td_norm_r in every thread;
//   2. every thread writes td_normed of the elements it read into the 2 m-byte LDS image of the
//      normalised row (elements past its registers are read again, from the cache);
//   3. after one barrier the workgroup gathers from LDS, eight consecutive positions per thread:
//      two 16-byte loads of g (the first pair issued before step 1), eight 16-bit LDS reads (padding
//      positions g < 0 give 0), one 16-byte store into x_sel[z][t][.].
// The launcher's grid is tokens x count: the norm is computed once per member, because at 2 tokens
// the launch is bound by its latency chain and not by its arithmetic.  The alternative, tokens x 1
// with every workgroup looping over the members (make EXTRA_HIPFLAGS=-DPT2Q_TS_NORM_LOOP=1), was timed
// against it: profiles/ternary_skinny_block_timing.txt.  The image caps the prologue at m <= 32768.
#ifndef PT2Q_TS_NORM_LOOP
#define PT2Q_TS_NORM_LOOP 0
#endif
constexpr int TS_NG_THREADS = TD_NORM_SUMS * 64;
constexpr int TS_NG_MAX_M = 32768;  // 64 KiB of dynamic LDS

template <bool BF16>
__global__ __launch_bounds__(TS_NG_THREADS) void ts_norm_gather_kernel(const uint16_t* x, long ldx, int m,
                                                                       const uint16_t* nw, float eps, TsGatherGroup G,
                                                                       int count, int P, uint16_t* xs, long xs_stride,
                                                                       int* cnt, int ncnt) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ts_img[];
  const int tid = threadIdx.x, t = blockIdx.x;
  if (blockIdx.y == 0)
    for (int c = t * TS_NG_THREADS + tid; c < ncnt; c += gridDim.x * TS_NG_THREADS) cnt[c] = 0;
  const uint16_t* xr = x + (long)t * ldx;
  uint32_t xc[TD_NORM_PREFETCH], wc[TD_NORM_PREFETCH];
#pragma unroll
  for (int j = 0; j < TD_NORM_PREFETCH; ++j) {
    const int i = tid + j * TS_NG_THREADS;
    xc[j] = i < m ? xr[i] : 0u;
    wc[j] = i < m ? nw[i] : 0u;
  }
  auto load_gi = [&](const int* g, int o, int (&gi)[8]) {  // g[8 o .. 8 o + 7], nothing past P
    if (o >= P / 8) return;
    if (((uintptr_t)g & 15) == 0) {
      const int4 g0 = *(const int4*)(g + 8 * o), g1 = *(const int4*)(g + 8 * o + 4);
      gi[0] = g0.x, gi[1] = g0.y, gi[2] = g0.z, gi[3] = g0.w;
      gi[4] = g1.x, gi[5] = g1.y, gi[6] = g1.z, gi[7] = g1.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) gi[j] = g[8 * o + j];
    }
  };
  int gn[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  load_gi(td_pick(G.g, (int)blockIdx.y), tid, gn);
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < TD_NORM_PREFETCH; ++j) {
    if (tid + j * TS_NG_THREADS < m) {
      const float xf = td_lo<BF16>(xc[j]);
      acc = fmaf(xf, xf, acc);
    }
  }
  for (int i = tid + TD_NORM_PREFETCH * TS_NG_THREADS; i < m; i += TS_NG_THREADS) {
    const float xf = td_lo<BF16>(xr[i]);
    acc = fmaf(xf, xf, acc);
  }
  acc = bfly64(acc);
  if ((tid & 63) == 0) ((float*)ts_img)[tid >> 6] = acc;
  __syncthreads();
  const float r = td_norm_r((const float*)ts_img, m, eps);
  __syncthreads();  // every thread has the sums: the image may take their place
  uint16_t* img = (uint16_t*)ts_img;
#pragma unroll
  for (int j = 0; j < TD_NORM_PREFETCH; ++j) {
    const int i = tid + j * TS_NG_THREADS;
    if (i < m) img[i] = td_normed<BF16>(xc[j], wc[j], r);
  }
  for (int i = tid + TD_NORM_PREFETCH * TS_NG_THREADS; i < m; i += TS_NG_THREADS) img[i] = td_normed<BF16>(xr[i], nw[i], r);
  __syncthreads();
  for (int z = blockIdx.y; z < count; z += gridDim.y) {
    const int* g = td_pick(G.g, z);
    if (z != (int)blockIdx.y) load_gi(g, tid, gn);
    uint16_t* dst = xs + z * xs_stride + (long)t * P;
    for (int o = tid; o < P / 8; o += TS_NG_THREADS) {  // positions 8 o .. 8 o + 7
      int gi[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) gi[j] = gn[j];
      load_gi(g, o + TS_NG_THREADS, gn);
      uint32_t e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = gi[j] >= 0 ? (uint32_t)img[gi[j]] : 0u;
      u32x4 v;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) v[jj] = e[2 * jj] | (e[2 * jj + 1] << 16);
      *(u32x4*)(dst + 8 * o) = v;
    }
  }
}

// blockIdx.x walks the members' 64-feature tiles one member after the other, blockIdx.y is the K
// slice.  Member z runs with the split count it has alone, so its workgroups compute the lone
// kernel's partial tiles bit for bit; workgroups of a slice its member does not have leave at once.
//   PLAIN   one counter per (member, tile): ts_body as the lone kernel runs it.
//   SWIGLU  gate tile i and up tile i share counter i, target splits_gate + splits_up, and both
//           members always write partials; the workgroup that draws the last ticket sums both
//           members' slices in slice order, rounds g and u as the lone calls store them and writes
//           h by contract SWIGLU16 (td_swiglu).  Nobody waits: the same hand-off as PLAIN.
// TsRes (pt2q_ternary_skinny_fused): the members' residuals, a by-value argument of the kernel that
// takes one (ts_group_res_kernel).  ts_group_kernel does not carry it: its arguments and its code are
// what they were.
struct TsRes {
  const uint16_t* res[PT2Q_DECODE_GROUP_MAX];  // RESADD16: per member, NULL for none
  long ldr[PT2Q_DECODE_GROUP_MAX];
  int rvec[PT2Q_DECODE_GROUP_MAX];
};
template <bool BF16, int NT, typename TY, bool SWIGLU, bool RES>
PT2Q_DEV void ts_group_body(int P, int bse, const uint16_t* xs, long xs_stride, int tokens, int* cnt, const TsGroup& G,
                            const TsRes& R) {
  int z = 0, t0 = 0;
#pragma unroll
  for (int j = 0; j < PT2Q_DECODE_GROUP_MAX - 1; ++j) {
    if ((int)blockIdx.x >= G.tile_end[j]) {
      z = j + 1;
      t0 = G.tile_end[j];
    }
  }
  const int splits = td_pick(G.splits, z);
  if ((int)blockIdx.y >= splits) return;
  const int bx = blockIdx.x - t0;  // the member's tile
  const int nP = (td_pick(G.tile_end, z) - t0) * TS_F;
  const int zy = SWIGLU ? 0 : z;  // whose y the workgroup may write
  const uint16_t* res = nullptr;
  long ldr = 0;
  int rvec = 0;
  if constexpr (RES) res = td_pick(R.res, z), ldr = td_pick(R.ldr, z), rvec = td_pick(R.rvec, z);
  ts_body<BF16, NT, TY, SWIGLU, RES>(
      td_pick(G.codes, z), P, td_pick(G.alpha, z), td_pick(G.mu, z), td_pick(G.B, z), bse, xs + z * xs_stride, tokens,
      td_pick(G.n, z), nP, splits, td_pick(G.part, z), cnt + (SWIGLU ? bx : (int)blockIdx.x), td_pick(G.bias, z),
      (TY*)td_pick(G.y, zy), td_pick(G.ldy, zy), td_pick(G.yvec, zy), bx * TS_F, blockIdx.y,
      TsPair{{G.part[0], G.part[1]}, {G.bias[0], G.bias[1]}, {G.splits[0], G.splits[1]}}, res, ldr, rvec);
}
template <bool BF16, int NT, typename TY, bool SWIGLU>
__global__ __launch_bounds__(256) void ts_group_kernel(int P, int bse, const uint16_t* xs, long xs_stride, int tokens,
                                                       int* cnt, TsGroup G) {
  ts_group_body<BF16, NT, TY, SWIGLU, false>(P, bse, xs, xs_stride, tokens, cnt, G, TsRes{});
}
// PLAIN with contract RESADD16 at the members' stores (16-bit y)
template <bool BF16, int NT, typename TY>
__global__ __launch_bounds__(256) void ts_group_res_kernel(int P, int bse, const uint16_t* xs, long xs_stride,
                                                           int tokens, int* cnt, TsGroup G, TsRes R) {
  ts_group_body<BF16, NT, TY, false, true>(P, bse, xs, xs_stride, tokens, cnt, G, R);
}

// Launch plan shared by the workspace query and the launcher (rule and reasons: header comment)
struct TsPlan {
  int P, tiles, splits, NT;
  size_t xs_bytes, cnt_bytes, part_bytes;
};
TsPlan ts_plan(int tokens, int n, int m) {
  TsPlan p;
  p.P = (int)pt2q_ternary_linear_positions(m);
  p.tiles = ceil_div(n, TS_F);
  const int nkb = p.P / TS_PB;
  int cap = nkb / 2 < 16 ? nkb / 2 : 16;
  if (cap < 1) cap = 1;
  const int want = ceil_div(TS_WGS, p.tiles);
  p.splits = want < cap ? want : cap;
  p.NT = ceil_div(tokens, 16);
  p.xs_bytes = ((size_t)tokens * p.P * 2 + 255) / 256 * 256;
  p.cnt_bytes = ((size_t)p.tiles * 4 + 255) / 256 * 256;
  p.part_bytes = p.splits > 1 ? (size_t)p.splits * tokens * p.tiles * TS_F * 4 : 0;
  return p;
}

template <bool BF16, typename TY>
void ts_launch(const TsPlan& pl, hipStream_t st, const uint8_t* codes, const float* alpha, const float* mu, int B,
               int bse, const uint16_t* xs, int tokens, int n, float* part, int* cnt, const float* bias, TY* y,
               long ldy) {
  const int yvec = ((uintptr_t)y % (4 * sizeof(TY)) == 0 && ldy % 4 == 0) ? 1 : 0;
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(pl.tiles, pl.splits), dim3(256), 0, st, codes, pl.P, alpha, mu, B, bse, xs, tokens,
                       n, pl.tiles * TS_F, pl.splits, part, cnt, bias, y, ldy, yvec);
  };
  switch (pl.NT) {
    case 1: go(ts_kernel<BF16, 1, TY>); break;
    case 2: go(ts_kernel<BF16, 2, TY>); break;
    case 3: go(ts_kernel<BF16, 3, TY>); break;
    default: go(ts_kernel<BF16, 4, TY>); break;
  }
}

// The grouped call's plan, shared by its workspace query and its launcher: every member's own
// ts_plan, and the workspace as count x_sel images, the counters (PLAIN: one per tile of every
// member; SWIGLU: one per tile of the gate), then the members' partial tiles (SWIGLU: always).
struct TsGroupPlan {
  TsPlan mem[PT2Q_DECODE_GROUP_MAX];
  bool swiglu;
  int tiles, max_splits, ncnt;
  size_t cnt_bytes, part_off[PT2Q_DECODE_GROUP_MAX], total;
};
// false for a call the entry refuses (and the query answers with 0)
bool ts_group_plan(int tokens, int m, int count, const int* n, int epilogue, TsGroupPlan& g) {
  if (tokens <= 0 || tokens > TS_MAX_TOKENS || m <= 0 || !n || count < 1 || count > PT2Q_DECODE_GROUP_MAX) return false;
  g.swiglu = epilogue == PT2Q_DECODE_SWIGLU;
  if (!g.swiglu && epilogue != PT2Q_DECODE_PLAIN) return false;
  if (g.swiglu && (count != 2 || n[0] != n[1])) return false;
  g.tiles = 0, g.max_splits = 1;
  size_t parts = 0;
  for (int z = 0; z < count; ++z) {
    if (n[z] <= 0) return false;
    TsPlan& p = g.mem[z] = ts_plan(tokens, n[z], m);
    if (g.swiglu) p.part_bytes = (size_t)p.splits * tokens * p.tiles * TS_F * 4;
    if (p.part_bytes >= ((size_t)1 << 31)) return false;  // the kernels' 32-bit byte offsets
    g.part_off[z] = parts;
    parts += p.part_bytes;
    g.tiles += p.tiles;
    if (p.splits > g.max_splits) g.max_splits = p.splits;
  }
  g.ncnt = g.swiglu ? g.mem[0].tiles : g.tiles;
  g.cnt_bytes = ((size_t)g.ncnt * 4 + 255) / 256 * 256;
  g.total = (size_t)count * g.mem[0].xs_bytes + g.cnt_bytes + parts + 256;
  return true;
}

template <bool BF16, typename TY, bool SWIGLU>
void ts_group_launch(const TsGroupPlan& g, hipStream_t st, int bse, const uint16_t* xs, int tokens, int* cnt,
                     const TsGroup& G) {
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(g.tiles, g.max_splits), dim3(256), 0, st, g.mem[0].P, bse, xs,
                       (long)(g.mem[0].xs_bytes / 2), tokens, cnt, G);
  };
  switch (g.mem[0].NT) {
    case 1: go(ts_group_kernel<BF16, 1, TY, SWIGLU>); break;
    case 2: go(ts_group_kernel<BF16, 2, TY, SWIGLU>); break;
    case 3: go(ts_group_kernel<BF16, 3, TY, SWIGLU>); break;
    default: go(ts_group_kernel<BF16, 4, TY, SWIGLU>); break;
  }
}

// the same grid for PLAIN with residuals
template <bool BF16, typename TY>
void ts_group_res_launch(const TsGroupPlan& g, hipStream_t st, int bse, const uint16_t* xs, int tokens, int* cnt,
                         const TsGroup& G, const TsRes& R) {
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(g.tiles, g.max_splits), dim3(256), 0, st, g.mem[0].P, bse, xs,
                       (long)(g.mem[0].xs_bytes / 2), tokens, cnt, G, R);
  };
  switch (g.mem[0].NT) {
    case 1: go(ts_group_res_kernel<BF16, 1, TY>); break;
    case 2: go(ts_group_res_kernel<BF16, 2, TY>); break;
    case 3: go(ts_group_res_kernel<BF16, 3, TY>); break;
    default: go(ts_group_res_kernel<BF16, 4, TY>); break;
  }
}

// pt2q_ternary_skinny_group and pt2q_ternary_skinny_fused (norm_weight and residual NULL from the
// former): every check, then the gather launch and the GEMM launch.
int ts_group_call(const void* x, int xdtype, int tokens, int64_t ldx, int m, int count, const int* n,
                  const uint8_t* const* codes, const int* const* gather, const float* const* alpha,
                  const float* const* mu, const int* B, int bs, const float* const* bias, void* const* y, int ydtype,
                  const int64_t* ldy, int epilogue, const void* norm_weight, float norm_eps,
                  const void* const* residual, const int64_t* ldr, void* workspace, size_t workspace_bytes,
                  void* stream) {
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
  if (norm_weight && !(norm_eps >= 0.0f && norm_eps <= FLT_MAX)) return PT2Q_E_ARG;  // finite, not NaN
  bool anyres = false;
  for (int z = 0; residual && z < nout; ++z) {
    if (!residual[z]) continue;
    if (swiglu || ydtype == PT2Q_F32 || !ldr || ldr[z] < n[z]) return PT2Q_E_ARG;  // RESADD16 is 16-bit, and h has no residual
    anyres = true;
  }
  if (xdtype != PT2Q_F16 && xdtype != PT2Q_BF16) return PT2Q_E_UNSUPPORTED;
  if (ydtype != xdtype && ydtype != PT2Q_F32) return PT2Q_E_ARG;
  if (tokens > TS_MAX_TOKENS) return PT2Q_E_UNSUPPORTED;
  if (bs < m && bs % 16 != 0) return PT2Q_E_UNSUPPORTED;  // alpha constant within a 16-group
  for (int z = 0; z < count; ++z)
    if ((long)ceil_div(m, bs < m ? bs : m) > B[z]) return PT2Q_E_ARG;
  for (int z = 0; z < count; ++z)
    if ((uintptr_t)codes[z] % 8 != 0) return PT2Q_E_UNSUPPORTED;
  if (!workspace || (uintptr_t)workspace % 256 != 0) return PT2Q_E_UNSUPPORTED;
  if (norm_weight && m > TS_NG_MAX_M) return PT2Q_E_UNSUPPORTED;  // the normalised row's LDS image
  TsGroupPlan g;
  if (!ts_group_plan(tokens, m, count, n, epilogue, g)) return PT2Q_E_UNSUPPORTED;
  if (workspace_bytes < g.total) return PT2Q_E_WORKSPACE;
  const int P = g.mem[0].P;
  const int bse = bs < m ? bs : P;  // per-channel: one scale for every position
  uint16_t* xs = (uint16_t*)workspace;
  int* cnt = (int*)((char*)workspace + (size_t)count * g.mem[0].xs_bytes);
  char* parts = (char*)cnt + g.cnt_bytes;
  const size_t ysize = ydtype == PT2Q_F32 ? 4 : 2;
  TsGroup G{};
  TsGatherGroup GG{};
  TsRes R{};
  int tile_end = 0;
  for (int z = 0; z < PT2Q_DECODE_GROUP_MAX; ++z) {
    const int s = z < count ? z : 0;  // entries past count repeat member 0 and own no workgroup
    if (z < count) tile_end += g.mem[z].tiles;
    G.codes[z] = codes[s], G.alpha[z] = alpha[s], G.mu[z] = mu[s], G.bias[z] = bias ? bias[s] : nullptr;
    G.n[z] = n[s], G.B[z] = B[s], G.splits[z] = g.mem[s].splits, G.tile_end[z] = tile_end;
    G.part[z] = (float*)(parts + g.part_off[s]);
    G.y[z] = s < nout ? y[s] : nullptr, G.ldy[z] = s < nout ? (long)ldy[s] : 0;
    G.yvec[z] = (s < nout && (uintptr_t)y[s] % (4 * ysize) == 0 && ldy[s] % 4 == 0) ? 1 : 0;
    GG.g[z] = gather[s];
    const bool r = anyres && s < nout && residual[s];
    R.res[z] = r ? (const uint16_t*)residual[s] : nullptr, R.ldr[z] = r ? (long)ldr[s] : 0;
    R.rvec[z] = (r && (uintptr_t)residual[s] % 8 == 0 && ldr[s] % 4 == 0) ? 1 : 0;
  }
  const bool bf16 = xdtype == PT2Q_BF16;
  const long xs_stride = (long)(g.mem[0].xs_bytes / 2);
  if (norm_weight) {
    const dim3 grid(tokens, PT2Q_TS_NORM_LOOP ? 1 : count);
    const size_t lds = ((size_t)m * 2 + 15) / 16 * 16 < 32 ? 32 : ((size_t)m * 2 + 15) / 16 * 16;  // the sums, then the image
    if (bf16)
      hipLaunchKernelGGL(ts_norm_gather_kernel<true>, grid, dim3(TS_NG_THREADS), lds, st, (const uint16_t*)x, (long)ldx,
                         m, (const uint16_t*)norm_weight, norm_eps, GG, count, P, xs, xs_stride, cnt, g.ncnt);
    else
      hipLaunchKernelGGL(ts_norm_gather_kernel<false>, grid, dim3(TS_NG_THREADS), lds, st, (const uint16_t*)x, (long)ldx,
                         m, (const uint16_t*)norm_weight, norm_eps, GG, count, P, xs, xs_stride, cnt, g.ncnt);
  } else {
    hipLaunchKernelGGL(ts_gather_group_kernel, dim3(ceil_div((long)tokens * P, 256), count), dim3(256), 0, st,
                       (const uint16_t*)x, (long)ldx, tokens, GG, P, xs, xs_stride, cnt, g.ncnt);
  }
  PT2Q_LAUNCH_CHECK();
  if (swiglu) {
    if (bf16)
      ts_group_launch<true, __bf16, true>(g, st, bse, xs, tokens, cnt, G);
    else
      ts_group_launch<false, _Float16, true>(g, st, bse, xs, tokens, cnt, G);
  } else if (ydtype == PT2Q_F32) {
    if (bf16)
      ts_group_launch<true, float, false>(g, st, bse, xs, tokens, cnt, G);
    else
      ts_group_launch<false, float, false>(g, st, bse, xs, tokens, cnt, G);
  } else if (anyres) {
    if (bf16)
      ts_group_res_launch<true, __bf16>(g, st, bse, xs, tokens, cnt, G, R);
    else
      ts_group_res_launch<false, _Float16>(g, st, bse, xs, tokens, cnt, G, R);
  } else if (bf16) {
    ts_group_launch<true, __bf16, false>(g, st, bse, xs, tokens, cnt, G);
  } else {
    ts_group_launch<false, _Float16, false>(g, st, bse, xs, tokens, cnt, G);
  }
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}

}  // namespace

extern "C" int pt2q_ternary_skinny_max_tokens(void) { return TS_MAX_TOKENS; }

extern "C" size_t pt2q_ternary_skinny_workspace_bytes(int tokens, int n, int m) {
  if (tokens <= 0 || tokens > TS_MAX_TOKENS || n <= 0 || m <= 0) return 0;
  const TsPlan pl = ts_plan(tokens, n, m);
  // gathered activations (tokens x P 16-bit), one counter per feature tile, the split partials
  return pl.xs_bytes + pl.cnt_bytes + pl.part_bytes + 256;
}

extern "C" int pt2q_ternary_skinny(const void* x, int xdtype, int tokens, int64_t ldx, int n, int m,
                                   const uint8_t* codes, const int* gather, const float* alpha, const float* mu,
                                   int B, int bs, const float* bias, void* y, int ydtype, int64_t ldy,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!x || !codes || !gather || !alpha || !mu || !y || tokens <= 0 || n <= 0 || m <= 0 || ldx < m || ldy < n ||
      B <= 0 || bs <= 0)
    return PT2Q_E_ARG;
  if (xdtype != PT2Q_F16 && xdtype != PT2Q_BF16) return PT2Q_E_UNSUPPORTED;
  if (ydtype != xdtype && ydtype != PT2Q_F32) return PT2Q_E_ARG;
  if (tokens > TS_MAX_TOKENS) return PT2Q_E_UNSUPPORTED;
  if (bs < m && bs % 16 != 0) return PT2Q_E_UNSUPPORTED;  // alpha constant within a 16-group
  if ((long)ceil_div(m, bs < m ? bs : m) > B) return PT2Q_E_ARG;
  // the lanes' 8-byte code loads; x_sel, counters and partials start on 256-byte boundaries, so the
  // partial rows of two feature tiles (64 floats each) never share a cache line
  if ((uintptr_t)codes % 8 != 0 || !workspace || (uintptr_t)workspace % 256 != 0) return PT2Q_E_UNSUPPORTED;
  if (workspace_bytes < pt2q_ternary_skinny_workspace_bytes(tokens, n, m)) return PT2Q_E_WORKSPACE;
  const TsPlan pl = ts_plan(tokens, n, m);
  const int bse = bs < m ? bs : pl.P;  // per-channel: one scale for every position
  uint16_t* xs = (uint16_t*)workspace;
  int* cnt = (int*)((char*)workspace + pl.xs_bytes);
  float* part = (float*)((char*)workspace + pl.xs_bytes + pl.cnt_bytes);
  hipLaunchKernelGGL(ts_gather_kernel, dim3(ceil_div((long)tokens * pl.P, 256)), dim3(256), 0, st,
                     (const uint16_t*)x, (long)ldx, tokens, gather, pl.P, xs, cnt, pl.tiles);
  PT2Q_LAUNCH_CHECK();
  if (ydtype == PT2Q_F32) {
    if (xdtype == PT2Q_BF16)
      ts_launch<true, float>(pl, st, codes, alpha, mu, B, bse, xs, tokens, n, part, cnt, bias, (float*)y, (long)ldy);
    else
      ts_launch<false, float>(pl, st, codes, alpha, mu, B, bse, xs, tokens, n, part, cnt, bias, (float*)y, (long)ldy);
  } else if (ydtype == PT2Q_BF16) {
    ts_launch<true, __bf16>(pl, st, codes, alpha, mu, B, bse, xs, tokens, n, part, cnt, bias, (__bf16*)y, (long)ldy);
  } else {
    ts_launch<false, _Float16>(pl, st, codes, alpha, mu, B, bse, xs, tokens, n, part, cnt, bias, (_Float16*)y,
                               (long)ldy);
  }
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}

extern "C" size_t pt2q_ternary_skinny_group_workspace_bytes(int tokens, int m, int count, const int* n, int epilogue) {
  TsGroupPlan g;
  return ts_group_plan(tokens, m, count, n, epilogue, g) ? g.total : 0;
}

extern "C" int pt2q_ternary_skinny_group(const void* x, int xdtype, int tokens, int64_t ldx, int m, int count,
                                         const int* n, const uint8_t* const* codes, const int* const* gather,
                                         const float* const* alpha, const float* const* mu, const int* B, int bs,
                                         const float* const* bias, void* const* y, int ydtype, const int64_t* ldy,
                                         int epilogue, void* workspace, size_t workspace_bytes, void* stream) {
  return ts_group_call(x, xdtype, tokens, ldx, m, count, n, codes, gather, alpha, mu, B, bs, bias, y, ydtype, ldy,
                       epilogue, nullptr, 0.0f, nullptr, nullptr, workspace, workspace_bytes, stream);
}

// The group entry with the RMSNorm prologue (in the gather launch) and the residual epilogue (where y
// is converted).  A call that asks for neither launches what pt2q_ternary_skinny_group launches.
extern "C" int pt2q_ternary_skinny_fused(const void* x, int xdtype, int tokens, int64_t ldx, int m, int count,
                                         const int* n, const uint8_t* const* codes, const int* const* gather,
                                         const float* const* alpha, const float* const* mu, const int* B, int bs,
                                         const float* const* bias, void* const* y, int ydtype, const int64_t* ldy,
                                         int epilogue, const void* norm_weight, float norm_eps,
                                         const void* const* residual, const int64_t* ldr, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  return ts_group_call(x, xdtype, tokens, ldx, m, count, n, codes, gather, alpha, mu, B, bs, bias, y, ydtype, ldy,
                       epilogue, norm_weight, norm_eps, residual, ldr, workspace, workspace_bytes, stream);
}
