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

// What the SWIGLU epilogue needs of the two members, gate then up (the grouped kernel's TsGroup entries)
struct TsPair {
  float* part[2];
  const float* bias[2];
  int splits[2];
};

// One workgroup's work, the body of the lone and of the grouped kernel: features fb .. fb + TS_F - 1
// of one layer (n features, partial rows of nP floats, K slice z of `splits`, ticket counter *ticket).
// SWIGLU (grouped kernel only): the layer is the gate or the up projection of `pair`, y is h.
template <bool BF16, int NT, typename TY, bool SWIGLU>
PT2Q_DEV void ts_body(const uint8_t* codes, int P, const float* alpha, const float* mu, int B, int bse,
                      const uint16_t* xs, int tokens, int n, int nP, int splits, float* part, int* ticket,
                      const float* bias, TY* y, long ldy, int yvec, int fb, int z, const TsPair& pair) {
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
  auto finish = [&](int f, int u, float (&v)[4]) {  // + bias, convert, store
    const int i0 = fb + (wv * TS_FT + f) * 16 + 4 * kq;
    if (bias) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (i0 + q < n) v[q] = v[q] + bias[i0 + q];
    }
    ts_store4(y, ldy, 16 * u + r, i0, n, yvec != 0, v);
  };
  if (!SWIGLU && splits == 1) {
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
  ts_body<BF16, NT, TY, false>(codes, P, alpha, mu, B, bse, xs, tokens, n, nP, splits, part, cnt + blockIdx.x, bias, y,
                               ldy, yvec, blockIdx.x * TS_F, blockIdx.y, TsPair{});
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

// blockIdx.x walks the members' 64-feature tiles one member after the other, blockIdx.y is the K
// slice.  Member z runs with the split count it has alone, so its workgroups compute the lone
// kernel's partial tiles bit for bit; workgroups of a slice its member does not have leave at once.
//   PLAIN   one counter per (member, tile): ts_body as the lone kernel runs it.
//   SWIGLU  gate tile i and up tile i share counter i, target splits_gate + splits_up, and both
//           members always write partials; the workgroup that draws the last ticket sums both
//           members' slices in slice order, rounds g and u as the lone calls store them and writes
//           h by contract SWIGLU16 (td_swiglu).  Nobody waits: the same hand-off as PLAIN.
template <bool BF16, int NT, typename TY, bool SWIGLU>
__global__ __launch_bounds__(256) void ts_group_kernel(int P, int bse, const uint16_t* xs, long xs_stride, int tokens,
                                                       int* cnt, TsGroup G) {
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
  ts_body<BF16, NT, TY, SWIGLU>(td_pick(G.codes, z), P, td_pick(G.alpha, z), td_pick(G.mu, z), td_pick(G.B, z), bse,
                                xs + z * xs_stride, tokens, td_pick(G.n, z), nP, splits, td_pick(G.part, z),
                                cnt + (SWIGLU ? bx : (int)blockIdx.x), td_pick(G.bias, z), (TY*)td_pick(G.y, zy),
                                td_pick(G.ldy, zy), td_pick(G.yvec, zy), bx * TS_F, blockIdx.y,
                                TsPair{{G.part[0], G.part[1]}, {G.bias[0], G.bias[1]}, {G.splits[0], G.splits[1]}});
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
  if (tokens > TS_MAX_TOKENS) return PT2Q_E_UNSUPPORTED;
  if (bs < m && bs % 16 != 0) return PT2Q_E_UNSUPPORTED;  // alpha constant within a 16-group
  for (int z = 0; z < count; ++z)
    if ((long)ceil_div(m, bs < m ? bs : m) > B[z]) return PT2Q_E_ARG;
  for (int z = 0; z < count; ++z)
    if ((uintptr_t)codes[z] % 8 != 0) return PT2Q_E_UNSUPPORTED;
  if (!workspace || (uintptr_t)workspace % 256 != 0) return PT2Q_E_UNSUPPORTED;
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
  }
  hipLaunchKernelGGL(ts_gather_group_kernel, dim3(ceil_div((long)tokens * P, 256), count), dim3(256), 0, st,
                     (const uint16_t*)x, (long)ldx, tokens, GG, P, xs, (long)(g.mem[0].xs_bytes / 2), cnt, g.ncnt);
  PT2Q_LAUNCH_CHECK();
  const bool bf16 = xdtype == PT2Q_BF16;
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
  } else if (bf16) {
    ts_group_launch<true, __bf16, false>(g, st, bse, xs, tokens, cnt, G);
  } else {
    ts_group_launch<false, _Float16, false>(g, st, bse, xs, tokens, cnt, G);
  }
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}
