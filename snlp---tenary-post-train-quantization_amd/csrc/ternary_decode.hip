// Fused decode kernel of the ternary linear layer: 1..8 tokens in ONE launch, no workspace
// (model.py:75-95; the buffers are those of pt2q_ternary_pack, csrc/ternary_linear.hip).  One
// kernel body, td_decode, with three uses: one linear (pt2q_ternary_decode, a group of one),
// up to four linears that read the same x (pt2q_ternary_decode_group PLAIN: the q/k/v projections
// of a decoder layer), and the gate and up projections of a gated MLP with the SwiGLU activation
// as epilogue (SWIGLU).  The members' pointers travel by value in the kernel's arguments
// (tl_decode_kernel: the group; tl_decode_one_kernel: the single linear's, as plain arguments).
//
// Arithmetic contract DOT64P.  A piece q = 2 kb + h is the 64 positions of one
// 16-byte load of a packed row (p = 128 kb + 16 g + 8 h + j, g then j ascending).  Lane l of the
// row's wave owns the pieces q ≡ l (mod 64) in ascending q and forms
//   acc = fmaf((float)w, (float)xs, acc)   from +0, pieces then positions in that order
// (the 16-bit x 16-bit product is exact in fp32), the 64 partials are folded by bfly64 and
// y = RN_TY(v + bias).  Nothing else -- tokens per call, token grouping, grid, rows per wave, the
// other members of a group -- enters the order, so a token's bits do not depend on its
// neighbours, and a PLAIN member's output has the bits of pt2q_ternary_decode on that member
// alone: both are this kernel.  The SWIGLU epilogue is contract SWIGLU16: g and u
// rounded as the separate calls would store them, then fp32 operations, each rounded to nearest
// even and none fused.
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
//   PLAIN   the grid's workgroups are shared out over the members in proportion to their rows
//           (wg_end); a workgroup serves one member, whose gather it follows.
//   SWIGLU  a workgroup gathers x twice, once per member, and the wave that owns row i walks
//           the items (row, round, member) with the member innermost: ring slot s holds member
//           s % 2, so the member of an item is known at compile time and both chains keep the
//           four loads in flight of the plain kernel.
//
// pt2q_ternary_decode_fused adds two switches to the same body (template parameter TdFx, arguments
// TdExtra; the plain entries' kernels carry neither and compile to what they were):
//   norm      contract RMSNORM16 on the staged rows, in place, before the gather: the
//             squares are accumulated while staging, the wave sums pass through the head of the
//             gathered image (no LDS of its own), one more barrier.  All three uses.
//   residual  contract RESADD16 at the store: y = RN_TY(f32(RN_TY(v + bias)) + f32(res)), per
//             output, res possibly y.  Single and PLAIN.
// pt2q_rmsnorm is RMSNORM16 as a kernel of its own, one workgroup per token.
#include <cfloat>

#include "common.hpp"
#include "internal.hpp"

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

struct TdMember {
  const uint8_t* codes;
  const int* gather;
  const float *alpha, *mu, *bias;
  int n, B;
};

struct TdGroup {  // the kernel's by-value argument: the members' host arrays, copied
  const uint8_t* codes[PT2Q_DECODE_GROUP_MAX];
  const int* gather[PT2Q_DECODE_GROUP_MAX];
  const float* alpha[PT2Q_DECODE_GROUP_MAX];
  const float* mu[PT2Q_DECODE_GROUP_MAX];
  const float* bias[PT2Q_DECODE_GROUP_MAX];
  void* y[PT2Q_DECODE_GROUP_MAX];
  long ldy[PT2Q_DECODE_GROUP_MAX];
  int n[PT2Q_DECODE_GROUP_MAX];
  int B[PT2Q_DECODE_GROUP_MAX];
  int wg_end[PT2Q_DECODE_GROUP_MAX];  // PLAIN: member z owns workgroups wg_end[z - 1] .. wg_end[z] - 1 of blockIdx.x
};
static_assert(PT2Q_DECODE_GROUP_MAX == 4, "td_pick and the member search name four entries");

template <int Z>
struct TdZ {
  static constexpr int value = Z;
};

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

// What pt2q_ternary_decode_fused adds to a call, as a by-value argument of the kernels that take it
// (tl_decode_fused_kernel, tl_decode_one_fused_kernel).  The kernels of the plain entries do not
// carry it: their argument blocks and their code are what they were.
struct TdExtra {
  const uint16_t* nw;  // RMSNORM16 weight, m elements of x's dtype (TD_FX_NORM)
  float eps;
  const void* res[PT2Q_DECODE_GROUP_MAX];  // RESADD16: per output, NULL for none
  long ldr[PT2Q_DECODE_GROUP_MAX];
};
// TD_FX_NONE: the plain entries.  TD_FX_RES: residual epilogue.  TD_FX_NORM: norm prologue, and the
// residual epilogue where the use has one (not SWIGLU).
enum TdFx { TD_FX_NONE, TD_FX_RES, TD_FX_NORM };

// r of contract RMSNORM16 from the eight wave sums of a row's squares: the sums
// added in order, then a division, an add, a square root and a division, each the correctly
// rounded fp32 operation (hipcc's default for / and sqrtf; no fast-math, no contraction).
PT2Q_DEV float td_norm_r(const float* sums, int m, float eps) {
  float ss = sums[0];
#pragma unroll
  for (int k = 1; k < TD_WAVES; ++k) ss = ss + sums[k];
  const float mean = ss / (float)m;
  return 1.0f / sqrtf(mean + eps);
}
// RN_TX(RN_TX(xf * r) * wf): both products fp32 values of their own (td_rounded)
template <bool BF16>
PT2Q_DEV uint16_t td_normed(uint32_t xu, uint32_t wu, float r) {
  const float xn = td_round<BF16>(td_rounded(td_lo<BF16>(xu) * r));
  return (uint16_t)td_bits<BF16>(td_rounded(xn * td_lo<BF16>(wu)));
}
constexpr int TD_NORM_PREFETCH = 16;  // weight elements a thread loads ahead of the sums' barrier: m <= 8192

// The kernel's body: all of a workgroup's work for the group G.
template <bool BF16, int TG, bool SWIGLU, TdFx FX>
PT2Q_DEV void td_decode(const uint16_t* x, long ldx, int tokens, int m, int P, int bse, int yf32, const TdGroup& G,
                        const TdExtra& X) {
  constexpr bool NORM = FX == TD_FX_NORM;
  constexpr bool RES = FX != TD_FX_NONE && !SWIGLU;
  constexpr int NZ = SWIGLU ? 2 : 1;  // members a wave computes per row
  static_assert(TD_DEPTH % NZ == 0, "ring slot s holds member s % NZ");
  extern __shared__ __attribute__((aligned(16))) uint8_t td_smem[];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int npieces = P / 64, nround = (npieces + 63) / 64;
  const int t0 = blockIdx.y * TG;
  const bool perpiece = bse % 128 == 0;  // one scale block per piece, else one per 16-position group
  const long rowbytes = P / 4;

  // the member(s) of this workgroup, its index among their workgroups and their number
  int z = 0, bx = blockIdx.x, nbx = gridDim.x;
  if constexpr (!SWIGLU) {
    int w0 = 0;
#pragma unroll
    for (int j = 0; j < PT2Q_DECODE_GROUP_MAX - 1; ++j) {
      if ((int)blockIdx.x >= G.wg_end[j]) {
        z = j + 1;
        w0 = G.wg_end[j];
      }
    }
    bx = blockIdx.x - w0;
    nbx = td_pick(G.wg_end, z) - w0;
  }
  TdMember M[NZ];
  M[0] = TdMember{td_pick(G.codes, z), td_pick(G.gather, z), td_pick(G.alpha, z), td_pick(G.mu, z),
                  td_pick(G.bias, z),  td_pick(G.n, z),      td_pick(G.B, z)};
  if constexpr (SWIGLU) M[1] = TdMember{G.codes[1], G.gather[1], G.alpha[1], G.mu[1], G.bias[1], G.n[1], G.B[1]};
  const int n = M[0].n;  // SWIGLU: both members' rows
  const int rstride = nbx * TD_WAVES;
  // gathered image of member zz: chunk ((k * TG + t) * 8 + g) * 64 + lane
  auto xs_of = [&](int zz) { return (u32x4*)td_smem + (long)zz * nround * TG * 512; };

  // codes (and, per piece, the scales; at a row's first piece its bias) of piece 64 k + lane of
  // `row` of member Z; nothing past a row's end
  auto fetch = [&](auto zc, int row, int k, TdItem& it) {
    const TdMember& mb = M[decltype(zc)::value];
    const int q = 64 * k + lane;
    it.cw = u32x4{0u, 0u, 0u, 0u};
    it.a = it.mm = it.bv = 0.0f;
    if (row < n && q < npieces) {
      it.cw = *(const u32x4*)(mb.codes + (long)row * rowbytes + 16 * q);
      if (perpiece) {
        const int blk = min((q >> 1) * 128 / bse, mb.B - 1);
        it.a = mb.alpha[(long)row * mb.B + blk];
        it.mm = mb.mu[(long)row * mb.B + blk];
      }
      if (k == 0 && mb.bias) it.bv = mb.bias[row];
    }
  };
  // the (row, round) of the item after one of member Z at (r, kk): the same until the last member
  auto step = [&](auto zc, int& r, int& kk) {
    if (decltype(zc)::value != NZ - 1) return;
    if (++kk == nround) {
      kk = 0;
      r += rstride;
    }
  };

  // the wave's first TD_DEPTH items are in flight across the gather below; from then on each
  // item's slot is refilled as soon as it has been used
  int row = bx * TD_WAVES + wv, k = 0;
  int frow = row, fk = 0;
  TdItem ring[TD_DEPTH];
  if constexpr (SWIGLU) {
    fetch(TdZ<0>{}, frow, fk, ring[0]);
    fetch(TdZ<1>{}, frow, fk, ring[1]);
    step(TdZ<1>{}, frow, fk);
    fetch(TdZ<0>{}, frow, fk, ring[2]);
    fetch(TdZ<1>{}, frow, fk, ring[3]);
    step(TdZ<1>{}, frow, fk);
  } else {
#pragma unroll
    for (int s = 0; s < TD_DEPTH; ++s) {
      fetch(TdZ<0>{}, frow, fk, ring[s]);
      step(TdZ<0>{}, frow, fk);
    }
  }

  // xs_of(zz)[t][p] = x[t0 + t][gather_zz[p]] (+0 for padding positions and tokens past the end).
  // A token's row is staged in LDS by coalesced loads and gathered from there, per member: 64
  // lanes reading 64 scattered 2-byte elements from global memory cost the L1 a cache line each,
  // per workgroup.  All TG rows are staged before one barrier, and every member's first eight
  // gather indices per thread are loaded ahead of it, so the prologue pays each global latency
  // once, not once per token.
  uint16_t* raw = (uint16_t*)(td_smem + (size_t)NZ * nround * TG * TD_ROUND_BYTES);
  const int rawstride = (m + 7) / 8 * 8;  // elements between staged rows
  auto load_gi = [&](const int* gather, int o, int (&gi)[8]) {  // gather[8 o .. 8 o + 7], nothing past P
    if (o >= P / 8) return;
    if (((uintptr_t)gather & 15) == 0) {
      const int4 g0 = *(const int4*)(gather + 8 * o), g1 = *(const int4*)(gather + 8 * o + 4);
      gi[0] = g0.x, gi[1] = g0.y, gi[2] = g0.z, gi[3] = g0.w;
      gi[4] = g1.x, gi[5] = g1.y, gi[6] = g1.z, gi[7] = g1.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) gi[j] = gather[8 * o + j];
    }
  };
  int gn[NZ][8];
#pragma unroll
  for (int zz = 0; zz < NZ; ++zz) {
#pragma unroll
    for (int j = 0; j < 8; ++j) gn[zz][j] = -1;
    load_gi(M[zz].gather, threadIdx.x, gn[zz]);
  }
  // NORM (RMSNORM16): thread j's chain of squares over the elements it stages is partial j; the
  // eight wave sums per token go to the head of the gathered image, which nothing has written yet,
  // and after the barrier every thread normalises the elements it staged, in place.  The weight
  // is loaded coalesced, its first TD_NORM_PREFETCH elements per thread ahead of that barrier.
  uint32_t wpre[NORM ? TD_NORM_PREFETCH : 1];
  if constexpr (NORM) {
#pragma unroll
    for (int j = 0; j < TD_NORM_PREFETCH; ++j) {
      const int i = threadIdx.x + j * TD_THREADS;
      wpre[j] = i < m ? X.nw[i] : 0u;
    }
  }
  float ssq[TG];
#pragma unroll
  for (int t = 0; t < TG; ++t) {
    ssq[t] = 0.0f;
    if (t0 + t < tokens) {
      const uint16_t* xr = x + (long)(t0 + t) * ldx;
      for (int i = threadIdx.x; i < m; i += TD_THREADS) {
        const uint16_t u = xr[i];
        raw[t * rawstride + i] = u;
        if constexpr (NORM) {
          const float xf = td_lo<BF16>(u);
          ssq[t] = fmaf(xf, xf, ssq[t]);
        }
      }
    }
  }
  if constexpr (NORM) {
    float* sums = (float*)td_smem;  // [token][wave]
#pragma unroll
    for (int t = 0; t < TG; ++t) {
      const float s = bfly64(ssq[t]);
      if (lane == 0) sums[t * TD_WAVES + wv] = s;
    }
  }
  __syncthreads();
  if constexpr (NORM) {
    const float* sums = (const float*)td_smem;
    float r[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) r[t] = td_norm_r(sums + t * TD_WAVES, m, X.eps);
#pragma unroll
    for (int j = 0; j < TD_NORM_PREFETCH; ++j) {
      const int i = threadIdx.x + j * TD_THREADS;
      if (i < m) {
#pragma unroll
        for (int t = 0; t < TG; ++t) {
          if (t0 + t < tokens) raw[t * rawstride + i] = td_normed<BF16>(raw[t * rawstride + i], wpre[j], r[t]);
        }
      }
    }
    for (int i = threadIdx.x + TD_NORM_PREFETCH * TD_THREADS; i < m; i += TD_THREADS) {
      const uint32_t wu = X.nw[i];
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        if (t0 + t < tokens) raw[t * rawstride + i] = td_normed<BF16>(raw[t * rawstride + i], wu, r[t]);
      }
    }
    __syncthreads();  // the sums are read, the rows normalised: the gather may overwrite the one and read the other
  }
#pragma unroll
  for (int zz = 0; zz < NZ; ++zz) {
    u32x4* xs = xs_of(zz);
    for (int o = threadIdx.x; o < P / 8; o += TD_THREADS) {  // positions 8 o .. 8 o + 7
      const int q = 2 * (o >> 4) + (o & 1), g = (o >> 1) & 7;
      int gi[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) gi[j] = gn[zz][j];
      load_gi(M[zz].gather, o + TD_THREADS, gn[zz]);
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
  }
  __syncthreads();

  float acc[NZ][TG], bv[NZ];
#pragma unroll
  for (int zz = 0; zz < NZ; ++zz) {
    bv[zz] = 0.0f;
#pragma unroll
    for (int t = 0; t < TG; ++t) acc[zz][t] = 0.0f;
  }
  // v + bias of member zz, before its one rounding
  auto biased = [&](int zz, int t) {
    float v = bfly64(acc[zz][t]);
    if (M[zz].bias) v = v + bv[zz];
    acc[zz][t] = 0.0f;
    return v;
  };
  // one item (row, round, member Z) out of its ring slot, the slot refilled at once; false past
  // the last row
  auto item = [&](auto zc, TdItem& slot) __attribute__((always_inline)) -> bool {
    constexpr int Z = decltype(zc)::value;
    if (row >= n) return false;
    const TdItem it = slot;
    fetch(zc, frow, fk, slot);
    step(zc, frow, fk);
    if (k == 0) bv[Z] = it.bv;
    const bool last = Z == NZ - 1 && k == nround - 1;  // the row's last item: fold and store
    // RESADD16: the residual of the elements this lane will store, asked for ahead of the piece
    const uint16_t* res = nullptr;
    float resv[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) resv[t] = 0.0f;
    if constexpr (RES) {
      res = (const uint16_t*)td_pick(X.res, z);
      if (last && res && lane == 0) {
#pragma unroll
        for (int t = 0; t < TG; ++t) {
          if (t0 + t < tokens) resv[t] = td_lo<BF16>(res[(long)(t0 + t) * td_pick(X.ldr, z) + row]);
        }
      }
    }
    const int q = 64 * k + lane;
    if (q < npieces) {
      td_piece<BF16, TG>(xs_of(Z) + (long)k * TG * 512 + lane, it, perpiece, q, bse, M[Z].B,
                         M[Z].alpha + (long)row * M[Z].B, M[Z].mu + (long)row * M[Z].B, acc[Z]);
    }
    const int r0 = row;
    step(zc, row, k);
    if (last) {
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        const long o = (long)(t0 + t) * td_pick(G.ldy, z) + r0;
        const bool st = lane == 0 && t0 + t < tokens;
        if constexpr (SWIGLU) {
          const float g = td_round<BF16>(biased(0, t)), u = td_round<BF16>(biased(1, t));
          const float s = td_round<BF16>(td_rounded(g * td_sigmoid(g)));
          const float h = td_rounded(s * u);
          if (st) {
            if constexpr (BF16)
              ((__bf16*)G.y[0])[o] = (__bf16)h;
            else
              ((_Float16*)G.y[0])[o] = (_Float16)h;
          }
        } else {
          float v = biased(0, t);
          void* y = td_pick(G.y, z);
          if (st) {
            if constexpr (RES) {  // the lane that stores an element is the one that read it: res may be y
              if (res) v = td_rounded(td_round<BF16>(v) + resv[t]);
            }
            if (yf32)
              ((float*)y)[o] = v;
            else if constexpr (BF16)
              ((__bf16*)y)[o] = (__bf16)v;
            else
              ((_Float16*)y)[o] = (_Float16)v;
          }
        }
      }
    }
    return true;
  };
  static_assert(TD_DEPTH == 4, "the ring is walked by four explicit calls");
  while (item(TdZ<0>{}, ring[0]) && item(TdZ<NZ - 1>{}, ring[1]) && item(TdZ<0>{}, ring[2]) &&
         item(TdZ<NZ - 1>{}, ring[3])) {
  }
}

template <bool BF16, int TG, bool SWIGLU>
__global__ __launch_bounds__(TD_THREADS, 4) void tl_decode_kernel(const uint16_t* x, long ldx, int tokens, int m, int P,
                                                                  int bse, int yf32, TdGroup G) {
  td_decode<BF16, TG, SWIGLU, TD_FX_NONE>(x, ldx, tokens, m, P, bse, yf32, G, TdExtra{});
}

// The group with the norm prologue and / or the residual epilogue (pt2q_ternary_decode_fused).
template <bool BF16, int TG, bool SWIGLU, TdFx FX>
__global__ __launch_bounds__(TD_THREADS, 4) void tl_decode_fused_kernel(const uint16_t* x, long ldx, int tokens, int m,
                                                                        int P, int bse, int yf32, TdGroup G, TdExtra X) {
  td_decode<BF16, TG, SWIGLU, FX>(x, ldx, tokens, m, P, bse, yf32, G, X);
}

// The same body for a PLAIN group of one whose member arrives as plain arguments.  Through
// tl_decode_kernel a wave reads wg_end, then the member's pointers at the offsets that gives,
// then its codes: three dependent trips to a kernarg segment nobody has touched yet.  That way a
// 1-token call of 6-15 us measured 0.6-0.8 us slower (profiles/ternary_decode_unify_ab.txt; the
// chain is read off the assembly, not timed apart).  Here every entry of the group is the one
// member, so the picks fold away and the pointers come with the first kernarg load.
template <bool BF16, int TG, TdFx FX>
PT2Q_DEV void td_decode_one(const uint16_t* x, long ldx, int tokens, int m, int P, int bse, int yf32, const TdMember& M,
                            void* y, long ldy, const uint16_t* nw, float eps, const void* res, long ldr) {
  TdGroup G;
  TdExtra X;
  X.nw = nw, X.eps = eps;
#pragma unroll
  for (int z = 0; z < PT2Q_DECODE_GROUP_MAX; ++z) {
    G.codes[z] = M.codes, G.gather[z] = M.gather, G.alpha[z] = M.alpha, G.mu[z] = M.mu, G.bias[z] = M.bias;
    G.y[z] = y, G.ldy[z] = ldy, G.n[z] = M.n, G.B[z] = M.B;
    G.wg_end[z] = gridDim.x;
    X.res[z] = res, X.ldr[z] = ldr;
  }
  td_decode<BF16, TG, false, FX>(x, ldx, tokens, m, P, bse, yf32, G, X);
}
template <bool BF16, int TG>
__global__ __launch_bounds__(TD_THREADS, 4) void tl_decode_one_kernel(const uint16_t* x, long ldx, int tokens, int m,
                                                                      int P, int bse, int yf32, TdMember M, void* y,
                                                                      long ldy) {
  td_decode_one<BF16, TG, TD_FX_NONE>(x, ldx, tokens, m, P, bse, yf32, M, y, ldy, nullptr, 0.0f, nullptr, 0);
}
// the single linear of pt2q_ternary_decode_fused: the extras as plain arguments too
template <bool BF16, int TG, TdFx FX>
__global__ __launch_bounds__(TD_THREADS, 4) void tl_decode_one_fused_kernel(const uint16_t* x, long ldx, int tokens,
                                                                            int m, int P, int bse, int yf32, TdMember M,
                                                                            void* y, long ldy, const uint16_t* nw,
                                                                            float eps, const void* res, long ldr) {
  td_decode_one<BF16, TG, FX>(x, ldx, tokens, m, P, bse, yf32, M, y, ldy, nw, eps, res, ldr);
}

// RMSNORM16 from x to y, one workgroup per token: thread j's chain is partial j, so the order is the
// prologue's by construction.  A thread keeps its first TD_NORM_PREFETCH elements in registers and
// reads the others again; it writes only elements it read itself, so y may be x.
template <bool BF16>
__global__ __launch_bounds__(TD_THREADS) void tl_rmsnorm_kernel(const uint16_t* x, long ldx, int m, const uint16_t* w,
                                                                float eps, uint16_t* y, long ldy) {
  __shared__ float sums[TD_WAVES];
  const uint16_t* xr = x + (long)blockIdx.x * ldx;
  uint16_t* yr = y + (long)blockIdx.x * ldy;
  uint32_t xc[TD_NORM_PREFETCH], wc[TD_NORM_PREFETCH];
#pragma unroll
  for (int j = 0; j < TD_NORM_PREFETCH; ++j) {
    const int i = threadIdx.x + j * TD_THREADS;
    xc[j] = i < m ? xr[i] : 0u;
    wc[j] = i < m ? w[i] : 0u;
  }
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < TD_NORM_PREFETCH; ++j) {
    if ((int)threadIdx.x + j * TD_THREADS < m) {
      const float xf = td_lo<BF16>(xc[j]);
      acc = fmaf(xf, xf, acc);
    }
  }
  for (int i = threadIdx.x + TD_NORM_PREFETCH * TD_THREADS; i < m; i += TD_THREADS) {
    const float xf = td_lo<BF16>(xr[i]);
    acc = fmaf(xf, xf, acc);
  }
  acc = bfly64(acc);
  if ((threadIdx.x & 63) == 0) sums[threadIdx.x >> 6] = acc;
  __syncthreads();
  const float r = td_norm_r(sums, m, eps);
#pragma unroll
  for (int j = 0; j < TD_NORM_PREFETCH; ++j) {
    const int i = threadIdx.x + j * TD_THREADS;
    if (i < m) yr[i] = td_normed<BF16>(xc[j], wc[j], r);
  }
  for (int i = threadIdx.x + TD_NORM_PREFETCH * TD_THREADS; i < m; i += TD_THREADS) yr[i] = td_normed<BF16>(xr[i], w[i], r);
}

int td_cus() {
  static const int cus = [] {
    int dev = 0, c = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev);
    return c > 0 ? c : 256;
  }();
  return cus;
}

struct TdPlan {  // what a valid call launches
  int P, bse, nround;
  int TG, groups, wgs;  // tokens per workgroup; the grid is wgs x groups
  size_t lds;
  bool bf16, swiglu, yf32;
  TdGroup G;  // the members and, PLAIN, the wg_end table
  TdFx fx;    // what the call asks beyond the plain entries, and the arguments of that
  TdExtra X;
};

// The argument rules of all three entries (include/pt2q.h) and, for a call that passes them, its
// plan.  The member arrays hold `count` entries (y, ldy, residual, ldr: one per output the call
// writes).  norm_weight and residual are NULL from the plain entries.
int td_plan(const void* x, int xdtype, int tokens, int64_t ldx, int m, int count, const int* n,
            const uint8_t* const* codes, const int* const* gather, const float* const* alpha, const float* const* mu,
            const int* B, int bs, const float* const* bias, void* const* y, int ydtype, const int64_t* ldy,
            int epilogue, const void* norm_weight, float norm_eps, const void* const* residual, const int64_t* ldr,
            TdPlan& p) {
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
  if (bs < m && bs % 16 != 0) return PT2Q_E_UNSUPPORTED;  // alpha constant within a 16-group
  for (int z = 0; z < count; ++z)
    if ((long)ceil_div(m, bs < m ? bs : m) > B[z]) return PT2Q_E_ARG;
  if (tokens > TD_MAX_TOKENS) return PT2Q_E_UNSUPPORTED;
  p.P = (int)pt2q_ternary_linear_positions(m);
  p.bse = bs < m ? bs : p.P;  // per-channel: one scale for every position
  p.nround = ceil_div(p.P / 64, 64);
  if (p.nround > TD_MAX_ROUNDS) return PT2Q_E_UNSUPPORTED;  // one token's activations past TD_LDS_MAX
  // LDS per token: one gathered image per member a workgroup follows (SWIGLU: two) and the staged
  // row of x.  Tokens per workgroup: as many (1, 2, 4) as TD_LDS_PLAIN holds, no more than the
  // call has; one token of a wide layer may need more than that (PLAIN: up to 128 KiB at
  // m = 32768), which the kernel is then allowed once.  SWIGLU needs up to 16 KiB per round of
  // 4096 positions plus 2 m bytes: m <= 20480 fits TD_LDS_MAX
  const size_t rawbytes = ((size_t)m * 2 + 15) / 16 * 16;
  auto lds_of = [&](int tg) { return ((size_t)(swiglu ? 2 : 1) * p.nround * TD_ROUND_BYTES + rawbytes) * tg; };
  if (lds_of(1) > (size_t)TD_LDS_MAX) return PT2Q_E_UNSUPPORTED;
  p.TG = 1;
  while (p.TG < 4 && p.TG < tokens && lds_of(2 * p.TG) <= (size_t)TD_LDS_PLAIN) p.TG *= 2;
  p.lds = lds_of(p.TG);
  // two workgroups per CU in all (one per token group when the call has several groups), shared
  // out over the members of a PLAIN group in proportion to their rows: one each, the rest by
  // floor(share), never more than a member has rows for (a group of one gets the whole budget)
  p.groups = ceil_div(tokens, p.TG);
  const int budget = td_cus() * (p.groups > 1 ? 1 : 2);
  p.G = TdGroup{};
  p.wgs = 0;
  if (swiglu) {
    p.wgs = min(ceil_div(n[0], TD_WAVES), budget);
  } else {
    long rows = 0;
    for (int z = 0; z < count; ++z) rows += n[z];
    for (int z = 0; z < count; ++z) {
      const int share = 1 + (int)((long)(budget - count) * n[z] / rows);
      p.wgs += min(ceil_div(n[z], TD_WAVES), share);
      p.G.wg_end[z] = p.wgs;
    }
  }
  for (int z = 0; z < PT2Q_DECODE_GROUP_MAX; ++z) {
    const int s = z < count ? z : 0;  // entries past count repeat member 0 and own no workgroup
    p.G.codes[z] = codes[s], p.G.gather[z] = gather[s], p.G.alpha[z] = alpha[s], p.G.mu[z] = mu[s];
    p.G.bias[z] = bias ? bias[s] : nullptr;
    p.G.n[z] = n[s], p.G.B[z] = B[s];
    p.G.y[z] = s < nout ? y[s] : nullptr, p.G.ldy[z] = s < nout ? (long)ldy[s] : 0;
    if (z >= count) p.G.wg_end[z] = p.wgs;
    const bool r = anyres && s < nout && residual[s];
    p.X.res[z] = r ? residual[s] : nullptr, p.X.ldr[z] = r ? (long)ldr[s] : 0;
  }
  p.X.nw = (const uint16_t*)norm_weight, p.X.eps = norm_weight ? norm_eps : 0.0f;
  p.fx = norm_weight ? TD_FX_NORM : anyres ? TD_FX_RES : TD_FX_NONE;
  p.bf16 = xdtype == PT2Q_BF16, p.swiglu = swiglu, p.yf32 = ydtype == PT2Q_F32;
  return PT2Q_OK;
}

enum TdUse { TD_ONE, TD_GROUP, TD_SWIGLU };  // which kernel runs the body

// One kernel instantiation's launch; false when it could not be given the LDS the plan needs.
template <auto KERN, class... Tail>
bool td_launch_kernel(const TdPlan& p, const void* x, int tokens, int64_t ldx, int m, hipStream_t st, Tail... tail) {
  if (p.lds > (size_t)TD_LDS_PLAIN) {
    static bool allowed = false;  // per kernel instantiation (this function's, one per KERN)
    if (!allowed) {
      if (hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, TD_LDS_MAX) != hipSuccess)
        return false;
      allowed = true;
    }
  }
  hipLaunchKernelGGL(KERN, dim3(p.wgs, p.groups), dim3(TD_THREADS), p.lds, st, (const uint16_t*)x, (long)ldx, tokens, m,
                     p.P, p.bse, p.yf32 ? 1 : 0, tail...);
  return true;
}

template <bool BF16, int TG, TdUse USE, TdFx FX>
bool td_launch_as(const TdPlan& p, const void* x, int tokens, int64_t ldx, int m, hipStream_t st) {
  const TdGroup& G = p.G;
  const TdMember one{G.codes[0], G.gather[0], G.alpha[0], G.mu[0], G.bias[0], G.n[0], G.B[0]};
  if constexpr (USE == TD_ONE && FX == TD_FX_NONE)
    return td_launch_kernel<tl_decode_one_kernel<BF16, TG>>(p, x, tokens, ldx, m, st, one, G.y[0], G.ldy[0]);
  else if constexpr (USE == TD_ONE)
    return td_launch_kernel<tl_decode_one_fused_kernel<BF16, TG, FX>>(p, x, tokens, ldx, m, st, one, G.y[0], G.ldy[0],
                                                                      p.X.nw, p.X.eps, p.X.res[0], p.X.ldr[0]);
  else if constexpr (FX == TD_FX_NONE)
    return td_launch_kernel<tl_decode_kernel<BF16, TG, USE == TD_SWIGLU>>(p, x, tokens, ldx, m, st, G);
  else
    return td_launch_kernel<tl_decode_fused_kernel<BF16, TG, USE == TD_SWIGLU, FX>>(p, x, tokens, ldx, m, st, G, p.X);
}

template <bool BF16, TdUse USE, TdFx FX>
bool td_launch_tg(const TdPlan& p, const void* x, int tokens, int64_t ldx, int m, hipStream_t st) {
  if constexpr (USE != TD_SWIGLU) {  // never SWIGLU: four tokens' two gathered images alone are TD_LDS_PLAIN
    if (p.TG == 4) return td_launch_as<BF16, 4, USE, FX>(p, x, tokens, ldx, m, st);
  }
  return p.TG == 2 ? td_launch_as<BF16, 2, USE, FX>(p, x, tokens, ldx, m, st)
                   : td_launch_as<BF16, 1, USE, FX>(p, x, tokens, ldx, m, st);
}

template <TdUse USE, TdFx FX = TD_FX_NONE>
int td_launch(const TdPlan& p, const void* x, int tokens, int64_t ldx, int m, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const bool ok = p.bf16 ? td_launch_tg<true, USE, FX>(p, x, tokens, ldx, m, st)
                         : td_launch_tg<false, USE, FX>(p, x, tokens, ldx, m, st);
  if (!ok) {
    (void)hipGetLastError();
    return PT2Q_E_UNSUPPORTED;
  }
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}

}  // namespace

extern "C" int pt2q_ternary_decode_max_tokens(void) { return TD_MAX_TOKENS; }

extern "C" int pt2q_ternary_decode_group(const void* x, int xdtype, int tokens, int64_t ldx, int m, int count,
                                         const int* n, const uint8_t* const* codes, const int* const* gather,
                                         const float* const* alpha, const float* const* mu, const int* B, int bs,
                                         const float* const* bias, void* const* y, int ydtype, const int64_t* ldy,
                                         int epilogue, void* stream) {
  TdPlan p;
  const int rc = td_plan(x, xdtype, tokens, ldx, m, count, n, codes, gather, alpha, mu, B, bs, bias, y, ydtype, ldy,
                         epilogue, nullptr, 0.0f, nullptr, nullptr, p);
  if (rc != PT2Q_OK) return rc;
  return p.swiglu ? td_launch<TD_SWIGLU>(p, x, tokens, ldx, m, stream) : td_launch<TD_GROUP>(p, x, tokens, ldx, m, stream);
}

// a PLAIN group of one: the same rules and plan, the member handed over as plain kernel arguments
extern "C" int pt2q_ternary_decode(const void* x, int xdtype, int tokens, int64_t ldx, int n, int m,
                                   const uint8_t* codes, const int* gather, const float* alpha,
                                   const float* mu, int B, int bs, const float* bias, void* y,
                                   int ydtype, int64_t ldy, void* stream) {
  TdPlan p;
  const int rc = td_plan(x, xdtype, tokens, ldx, m, 1, &n, &codes, &gather, &alpha, &mu, &B, bs, &bias, &y, ydtype, &ldy,
                         PT2Q_DECODE_PLAIN, nullptr, 0.0f, nullptr, nullptr, p);
  return rc != PT2Q_OK ? rc : td_launch<TD_ONE>(p, x, tokens, ldx, m, stream);
}

// The group entry with the RMSNorm prologue and the residual epilogue.  A call that asks for
// neither launches what pt2q_ternary_decode_group launches; a PLAIN group of one with either takes
// its member and extras as plain kernel arguments, as pt2q_ternary_decode does.
extern "C" int pt2q_ternary_decode_fused(const void* x, int xdtype, int tokens, int64_t ldx, int m, int count,
                                         const int* n, const uint8_t* const* codes, const int* const* gather,
                                         const float* const* alpha, const float* const* mu, const int* B, int bs,
                                         const float* const* bias, void* const* y, int ydtype, const int64_t* ldy,
                                         int epilogue, const void* norm_weight, float norm_eps,
                                         const void* const* residual, const int64_t* ldr, void* stream) {
  TdPlan p;
  const int rc = td_plan(x, xdtype, tokens, ldx, m, count, n, codes, gather, alpha, mu, B, bs, bias, y, ydtype, ldy,
                         epilogue, norm_weight, norm_eps, residual, ldr, p);
  if (rc != PT2Q_OK) return rc;
  if (p.swiglu)
    return p.fx == TD_FX_NORM ? td_launch<TD_SWIGLU, TD_FX_NORM>(p, x, tokens, ldx, m, stream)
                              : td_launch<TD_SWIGLU>(p, x, tokens, ldx, m, stream);
  if (p.fx == TD_FX_NONE) return td_launch<TD_GROUP>(p, x, tokens, ldx, m, stream);
  if (count == 1)
    return p.fx == TD_FX_NORM ? td_launch<TD_ONE, TD_FX_NORM>(p, x, tokens, ldx, m, stream)
                              : td_launch<TD_ONE, TD_FX_RES>(p, x, tokens, ldx, m, stream);
  return p.fx == TD_FX_NORM ? td_launch<TD_GROUP, TD_FX_NORM>(p, x, tokens, ldx, m, stream)
                            : td_launch<TD_GROUP, TD_FX_RES>(p, x, tokens, ldx, m, stream);
}

extern "C" int pt2q_rmsnorm(const void* x, int xdtype, int tokens, int64_t ldx, int m, const void* weight, float eps,
                            void* y, int64_t ldy, void* stream) {
  if (!x || !weight || !y || tokens <= 0 || m <= 0 || ldx < m || ldy < m || !(eps >= 0.0f && eps <= FLT_MAX))
    return PT2Q_E_ARG;
  if (xdtype != PT2Q_F16 && xdtype != PT2Q_BF16) return PT2Q_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (xdtype == PT2Q_BF16)
    hipLaunchKernelGGL(tl_rmsnorm_kernel<true>, dim3((unsigned)tokens), dim3(TD_THREADS), 0, st, (const uint16_t*)x,
                       (long)ldx, m, (const uint16_t*)weight, eps, (uint16_t*)y, (long)ldy);
  else
    hipLaunchKernelGGL(tl_rmsnorm_kernel<false>, dim3((unsigned)tokens), dim3(TD_THREADS), 0, st, (const uint16_t*)x,
                       (long)ldx, m, (const uint16_t*)weight, eps, (uint16_t*)y, (long)ldy);
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}
