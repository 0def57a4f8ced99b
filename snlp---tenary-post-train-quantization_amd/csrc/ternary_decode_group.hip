// Grouped fused decode: up to four packed ternary linears that read the same x, 1..8 tokens, in
// ONE launch with no workspace (the q/k/v projections of a decoder layer), or the gate and up
// projections of a gated MLP with the SwiGLU activation as epilogue.  The members' buffers are
// those of pt2q_ternary_pack; their pointers travel by value in the kernel's arguments.
//
// Arithmetic: every projection value is DOT64P of csrc/ternary_decode.hip -- the
// chain runs through the same td_piece, the fold through the same bfly64 -- so a PLAIN member's
// output has the bits of pt2q_ternary_decode on that member alone; the SWIGLU epilogue is
// contract SWIGLU16: g and u rounded as the separate calls would store them, then
// fp32 operations, each rounded to nearest even and none fused.
//
// Structure: that of tl_decode_kernel -- one wave per output row, 8 waves per workgroup, x staged
// in LDS and gathered LDS to LDS, TD_DEPTH code loads in flight per wave.
//   PLAIN   the grid's workgroups are shared out over the members in proportion to their rows
//           (wg_end); a workgroup serves one member, whose gather it follows.
//   SWIGLU  a workgroup gathers x twice, once per member, and the wave that owns row i walks
//           the items (row, round, member) with the member innermost: ring slot s holds member
//           s % 2, so the member of an item is known at compile time and both chains keep the
//           four loads in flight of the plain kernel.
#include "common.hpp"
#include "internal.hpp"
#include "ternary_decode.hpp"

namespace {

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

template <bool BF16, int TG, bool SWIGLU>
__global__ __launch_bounds__(TD_THREADS, 4) void tl_decode_group_kernel(const uint16_t* x, long ldx, int tokens, int m,
                                                                        int P, int bse, int yf32, TdGroup G) {
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

  // xs_of(zz)[t][p] = x[t0 + t][gather_zz[p]] (+0 for padding positions and tokens past the end):
  // the TG rows of x are staged once by coalesced loads and gathered from LDS, per member; every
  // member's first eight indices per thread are loaded ahead of the staging barrier
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
#pragma unroll
  for (int t = 0; t < TG; ++t) {
    if (t0 + t < tokens) {
      const uint16_t* xr = x + (long)(t0 + t) * ldx;
      for (int i = threadIdx.x; i < m; i += TD_THREADS) raw[t * rawstride + i] = xr[i];
    }
  }
  __syncthreads();
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
  // v + bias of member zz, as pt2q_ternary_decode forms it before its one rounding
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
    const int q = 64 * k + lane;
    if (q < npieces) {
      td_piece<BF16, TG>(xs_of(Z) + (long)k * TG * 512 + lane, it, perpiece, q, bse, M[Z].B,
                         M[Z].alpha + (long)row * M[Z].B, M[Z].mu + (long)row * M[Z].B, acc[Z]);
    }
    const int r0 = row;
    const bool last = Z == NZ - 1 && k == nround - 1;  // the row's last item: fold and store
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
          const float v = biased(0, t);
          void* y = td_pick(G.y, z);
          if (st) {
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
  if constexpr (SWIGLU) {
    while (item(TdZ<0>{}, ring[0]) && item(TdZ<1>{}, ring[1]) && item(TdZ<0>{}, ring[2]) &&
           item(TdZ<1>{}, ring[3])) {
    }
  } else {
    while (item(TdZ<0>{}, ring[0]) && item(TdZ<0>{}, ring[1]) && item(TdZ<0>{}, ring[2]) &&
           item(TdZ<0>{}, ring[3])) {
    }
  }
}

}  // namespace

extern "C" int pt2q_ternary_decode_group(const void* x, int xdtype, int tokens, int64_t ldx, int m, int count,
                                         const int* n, const uint8_t* const* codes, const int* const* gather,
                                         const float* const* alpha, const float* const* mu, const int* B, int bs,
                                         const float* const* bias, void* const* y, int ydtype, const int64_t* ldy,
                                         int epilogue, void* stream) {
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
  if (bs < m && bs % 16 != 0) return PT2Q_E_UNSUPPORTED;  // alpha constant within a 16-group
  for (int z = 0; z < count; ++z)
    if ((long)ceil_div(m, bs < m ? bs : m) > B[z]) return PT2Q_E_ARG;
  if (tokens > TD_MAX_TOKENS) return PT2Q_E_UNSUPPORTED;
  const int P = (int)pt2q_ternary_linear_positions(m);
  const int bse = bs < m ? bs : P;  // per-channel: one scale for every position
  const int nround = ceil_div(P / 64, 64);
  if (nround > TD_MAX_ROUNDS) return PT2Q_E_UNSUPPORTED;
  // LDS per token: one gathered image per member a workgroup follows (SWIGLU: two) and the staged
  // row of x; TG as pt2q_ternary_decode picks it.  SWIGLU needs up to 16 KiB per round of 4096
  // positions plus 2 m bytes: m <= 20480 fits TD_LDS_MAX
  const size_t rawbytes = ((size_t)m * 2 + 15) / 16 * 16;
  auto lds_of = [&](int tg) { return ((size_t)(swiglu ? 2 : 1) * nround * TD_ROUND_BYTES + rawbytes) * tg; };
  if (lds_of(1) > (size_t)TD_LDS_MAX) return PT2Q_E_UNSUPPORTED;
  int TG = 1;
  while (TG < 4 && TG < tokens && lds_of(2 * TG) <= (size_t)TD_LDS_PLAIN) TG *= 2;
  const size_t lds = lds_of(TG);
  // two workgroups per CU in all (one per token group when the call has several groups), shared
  // out over the members of a PLAIN group in proportion to their rows: one each, the rest by
  // floor(share), never more than a member has rows for
  const int groups = ceil_div(tokens, TG);
  const int budget = td_cus() * (groups > 1 ? 1 : 2);
  TdGroup G = {};
  int wgs = 0;
  if (swiglu) {
    wgs = min(ceil_div(n[0], TD_WAVES), budget);
  } else {
    long rows = 0;
    for (int z = 0; z < count; ++z) rows += n[z];
    for (int z = 0; z < count; ++z) {
      const int share = 1 + (int)((long)(budget - count) * n[z] / rows);
      wgs += min(ceil_div(n[z], TD_WAVES), share);
      G.wg_end[z] = wgs;
    }
  }
  for (int z = 0; z < PT2Q_DECODE_GROUP_MAX; ++z) {
    const int s = z < count ? z : 0;  // entries past count repeat member 0 and own no workgroup
    G.codes[z] = codes[s], G.gather[z] = gather[s], G.alpha[z] = alpha[s], G.mu[z] = mu[s];
    G.bias[z] = bias ? bias[s] : nullptr;
    G.n[z] = n[s], G.B[z] = B[s];
    G.y[z] = s < nout ? y[s] : nullptr, G.ldy[z] = s < nout ? (long)ldy[s] : 0;
    if (z >= count) G.wg_end[z] = wgs;
  }
  const dim3 grid(wgs, groups);
  bool attr_failed = false;
  auto launch = [&](auto kern) {
    if (lds > (size_t)TD_LDS_PLAIN) {
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
    hipLaunchKernelGGL(kern, grid, dim3(TD_THREADS), lds, st, (const uint16_t*)x, (long)ldx, tokens, m, P, bse,
                       ydtype == PT2Q_F32 ? 1 : 0, G);
  };
  auto launch_tg = [&](auto bf, auto sw) {
    constexpr bool BF = decltype(bf)::value, SW = decltype(sw)::value;
    if (TG == 4) {  // never SWIGLU: four tokens' two gathered images alone are TD_LDS_PLAIN
      if constexpr (!SW) launch(tl_decode_group_kernel<BF, 4, false>);
    } else {
      TG == 2 ? launch(tl_decode_group_kernel<BF, 2, SW>) : launch(tl_decode_group_kernel<BF, 1, SW>);
    }
  };
  if (xdtype == PT2Q_BF16)
    swiglu ? launch_tg(TdZ<1>{}, TdZ<1>{}) : launch_tg(TdZ<1>{}, TdZ<0>{});
  else
    swiglu ? launch_tg(TdZ<0>{}, TdZ<1>{}) : launch_tg(TdZ<0>{}, TdZ<0>{});
  if (attr_failed) {
    (void)hipGetLastError();
    return PT2Q_E_UNSUPPORTED;
  }
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}
