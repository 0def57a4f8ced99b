// GPTQ error feedback of one block (main.py:214, gptq.py:181-186):
//   W[:, rem] -= E · C,   E = W_b − (α T + μ) (n × bs),  C = Hinv[blk][:, rem] / diag (bs × nr)
// in the feature-major layout: Wt[rem_e][i] -= Σ_k C[k][e] · E[k][i], the product a k-ascending
// f32 chain (v_mfma_f32_32x32x2_f32 issues k in ascending pairs: D = fma(a1,b1, fma(a0,b0, C)),
// the oracle's order), rounded once, then one subtraction -- the contract of DESIGN.md §3.
//
// A K <= 128 GEMM is too short for the generic tile loop (load, sync, compute, reload C): here a
// persistent workgroup (ef2_gemm_kernel) walks 128 × 128 output tiles and keeps the operand stream
// running across them.  A tile's K runs through a ring of two 32-row LDS stages (A: C[k][e0..],
// B: E[k][i0..], 32 KiB per stage) filled by LDS-DMA: while one stage is multiplied the stage after
// next -- of this tile or the next one -- is fetched into the slot just consumed, and the old Wt
// values of the tile are loaded while its MFMAs run.  With 66 KiB of LDS and at most 256 registers
// per lane two workgroups share every CU, so each SIMD interleaves two waves: one issues MFMAs
// while the other waits on LDS, a barrier or a DMA.  Every wave issues the same number of memory
// instructions per tile (out-of-range rows and columns go through buffer ops with offsets past
// the end, which the hardware drops), so the hand-counted s_waitcnt vmcnt values below are exact.
//
// With a partial buffer the epilogue also forms the next block's SSR mean partials (the w-bar of
// ssr.hip over the rows just written, crow = the next block's rem): a tile's 128 rows e are
// exactly one w-bar chunk, so per column i its new values are folded in registers -- rows e and
// e + 32 of a lane added, a butterfly over the 32 lanes (xor 16 by ds_swizzle, then bfly16), the
// two waves of a column half combined through LDS -- the CHUNK128 order of DESIGN.md §3.  That
// removes the separate w-bar pass over W[:, rem] (one full read per block).
#include "common.hpp"
#include "internal.hpp"
#include "probe.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int EF_T = 128;                    // output tile (e and i)
constexpr int EF_ROWB = EF_T * 4;            // 512 B per k row of a panel
constexpr int E2_KS = 32;                    // k rows per LDS stage (16 k-pairs)
constexpr int E2_PANEL = E2_KS * EF_ROWB;    // 16 KiB
constexpr int E2_STAGE = 2 * E2_PANEL;       // A + B: 32 KiB
constexpr int EF_CV = 16;                    // C float4 loads (= stores) per lane per tile
constexpr unsigned EF_DROP = 0x80000000u;    // buffer offset past any Wt (dropped access)

__device__ uint4 ef_zero16;  // DMA source of the k rows past bs (zero-initialised)

// wave index inside the workgroup of 4 waves
PT2Q_DEV int ef_wave() { return (int)(threadIdx.x >> 6); }

struct EfArgs {
  const float* Ck;  // C[k][e], ld m
  long ldk;
  const float* Et;  // E[k][i], ld ldw
  float* Wt;        // Wt[j][i], ld ldw
  long ldw;
  const int* crow;  // rem (nr entries)
  int nr, bs, te, ti, ntile;
  long zs;          // grouped: bytes between the linears' workspace slices (Ck, Et, Wt, crow, part)
  int nz;           // linears; the work line is nz * ntile tiles, linear-major
  float* part;      // nullable: w-bar chunk partials part[c][i] of the updated rows, i < n
  int n;
};

// The arguments of linear z (its workspace slice).
PT2Q_DEV EfArgs ef_linear(const EfArgs& a0, int z) {
  EfArgs a = a0;
  const long o = (long)z * a0.zs;
  a.Ck = (const float*)((const char*)a0.Ck + o);
  a.Et = (const float*)((const char*)a0.Et + o);
  a.Wt = (float*)((char*)a0.Wt + o);
  a.crow = (const int*)((const char*)a0.crow + o);
  if (a0.part) a.part = (float*)((char*)a0.part + o);
  return a;
}

// one 16-B LDS-DMA: global (sbase + voff) -> LDS m0 + 16 lane (m0 is set afresh by every DMA)
PT2Q_DEV void ef_dma_asm(const char* sbase, uint32_t voff, uint32_t m0) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(m0)
               : "memory");
}

template <int OFF>
PT2Q_DEV float ef_ld(uint32_t addr) {
  float r;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "i"(OFF));
  return r;
}

// wait until at most N LDS operations are outstanding, tying the operand registers a, b
template <int N>
PT2Q_DEV void ef_wait(float (&a)[2], float (&b)[2]) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]) : "n"(N));
}

// k-pair S of a stage: lane reads A rows e (2 MFMA row blocks) and B columns i (2 blocks).
template <int S>
PT2Q_DEV void ef_read(uint32_t baseA, uint32_t baseB, float (&a)[2], float (&b)[2]) {
  a[0] = ef_ld<S * 2 * EF_ROWB>(baseA);
  a[1] = ef_ld<S * 2 * EF_ROWB + 128>(baseA);
  b[0] = ef_ld<S * 2 * EF_ROWB>(baseB);
  b[1] = ef_ld<S * 2 * EF_ROWB + 128>(baseB);
}

struct EfAcc {
  f32x16 acc[2][2];  // [rm][rn], transposed MFMA: lane <-> e row, registers <-> i columns

  // k-pair S: its operands are in set S % 4; the reads of pair S+2 go to set (S+2) % 4, whose
  // registers the MFMAs of pair S-2 read long ago (no overwrite of an operand in flight), so an
  // LDS read has two pairs (~500 cycles) to land instead of one.  The order reads -> MFMAs ->
  // wait is pinned.
  template <int S>
  PT2Q_DEV void run(uint32_t bA, uint32_t bB, float (&a)[4][2], float (&b)[4][2]) {
    constexpr int NP = E2_KS / 2;
    if constexpr (S < NP) {
      constexpr int c = S % 4;
      if constexpr (S + 2 < NP) ef_read<S + 2>(bA, bB, a[(S + 2) % 4], b[(S + 2) % 4]);
      if constexpr (S > 0) {  // pair S-1's operands stay allocated until these reads are out
        constexpr int p = (S + 3) % 4;
        asm volatile("" ::"v"(a[p][0]), "v"(a[p][1]), "v"(b[p][0]), "v"(b[p][1]));
      }
      __builtin_amdgcn_sched_barrier(0);
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[c][0], a[c][0], acc[0][0], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[c][1], a[c][0], acc[0][1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[c][0], a[c][1], acc[1][0], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[c][1], a[c][1], acc[1][1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (S + 1 < NP) {  // pair S+1's reads (issued at pair S-1) landed; younger LDS
        // operations: pair S+2's reads
        ef_wait<(S + 2 < NP ? 4 : 0)>(a[(S + 1) % 4], b[(S + 1) % 4]);
      }
      run<S + 1>(bA, bB, a, b);
    }
  }

  // the E2_KS / 2 k-pairs of one stage (k rows past bs are zero in LDS: exact no-op steps)
  PT2Q_DEV void stage(uint32_t stg) {
    const int lane = threadIdx.x & 63, wave = ef_wave();
    const int wr = wave >> 1, wc = wave & 1, li = lane & 31, lk = lane >> 5;
    const uint32_t bA = stg + lk * EF_ROWB + (wr * 64 + li) * 4;
    const uint32_t bB = stg + E2_PANEL + lk * EF_ROWB + (wc * 64 + li) * 4;
    float a[4][2], b[4][2];
    ef_read<0>(bA, bB, a[0], b[0]);
    ef_read<1>(bA, bB, a[1], b[1]);
    ef_wait<4>(a[0], b[0]);
    run<0>(bA, bB, a, b);
  }
};

PT2Q_DEV int ef_row(int e0, int rm) {
  const int lane = threadIdx.x & 63, wr = ef_wave() >> 1;
  return e0 + wr * 64 + rm * 32 + (lane & 31);
}

// The byte offsets of this lane's old / new Wt values as a per-tile row base: group (rm, rn, q) sits
// at rb[rm] + 4 (32 rn + 8 q) bytes (the constant folds into the buffer instruction's offset field), rb[rm] = EF_DROP for a row
// past nr or a column half past ldw (ldw % 64 == 0, so a wave's 64 columns are in or out together)
PT2Q_DEV void ef_rowbase(const EfArgs& a, const int (&wrow)[2], int i0, uint32_t (&rb)[2]) {
  const int lane = threadIdx.x & 63, wc = ef_wave() & 1;
  const int i = i0 + wc * 64 + 4 * (lane >> 5);
#pragma unroll
  for (int rm = 0; rm < 2; ++rm)
    rb[rm] = (wrow[rm] < 0 || i0 + wc * 64 >= a.ldw || probe::ef_drop_wt)
                 ? EF_DROP
                 : (uint32_t)(((long)wrow[rm] * a.ldw + i) * 4);
}

// the Wt rows of this lane's two output rows (crow from L2: two loads per lane, issued uniformly
// by every wave and older than every operation a later hand-counted vmcnt wait covers)
PT2Q_DEV void ef_rows(const EfArgs& a, int e0, int (&wrow)[2]) {
  int v[2];
#pragma unroll
  for (int rm = 0; rm < 2; ++rm) {
    const int e = ef_row(e0, rm);
    v[rm] = a.crow[e < a.nr ? e : 0];
  }
#pragma unroll
  for (int rm = 0; rm < 2; ++rm) wrow[rm] = ef_row(e0, rm) < a.nr ? v[rm] : -1;
}

// ---- the next block's w-bar partials (see the file header).  Column j = (rn, q, u) of the
// tile's results pend; the lane sum over
// rows e and e + 32 (its two row blocks rm), bfly16 inside each 16-lane row, then row_bcast:15
// adds row 0's sum into row 1 (row 2's into row 3): lanes 16 and 48 hold the wave's 64-row sum
// for column halves h = 0, 1 and store it to LDS (the other lanes to a per-lane spare slot).
constexpr int EF_PS = 8;    // w-bar partial stores per wave per tile (float4; dropped where unused)
constexpr int EF_RED = 512; // LDS floats: [wave][64] sums + [wave][64] spare slots

template <int J>
PT2Q_DEV void ef_wbar_step(const int (&prow)[2], const u32x4 (&pend)[EF_CV], float* red) {
  constexpr int rn = J >> 4, q = (J >> 2) & 3, u = J & 3;
  const int lane = threadIdx.x & 63, wave = ef_wave();
  const float v0 = prow[0] >= 0 ? __uint_as_float(pend[rn * 4 + q][u]) : 0.0f;
  const float v1 = prow[1] >= 0 ? __uint_as_float(pend[(2 + rn) * 4 + q][u]) : 0.0f;
  float x = bfly16(v0 + v1);
  x = x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x142, 0xA, 0xF, false));  // row_bcast:15
  const bool sel = (lane & 31) == 16;
  red[sel ? wave * 64 + (lane >> 5) * 32 + J : 256 + wave * 64 + lane] = x;
}

// The w-bar partials of a finished tile (e0, i0) from the wave sums in LDS: part[c][i] = X + Y,
// X from the row-half-0 wave of the column half, Y from the row-half-1 wave.  Branch-free: every
// lane reads (b128, all in flight) and every wave issues exactly EF_PS buffer stores (real ones:
// lanes 0 and 32 of the row-half-0 waves, i < n; the rest dropped).
PT2Q_DEV void ef_wbar_store(int n, __amdgpu_buffer_rsrc_t rp, bool valid, int e0, int i0, const float* red) {
  const int lane = threadIdx.x & 63, wave = ef_wave(), wr = wave >> 1, wc = wave & 1;
  const int h = lane >> 5;
  const bool mine = valid && wr == 0 && (lane & 31) == 0;
  const long cb = (long)(e0 / EF_T) * n;
  const f32x4* X = (const f32x4*)(red + wc * 64 + h * 32);
  const f32x4* Y = (const f32x4*)(red + (wc + 2) * 64 + h * 32);
#pragma unroll
  for (int rn = 0; rn < 2; ++rn) {
    f32x4 x[4], y[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      x[q] = X[rn * 4 + q];
      y[q] = Y[rn * 4 + q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + wc * 64 + rn * 32 + 8 * q + 4 * h;
      const f32x4 o = x[q] + y[q];
      const unsigned off = (mine && i < n) ? (unsigned)((cb + i) * 4) : EF_DROP;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rp, off, 0, 0);
    }
  }
}

// ---- ef2_gemm_kernel ------------------------------------------------------------------------
// Per tile: the old Wt values are loaded at the top (their latency hides under the tile's MFMAs),
// the K stages stream through the ring (running on into the next tile's first two stages), and the
// epilogue subtracts, stores, and forms the tile's own w-bar partials.  The k-pairs are issued in
// ascending order into the same accumulators, the product is subtracted once, and the w-bar is the
// CHUNK128 tree: bit-identical to oracle/pt2q_oracle.c (tests/test_gpu_parity.py).

struct E2Vo {
  uint32_t a[4], b[4];
};

PT2Q_DEV void e2_voff(const EfArgs& a, E2Vo& v) {
  const int lane = threadIdx.x & 63, wave = ef_wave();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int kr = (wave * 4 + q) * 2 + (lane >> 5), d = 4 * (lane & 31);
    v.a[q] = (uint32_t)(((long)kr * a.ldk + d) * 4);
    v.b[q] = (uint32_t)(((long)kr * a.ldw + d) * 4);
  }
}

// One 16-B chunk q (< 4) of a ragged stage s of tile (e0, i0): the fast path's addresses (panel
// bases ba / bb + this lane's offsets v), except that k rows past bs come from a zero chunk (their
// MFMA steps are then exact no-ops) and columns past the data from the operand's first element
// (garbage in rows / columns whose results are dropped), so every wave issues the same DMAs.
PT2Q_DEV void e2_stage_q(const EfArgs& a, int e0, int i0, int s, const char* ba, const char* bb, const E2Vo& v,
                         uint8_t* stg, int q, bool withB) {
  const int lane = threadIdx.x & 63, wave = ef_wave();
  typedef __attribute__((address_space(3))) void* lptr;
  const int k = s * E2_KS + (wave * 4 + q) * 2 + (lane >> 5);
  const int d = 4 * (lane & 31);
  const bool kin = k < a.bs;
  const void* sa = kin ? (const void*)(e0 + d < a.nr ? ba + v.a[q] : (const char*)a.Ck) : (const void*)&ef_zero16;
  const void* sb = kin ? (const void*)(i0 + d < a.ldw ? bb + v.b[q] : (const char*)a.Et) : (const void*)&ef_zero16;
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  __builtin_amdgcn_global_load_lds(sa, (lptr)(stg + (wv * 4 + q) * 1024), 16, 0, 0);
  if (withB) __builtin_amdgcn_global_load_lds(sb, (lptr)(stg + E2_PANEL + (wv * 4 + q) * 1024), 16, 0, 0);
}

// stage s of tile (e0, i0) into slot `stg`: scalar-base DMAs when whole (every k row and column of
// the stage in range: a DMA is then s_mov m0 + one global_load_lds with a scalar base instead of
// ~35 instructions of per-lane address math), else per lane; returns the DMA instructions issued per wave (8, or 4 without the B panel)
PT2Q_DEV int e2_stage(const EfArgs& a, int e0, int i0, int s, uint8_t* stg, uint32_t stg_lds, const E2Vo& v,
                      bool withB) {
  if constexpr ((PT2Q_EF2_KPROBE & 2) != 0) {  // knock-out: every DMA from the one zero chunk (L2-hot)
    typedef __attribute__((address_space(3))) void* lptr;
    const int wv = __builtin_amdgcn_readfirstlane(ef_wave());
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      __builtin_amdgcn_global_load_lds(&ef_zero16, (lptr)(stg + (wv * 4 + q) * 1024), 16, 0, 0);
      if (withB) __builtin_amdgcn_global_load_lds(&ef_zero16, (lptr)(stg + E2_PANEL + (wv * 4 + q) * 1024), 16, 0, 0);
    }
    return withB ? 8 : 4;
  }
  const bool fast = (s + 1) * E2_KS <= a.bs && e0 + EF_T <= a.nr && i0 + EF_T <= a.ldw;
  const char* ba = (const char*)(a.Ck + (long)s * E2_KS * a.ldk + e0);
  const char* bb = (const char*)(a.Et + (long)s * E2_KS * a.ldw + i0);
  if (!fast) {
#pragma unroll
    for (int q = 0; q < 4; ++q) e2_stage_q(a, e0, i0, s, ba, bb, v, stg, q, withB);
    return withB ? 8 : 4;
  }
  const int wv = __builtin_amdgcn_readfirstlane(ef_wave());
  const uint32_t mA = stg_lds + (uint32_t)(wv * 4 * 1024), mB = mA + E2_PANEL;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    ef_dma_asm(ba, v.a[q], mA + q * 1024);
    if (withB) ef_dma_asm(bb, v.b[q], mB + q * 1024);
  }
  return withB ? 8 : 4;
}

// s_waitcnt vmcnt(n), n < 64 (immediate operand)
PT2Q_DEV void e2_vmcnt(int n) {
  switch (n) {
#define E2_W(k) \
  case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
    E2_W(0) E2_W(1) E2_W(2) E2_W(3) E2_W(4) E2_W(5) E2_W(6) E2_W(7) E2_W(8) E2_W(9) E2_W(10) E2_W(11) E2_W(12)
    E2_W(13) E2_W(14) E2_W(15) E2_W(16) E2_W(17) E2_W(18) E2_W(19) E2_W(20) E2_W(21) E2_W(22) E2_W(23) E2_W(24)
    E2_W(25) E2_W(26) E2_W(27) E2_W(28) E2_W(29) E2_W(30) E2_W(31) E2_W(32) E2_W(33) E2_W(34) E2_W(35) E2_W(36)
    E2_W(37) E2_W(38) E2_W(39) E2_W(40) E2_W(41) E2_W(42) E2_W(43) E2_W(44) E2_W(45) E2_W(46) E2_W(47) E2_W(48)
    E2_W(49) E2_W(50) E2_W(51) E2_W(52) E2_W(53) E2_W(54) E2_W(55) E2_W(56) E2_W(57) E2_W(58) E2_W(59) E2_W(60)
    E2_W(61) E2_W(62)
#undef E2_W
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

template <int J, int JE>
PT2Q_DEV void ef_wbar_span(const int (&prow)[2], const u32x4 (&pend)[EF_CV], float* red) {
  if constexpr (J < JE) {
    ef_wbar_step<J>(prow, pend, red);
    ef_wbar_span<J + 1, JE>(prow, pend, red);
  }
}

// old values of column group rn (c[j], j = (rm * 2 + rn) * 4 + q: 8 loads), or their results
template <int RN>
PT2Q_DEV void e2_load(u32x4 (&c)[EF_CV], __amdgpu_buffer_rsrc_t rc, const uint32_t (&rb)[2]) {
#pragma unroll
  for (int rm = 0; rm < 2; ++rm)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      c[(rm * 2 + RN) * 4 + q] = __builtin_amdgcn_raw_buffer_load_b128(rc, rb[rm] + 4 * (32 * RN + 8 * q), 0, 0);
}

template <int RN>
PT2Q_DEV void e2_sub(u32x4 (&c)[EF_CV], const EfAcc& F) {
#pragma unroll
  for (int rm = 0; rm < 2; ++rm)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = (rm * 2 + RN) * 4 + q;
#pragma unroll
      for (int u = 0; u < 4; ++u) c[j][u] = __float_as_uint(__uint_as_float(c[j][u]) - F.acc[rm][RN][4 * q + u]);
    }
}

// Column group 0's old Wt values are loaded this many stages before the tile's last (clamped to
// the first stage): 3 = at the tile's top, under all its MFMAs -- the grouped 16-linear 4096^2 loop
// 13.26-13.34 -> 12.93-13.03 ms (1 and 2 stages: 13.22-13.26; tools/ef2_g0_lib_ab.sh): PT2Q_EF2_G0_EARLY
// (probe.hpp).  PT2Q_EF2_STORE_AUX is the cache policy of the Wt stores (probe builds may set it:
// 16 = sc1, the line dropped from L2; 2 = nt).
template <int RN>
PT2Q_DEV void e2_store(const u32x4 (&c)[EF_CV], __amdgpu_buffer_rsrc_t rc, const uint32_t (&rb)[2]) {
#pragma unroll
  for (int rm = 0; rm < 2; ++rm)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      __builtin_amdgcn_raw_buffer_store_b128(c[(rm * 2 + RN) * 4 + q], rc, rb[rm] + 4 * (32 * RN + 8 * q), 0,
                                             PT2Q_EF2_STORE_AUX);
}

// Column group 1's old values by LDS-DMA (NST = 4): 8 buffer-to-LDS loads per wave, 16 bytes per lane,
// into the wave's own chunks of a ring slot -- exactly the bytes its own stage DMAs (e2_stage: wave
// w owns A chunks (4 w + q) and B chunks E2_PANEL + (4 w + q) KiB) write next, so no other wave
// reads or writes them in between.  The loads are row-contiguous: load j brings rows 8 j .. 8 j + 7
// of the wave's 64 output rows, 8 lanes per row covering its 128-byte group-1 segment (a whole
// cache line per row, 8 lines per instruction -- the register-path loads touched 32 rows x 32
// bytes each); lane L of load j holds row 8 j + L / 8, 16-byte piece L % 8, and the epilogue
// reads each lane's own pieces back from there.
PT2Q_DEV uint32_t e2_g1_chunk(int wv, int j) {
  return (uint32_t)(j < 4 ? (wv * 4 + j) * 1024 : E2_PANEL + (wv * 4 + j - 4) * 1024);
}
PT2Q_DEV void e2_g1_dma(__amdgpu_buffer_rsrc_t rc, const uint32_t (&rb)[2], uint8_t* slot) {
  typedef __attribute__((address_space(3))) void* lptr;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(ef_wave());
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    // row 8 j + lane / 8 of the wave: row block rm = j / 4, its base from that row's h = 0 lane
    const uint32_t src = (uint32_t)__shfl((int)rb[j >> 2], 8 * (j & 3) + (lane >> 3));
    const uint32_t off = src == EF_DROP ? EF_DROP : src + 4 * (32 + 4 * (lane & 7));
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rc, (lptr)(slot + e2_g1_chunk(wv, j)), 16, off, 0, 0, 0);
  }
}
PT2Q_DEV void e2_g1_read(u32x4 (&c)[EF_CV], const uint8_t* slot) {
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(ef_wave());
  const int li = lane & 31, h = lane >> 5;
#pragma unroll
  for (int rm = 0; rm < 2; ++rm)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = rm * 4 + (li >> 3), piece = ((li & 7) << 3) | (2 * q + h);
      c[(rm * 2 + 1) * 4 + q] = *(const u32x4*)(slot + e2_g1_chunk(wv, j) + 16 * piece);
    }
}

// NST = K stages per tile (2: bs <= 64, 4: bs <= 128; stages past bs are zero chunks: no-op pairs).
// NST = 2, issue order per tile, for the hand-counted vmcnt waits: [next rows: 2] [old values,
// column group 0: 8, before stage 0's compute (PT2Q_EF2_G0_EARLY)] [the next tile's stages 0 and 1
// after computes 0 and 1]; the epilogue then [waits for group 0] [loads group 1: 8] [stores group
// 0: 8] [waits for group 1] [stores it: 8] [w-bar partials: P].  So at the next tile's top only
// that tile's stores (SP) may still be in flight beside its stages.
// NST = 4 (G1L): column group 1's old values come by LDS-DMA (e2_g1_dma) issued after stage 2's
// compute into the slot it freed, so their latency hides under stage 3's MFMAs instead of the
// epilogue's; the next tile's stage 0 then goes into stage 3's slot and its stage 1 into the
// group-1 slot once the waves have read it (mid-epilogue), so the slots' roles alternate from
// tile to tile (par).  Issue order: [rows: 2] [group 0 loads: 8] [stage 2, 3 after compute 0, 1]
// [group 1: 8 after compute 2] [next stage 0 after compute 3] [epilogue: stores 0: 8, next stage
// 1, stores 1: 8, w-bar: P].  Same products, same order: the same bits.
template <int NST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void ef2_gemm_kernel(
    EfArgs a0, long wt_bytes, long part_bytes) {
  static_assert(NST == 2 || NST == 4, "two or four K stages per tile");
  constexpr bool G1L = NST == 4;
  __shared__ __attribute__((aligned(1024))) uint8_t smem[2 * E2_STAGE];
  __shared__ __attribute__((aligned(16))) float red[EF_RED];  // w-bar wave sums (ef_wbar_step)
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem;
  const int total = a0.ntile * a0.nz;
  int t = (int)blockIdx.x;
  if (t >= total) return;
  PT2Q_EF2_CLK(0);
  auto corner = [&](int t, EfArgs& a, int& e0, int& i0) {
    const int z = t / a0.ntile, tl = t - z * a0.ntile;
    a = ef_linear(a0, z);
    e0 = (tl / a0.ti) * EF_T;
    i0 = (tl % a0.ti) * EF_T;
  };
  auto rsrc = [&](const EfArgs& a) { return __builtin_amdgcn_make_buffer_rsrc(a.Wt, 0, (int)wt_bytes, 0x00020000); };
  auto prsrc = [&](const EfArgs& x) { return __builtin_amdgcn_make_buffer_rsrc(x.part, 0, (int)part_bytes, 0x00020000); };
  const int P = a0.part ? EF_PS : 0;  // w-bar partial stores per wave per tile
  EfArgs a;
  int e0, i0, wrow[2];
  corner(t, a, e0, i0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
  ef_rows(a, e0, wrow);
  E2Vo vo;
  e2_voff(a0, vo);
  e2_stage(a, e0, i0, 0, smem, lds0, vo, true);
  int Dn1 = e2_stage(a, e0, i0, 1, smem + E2_STAGE, lds0 + E2_STAGE, vo, true);
  int SP = 0;
  int par = 0;  // G1L: the slot of this tile's stage 0 (stage s in slot (s + par) & 1)
  constexpr int G0S = NST - 1 - PT2Q_EF2_G0_EARLY < 0 ? 0 : NST - 1 - PT2Q_EF2_G0_EARLY;
  for (;;) {
    const int tn = t + (int)gridDim.x;
    const bool more = tn < total;
    int en = e0, in = i0, nrow[2];
    EfArgs an = a;
    if (more) corner(tn, an, en, in);
    // the next tile's stage j lands in the slot that held this tile's stage NST - 2 + j: its E
    // panel is still there only when that is the same stage (NST == 2), same linear, same i0
    const bool newB = NST != 2 || !(more && an.Et == a.Et && in == i0);
    const __amdgpu_buffer_rsrc_t rc = rsrc(a);
    uint32_t rb[2];
    ef_rowbase(a, wrow, i0, rb);
    // probe tools only (build-time PT2Q_EF2_KPROBE, probe.hpp): 1 = the Wt traffic dropped, 8 / 16 =
    // the old-value loads / the stores go to the first rows of Wt (L2-hot) -- same instructions
    // and counts, results garbage
    if constexpr ((PT2Q_EF2_KPROBE & 1) != 0) rb[0] = rb[1] = EF_DROP;
    uint32_t rbl[2] = {rb[0], rb[1]}, rbs[2] = {rb[0], rb[1]};
    if constexpr ((PT2Q_EF2_KPROBE & 8) != 0) rbl[0] = rbl[1] = 0;
    if constexpr ((PT2Q_EF2_KPROBE & 16) != 0) rbs[0] = rbs[1] = 0;
    ef_rows(an, en, nrow);  // 2 loads, issued by every wave whether or not a next tile exists
    EfAcc F;
#pragma unroll
    for (int rm = 0; rm < 2; ++rm)
#pragma unroll
      for (int rn = 0; rn < 2; ++rn) F.acc[rm][rn] = f32x16{};
    u32x4 c[EF_CV];
    int X[NST];  // DMAs issued after compute s (into the slot it freed)
#pragma unroll
    for (int s = 0; s < NST; ++s) {
      // this stage landed: everything younger than it may still be in flight (G1L: the stage-1
      // DMA of this tile was issued after the previous tile's group-0 stores, not before them)
      // (group 0's old values issued after stage 0's wait are younger than stage 1's DMAs)
      const int young = s == 0   ? Dn1 + SP + 2
                        : s == 1 ? (G1L && SP > 0 ? SP - EF_CV / 2 : SP) + 2 + (G0S == 0 ? EF_CV / 2 : 0) + X[0]
                                 : X[s - 1];
      e2_vmcnt(young);
      asm volatile("s_barrier" ::: "memory");
      if (s == G0S) e2_load<0>(c, rc, rbl);  // column group 0's old values (PT2Q_EF2_G0_EARLY)
      const int sl = G1L ? (s + par) & 1 : s & 1;
      if constexpr ((PT2Q_EF2_KPROBE & 4) == 0) F.stage(lds0 + sl * E2_STAGE);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // every wave done with the slot
      uint8_t* slot = smem + sl * E2_STAGE;
      const uint32_t slot_lds = lds0 + sl * E2_STAGE;
      if (s + 2 < NST) {
        X[s] = e2_stage(a, e0, i0, s + 2, slot, slot_lds, vo, true);
      } else if (G1L && s == NST - 2) {
        e2_g1_dma(rc, rbl, slot);  // column group 1's old values into the slot stage 2 freed
        X[s] = EF_CV / 2;
      } else if (G1L) {
        X[s] = more ? e2_stage(an, en, in, 0, slot, slot_lds, vo, newB) : 0;
      } else if (more) {
        X[s] = e2_stage(an, en, in, s + 2 - NST, slot, slot_lds, vo, newB);
        if (s == NST - 1) Dn1 = X[s];
      } else {
        X[s] = 0;
      }
    }
    e2_vmcnt(X[NST - 1]);  // column group 0's old values landed (G1L: and group 1's, older)
    e2_sub<0>(c, F);
    if constexpr (!G1L) e2_load<1>(c, rc, rbl);  // before group 0's stores: waiting for it then leaves those in flight
    e2_store<0>(c, rc, rbs);
    if (P) {  // this tile's w-bar partials (the next block's SSR mean, DESIGN.md §3 CHUNK128)
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // red free (last readers done)
      ef_wbar_span<0, 16>(wrow, c, red);
    }
    if constexpr (G1L) {
      uint8_t* g1 = smem + par * E2_STAGE;  // stage 2's slot
      e2_g1_read(c, g1);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's chunks read: its DMAs may overwrite them
      Dn1 = more ? e2_stage(an, en, in, 1, g1, lds0 + par * E2_STAGE, vo, newB) : 0;
      par ^= 1;
    } else {
      e2_vmcnt(EF_CV / 2);  // group 1 landed (younger: group 0's stores)
    }
    e2_sub<1>(c, F);
    e2_store<1>(c, rc, rbs);
    if (P) {
      ef_wbar_span<16, 32>(wrow, c, red);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      ef_wbar_store(a0.n, prsrc(a), true, e0, i0, red);
    }
    SP = EF_CV + P;
    if (!more) break;
    t = tn;
    a = an;
    e0 = en;
    i0 = in;
    wrow[0] = nrow[0];
    wrow[1] = nrow[1];
  }
  PT2Q_EF2_CLK(1);
}

}  // namespace

// Wt[crow[e]][i] -= sum_k Ck[k][e] * Et[k][i] for e < nr, i < ldw (the padding columns of Wt
// beyond n are scratch), k < bs <= 128.  Wt has wt_rows rows of ldw floats.
int pt2q_launch_ef(const float* Ck, long ldk, const float* Et, float* Wt, long ldw, long wt_rows,
                   const int* crow, int nr, int bs, hipStream_t st, const Grp* grp, float* part, int n) {
  if (nr <= 0) return PT2Q_OK;
  const long wt_bytes = wt_rows * ldw * 4;
  const long part_bytes = part ? (long)ceil_div(nr, EF_T) * n * 4 : 0;
  if (bs <= 0 || bs > 4 * E2_KS || ldw % 4 || ldk % 4 || (uintptr_t)Ck % 16 || (uintptr_t)Et % 16 ||
      (uintptr_t)Wt % 16 || wt_bytes >= (long)EF_DROP || wt_rows > 65536)
    return PT2Q_E_UNSUPPORTED;
  if (part && (n <= 0 || n % 4 || n > ldw || (uintptr_t)part % 16 || part_bytes >= (long)EF_DROP))
    return PT2Q_E_UNSUPPORTED;
  EfArgs a{Ck, ldk, Et, Wt, ldw, crow, nr, bs, ceil_div(nr, EF_T), ceil_div(ldw, EF_T), 0,
           grp ? grp->ws : 0l, (int)grp_z(grp), part, n};
  a.ntile = a.te * a.ti;
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const int grid = std::min(a.ntile * a.nz, 2 * cus);  // two workgroups per CU
  if (bs <= 2 * E2_KS)
    hipLaunchKernelGGL(ef2_gemm_kernel<2>, dim3(grid), dim3(256), 0, st, a, wt_bytes, part_bytes);
  else
    hipLaunchKernelGGL(ef2_gemm_kernel<4>, dim3(grid), dim3(256), 0, st, a, wt_bytes, part_bytes);
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}
