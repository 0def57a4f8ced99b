// S1 = S·1 and d = 1ᵀS1 of the AGA (quantizer.py:202-218).
//
// The contract, the same in every kernel here and in atq.hip's in-launch form:
//   S1[j] = the l-ascending sequential sum of S[j][l], d = the j-ascending sequential sum of S1[j]
// (s1_chain, common.hpp) -- the oracle's s1_from_gram and s1_from_hess_block.
//   variant M: S[j][l] = A[blk_j][blk_l], A = the raw Gram XᵀX (== X_bᵀX_b);
//   variant G: S = H_bbᵀ H_bb with H_bb = A[blk][:, blk] (t-ascending fmaf chains).
//
// Which entry reaches which kernel (pt2q_launch_s1 holds the table; b = block / Gram width):
//   the block loop's variant M blocks and pt2q_s1_from_gram (S1_BLOCK, optional block indices):
//     b <= 128 s1_fused_kernel; b <= 512 s1_row_wg_kernel; wider s1_rows_kernel (+ s1_total_kernel)
//     (blocks <= 128 inside the block loop: atq.hip forms S1 / d in the ATQ launch itself);
//   pt2q_s1_from_gram_batched, pt2q_ssr_static_order (S1_GRAMS, whole Grams, grid.y = item): the
//     same, but b > 512 takes s1_ring_kernel where its DMA conditions hold;
//   pt2q_s1_from_upper_batched (S1_UPPER_GRAMS): s1_upper_ring_kernel, b > 512 only;
//   variant G: b <= 128 s1_hess_block_kernel; wider pt2q_launch_s1_hess_wide (S on the f32 GEMM,
//     then the S1_BLOCK kernels on S).
#include "common.hpp"
#include "internal.hpp"

namespace {

// S1 / d of one b <= 128 block by one workgroup: every gather load of a thread is in flight before
// the first LDS store; gb >= b*(b+1) floats of LDS, s1 >= b floats of LDS, bl = the b indices in LDS.
PT2Q_DEV void s1_block(const float* A, long lda, const int* bl, int b, float* gb, float* s1,
                       float* S1, float* d) {
  const int tid = threadIdx.x, nt = blockDim.x, ld = b + 1, tot = b * b;
  for (int q0 = 0; q0 < tot; q0 += 16 * nt) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int q = q0 + u * nt + tid, qq = q < tot ? q : 0;
      v[u] = A[(long)bl[qq / b] * lda + bl[qq % b]];
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int q = q0 + u * nt + tid;
      if (q < tot) gb[(q / b) * ld + (q % b)] = v[u];
    }
  }
  __syncthreads();
  for (int j = tid; j < b; j += nt) S1[j] = s1[j] = s1_chain(gb + j * ld, b);
  __syncthreads();
  if (tid == 0) *d = s1_chain(s1, b);
}

// Single-kernel S1 / d for b <= 128 (raw Gram); item blockIdx.y (strides 0 for one item).
__global__ __launch_bounds__(1024) void s1_fused_kernel(const float* A, long lda, const int* blk,
                                                        int b, float* S1, float* d, long sA, long sS) {
  __shared__ float gb[128 * 129];
  __shared__ float s1[128];
  __shared__ int bl[128];
  A += blockIdx.y * sA;
  S1 += blockIdx.y * sS;
  d += blockIdx.y * sS;
  for (int j = threadIdx.x; j < b; j += blockDim.x) bl[j] = blk ? blk[j] : j;
  __syncthreads();
  s1_block(A, lda, bl, b, gb, s1, S1, d);
}

// Variant G, b <= 128 (wider blocks: pt2q_launch_s1_hess_wide): H_bb gathered into LDS, S in LDS.
__global__ __launch_bounds__(256) void s1_hess_block_kernel(const float* A, long lda, const int* blk,
                                                            int b, float* S1, float* d) {
  extern __shared__ float sm[];
  const int tid = threadIdx.x, ld = b + 1;
  float* s1 = sm;              // b
  float* hb = sm + b;          // b x (b+1)
  float* S = hb + b * ld;      // b x (b+1)
  for (int q = tid; q < b * b; q += blockDim.x) {
    int t = q / b, j = q % b;
    hb[t * ld + j] = A[(long)(blk ? blk[t] : t) * lda + (blk ? blk[j] : j)];
  }
  __syncthreads();
  for (int q = tid; q < b * b; q += blockDim.x) {
    int j = q / b, l = q % b;
    float acc = 0.0f;
    for (int t = 0; t < b; ++t) acc = fmaf(hb[t * ld + j], hb[t * ld + l], acc);
    S[j * ld + l] = acc;
  }
  __syncthreads();
  for (int j = tid; j < b; j += blockDim.x) S1[j] = s1[j] = s1_chain(S + j * ld, b);
  __syncthreads();
  if (tid == 0) *d = s1_chain(s1, b);
}

// Wide blocks (b > 512, per-channel): a workgroup owns S1W_ROWS rows j: all 256 threads stage a
// S1W_ROWS x S1W_COLS tile of them (coalesced along l) into one of two LDS buffers while lanes
// 0..S1W_ROWS-1 of wave 0 run their rows' serial chains over the other buffer, so the chains never
// wait on a global load and every load instruction reads whole rows segments (one thread per j
// striding over whole rows read 64 rows per instruction and ran 3.3 ms at b = 13824).
constexpr int S1W_ROWS = 32, S1W_COLS = 256;
__global__ __launch_bounds__(256) void s1_rows_kernel(const float* A, long lda, const int* blk,
                                                      int b, float* S1, long sA, long sS) {
  __shared__ float tile[2][S1W_ROWS][S1W_COLS + 1];
  A += blockIdx.y * sA;  // batched: item blockIdx.y (strides 0 for one item)
  S1 += blockIdx.y * sS;
  const int tid = threadIdx.x, j0 = blockIdx.x * S1W_ROWS;
  const int nj = min(S1W_ROWS, b - j0);
  auto stage = [&](int c, int buf) {  // columns [c, c + S1W_COLS) of the workgroup's rows
    const int l = c + tid;
    const int bl = l < b ? (blk ? blk[l] : l) : 0;
    float v[S1W_ROWS];
#pragma unroll
    for (int r = 0; r < S1W_ROWS; ++r) {
      const int j = j0 + (r < nj ? r : 0);
      v[r] = A[(long)(blk ? blk[j] : j) * lda + bl];
    }
#pragma unroll
    for (int r = 0; r < S1W_ROWS; ++r) tile[buf][r][tid] = v[r];
  };
  float s = 0.0f;
  stage(0, 0);
  __syncthreads();
  int buf = 0;
  for (int c = 0; c < b; c += S1W_COLS) {
    if (c + S1W_COLS < b) stage(c + S1W_COLS, buf ^ 1);
    if (tid < nj) s = s1_chain(tile[buf][tid], min(S1W_COLS, b - c), s);
    __syncthreads();
    buf ^= 1;
  }
  if (tid < nj) S1[j0 + tid] = s;
}

// Blocks up to 512 columns: one workgroup per row j gathers A[blk_j][blk_l] (all loads in
// flight at once), then one lane sums them.
__global__ __launch_bounds__(128) void s1_row_wg_kernel(const float* A, long lda, const int* blk,
                                                        int b, float* S1, long sA, long sS) {
  __shared__ float v[512];
  A += blockIdx.y * sA;
  S1 += blockIdx.y * sS;
  const int j = blockIdx.x;
  const float* row = A + (long)(blk ? blk[j] : j) * lda;
  for (int l = threadIdx.x; l < b; l += 128) v[l] = row[blk ? blk[l] : l];
  __syncthreads();
  if (threadIdx.x == 0) S1[j] = s1_chain(v, b);
}

// S1 of whole wide Grams (the batched per-channel S1 / d, m > 512; m % 4 == 0, 16-byte aligned
// rows): the same sequential row chains as s1_rows_kernel, fed by a wave-private LDS-DMA ring.
// s1_rows_kernel staged each tile by register loads whose LDS stores waited for them before the
// chains ran, one tile in flight per workgroup: ~3.5 TB/s, and a shard's few Grams could not
// hide the round trips (1.8 ms for the S1 phase of one rank's C5 shard).  Here a one-wave
// workgroup owns 64 rows (lane l: row r0 + l's chain) and DMAs them 32 columns per tile (8 KiB,
// 8 x 1 KiB global_load_lds_dwordx4) into an S1R_STAGES-deep LDS ring, S1R_STAGES - 1 tiles ahead,
// with no barrier.  32 KiB per workgroup: five share a CU, so a shard's 1,080 row groups of its
// m = 13824 Grams are resident at once (256-row workgroups left a second round of 14 on a few CUs,
// doubling the launch).  LDS layout: row rr at 128 rr bytes,
// its 16-byte chunk k at slot k ^ ((rr >> 1) & 7) -- the DMA lanes load the permuted chunks, so
// the chain lanes' ds_read_b128 of one chunk index hit 16 distinct bank groups per 16 lanes.
constexpr int S1R_COLS = 32, S1R_STAGES = 4, S1R_WROWS = 64;
constexpr int S1R_WSTAGE = S1R_WROWS * S1R_COLS * 4;  // 8 KiB per wave and stage

typedef float s1f4 __attribute__((ext_vector_type(4)));

template <int N>
PT2Q_DEV void s1r_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
PT2Q_DEV void s1r_vmcnt(int younger) {  // tiles still in flight after the one to read (x 8 DMAs)
  switch (younger) {
    case 0: s1r_vm<0>(); break;
    case 1: s1r_vm<8>(); break;
    case 2: s1r_vm<16>(); break;
    case 3: s1r_vm<24>(); break;
    default: s1r_vm<32>(); break;
  }
}

// The row tile (64 rows at row0, 32 columns) of both ring kernels.  DMA instruction q of a lane
// loads row rr = 8 q + lane / 8, chunk k = (lane % 8) ^ ((rr >> 1) & 7): s1r_chunk is that chunk's
// first column, src[q] its address at column tile 0 (rows past m read row 0, results dropped).
PT2Q_DEV int s1r_chunk(int q, int lane) { return 4 * ((lane & 7) ^ (((8 * q + (lane >> 3)) >> 1) & 7)); }
PT2Q_DEV void s1r_row_src(const float* G, long ldg, int m, int row0, int lane, const float* (&src)[8]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int rr = 8 * q + (lane >> 3);
    src[q] = G + (long)(row0 + rr < m ? row0 + rr : 0) * ldg + s1r_chunk(q, lane);
  }
}
// Issue the tile at columns c0 .. c0 + 31 into stage stg; chunks past m (only in the last tile;
// m % 4 == 0) read column 0 and are masked by s1r_own_row.
PT2Q_DEV void s1r_issue_rows(const float* const (&src)[8], int c0, int m, int lane, uint8_t* stg) {
  typedef __attribute__((address_space(3))) void* lptr;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int k4 = s1r_chunk(q, lane);
    __builtin_amdgcn_global_load_lds(c0 + k4 < m ? src[q] + c0 : src[q] - k4, (lptr)(stg + q * 1024), 16, 0, 0);
  }
}
// s continued over the lane's own row of a landed row tile (stage at LDS address st0), l ascending
PT2Q_DEV float s1r_own_row(uint32_t st0, int lane, int c0, int m, float s) {
  const uint32_t base = st0 + lane * 128;
  const int f = (lane >> 1) & 7;
  s1f4 x[8];
#pragma unroll
  for (int k = 0; k < 8; ++k)
    asm volatile("ds_read_b128 %0, %1" : "=v"(x[k]) : "v"(base + ((k ^ f) << 4)));
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])
               :: "memory");
  if (c0 + S1R_COLS <= m) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int u = 0; u < 4; ++u) s = s + x[k][u];
  } else {  // the last, partial tile: only the columns < m (whole chunks)
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (c0 + 4 * k < m)
#pragma unroll
        for (int u = 0; u < 4; ++u) s = s + x[k][u];
  }
  return s;
}

__global__ __launch_bounds__(64) void s1_ring_kernel(const float* G, long ldg, int m, float* S1, long sG, long sS) {
  __shared__ __attribute__((aligned(1024))) uint8_t ring[S1R_STAGES * S1R_WSTAGE];
  const int lane = threadIdx.x & 63;
  G += blockIdx.y * sG;
  S1 += blockIdx.y * sS;
  const int r0 = blockIdx.x * S1R_WROWS;
  const uint32_t wlds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)ring;
  const int ntile = (m + S1R_COLS - 1) / S1R_COLS;
  const float* src[8];
  s1r_row_src(G, ldg, m, r0, lane, src);
  auto issue = [&](int t) { s1r_issue_rows(src, t * S1R_COLS, m, lane, ring + (t % S1R_STAGES) * S1R_WSTAGE); };
  const int pre = ntile < S1R_STAGES - 1 ? ntile : S1R_STAGES - 1;
  for (int t = 0; t < pre; ++t) issue(t);
  float s = 0.0f;
  for (int t = 0; t < ntile; ++t) {
    if (t + S1R_STAGES - 1 < ntile) issue(t + S1R_STAGES - 1);
    const int ahead = ntile - 1 - t;  // tiles issued after tile t
    s1r_vmcnt(ahead < S1R_STAGES - 1 ? ahead : S1R_STAGES - 1);
    s = s1r_own_row(wlds + (t % S1R_STAGES) * S1R_WSTAGE, lane, t * S1R_COLS, m, s);
  }
  if (r0 + lane < m) S1[r0 + lane] = s;
}

// S1 of UPPER-only Grams (G[r][c] stored for c >= r only: pt2q_gram_batched_upper): row j's chain
// takes G[l][j] for l < j and G[j][l] for l >= j, l ascending -- on a Gram whose mirror is an
// exact copy these are s1_ring_kernel's values in s1_ring_kernel's order, so S1 is bit-identical.
// A one-wave workgroup owns rows j0 .. j0 + 63 (lane: row j = j0 + lane) and streams 8 KiB tiles
// through the same four-stage LDS-DMA ring:
//  * column tiles t < nA = j0 / 32: G rows l = 32 t .. 32 t + 31, columns j0 .. j0 + 63 (natural
//    layout, 256 B per row; 16 lanes x 16 B per row in a DMA): lane j reads its column, l < j;
//  * row tiles u = t - nA: rows j0 .. j0 + 63, columns j0 + 32 u .. + 31 (s1_ring_kernel's
//    swizzled layout): lane j reads its own row, l >= j -- except in the two diagonal tiles
//    (u = 0, 1), where l < j reads element (l, j) of the tile holding column j (both resident).
__global__ __launch_bounds__(64) void s1_upper_ring_kernel(const float* G, long ldg, int m, float* S1, long sG,
                                                           long sS) {
  __shared__ __attribute__((aligned(1024))) uint8_t ring[S1R_STAGES * S1R_WSTAGE];
  typedef __attribute__((address_space(3))) void* lptr;
  const int lane = threadIdx.x & 63;
  G += blockIdx.y * sG;
  S1 += blockIdx.y * sS;
  const int j0 = blockIdx.x * S1R_WROWS;
  const int j = j0 + lane;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)ring;
  const int nA = j0 / S1R_COLS, nC = (m - j0 + S1R_COLS - 1) / S1R_COLS, ntile = nA + nC;
  auto issue = [&](int t) {
    uint8_t* stg = ring + (t % S1R_STAGES) * S1R_WSTAGE;
    if (t < nA) {  // rows 32 t + 4 q + lane / 16, 16-byte chunk lane % 16 of columns j0 ..
      const int col = j0 + 4 * (lane & 15);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int row = S1R_COLS * t + 4 * q + (lane >> 4);
        __builtin_amdgcn_global_load_lds(G + (long)row * ldg + (col < m ? col : 0), (lptr)(stg + q * 1024), 16, 0, 0);
      }
    } else {  // the row tile at columns j0 + 32 (t - nA)
      const float* src[8];
      s1r_row_src(G, ldg, m, j0, lane, src);
      s1r_issue_rows(src, j0 + S1R_COLS * (t - nA), m, lane, stg);
    }
  };
  const int pre = ntile < S1R_STAGES - 1 ? ntile : S1R_STAGES - 1;
  for (int t = 0; t < pre; ++t) issue(t);
  const int f = (lane >> 1) & 7;
  float s = 0.0f;
  for (int t = 0; t < ntile; ++t) {
    if (t + S1R_STAGES - 1 < ntile) issue(t + S1R_STAGES - 1);
    // this tile landed -- and at the first diagonal tile the second one too
    const int need = (t == nA && nC > 1) ? t + 1 : t;
    const int ahead = ntile - 1 - need;
    s1r_vmcnt(ahead < S1R_STAGES - 1 - (need - t) ? ahead : S1R_STAGES - 1 - (need - t));
    const uint32_t st0 = lds0 + (t % S1R_STAGES) * S1R_WSTAGE;
    if (t < nA) {  // column tile: l = 32 t + r < j0 <= j
      float x[S1R_COLS];
#pragma unroll
      for (int r = 0; r < S1R_COLS; ++r)
        asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(x[r]) : "v"(st0 + 4 * lane), "i"(256 * r));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < S1R_COLS; ++r) s = s + x[r];
      continue;
    }
    const int u = t - nA;
    const int c0 = j0 + S1R_COLS * u;
    if (u >= 2) {  // own row only (l >= j0 + 64 > j)
      s = s1r_own_row(st0, lane, c0, m, s);
      continue;
    }
    // diagonal tile u (l = c0 + c): l < j -> element (l, j) of the tile holding column j; else
    // element (j, l) of this tile (own row)
    const int uj = lane >> 5, cj = lane & 31;  // column j's tile (0 / 1) and column in it
    const uint32_t colj = lds0 + ((nA + uj) % S1R_STAGES) * S1R_WSTAGE + (uint32_t)((cj & 3) << 2);
    float x[S1R_COLS];
#pragma unroll
    for (int c = 0; c < S1R_COLS; ++c) {
      const int l = c0 + c, rr = l - j0;  // row of the diagonal block
      const uint32_t a_col = colj + rr * 128 + ((((cj >> 2) ^ ((rr >> 1) & 7))) << 4);
      const uint32_t a_row = st0 + lane * 128 + ((((c >> 2) ^ f)) << 4) + ((c & 3) << 2);
      asm volatile("ds_read_b32 %0, %1" : "=v"(x[c]) : "v"(l < j ? a_col : a_row));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < S1R_COLS; ++c)
      if (c0 + c < m) s = s + x[c];
  }
  if (j < m) S1[j] = s;
}

// d = sequential sum of S1 (j ascending); S1 is staged through LDS in chunks so the serial
// chain never waits on a global load.  Its own schedule on purpose (b reaches 13824 on one lane).
__global__ __launch_bounds__(256) void s1_total_kernel(const float* S1, int b, float* d, long sS, long sD) {
  __shared__ float v[4096];
  S1 += blockIdx.x * sS;  // batched: item blockIdx.x (strides 0 for one item)
  d += blockIdx.x * sD;
  float dd = 0.0f;
  for (int j0 = 0; j0 < b; j0 += 4096) {
    const int len = min(4096, b - j0);
    __syncthreads();
    for (int j = threadIdx.x; j < len; j += 256) v[j] = S1[j0 + j];
    __syncthreads();
    if (threadIdx.x == 0) {
      // the next 16 values are read while the current 16 are added (the chain never waits on LDS)
      int j = 0;
      if (len >= 16) {
        float t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) t[u] = v[u];
        for (; j + 32 <= len; j += 16) {
          float nx[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) nx[u] = v[j + 16 + u];
#pragma unroll
          for (int u = 0; u < 16; ++u) dd = dd + t[u];
#pragma unroll
          for (int u = 0; u < 16; ++u) t[u] = nx[u];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) dd = dd + t[u];
        j += 16;
      }
      for (; j < len; ++j) dd = dd + v[j];
    }
  }
  if (threadIdx.x == 0) *d = dd;
}

// hb[t][j] = A[blk[t]][blk[j]] (bs x bs, ld bs): variant G's X_block = H[blk][:, blk] (gptq.py:147)
__global__ void gather_block_kernel(const float* A, long lda, const int* blk, int bs, float* hb) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
  if (j < bs) hb[(long)t * bs + j] = A[(long)blk[t] * lda + blk[j]];
}

}  // namespace

// The one size-to-kernel table (header comment).  Item z of `batch` at A + z * sA,
// its S1 / d at S1 / d + z * sS.  The ring kernels need 16-byte rows in every item.
int pt2q_launch_s1(const float* A, long lda, const int* blk, int b, float* S1, float* d, hipStream_t st,
                   int batch, long sA, long sS, int kind) {
  const bool ring = b > 512 && b % 4 == 0 && lda % 4 == 0 && sA % 4 == 0 && ((uintptr_t)A & 15) == 0;
  if (kind == S1_UPPER_GRAMS && !ring) return PT2Q_E_UNSUPPORTED;
  if (b <= 128) {
    hipLaunchKernelGGL(s1_fused_kernel, dim3(1, batch), dim3(1024), 0, st, A, lda, blk, b, S1, d, sA, sS);
    PT2Q_LAUNCH_CHECK();
    return PT2Q_OK;
  }
  if (kind == S1_UPPER_GRAMS)
    hipLaunchKernelGGL(s1_upper_ring_kernel, dim3(ceil_div(b, S1R_WROWS), batch), dim3(64), 0, st, A, lda, b, S1, sA,
                       sS);
  else if (kind == S1_GRAMS && ring)
    hipLaunchKernelGGL(s1_ring_kernel, dim3(ceil_div(b, S1R_WROWS), batch), dim3(64), 0, st, A, lda, b, S1, sA, sS);
  else if (b > 512)
    hipLaunchKernelGGL(s1_rows_kernel, dim3(ceil_div(b, S1W_ROWS), batch), dim3(256), 0, st, A, lda, blk, b, S1, sA,
                       sS);
  else
    hipLaunchKernelGGL(s1_row_wg_kernel, dim3(b, batch), dim3(128), 0, st, A, lda, blk, b, S1, sA, sS);
  PT2Q_LAUNCH_CHECK();
  hipLaunchKernelGGL(s1_total_kernel, dim3(batch), dim3(256), 0, st, S1, b, d, sS, sS);
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}

int pt2q_launch_s1_hess_block(const float* A, long lda, const int* blk, int b, float* S1, float* d,
                              hipStream_t st) {
  const size_t lds = ((size_t)b + 2 * (size_t)b * (b + 1)) * sizeof(float);
  if (lds > 160 * 1024) return PT2Q_E_UNSUPPORTED;
  hipLaunchKernelGGL(s1_hess_block_kernel, dim3(1), dim3(256), lds, st, A, lda, blk, b, S1, d);
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}

// S1 = (H_bbᵀH_bb)·1, d = 1ᵀS1 for blocks > 128 columns (quantizer.py:202-218 with X = H_bb):
// S on the f32 MFMA GEMM (t-ascending fmaf chains, as s1_hess_block_kernel's), then the row sums
// in l order and d in j order (the S1_BLOCK kernels on S itself).  hb, hS: bs x bs floats each.
int pt2q_launch_s1_hess_wide(const float* A, long lda, const int* blk, int bs, float* hb, float* hS, float* S1,
                             float* d, hipStream_t st) {
  hipLaunchKernelGGL(gather_block_kernel, dim3(ceil_div(bs, 256), bs), dim3(256), 0, st, A, lda, blk, bs, hb);
  PT2Q_LAUNCH_CHECK();
  GemmDesc g{};
  g.M = bs; g.N = bs; g.K = bs;
  g.A = hb; g.lda = bs; g.a_layout = LAY_KMAJOR;  // (j, t) = hb[t][j]
  g.B = hb; g.ldb = bs; g.b_layout = LAY_KMAJOR;  // (t, l) = hb[t][l]
  g.in_dtype = PT2Q_F32;
  g.C = hS; g.ldc = bs;
  g.mode = GEMM_STORE;
  int rc = pt2q_launch_gemm(g, st);
  if (rc != PT2Q_OK) return rc;
  return pt2q_launch_s1(hS, bs, nullptr, bs, S1, d, st);
}
