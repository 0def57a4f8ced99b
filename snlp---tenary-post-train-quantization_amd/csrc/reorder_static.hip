// Static SSR reorder (reference reorder.py:15-33 and :64-104): column norms and normalisation
// for the cosine-similarity matrix, and the greedy column order on a given symmetric S.
// The Gram S = WnᵀWn and the row sums S·1 come from the existing launchers (gemm.hip, ssr.hip);
// the arithmetic contract of every step is DESIGN.md §3 "Static reorder".
#include "common.hpp"
#include "internal.hpp"

namespace {

template <typename T>
PT2Q_DEV float ld_f32(const T* p);
template <>
PT2Q_DEV float ld_f32<float>(const float* p) { return *p; }
template <>
PT2Q_DEV float ld_f32<_Float16>(const _Float16* p) { return (float)*p; }
template <>
PT2Q_DEV float ld_f32<uint16_t>(const uint16_t* p) { return __uint_as_float(((uint32_t)*p) << 16); }

// nrm[j] = clamp(sqrt(q_j), 1e-8), q_j the k-ascending fmaf(w_kj, w_kj, q) chain from +0 over the
// n rows: one thread per column, so adjacent lanes read adjacent columns of a row (coalesced).
// The chain is sequential by contract; CN_UNROLL rows of loads are in flight ahead of it.
constexpr int CN_UNROLL = 16;
template <typename T>
__global__ __launch_bounds__(64) void colnorm_kernel(const T* W, long ldw, int n, int m, float* nrm) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= m) return;
  const T* col = W + j;
  float q = 0.0f;
  int k = 0;
  for (; k + CN_UNROLL <= n; k += CN_UNROLL) {
    float v[CN_UNROLL];
#pragma unroll
    for (int u = 0; u < CN_UNROLL; ++u) v[u] = ld_f32<T>(col + (long)(k + u) * ldw);
#pragma unroll
    for (int u = 0; u < CN_UNROLL; ++u) q = fmaf(v[u], v[u], q);
  }
  for (; k < n; ++k) {
    const float v = ld_f32<T>(col + (long)k * ldw);
    q = fmaf(v, v, q);
  }
  nrm[j] = clampmin(sqrtf(q));
}

// Wn[k][j] = w_kj / nrm[j], one correctly rounded division; fp32 out, leading dimension ldn.
// Pad columns [m, ldn) of Wn are never read by the Gram and are left alone.
template <typename T>
__global__ __launch_bounds__(256) void normalize_kernel(const T* W, long ldw, int n, int m, const float* nrm,
                                                        float* Wn, long ldn) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const float nj = nrm[j];
  for (int k = blockIdx.y; k < n; k += gridDim.y) Wn[(long)k * ldn + j] = ld_f32<T>(W + (long)k * ldw + j) / nj;
}

// ---- greedy order

constexpr int GO_THREADS = 1024, GO_WAVES = GO_THREADS / 64;

// The order-preserving integer image of a score in the high word, ~index in the low word: a plain
// unsigned max picks the largest score and, among equal scores, the lowest index.  v + 0 folds
// -0 onto +0 (equal scores by the contract's comparison).  0 is no candidate: no key is 0.
PT2Q_DEV unsigned long long go_key(float v, int i) {
  const unsigned u = __float_as_uint(v + 0.0f);
  const unsigned img = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)img << 32) | (unsigned)~i;
}

template <int K>
PT2Q_DEV unsigned long long go_xor_lane(unsigned long long k) {
  const unsigned lo = __float_as_uint(xor_lane<K>(__uint_as_float((unsigned)k)));
  const unsigned hi = __float_as_uint(xor_lane<K>(__uint_as_float((unsigned)(k >> 32))));
  return ((unsigned long long)hi << 32) | lo;
}
PT2Q_DEV unsigned long long go_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// Max over the 16 lanes of a DPP row; every lane ends with it.
PT2Q_DEV unsigned long long go_max16(unsigned long long k) {
  k = go_max(k, go_xor_lane<8>(k));
  k = go_max(k, go_xor_lane<4>(k));
  k = go_max(k, go_xor_lane<2>(k));
  k = go_max(k, go_xor_lane<1>(k));
  return k;
}

// The greedy order of reorder.py:81-104 on a symmetric S with running sums: ONE workgroup of 1024
// threads, one launch, m steps.  Thread t owns columns t + 1024 q (q < Q) in registers: their
// running sums acc and a bit mask of the selected ones (bit q; columns >= m start selected, so a
// ragged m predicates and no thread leaves the loop).  A step adds row p of S (coalesced; row p
// is column p bit for bit), takes the masked maximum as a packed key, reduces it in the wave by
// cross-lane moves and across the 16 waves through LDS slots.  The slots are double-buffered:
// step t+1 writes the other buffer, and the buffer of step t is rewritten only behind the barrier
// of step t+1, which no wave passes before all have read step t -- one barrier per step.  The
// trip count and every barrier are workgroup-uniform; nothing waits on another workgroup.
template <int Q>
__global__ __launch_bounds__(GO_THREADS) void greedy_order_kernel(const float* S, long lds, int m,
                                                                  const float* rowsum, int64_t* perm,
                                                                  int64_t* inv_perm) {
  __shared__ unsigned long long slot[2][GO_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float acc[Q];
  unsigned sel = 0;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = tid + GO_THREADS * q;
    acc[q] = i < m ? rowsum[i] : 0.0f;  // step 0 scores the row sums
    if (i >= m) sel |= 1u << q;
  }
  for (int t = 0; t < m; ++t) {
    unsigned long long best = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (!(sel >> q & 1)) best = go_max(best, go_key(acc[q], tid + GO_THREADS * q));
    best = go_max(best, __shfl_xor(best, 32));
    best = go_max(best, __shfl_xor(best, 16));
    best = go_max16(best);
    if (lane == 0) slot[t & 1][wv] = best;
    __syncthreads();
    best = go_max16(slot[t & 1][lane & (GO_WAVES - 1)]);
    // every step has an unselected column < m, so best != 0 and p is in [0, m)
    const int p = (int)~(unsigned)best;
    if (tid == 0) {
      perm[t] = p;
      if (inv_perm) inv_perm[p] = t;
    }
    if (tid == (p & (GO_THREADS - 1))) sel |= 1u << (p >> 10);
    if (t + 1 == m) break;
    const float* row = S + (long)p * lds;
    float v[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i = tid + GO_THREADS * q;
      v[q] = i < m ? row[i] : 0.0f;
    }
    if (t == 0) {  // the running sums start from +0 after the row-sum step
#pragma unroll
      for (int q = 0; q < Q; ++q) acc[q] = 0.0f;
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = acc[q] + v[q];
  }
}

template <typename T>
int launch_colnorm_t(const T* W, long ldw, int n, int m, float* nrm, float* Wn, long ldn, hipStream_t st) {
  hipLaunchKernelGGL(colnorm_kernel<T>, dim3(ceil_div(m, 64)), dim3(64), 0, st, W, ldw, n, m, nrm);
  PT2Q_LAUNCH_CHECK();
  const int gy = n < 1024 ? n : 1024;
  hipLaunchKernelGGL(normalize_kernel<T>, dim3(ceil_div(m, 256), gy), dim3(256), 0, st, W, ldw, n, m, nrm, Wn,
                     ldn);
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}

}  // namespace

int pt2q_launch_colnorm_normalize(const void* W, int wdtype, long ldw, int n, int m, float* nrm, float* Wn,
                                  long ldn, hipStream_t st) {
  switch (wdtype) {
    case PT2Q_F32: return launch_colnorm_t((const float*)W, ldw, n, m, nrm, Wn, ldn, st);
    case PT2Q_F16: return launch_colnorm_t((const _Float16*)W, ldw, n, m, nrm, Wn, ldn, st);
    case PT2Q_BF16: return launch_colnorm_t((const uint16_t*)W, ldw, n, m, nrm, Wn, ldn, st);
    default: return PT2Q_E_ARG;
  }
}

int pt2q_launch_greedy_order(const float* S, long lds, int m, const float* rowsum, int64_t* perm,
                             int64_t* inv_perm, hipStream_t st) {
  if (m > PT2Q_STATIC_ORDER_MAX) return PT2Q_E_UNSUPPORTED;
  const int q = ceil_div(m, GO_THREADS);
#define PT2Q_GO_LAUNCH(Q)                                                                               \
  hipLaunchKernelGGL(greedy_order_kernel<Q>, dim3(1), dim3(GO_THREADS), 0, st, S, lds, m, rowsum, perm, \
                     inv_perm)
  if (q <= 1) PT2Q_GO_LAUNCH(1);
  else if (q <= 2) PT2Q_GO_LAUNCH(2);
  else if (q <= 4) PT2Q_GO_LAUNCH(4);
  else if (q <= 8) PT2Q_GO_LAUNCH(8);
  else if (q <= 12) PT2Q_GO_LAUNCH(12);
  else PT2Q_GO_LAUNCH(16);
#undef PT2Q_GO_LAUNCH
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}
