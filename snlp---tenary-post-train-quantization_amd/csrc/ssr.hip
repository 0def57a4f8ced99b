// SSR (structural-similarity reordering) block selection and the error-feedback coefficients.
//
// Reference: reorder.py:36-61 (compute_column_similarity_to_mean), reorder.py:107-143
// (select_next_block_ssr), main.py:176-177 / gptq.py:142-150 (block operands),
// main.py:199-209 (coefficients Hinv[blk][:,rem] / diag).
//
// Weights live feature-major (Wt[j] = column j of W, contiguous over the n rows), so every
// "column" gather of the reference is a gather of whole contiguous rows here.
#include "common.hpp"
#include "internal.hpp"
#include "probe.hpp"

namespace {

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

constexpr int CHUNK = 128;  // canonical wbar chunk (rem entries per partial sum)

// Leaf k of the CHUNK128 half tree: bfly16 over l in [0, 16) (leaves in 4-bit bit-reversed
// order), then the same over [16, 32), the two sums added.
PT2Q_DEV constexpr int brev5(int k) {
  return (k & 16) | ((k & 1) << 3) | ((k & 2) << 1) | ((k & 4) >> 1) | ((k & 8) >> 3);
}

// Half of a chunk's w-bar partial (DESIGN.md §3 CHUNK128): x_l = v[o+l] + v[o+l+32] (l < 32),
// bfly16(x[0..16)) + bfly16(x[16..32)), evaluated as a pairwise stack over the leaves in the
// tree's order, 8 leaves' loads in flight at a time.  ld(j) = v[j] (zero past the chunk's end).
template <typename V, typename LD>
PT2Q_DEV V wbar_half(LD&& ld, int o) {
  V acc[6];
#pragma unroll
  for (int k0 = 0; k0 < 32; k0 += 8) {
    V a[8], b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      a[u] = ld(o + brev5(k0 + u));
      b[u] = ld(o + brev5(k0 + u) + 32);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k0 + u;
      V v = a[u] + b[u];
      int lvl = 0;
#pragma unroll
      for (; lvl < 5 && ((k >> lvl) & 1); ++lvl) v = acc[lvl] + v;
      acc[lvl] = v;
    }
  }
  return acc[5];
}

// The w-bar partial of one chunk: X + Y (X over entries 0..63, Y over 64..127) -- the order the
// error-feedback tile that last wrote these columns forms it in (ef.hip), oracle orc_wbar_chunk.
template <typename V, typename LD>
PT2Q_DEV V wbar_chunk(LD&& ld) {
  const V x = wbar_half<V>(ld, 0);
  return x + wbar_half<V>(ld, 64);
}

// part[c][i] = wbar_chunk over rem[c*128 .. c*128+127] of Wt[rem[e]][i]
__global__ __launch_bounds__(256) void ssr_wbar_partial_kernel(const float* Wt, long ldw, int n,
                                                               const int* rem, int r,
                                                               float* part) {
  __shared__ long rows[CHUNK];
  const int c = blockIdx.x;
  const int e0 = c * CHUNK, cnt = min(r, e0 + CHUNK) - e0;
  for (int e = threadIdx.x; e < cnt; e += blockDim.x) rows[e] = (long)rem[e0 + e] * ldw;
  __syncthreads();
  const int i = blockIdx.y * 256 + threadIdx.x;
  if (i >= n) return;
  part[(long)c * n + i] = wbar_chunk<float>([&](int j) { return j < cnt ? Wt[rows[j] + i] : 0.0f; });
}

// The three wbar steps in one launch (n <= 16384, n % 4 == 0): every workgroup (one wave: 256
// rows i, four per lane, so the reads spread over every CU) forms its partial
// part[c][i] as ssr_wbar_partial_kernel; the last workgroup to finish a 256-row slice sums that
// slice's partials in chunk order (wbar = sum / r); the last slice to finish forms
// nw = clamp(sqrt(SUMN fma wbar^2)) and wn = wbar / nw.  Hand-offs: write-through (sc1) stores,
// drained by every storing wave before the barrier that precedes the counter add, and sc1 loads
// on the consuming side (no fences).  cnt: nslices + 1 ints, zero before the first launch; the
// last arrivers put them back to zero.
__global__ __launch_bounds__(256) void ssr_wbar_fused_kernel(const float* Wt, long ldw, int n,
                                                             const int* rem, int r, float* part,
                                                             float* wn, int* cnt, long zs, int pre) {
  __shared__ long rows[CHUNK];
  Wt = zws(Wt, zs);  // grouped launch: linear blockIdx.z's slice
  rem = zws(rem, zs);
  part = zws(part, zs);
  wn = zws(wn, zs);
  cnt = zws(cnt, zs);
  __shared__ int last;
  const int c = blockIdx.x, nchunks = (r + CHUNK - 1) / CHUNK, nsl = gridDim.y;
  const int e0 = c * CHUNK, ce = min(r, e0 + CHUNK) - e0;
  if (!pre) {
    for (int e = threadIdx.x; e < ce; e += blockDim.x) rows[e] = (long)rem[e0 + e] * ldw;
    __syncthreads();
  }
  // four consecutive rows i per thread (float4; n % 4 == 0), each its own chain over e
  typedef float f4 __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(part, 0, nchunks * n * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(wn, 0, n * 4, 0x00020000);
  const int i = (blockIdx.y * blockDim.x + threadIdx.x) * 4;
  if (!pre) {  // (pre: the partials came from the error feedback that wrote these columns)
    if (i < n) {
      const f4 z = {0.0f, 0.0f, 0.0f, 0.0f};
      const f4 p = wbar_chunk<f4>([&](int j) { return j < ce ? *(const f4*)(Wt + rows[j] + i) : z; });
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, p), rp, (c * n + i) * 4, 0, 16);  // sc1
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(cnt + blockIdx.y, 1) == nchunks - 1;
    __syncthreads();
    if (!last) return;
  }
  if (i < n) {
    f4 t = {0.0f, 0.0f, 0.0f, 0.0f};
    int k = 0;
    for (; k + 8 <= nchunks; k += 8) {
      f4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rp, ((k + u) * n + i) * 4, 0, 16));
#pragma unroll
      for (int u = 0; u < 8; ++u) t = t + v[u];
    }
    for (; k < nchunks; ++k) t = t + __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rp, (k * n + i) * 4, 0, 16));
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, t / (float)r), rw, i * 4, 0, 16);  // sc1
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_store(cnt + blockIdx.y, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = atomicAdd(cnt + nsl, 1) == nsl - 1;
  }
  __syncthreads();
  if (!last) return;
  if (threadIdx.x >= 64) return;
  // wave 0: lane t takes elements {256u + 4t + q} (sumn_lane's order), 16 float4 in flight;
  // a second pass writes wn = wbar / nw (loads past n return zero, stores past n are dropped)
  const __amdgpu_buffer_rsrc_t rs = rw;
  const int t = threadIdx.x;
  float q = 0.0f;
  for (int u0 = 0; u0 < n; u0 += 4096) {
    f4 v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u)
      v[u] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, (u0 + 4 * t + 256 * u) * 4, 0, 16));
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (u0 + 4 * t + 256 * u < n) {
        q = fmaf(v[u][0], v[u][0], q);
        q = fmaf(v[u][1], v[u][1], q);
        q = fmaf(v[u][2], v[u][2], q);
        q = fmaf(v[u][3], v[u][3], q);
      }
  }
  const float nw = clampmin(sqrtf(bfly64(q)));
  for (int u0 = 0; u0 < n; u0 += 4096) {
    f4 v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u)
      v[u] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, (u0 + 4 * t + 256 * u) * 4, 0, 16));
#pragma unroll
    for (int u = 0; u < 16; ++u)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v[u] / nw), rs,
                                             (u0 + 4 * t + 256 * u) * 4, 0, 0);
  }
  if (t == 0) __hip_atomic_store(cnt + nsl, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// wbar[i] = (chunk partials summed in chunk order) / r
__global__ __launch_bounds__(256) void ssr_wbar_sum_kernel(const float* part, int nchunks, int n,
                                                           int r, float* wbar) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float t = 0.0f;
  for (int c = 0; c < nchunks; ++c) t = t + part[(long)c * n + i];
  wbar[i] = t / (float)r;
}

// wbar[i] = (chunk partials summed in chunk order) / r, then nw = clamp(sqrt(SUMN fma wbar^2))
// and wn = wbar / nw -- one workgroup, n <= SUMN_LDS_MAX (ssr_wbar_sum + ssr_wbar_final fused)
__global__ __launch_bounds__(1024) void ssr_wbar_sumfinal_kernel(const float* part, int nchunks,
                                                                 int n, int r, float* wn) {
  __shared__ float nws, tot;
  __shared__ float stage[SUMN_LDS_MAX];
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    float t = 0.0f;
    int c = 0;
    for (; c + 8 <= nchunks; c += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[(long)(c + u) * n + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) t = t + v[u];
    }
    for (; c < nchunks; ++c) t = t + part[(long)c * n + i];
    stage[i] = t / (float)r;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    float p = sumn_lane<true>(stage, n, 1, threadIdx.x);
    p = bfly64(p);
    if (threadIdx.x == 0) nws = clampmin(sqrtf(p));
  }
  __syncthreads();
  const float nw = nws;
  for (int i = threadIdx.x; i < n; i += blockDim.x) wn[i] = stage[i] / nw;
  (void)tot;
}

// nw = clamp(sqrt(SUMN fma wbar^2)) ; wn = wbar / nw   (in place)
__global__ __launch_bounds__(1024) void ssr_wbar_final_kernel(float* wn, int n) {
  __shared__ float nws, tot;
  __shared__ float stage[SUMN_LDS_MAX];
  if (n <= SUMN_LDS_MAX) {
    const float p = block_sumn_lds<true>(wn, n, 1, stage, &tot);
    if (threadIdx.x == 0) nws = clampmin(sqrtf(p));
  } else if (threadIdx.x < 64) {
    float p = sumn_lane<true>(wn, n, 1, threadIdx.x);
    p = bfly64(p);
    if (threadIdx.x == 0) nws = clampmin(sqrtf(p));
  }
  __syncthreads();
  const float nw = nws;
  for (int i = threadIdx.x; i < n; i += blockDim.x) wn[i] = wn[i] / nw;
}

// RN(x / nj) from one correctly rounded reciprocal y = RN(1 / nj) (Markstein): with r = x - nj q
// exact (fma), RN(q + r y) = RN(x / nj) whenever q is within one ulp of x / nj and nothing
// underflows.  q0 = RN(x y) can be 1.5 ulp off, so one correction first brings it within
// 0.5 ulp + 2^-23 ulp, and the second is exact.  No underflow: every nonzero |x| >= 2^-80 and
// nj in [1e-8, 2^40] (nj >= |x|: the clamped norm of the column holding x), so |q| >= 2^-120 is
// normal and r (about 2^-24 |x|) is too.  x = 0 gives a zero quotient (its sign may differ from
// the division's: q0 = -0, the corrections +0), and a signed zero cannot change the similarity
// chain p = fma(q, w, p) -- p starts at +0 and an exactly-zero fma result is -0 only if both
// addends are, so p is never -0 and fma(+-0, w, p) = p.  A column with a nonzero |x| < 2^-80 or
// a norm above 2^40 takes the division (wave-uniform branch).  5 VALU instead of the division's
// scaled Newton sequence; pinned against the division by orc_fp_rule_mismatches (rule 1).
constexpr float RCP_X_MIN = 0x1p-80f, RCP_NJ_MAX = 0x1p40f;
PT2Q_DEV float div_rcp(float x, float nj, float y) {
  const float q0 = x * y;
  const float q1 = fmaf(fmaf(-nj, q0, x), y, q0);
  return fmaf(fmaf(-nj, q1, x), y, q1);
}
PT2Q_DEV bool rcp_column_ok(float minabs, float nj) { return minabs >= RCP_X_MIN && nj <= RCP_NJ_MAX; }
// The gate's re-check when a lane's min |x| failed it: the smallest NONZERO |x| of its registers
// (zeros -- pruned or padded weights -- keep the fast path; rare, so off the common path).
template <int U, typename V>
PT2Q_DEV float min_nonzero_abs(const V (&v)[U], int n, int t, int u0) {
  float mz = 0x1p64f;
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (4 * t + 256 * (u0 + u) < n) {
#pragma unroll
      for (int q = 0; q < 4; ++q) mz = fminf(mz, v[u][q] == 0.0f ? 0x1p64f : fabsf(v[u][q]));
    }
  return mz;
}

// One wave per remaining column: nj = clamp(sqrt(SUMN fma x^2)); s = SUMN fma (x/nj) * wn.
// NV > 0 (n % 4 == 0, n <= 256 NV): one pass over the column, its NV float4 per lane kept in
// registers for both chains; NV == 0: the generic two-pass paths.
template <int NV>
__global__ __launch_bounds__(256) void ssr_sim_kernel(const float* Wt, long ldw, int n,
                                                      const int* rem, int r, const float* wn,
                                                      float* sim, long zs) {
  Wt = zws(Wt, zs);  // grouped launch: linear blockIdx.z's slice
  rem = zws(rem, zs);
  wn = zws(wn, zs);
  sim = zws(sim, zs);
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int t = threadIdx.x & 63;
  if (e >= r) return;
  const float* x = Wt + (long)rem[e] * ldw;
  float p = 0.0f;
  typedef float f4 __attribute__((ext_vector_type(4)));
  if constexpr (NV > 0) {
    // NV <= 16: the column and the (shared, L2-resident) mean vector are both loaded up front, so
    // the dot pass does not wait a second L2 round trip after the norm (NV = 48 keeps the mean's
    // loads in the dot loop: 256 VGPRs)
    constexpr bool PRE = NV <= 16;
    f4 v[NV], w[PRE ? NV : 1];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const long base = 4 * t + 256 * u;
      if (base < n) v[u] = *(const f4*)(x + base);
    }
    if constexpr (PRE) {
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const long base = 4 * t + 256 * u;
        if (base < n) w[u] = *(const f4*)(wn + base);
      }
    }
    float ss = 0.0f, mn = 0x1p64f;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      if (4 * t + 256 * u < n) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          ss = fmaf(v[u][q], v[u][q], ss);
          mn = fminf(mn, fabsf(v[u][q]));
        }
      }
    }
    const float nj = clampmin(sqrtf(bfly64(ss)));
    bool fast = __all(rcp_column_ok(mn, nj));
    if (!fast && nj <= RCP_NJ_MAX) fast = __all(min_nonzero_abs(v, n, t, 0) >= RCP_X_MIN);
    if (fast) {
      const float y = 1.0f / nj;
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const long base = 4 * t + 256 * u;
        if (base < n) {
          const f4 wu = PRE ? w[PRE ? u : 0] : *(const f4*)(wn + base);
#pragma unroll
          for (int q = 0; q < 4; ++q) p = fmaf(div_rcp(v[u][q], nj, y), wu[q], p);
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const long base = 4 * t + 256 * u;
        if (base < n) {
          const f4 wu = PRE ? w[PRE ? u : 0] : *(const f4*)(wn + base);
#pragma unroll
          for (int q = 0; q < 4; ++q) p = fmaf(v[u][q] / nj, wu[q], p);
        }
      }
    }
  } else if ((n & 3) == 0 && (ldw & 3) == 0) {
    // float4 path (same per-lane element order {256u + 4t + q})
    float ss = 0.0f;
    for (long base = 4 * t; base < n; base += 256) {
      f4 v = *(const f4*)(x + base);
      ss = fmaf(v[0], v[0], ss);
      ss = fmaf(v[1], v[1], ss);
      ss = fmaf(v[2], v[2], ss);
      ss = fmaf(v[3], v[3], ss);
    }
    const float nj = clampmin(sqrtf(bfly64(ss)));
    for (long base = 4 * t; base < n; base += 256) {
      f4 v = *(const f4*)(x + base);
      f4 w = *(const f4*)(wn + base);
      p = fmaf(v[0] / nj, w[0], p);
      p = fmaf(v[1] / nj, w[1], p);
      p = fmaf(v[2] / nj, w[2], p);
      p = fmaf(v[3] / nj, w[3], p);
    }
  } else {
    float ss = bfly64(sumn_lane<true>(x, n, 1, t));
    const float nj = clampmin(sqrtf(ss));
    for (long base = 4 * t; base < n; base += 256) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        long i = base + q;
        if (i < n) p = fmaf(x[i] / nj, wn[i], p);
      }
    }
  }
  p = bfly64(p);
  if (t == 0) sim[e] = p;
}

// Columns of 4096 < n <= 16384 rows (n % 4 == 0): S = ceil(n / 4096) waves per column, wave s
// holding the float4s u in [16 s, 16 s + 16) of lane t (elements {256u + 4t + q}) in registers,
// so the whole column is loaded at once with 16 float4 per lane (~110 VGPRs: 4 waves per SIMD,
// where one wave holding all 48 needs 256 VGPRs and runs alone on its SIMD).  Each lane's chain
// continues across the waves in s order through LDS -- the per-lane order of ssr_sim_kernel<48>
// -- and wave S-1 folds it (bfly64): the same bits.
template <int S>
__global__ __launch_bounds__(64 * S) void ssr_sim_split_kernel(const float* Wt, long ldw, int n, const int* rem,
                                                               int r, const float* wn, float* sim, long zs) {
  __shared__ float part[64];
  __shared__ float njs;
  __shared__ bool okw[S];
  Wt = zws(Wt, zs);
  rem = zws(rem, zs);
  wn = zws(wn, zs);
  sim = zws(sim, zs);
  const int e = blockIdx.x;
  const int s = threadIdx.x >> 6, t = threadIdx.x & 63;
  const float* x = Wt + (long)rem[e] * ldw;
  typedef float f4 __attribute__((ext_vector_type(4)));
  f4 v[16], w[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const long base = 4 * t + 256 * (16 * s + u);
    if (base < n) v[u] = *(const f4*)(x + base);
  }
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const long base = 4 * t + 256 * (16 * s + u);
    if (base < n) w[u] = *(const f4*)(wn + base);
  }
  float ss = 0.0f, mn = 0x1p64f;
#pragma unroll
  for (int u = 0; u < 16; ++u)
    if (4 * t + 256 * (16 * s + u) < n) {
#pragma unroll
      for (int q = 0; q < 4; ++q) mn = fminf(mn, fabsf(v[u][q]));
    }
  for (int q = 0; q < S; ++q) {
    if (s == q) {
      if (q > 0) ss = part[t];
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (4 * t + 256 * (16 * s + u) < n) {
          ss = fmaf(v[u][0], v[u][0], ss);
          ss = fmaf(v[u][1], v[u][1], ss);
          ss = fmaf(v[u][2], v[u][2], ss);
          ss = fmaf(v[u][3], v[u][3], ss);
        }
      if (q < S - 1) part[t] = ss;
    }
    __syncthreads();
  }
  bool wave_ok = __all(mn >= RCP_X_MIN);
  if (!wave_ok) wave_ok = __all(min_nonzero_abs(v, n, t, 16 * s) >= RCP_X_MIN);
  if (t == 0) okw[s] = wave_ok;
  if (s == S - 1) {
    const float tot = bfly64(ss);
    if (t == 0) njs = clampmin(sqrtf(tot));
  }
  __syncthreads();
  const float nj = njs;
  bool fast = nj <= RCP_NJ_MAX;
  for (int q = 0; q < S; ++q) fast = fast && okw[q];  // workgroup-uniform
  // chain p = fma(x / nj, w, p) over this wave's elements, continued across the waves in order.
  float p = 0.0f;
  if (fast) {  // workgroup-uniform
    // the quotients in place first, every wave at once: only the chain is serial over the waves
    const float y = 1.0f / nj;
#pragma unroll
    for (int u = 0; u < 16; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) v[u][c] = div_rcp(v[u][c], nj, y);
    for (int q = 0; q < S; ++q) {
      if (s == q) {
        if (q > 0) p = part[t];
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (4 * t + 256 * (16 * s + u) < n) {
#pragma unroll
            for (int c = 0; c < 4; ++c) p = fmaf(v[u][c], w[u][c], p);
          }
        if (q < S - 1) part[t] = p;
      }
      __syncthreads();
    }
  } else {
    // the division (rare columns): a rolled loop re-reading the column and the mean (L2 hits),
    // so its register image stays small -- unrolled beside the fast path, the two need 200 VGPRs
    // (two waves per SIMD instead of three)
    for (int q = 0; q < S; ++q) {
      if (s == q) {
        if (q > 0) p = part[t];
#pragma unroll 1
        for (int u = 0; u < 16; ++u) {
          const long base = 4 * t + 256 * (16 * s + u);
          if (base < n) {
            const f4 xv = *(const f4*)(x + base), wv = *(const f4*)(wn + base);
#pragma unroll
            for (int c = 0; c < 4; ++c) p = fmaf(xv[c] / nj, wv[c], p);
          }
        }
        if (q < S - 1) part[t] = p;
      }
      __syncthreads();
    }
  }
  if (s == S - 1) {
    p = bfly64(p);
    if (t == 0) sim[e] = p;
  }
}

PT2Q_DEV uint32_t orderable(float f) {
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

PT2Q_DEV int wave_incl_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(v, off);
    if (lane >= off) v += y;
  }
  return v;
}

// Exclusive workgroup scan of v (blockDim.x <= 4096); sc >= 65 ints of LDS.  *total = sum.
PT2Q_DEV int block_excl_scan(int v, int* sc, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
  const int incl = wave_incl_scan(v);
  if (lane == 63) sc[wv] = incl;
  __syncthreads();
  if (wv == 0) {
    const int x = lane < nw ? sc[lane] : 0;
    const int xi = wave_incl_scan(x);
    if (lane < nw) sc[lane] = xi - x;
    if (lane == 63) sc[64] = xi;
  }
  __syncthreads();
  const int r = sc[wv] + incl - v;
  *total = sc[64];
  __syncthreads();  // sc may be reused at once
  return r;
}

constexpr int TOPK_THREADS = 1024;
constexpr int TOPK_HPAD = 257;  // per-wave histogram stride (bank-spread)

// Ordered top-b of r similarities under the total order (value desc, position asc) -- the order
// torch.topk(sorted=True) gives here (reorder.py:133), keys being unique -- by radix selection:
// four 8-bit histogram passes over the orderable value bits find the b-th largest value v*;
// every value > v* is taken, plus the first (by position) b - #(> v*) values equal to v*; the
// b picks are then ranked among themselves.  Writes blk (selection order), newrem (ascending,
// reorder.py:139-141), perm_out (int64, nullable).
// LDS: region0 (r + 32*257 words: values + two banks of wave histograms), r flag bytes, scan ints,
// b picks / their values (and 2 b spare words the launch keeps in its LDS size).
__global__ __launch_bounds__(TOPK_THREADS) void ssr_topk_kernel(const float* sim, const int* rem, int r,
                                                                int b, int* blk, int* newrem,
                                                                int64_t* perm_out, int region0, long zs) {
  extern __shared__ uint32_t vals[];
  sim = zws(sim, zs);  // grouped launch: linear blockIdx.z's slice
  rem = zws(rem, zs);
  blk = zws(blk, zs);
  newrem = zws(newrem, zs);
  perm_out = zws(perm_out, zs);
  int* hist = (int*)(vals + r);
  unsigned char* sel = (unsigned char*)(vals + region0);
  int* sc = (int*)(sel + ((r + 15) & ~15));
  int* pick = sc + 80;                  // b positions, ascending
  uint32_t* pv = (uint32_t*)(pick + b); // their values
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6;
  PT2Q_TOPK_STAMP(0);
  for (int e = tid; e < r; e += nt) vals[e] = orderable(sim[e]);
  uint32_t prefix = 0, pmask = 0;
  int kk = b;  // rank (1-based) of v* among the values matching prefix
  // Two banks of 16 per-wave histograms: a pass counts into one while clearing the other, and
  // wave 0 merges + scans in one go -- two barriers per pass.  res: the pass results, in two
  // alternating slots (read after the pass's second barrier, rewritten two passes later).
  for (int i = tid; i < 32 * TOPK_HPAD; i += nt) hist[i] = 0;
  __syncthreads();
  PT2Q_TOPK_STAMP(4);
  int* res = sc + 70;
#pragma unroll 1
  for (int p = 0; p < 4; ++p) {
    const int shift = 24 - 8 * p;
    int* hcur = hist + (p & 1) * 16 * TOPK_HPAD;
    int* hnext = hist + ((p + 1) & 1) * 16 * TOPK_HPAD;
    int* hw = hcur + wv * TOPK_HPAD;
    // similarities crowd into one bin in the high passes: a wave whose active lanes all share
    // a bin adds once (same-word LDS atomics of 64 lanes would serialise), others per lane
    for (int base = 0; base < r; base += nt) {
      const int e = base + tid;
      const uint32_t u = e < r ? vals[e] : 0u;
      const bool act = e < r && (u & pmask) == prefix;
      const int bin = (int)((u >> shift) & 255);
      const uint64_t am = __ballot(act);
      if (am) {
        const int leader = __ffsll((unsigned long long)am) - 1;
        const int lb = __shfl(bin, leader);
        const uint64_t same = __ballot(act && bin == lb);
        if (same == am) {
          if (lane == leader) atomicAdd(&hw[lb], __popcll(am));
        } else if (act) {
          atomicAdd(&hw[bin], 1);
        }
      }
    }
    if (p + 1 < 4)
      for (int i = tid; i < 16 * TOPK_HPAD; i += nt) hnext[i] = 0;
    __syncthreads();
    if (wv == 0) {  // lane l owns bins 255-4l .. 252-4l (descending)
      int c[4] = {0, 0, 0, 0}, s = 0;
#pragma unroll
      for (int w = 0; w < TOPK_THREADS / 64; ++w)
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] += hcur[w * TOPK_HPAD + 255 - 4 * lane - q];
#pragma unroll
      for (int q = 0; q < 4; ++q) s += c[q];
      const int incl = wave_incl_scan(s);
      int run = incl - s;
      if (run < kk && kk <= incl) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (run < kk && kk <= run + c[q]) {
            res[2 * (p & 1)] = 255 - 4 * lane - q;
            res[2 * (p & 1) + 1] = kk - run;
          }
          run += c[q];
        }
      }
    }
    __syncthreads();
    if (p == 0) PT2Q_TOPK_STAMP(5);
    prefix |= (uint32_t)res[2 * (p & 1)] << shift;
    pmask |= 255u << shift;
    kk = res[2 * (p & 1) + 1];
  }
  PT2Q_TOPK_STAMP(1);
  // prefix = v*; the first kk positions holding v* are picked, with every value above it
  const int per = (r + nt - 1) / nt;
  const int e0 = min(r, tid * per), e1 = min(r, e0 + per);
  int ceq = 0, tot;
  for (int e = e0; e < e1; ++e) ceq += vals[e] == prefix;
  int eq = block_excl_scan(ceq, sc, &tot);
  int cs = 0, cu = 0;
  for (int e = e0; e < e1; ++e) {
    const uint32_t u = vals[e];
    const bool s = u > prefix || (u == prefix && eq++ < kk);
    sel[e] = s;
    cs += s;
    cu += !s;
  }
  PT2Q_TOPK_STAMP(2);
  // one scan for both compactions (r < 2^16): picks and the unselected remainder, ascending
  const int both = block_excl_scan((cs << 16) | cu, sc, &tot);
  int os = both >> 16, ou = both & 0xFFFF;
  for (int e = e0; e < e1; ++e) {
    if (sel[e]) {
      pick[os] = e;
      pv[os++] = vals[e];
    } else {
      newrem[ou++] = rem[e];
    }
  }
  __syncthreads();
  PT2Q_TOPK_STAMP(3);
  // rank of pick t: picks above it in (value desc, position asc); picks are position-ascending.
  // Eight threads per pick, each over every eighth other pick, then summed across the eight.
  for (int t0 = 0; t0 < b; t0 += nt / 8) {
    const int t = t0 + tid / 8, sub = tid & 7;
    int rank = 0;
    if (t < b) {
      const uint32_t ut = pv[t];
      for (int s = sub; s < b; s += 8) {
        const uint32_t us = pv[s];
        rank += (us > ut) | ((us == ut) & (s < t));
      }
    }
    rank += __shfl_xor(rank, 4);
    rank += __shfl_xor(rank, 2);
    rank += __shfl_xor(rank, 1);
    if (t < b && sub == 0) {
      const int j = rem[pick[t]];
      blk[rank] = j;
      if (perm_out) perm_out[rank] = j;
    }
  }
  PT2Q_TOPK_STAMP(6);
}

// Sequential block (use_ssr=False: main.py:167-169, gptq.py:135-137) or "take the rest"
// (reorder.py:125-126 when |rem| <= b).
__global__ void select_seq_kernel(int mode, int p0, int bs, int m, const int* rem, int* blk,
                                  int* newrem, int64_t* perm_out, long zs) {
  rem = zws(rem, zs);  // grouped launch: linear blockIdx.z's slice
  blk = zws(blk, zs);
  newrem = zws(newrem, zs);
  perm_out = zws(perm_out, zs);
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < bs) {
    int j = (mode == 0) ? p0 + t : rem[t];
    blk[t] = j;
    if (perm_out) perm_out[t] = j;
  }
  if (mode == 0) {
    int nr = m - p0 - bs;
    for (int e = t; e < nr; e += gridDim.x * blockDim.x) newrem[e] = p0 + bs + e;
  }
}

// C[k][e] = Hinv[blk_k][rem_e] / clamp(Hinv[blk_k][blk_k])   (main.py:201-209)
__global__ __launch_bounds__(256) void ef_coeff_kernel(const float* Hinv, long ldh,
                                                       const int* blk, const int* rem, int nr,
                                                       float* C, long ldc) {
  const int k = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nr) return;
  const long rowb = (long)blk[k] * ldh;
  const float dg = clampmin(Hinv[rowb + blk[k]]);
  C[(long)k * ldc + e] = Hinv[rowb + rem[e]] / dg;
}

}  // namespace

size_t pt2q_ssr_scratch_floats(int n, int m) {
  // part (ceil(m/128) x n) + wn (n) + sim (m)
  return (size_t)ceil_div(m, CHUNK) * n + (size_t)n + (size_t)m;
}

int pt2q_launch_ssr_similarity(const float* Wt, long ldw, int n, const int* rem, int r,
                               float* part, float* wn, float* sim, hipStream_t st, int* cnt,
                               const Grp* grp, bool pre) {
  if (r <= 0 || n <= 0) return PT2Q_E_ARG;
  if ((size_t)(n + 1) * sizeof(float) > 160 * 1024) return PT2Q_E_UNSUPPORTED;
  int nchunks = ceil_div(r, CHUNK);
  const unsigned nz = grp_z(grp);
  const long zs = grp ? grp->ws : 0;
  const bool fused = cnt && n <= 16384 && n % 4 == 0 && ldw % 4 == 0 && (uintptr_t)Wt % 16 == 0;
  if ((nz > 1 || pre) && !fused) return PT2Q_E_UNSUPPORTED;  // grouped launches use the fused w-bar only
  if (fused) {
    hipLaunchKernelGGL(ssr_wbar_fused_kernel, dim3(pre ? 1 : nchunks, ceil_div(n, 256), nz), dim3(64), 0, st, Wt,
                       ldw, n, rem, r, part, wn, cnt, zs, pre ? 1 : 0);
    PT2Q_LAUNCH_CHECK();
  } else {
    hipLaunchKernelGGL(ssr_wbar_partial_kernel, dim3(nchunks, ceil_div(n, 256)), dim3(256), 0, st,
                       Wt, ldw, n, rem, r, part);
    PT2Q_LAUNCH_CHECK();
    if (n <= SUMN_LDS_MAX) {
      hipLaunchKernelGGL(ssr_wbar_sumfinal_kernel, dim3(1), dim3(1024), 0, st, part, nchunks, n, r, wn);
      PT2Q_LAUNCH_CHECK();
    } else {
      hipLaunchKernelGGL(ssr_wbar_sum_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, part, nchunks,
                         n, r, wn);
      PT2Q_LAUNCH_CHECK();
      hipLaunchKernelGGL(ssr_wbar_final_kernel, dim3(1), dim3(1024), 0, st, wn, n);
      PT2Q_LAUNCH_CHECK();
    }
  }
  const bool v4 = (n & 3) == 0 && (ldw & 3) == 0 && (uintptr_t)Wt % 16 == 0;
  const int S = ceil_div(n, 4096);
  if (v4 && n > 4096 && n <= 16384) {
    auto k = S == 2 ? ssr_sim_split_kernel<2> : S == 3 ? ssr_sim_split_kernel<3> : ssr_sim_split_kernel<4>;
    hipLaunchKernelGGL(k, dim3(r, 1, nz), dim3(64 * S), 0, st, Wt, ldw, n, rem, r, wn, sim, zs);
  } else {
    auto sim_k = !v4 ? ssr_sim_kernel<0> : n <= 4096 ? ssr_sim_kernel<16> : n <= 12288 ? ssr_sim_kernel<48>
                                                                                     : ssr_sim_kernel<0>;
    hipLaunchKernelGGL(sim_k, dim3(ceil_div(r, 4), 1, nz), dim3(256), 0, st, Wt, ldw, n, rem, r, wn, sim, zs);
  }
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}

int pt2q_launch_ssr_topk(const float* sim, const int* rem, int r, int b, int* blk, int* newrem,
                         int64_t* perm_out, hipStream_t st, const Grp* grp) {
  if (b <= 0 || b > r || r >= 65536) return PT2Q_E_UNSUPPORTED;
  const int region0 = (r + 32 * TOPK_HPAD + 3) & ~3;
  const size_t lds = (size_t)region0 * 4 + (size_t)((r + 15) & ~15) + 80 * sizeof(int) +
                     (size_t)b * 4 * sizeof(int);
  if (lds > 160 * 1024) return PT2Q_E_UNSUPPORTED;
  hipLaunchKernelGGL(ssr_topk_kernel, dim3(1, 1, grp_z(grp)), dim3(TOPK_THREADS), lds, st, sim, rem, r, b, blk,
                     newrem, perm_out, region0, grp ? grp->ws : 0l);
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}

int pt2q_launch_select_seq(int mode, int p0, int bs, int m, const int* rem, int* blk,
                           int* newrem, int64_t* perm_out, hipStream_t st, const Grp* grp) {
  int work = (mode == 0) ? (m - p0) : bs;
  int grid = ceil_div(work > 0 ? work : 1, 256);
  if (grid > 64) grid = 64;
  hipLaunchKernelGGL(select_seq_kernel, dim3(grid, 1, grp_z(grp)), dim3(256), 0, st, mode, p0, bs, m, rem,
                     blk, newrem, perm_out, grp ? grp->ws : 0l);
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}

int pt2q_launch_ef_coeffs(const float* Hinv, long ldh, const int* blk, int bs, const int* rem,
                          int nr, float* C, long ldc, hipStream_t st) {
  hipLaunchKernelGGL(ef_coeff_kernel, dim3(ceil_div(nr, 256), bs), dim3(256), 0, st, Hinv, ldh,
                     blk, rem, nr, C, ldc);
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}
