// Exported C ABI of libpt2q (include/pt2q.h): argument checks, workspace carving and the
// per-layer launch schedule.  All launches are stream-ordered; nothing here synchronises or
// allocates, so a caller may capture a whole layer into a hipGraph.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>
#include <climits>

#include "common.hpp"
#include "internal.hpp"

namespace {

// The spin caps, read once at library load -- see Pt2qSpinCaps.  PT2Q_DEBUG_SPIN_CAP, the
// stall-reporting test hook (tests/test_gpu_status.py), is the only environment variable the
// library reads; every kernel choice is fixed in the code.
Pt2qSpinCaps load_spin_caps() {
  Pt2qSpinCaps t;
  if (const char* e = std::getenv("PT2Q_DEBUG_SPIN_CAP")) {
    const long c = std::atol(e);
    if (c >= 0) t.spin_cap_long = t.spin_cap_fallback = c;
  }
  return t;
}

}  // namespace

const Pt2qSpinCaps& pt2q_spin_caps() {
  static const Pt2qSpinCaps t = load_spin_caps();
  return t;
}

namespace {

const Pt2qSpinCaps& g_spin_caps_at_load = pt2q_spin_caps();  // forces the read at dlopen

struct Carve {
  char* p;
  size_t left;
  bool ok = true;
  bool dry = false;  // count only (used bytes in `used`)
  size_t used = 0;
  template <typename T>
  T* take(size_t count) {
    size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
    used += bytes;
    if (dry) return nullptr;
    if (!p || bytes > left) {
      ok = false;
      return nullptr;
    }
    T* r = (T*)p;
    p += bytes;
    left -= bytes;
    return r;
  }
};

inline long round_up(long a, long b) { return (a + b - 1) / b * b; }

// ---- stage timing (measurement only, pt2q_stage_timing): while enabled, the launches of each
// block-loop stage are bracketed by a pair of HIP events on their stream.  One host thread, no
// graph capture; read back after the stream has drained.
struct StageRec {
  int stage;
  hipEvent_t a, b;
};
struct StageLog {
  bool on = false;
  std::vector<StageRec> recs;
  std::vector<hipEvent_t> pool;
  size_t next = 0;
  hipEvent_t take() {
    if (next == pool.size()) {
      hipEvent_t e = nullptr;
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
      pool.push_back(e);
    }
    return pool[next++];
  }
};
StageLog& stage_log() {
  static StageLog l;
  return l;
}
struct StageScope {
  int stage;
  hipStream_t st;
  hipEvent_t a = nullptr;
  StageScope(int s, hipStream_t stream) : stage(s), st(stream) {
    StageLog& l = stage_log();
    if (l.on && (a = l.take()) && hipEventRecord(a, st) != hipSuccess) a = nullptr;
  }
  void close() {
    if (!a) return;
    StageLog& l = stage_log();
    hipEvent_t b = l.take();
    if (b && hipEventRecord(b, st) == hipSuccess) l.recs.push_back({stage, a, b});
    a = nullptr;
  }
  ~StageScope() { close(); }
};

struct BlockWs {
  int* status;  // the call's status word (stall reports)
  float* Wt;
  int8_t* Tt;
  float* Et;
  float* Ck;
  float* alpha_t;
  float* mu_t;
  float* S1;
  float* d;
  float* ssr;
  int* rem[2];
  int* blk;
  int* counters;
  int* iters;
  int* iters_part;
  float* hb;  // variant G, blocks > 128: the gathered H[blk][blk] and S = H_bbᵀH_bb (bb x bb)
  float* hS;
  long ldw;
};

// Whether the error feedback may hand the next block's SSR its w-bar partials (ef.hip / ssr.hip
// pre path: the fused w-bar launch's conditions).
inline bool ef_wbar_ok(int n, long ldw, const float* Wt) {
  return n <= 16384 && n % 4 == 0 && ldw % 4 == 0 && (uintptr_t)Wt % 16 == 0;
}

// variant G's AGA matrix for blocks wider than one workgroup's LDS holds (> 128 columns)
inline bool hess_wide(int flags, int bb) { return (flags & PT2Q_AGA_MASK) == PT2Q_AGA_HESS && bb > 128; }

bool carve_blocks(Carve& c, int n, int m, int b, BlockWs& w, int flags = 0) {
  const long ldw = round_up(n, 64);
  const int bb = b < m ? b : m;
  const int B = b < m ? ceil_div(m, b) : 1;
  w.ldw = ldw;
  w.Wt = c.take<float>((size_t)m * ldw);
  w.Tt = c.take<int8_t>((size_t)m * ldw);
  // E and the feedback coefficients exist only when a block leaves columns behind (B > 1)
  w.Et = c.take<float>(B > 1 ? (size_t)bb * ldw : 1);
  w.Ck = c.take<float>(B > 1 ? (size_t)bb * m : 1);
  w.alpha_t = c.take<float>((size_t)B * n);
  w.mu_t = c.take<float>((size_t)B * n);
  w.S1 = c.take<float>((size_t)bb);
  w.d = c.take<float>(1);
  w.ssr = c.take<float>(pt2q_ssr_scratch_floats(n, m));
  w.rem[0] = c.take<int>((size_t)m);
  w.rem[1] = c.take<int>((size_t)m);
  w.blk = c.take<int>((size_t)bb);
  // [2k, 2k+1] ATQ; [2B+2k, 2B+2k+1] the ATQ launch's S1 sync; [4B ..) the wbar hand-off counters
  w.counters = c.take<int>((size_t)4 * B + pt2q_ssr_counter_ints(n));
  w.iters = c.take<int>((size_t)B);
  w.iters_part = c.take<int>((size_t)ceil_div(n, 16) * 4);  // one per ATQ wave (4 waves of 4 rows per workgroup)
  w.hb = w.hS = nullptr;
  if (hess_wide(flags, bb)) {
    w.hb = c.take<float>((size_t)bb * bb);
    w.hS = c.take<float>((size_t)bb * bb);
  }
  return c.ok;
}

size_t blocks_bytes(int n, int m, int b, int flags = 0) {  // a dry run of carve_blocks
  Carve c{nullptr, 0};
  c.dry = true;
  BlockWs w;
  carve_blocks(c, n, m, b, w, flags);
  return c.used;
}

// per-channel setup in one launch, linear z = blockIdx.y: perm = [0, m) (the block is every column
// in ascending order), the wide ATQ's counters (2 ints) and the iteration count zeroed -- instead
// of two memsets and a select_seq launch per linear
struct PcSetupGroup {
  int64_t* perm[PT2Q_PC_GROUP_MAX];
  int* counters[PT2Q_PC_GROUP_MAX];
  int* iters[PT2Q_PC_GROUP_MAX];
};
__global__ void pc_setup_group_kernel(PcSetupGroup g, int m) {
  const int z = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) g.perm[z][i] = i;
  if (i < 2) g.counters[z][i] = 0;
  if (i == 0) *g.iters[z] = 0;
}

__global__ void i64_to_i32_kernel(const int64_t* a, int n, int* b) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) b[i] = (int)a[i];
}
__global__ void i32_to_i64_kernel(const int* a, int n, int64_t* b) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) b[i] = a[i];
}

// Per-channel blocks (one block of every column, m > 512) of `count` linears: the setup, then the
// wide ATQ on each caller's row-major W, writing T, alpha, mu (n x 1) straight into the outputs.
int run_perchannel(int count, const PcLinear* lin, int wdtype, int m, int max_iter, int tdtype,
                   hipStream_t st) {
  PcSetupGroup sg{};
  for (int z = 0; z < count; ++z) {
    sg.perm[z] = lin[z].perm;
    sg.counters[z] = lin[z].counters;
    sg.iters[z] = lin[z].iters;
  }
  {
    StageScope ts(PT2Q_TIMER_SETUP, st);
    hipLaunchKernelGGL(pc_setup_group_kernel, dim3(ceil_div(m, 256), count), dim3(256), 0, st, sg, m);
    PT2Q_LAUNCH_CHECK();
  }
  StageScope ts_atq(PT2Q_TIMER_ATQ, st);
  return pt2q_launch_atq_rm_group(count, lin, wdtype, m, max_iter, tdtype, st);
}

// ---- the block loop of one linear (grp == nullptr, count == 1) or of a group of same-shaped
// linears (pt2q_quantize_blocks_group: grp given, w = linear 0's slice of `count` workspace slices
// grp->ws bytes apart, perm64 in the slice)

// A linear's slice: the block-loop buffers plus its permutation (int64, written by the
// selection launches and copied out at the end).
size_t group_slice_bytes(int n, int m, int b, int flags) {
  return blocks_bytes(n, m, b, flags) + (((size_t)m * 8 + 255) & ~(size_t)255);
}

// Every linear's counters and ITF iteration slots zeroed, its remaining set = [0, m).
__global__ void group_init_kernel(int* counters, int ncnt, int* iters, int B, int* rem0, int m, long zs) {
  counters = zws(counters, zs);
  iters = zws(iters, zs);
  rem0 = zws(rem0, zs);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < ncnt) counters[t] = 0;
  if (t < B) iters[t] = 0;
  if (t < m) rem0[t] = t;
}

int run_blocks(int count, const void* const* W, int wdtype, long ldw_in, int n, int m, int b, int flags,
               const float* const* A, long lda, const float* const* Hinv, long ldhi, int max_iter,
               float* const* alpha, float* const* mu, void* const* T, int tdtype, int64_t* const* perm,
               int* const* iters_dev, BlockWs& w, const Grp* grp, int64_t* perm64, hipStream_t st) {
  int rc;
  const int B = b < m ? ceil_div(m, b) : 1;
  const long zs = grp ? grp->ws : 0;
  const bool ssr = (flags & PT2Q_FLAG_SSR) != 0;
  const int aga = flags & PT2Q_AGA_MASK;
  // one linear: perm and iters straight into the caller's buffers; a group: into the slices
  int64_t* pout = grp ? perm64 : perm[0];
  int* iters = !grp && iters_dev[0] ? iters_dev[0] : w.iters;
  if (B == 1 && m > 512 && aga != PT2Q_AGA_HESS) {
    // Per-channel (block_size >= m, main.py:176-189 with one block; never a group, group_ok): the
    // block is every column in ascending order -- SSR over the whole remaining set returns it in
    // rem order, and rem is [0, m) -- so the wide ATQ reads the caller's row-major W in place (no
    // feature-major copy, no code transpose).
    const bool act = aga == PT2Q_AGA_ACT;
    // S1 / d given (PT2Q_FLAG_S1_GIVEN: A = S1 then d, formed once per Gram) or formed here
    const bool given = act && (flags & PT2Q_FLAG_S1_GIVEN) != 0;
    if (act && !given) {
      StageScope ts_s1(PT2Q_TIMER_ATQ, st);  // part of the ATQ stage, as the rows' launches
      if ((rc = pt2q_launch_s1(A[0], lda, nullptr, m, w.S1, w.d, st)) != PT2Q_OK) return rc;
    }
    const PcLinear lin{W[0], ldw_in, n, !act ? nullptr : given ? A[0] : w.S1, given ? A[0] + m : w.d,
                       alpha[0], mu[0], T[0], (long)m, iters, w.counters, perm[0]};
    return run_perchannel(1, &lin, wdtype, m, max_iter, tdtype, st);
  }
  {
    StageScope ts(PT2Q_TIMER_SETUP, st);
    for (int z = 0; z < count; ++z)  // W (n x m) -> Wt (m x ldw, fp32) of every linear
      if ((rc = pt2q_launch_transpose_to_f32(W[z], wdtype, ldw_in, n, m, (float*)((char*)w.Wt + z * zs), w.ldw,
                                             st)) != PT2Q_OK)
        return rc;
    const int ncnt = 4 * B + pt2q_ssr_counter_ints(n);
    hipLaunchKernelGGL(group_init_kernel, dim3(ceil_div(std::max(std::max(ncnt, B), m), 256), 1, count), dim3(256),
                       0, st, w.counters, ncnt, iters, B, w.rem[0], m, zs);
    PT2Q_LAUNCH_CHECK();
  }
  float* part = w.ssr;
  float* wn = part + (size_t)ceil_div(m, 128) * n;
  float* sim = wn + n;
  int processed = 0, r = m, cur = 0;
  bool pre = false;  // part holds rem's w-bar partials (from the previous block's error feedback)
  for (int k = 0; k < B; ++k) {
    const int bs = r < b ? r : b;
    const int nr = r - bs;
    int* rem = w.rem[cur];
    int* nrem = w.rem[cur ^ 1];
    // variant M with blocks <= 128: the ATQ launch also forms S1/d (no separate launch; off
    // the critical path of the rows, which need it only for their AGA)
    const bool s1_in_atq = aga == PT2Q_AGA_ACT && bs <= 128;
    StageScope ts_ssr(PT2Q_TIMER_SSR, st);
    if (ssr && r > b) {
      if ((rc = pt2q_launch_ssr_similarity(w.Wt, w.ldw, n, rem, r, part, wn, sim, st, w.counters + 4 * B, grp,
                                           pre)) != PT2Q_OK)
        return rc;
      if ((rc = pt2q_launch_ssr_topk(sim, rem, r, b, w.blk, nrem, pout + processed, st, grp)) != PT2Q_OK)
        return rc;
    } else if ((rc = pt2q_launch_select_seq(ssr ? 1 : 0, ssr ? 0 : processed, bs, m, ssr ? rem : nullptr, w.blk,
                                            nrem, pout + processed, st, grp)) != PT2Q_OK) {
      return rc;
    }
    ts_ssr.close();
    StageScope ts_atq(PT2Q_TIMER_ATQ, st);
    const float* S1 = nullptr;
    if (aga == PT2Q_AGA_ACT || aga == PT2Q_AGA_HESS) {
      // one linear only (group_ok): variant G, and variant M's blocks wider than 128 columns
      if (hess_wide(flags, bs))
        rc = pt2q_launch_s1_hess_wide(A[0], lda, w.blk, bs, w.hb, w.hS, w.S1, w.d, st);
      else if (aga == PT2Q_AGA_HESS)
        rc = pt2q_launch_s1_hess_block(A[0], lda, w.blk, bs, w.S1, w.d, st);
      else
        rc = s1_in_atq ? PT2Q_OK : pt2q_launch_s1(A[0], lda, w.blk, bs, w.S1, w.d, st);
      if (rc != PT2Q_OK) return rc;
      S1 = w.S1;
    }
    // (a group: the Gram and the inverse Hessian of linear z from grp's tables)
    if ((rc = pt2q_launch_atq_block(w.Wt, w.ldw, n, w.blk, bs, S1, w.d, max_iter,
                                    w.alpha_t + (size_t)k * n, w.mu_t + (size_t)k * n, w.Tt, w.ldw,
                                    nr > 0 ? w.Et : nullptr, w.ldw, iters + k, w.counters + 2 * k,
                                    st, Hinv[0], ldhi, nrem, nr, w.Ck, m, w.iters_part,
                                    s1_in_atq ? A[0] : nullptr, lda,
                                    s1_in_atq ? w.counters + 2 * B + 2 * k : nullptr, w.status, grp)) != PT2Q_OK)
      return rc;  // (also forms the EF coefficients C[k][e] when nr > 0)
    ts_atq.close();
    StageScope ts_ef(PT2Q_TIMER_EF, st);
    const bool want = ssr && nr > b && ef_wbar_ok(n, w.ldw, w.Wt);  // the next block runs SSR over nrem
    rc = nr > 0 ? pt2q_launch_ef(w.Ck, m, w.Et, w.Wt, w.ldw, m, nrem, nr, bs, st, grp, want ? part : nullptr, n)
                : PT2Q_OK;
    pre = want && rc == PT2Q_OK;
    if (rc == PT2Q_E_UNSUPPORTED && !grp) {  // blocks wider than the EF kernel takes: the GEMM
      GemmDesc g{};
      g.M = nr; g.N = n; g.K = bs;
      g.A = w.Ck; g.lda = m; g.a_layout = LAY_KMAJOR;     // (e, k) = C[k][e]
      g.B = w.Et; g.ldb = w.ldw; g.b_layout = LAY_KMAJOR; // (k, i) = E[k][i]
      g.in_dtype = PT2Q_F32;
      g.C = w.Wt; g.ldc = w.ldw; g.crow = nrem;
      g.mode = GEMM_SUB;
      rc = pt2q_launch_gemm(g, st);
    }
    if (rc != PT2Q_OK) return rc;
    processed += bs;
    r = nr;
    cur ^= 1;
  }
  StageScope ts(PT2Q_TIMER_OUT, st);
  for (int z = 0; z < count; ++z) {
    // outputs: T (n x m) from Tt (m x ldw); alpha / mu (n x B) from (B x n); a group's perm, iters
    auto sl = [&](auto* p) { return (decltype(p))((char*)p + z * zs); };
    if ((rc = pt2q_launch_transpose_i8(sl(w.Tt), w.ldw, m, n, T[z], tdtype, m, st)) != PT2Q_OK) return rc;
    if ((rc = pt2q_launch_transpose_f32(sl(w.alpha_t), n, B, n, alpha[z], B, st)) != PT2Q_OK) return rc;
    if ((rc = pt2q_launch_transpose_f32(sl(w.mu_t), n, B, n, mu[z], B, st)) != PT2Q_OK) return rc;
    if (grp && hipMemcpyAsync(perm[z], sl(perm64), sizeof(int64_t) * m, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return PT2Q_E_HIP;
    if (grp && iters_dev && iters_dev[z] &&
        hipMemcpyAsync(iters_dev[z], sl(w.iters), sizeof(int) * B, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return PT2Q_E_HIP;
  }
  return PT2Q_OK;
}

bool dtype_ok(int dt) { return dt == PT2Q_F32 || dt == PT2Q_F16 || dt == PT2Q_BF16; }

// Every condition under which pt2q_quantize_blocks_group runs (else PT2Q_E_UNSUPPORTED): blocks
// of <= 128 columns with b < m, variant M (S1 in the ATQ launch) or no AGA, the fused w-bar's
// n <= 16384 with n % 4 == 0, and the error feedback's own
// limits (pt2q_launch_ef: coefficient rows 16-byte aligned, every Wt under 2 GiB of buffer range).
bool group_ok(int n, int m, int b, int flags) {
  const int aga = flags & PT2Q_AGA_MASK;
  return n > 0 && m > 0 && b > 0 && b <= 128 && b < m && m < 65536 &&
         (aga == PT2Q_AGA_ACT || aga == PT2Q_AGA_NONE) &&
         n <= 16384 && n % 4 == 0 && m % 4 == 0 && (long)m * round_up(n, 64) * 4 < 0x80000000L;
}

// The status word every workspace-taking call reserves first (PT2Q_STATUS_BYTES), zeroed on the
// call's stream before any kernel that may report into it.
int* take_status(Carve& c, hipStream_t st, int& rc) {
  int* s = c.take<int>(PT2Q_STATUS_BYTES / sizeof(int));
  rc = PT2Q_OK;
  if (s && hipMemsetAsync(s, 0, sizeof(int), st) != hipSuccess) rc = PT2Q_E_HIP;
  return s;
}

}  // namespace

extern "C" const char* pt2q_version(void) { return "pt2q-mi355x 0.1.0 (gfx950)"; }

extern "C" const char* pt2q_strerror(int status) {
  switch (status) {
    case PT2Q_OK: return "ok";
    case PT2Q_E_ARG: return "invalid argument";
    case PT2Q_E_NOT_SPD: return "Hessian not positive definite (Cholesky breakdown)";
    case PT2Q_E_UNSUPPORTED: return "unsupported shape/configuration";
    case PT2Q_E_HIP: return "HIP runtime error";
    case PT2Q_E_WORKSPACE: return "workspace too small";
    case PT2Q_E_STALL: return "a cross-workgroup wait timed out (results invalid)";
  }
  return "unknown status";
}

extern "C" int pt2q_stage_timing(int enable) {
  StageLog& l = stage_log();
  if (enable) {
    l.recs.clear();
    l.next = 0;
  }
  l.on = enable != 0;
  return PT2Q_OK;
}

extern "C" int pt2q_stage_timing_read(double* ms, int nstages, int* records) {
  if (!ms || nstages <= 0) return PT2Q_E_ARG;
  StageLog& l = stage_log();
  for (int i = 0; i < nstages; ++i) ms[i] = 0.0;
  for (const StageRec& r : l.recs) {
    float t = 0.f;
    if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&t, r.a, r.b) != hipSuccess)
      return PT2Q_E_HIP;
    if (r.stage >= 0 && r.stage < nstages) ms[r.stage] += t;
  }
  if (records) *records = (int)l.recs.size();
  return PT2Q_OK;
}

extern "C" int pt2q_quantize_blocks_group_supported(int n, int m, int b, int flags) {
  return group_ok(n, m, b, flags) ? 1 : 0;
}

extern "C" size_t pt2q_blocks_workspace_bytes(int n, int m, int b, int flags) {
  if (n <= 0 || m <= 0 || b <= 0) return 0;
  return PT2Q_STATUS_BYTES + blocks_bytes(n, m, b, flags);
}

extern "C" size_t pt2q_cholesky_workspace_bytes(int m) {
  return 2 * (((size_t)m * m * 4 + 255) & ~(size_t)255);
}

extern "C" size_t pt2q_layer_workspace_bytes(int n, int m, int b, int flags) {
  if (n <= 0 || m <= 0 || b <= 0) return 0;
  size_t mm = ((size_t)m * m * 4 + 255) & ~(size_t)255;
  return PT2Q_STATUS_BYTES + blocks_bytes(n, m, b, flags) + 4 * mm + 2 * 256 + pt2q_gram_workspace_bytes(m);
}

extern "C" size_t pt2q_ssr_workspace_bytes(int n, int m) {
  return PT2Q_STATUS_BYTES + blocks_bytes(n, m, 128);
}

extern "C" size_t pt2q_gram_workspace_bytes(int m) {
  return m > 0 ? PT2Q_STATUS_BYTES + ((pt2q_gram_flags_ints(m) * sizeof(int) + 255) & ~(size_t)255) : 0;
}

extern "C" int pt2q_gram(const void* X, int xdtype, int64_t N, int m, int64_t ldx, float* G,
                         int64_t ldg, int accumulate, void* workspace, size_t workspace_bytes,
                         void* stream) {
  if ((!X && N > 0) || !G || N < 0 || N > INT_MAX || m <= 0 || !dtype_ok(xdtype) || ldx < m ||
      ldg < m)
    return PT2Q_E_ARG;
  GemmDesc g{};
  g.M = m; g.N = m; g.K = (int)N;
  g.A = X; g.lda = ldx; g.a_layout = LAY_KMAJOR;
  g.B = X; g.ldb = ldx; g.b_layout = LAY_KMAJOR;
  g.in_dtype = xdtype;
  g.C = G; g.ldc = ldg;
  if (accumulate < 0 || accumulate > 2) return PT2Q_E_ARG;
  g.mode = accumulate == 2 ? GEMM_CHAIN_POS : accumulate ? GEMM_ADD : GEMM_STORE;
  g.upper = 1; g.mirror = 1;
  // workspace: [status word][split flags]; without it every tile is one chain (nothing waits)
  int *status = nullptr, *flags = nullptr;
  if (workspace && workspace_bytes >= pt2q_gram_workspace_bytes(m)) {
    Carve c{(char*)workspace, workspace_bytes};
    int rc;
    status = take_status(c, (hipStream_t)stream, rc);
    if (rc != PT2Q_OK) return rc;
    flags = c.take<int>(pt2q_gram_flags_ints(m));
  }
  StageScope ts(PT2Q_TIMER_GRAM, (hipStream_t)stream);
  return pt2q_launch_gram(g, flags, (hipStream_t)stream, status);
}

extern "C" int pt2q_gram_batched(int batch, const void* const* X, int xdtype, int64_t N, int m, int64_t ldx,
                                 float* G, void* stream) {
  if (batch <= 0 || !X || !G || N < 0 || N > INT_MAX || m <= 0 || ldx < m) return PT2Q_E_ARG;
  StageScope ts(PT2Q_TIMER_GRAM, (hipStream_t)stream);
  if (xdtype == PT2Q_F32)
    return pt2q_launch_gram_f32_batched((const float* const*)X, N, m, ldx, G, (long)m * m, batch, (hipStream_t)stream);
  return pt2q_launch_gram16_batched(X, xdtype, N, m, ldx, G, (long)m * m, batch, (hipStream_t)stream);
}

extern "C" int pt2q_gram_batched_upper(int batch, const void* const* X, int xdtype, int64_t N, int m,
                                       int64_t ldx, float* G, void* stream) {
  if (batch <= 0 || !X || !G || N < 0 || N > INT_MAX || m <= 0 || ldx < m) return PT2Q_E_ARG;
  if (xdtype != PT2Q_F16 && xdtype != PT2Q_BF16) return PT2Q_E_UNSUPPORTED;
  StageScope ts(PT2Q_TIMER_GRAM, (hipStream_t)stream);
  return pt2q_launch_gram16_batched(X, xdtype, N, m, ldx, G, (long)m * m, batch, (hipStream_t)stream, true);
}

extern "C" int pt2q_prepare_hessian(const float* G, int64_t ldg, int m, int64_t nsamples,
                                    float percdamp, float* H, int64_t ldh, float* damp_dev,
                                    void* stream) {
  if (!G || !H || m <= 0 || nsamples <= 0 || ldg < m || ldh < m) return PT2Q_E_ARG;
  return pt2q_launch_prepare_hessian(G, ldg, m, nsamples, percdamp, H, ldh, damp_dev,
                                     (hipStream_t)stream);
}

extern "C" int pt2q_cholesky_inverse(const float* H, int64_t ldh, int m, float* Hinv,
                                     int64_t ldhi, void* workspace, size_t workspace_bytes,
                                     int* info_dev, void* stream) {
  if (!H || !Hinv || !info_dev || m <= 0 || ldh < m || ldhi < m) return PT2Q_E_ARG;
  Carve c{(char*)workspace, workspace_bytes};
  float* U = c.take<float>((size_t)m * m);
  float* Ui = c.take<float>((size_t)m * m);
  if (!c.ok) return PT2Q_E_WORKSPACE;
  StageScope ts(PT2Q_TIMER_INVERSE, (hipStream_t)stream);
  return pt2q_launch_cholesky_inverse(H, ldh, m, Hinv, ldhi, U, Ui, info_dev, (hipStream_t)stream);
}

// ---- a batch of units' damped Hessian inverses (main.py:129-139 per unit, one launch sequence)
extern "C" size_t pt2q_hessian_inverse_batched_workspace_bytes(int m, int batch) {
  if (m <= 0 || batch <= 0) return 0;
  return (((size_t)m * m * batch * 4 + 255) & ~(size_t)255) + (((size_t)batch * 4 + 255) & ~(size_t)255);
}

extern "C" int pt2q_hessian_inverse_batched(const float* G, int m, int batch, int64_t nsamples,
                                            float percdamp, float* H, float* Hinv, void* workspace,
                                            size_t workspace_bytes, int* info_dev, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!G || !H || !Hinv || !info_dev || m <= 0 || batch <= 0 || nsamples <= 0 || G == H || H == Hinv)
    return PT2Q_E_ARG;
  Carve c{(char*)workspace, workspace_bytes};
  float* Ui = c.take<float>((size_t)m * m * batch);
  float* damp = c.take<float>((size_t)batch);
  if (!c.ok) return PT2Q_E_WORKSPACE;
  const long mm = (long)m * m;
  // H written as the Cholesky work matrix at once (strictly lower part zero) where the damping
  // pass can (m <= SUMN_LDS_MAX); else in full form, then made upper in place by the factor
  const bool upper = m <= SUMN_LDS_MAX;
  int rc;
  StageScope ts(PT2Q_TIMER_INVERSE, st);
  if (upper) {  // every item in one launch pair
    if ((rc = pt2q_launch_prepare_hessian(G, m, m, nsamples, percdamp, H, m, damp, st, true, batch, mm)) != PT2Q_OK)
      return rc;
  } else {
    for (int z = 0; z < batch; ++z)
      if ((rc = pt2q_launch_prepare_hessian(G + z * mm, m, m, nsamples, percdamp, H + z * mm, m, damp + z, st,
                                            false)) != PT2Q_OK)
        return rc;
  }
  return pt2q_launch_cholesky_inverse(H, m, m, Hinv, m, H, Ui, info_dev, st, upper, batch);
}

extern "C" int pt2q_quantize_blocks(const void* W, int wdtype, int64_t ldw, int n, int m, int b,
                                    int flags, const float* A, int64_t lda, const float* Hinv,
                                    int64_t ldhi, int max_iter, float* alpha, float* mu, void* T,
                                    int tdtype, int64_t* perm, int* iters_dev, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  // Hinv feeds only the error feedback: a single block (per-channel, b >= m) leaves no columns
  // behind and never reads it, so it may be NULL there
  if (!W || (!Hinv && b < m) || !alpha || !mu || !T || !perm || n <= 0 || m <= 0 || b <= 0 ||
      !dtype_ok(wdtype) || (tdtype != PT2Q_I8 && tdtype != PT2Q_F32) || max_iter < 0 || ldw < m ||
      (Hinv && ldhi < m))
    return PT2Q_E_ARG;
  int aga = flags & PT2Q_AGA_MASK;
  if (flags & PT2Q_FLAG_S1_GIVEN) {  // A = S1 (m) then d: only the per-channel path reads it so
    if (aga != PT2Q_AGA_ACT || b < m || m <= 512 || !A) return PT2Q_E_ARG;
  } else if (aga != PT2Q_AGA_NONE && (!A || lda < m)) {
    return PT2Q_E_ARG;
  }
  Carve c{(char*)workspace, workspace_bytes};
  BlockWs w;
  int rc;
  w.status = take_status(c, (hipStream_t)stream, rc);
  if (rc != PT2Q_OK) return rc;
  if (!carve_blocks(c, n, m, b, w, flags)) return PT2Q_E_WORKSPACE;
  return run_blocks(1, &W, wdtype, ldw, n, m, b, flags, &A, lda, &Hinv, ldhi, max_iter, &alpha, &mu, &T,
                    tdtype, &perm, &iters_dev, w, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" size_t pt2q_quantize_perchannel_group_workspace_bytes(int count) {
  if (count <= 0) return 0;
  return PT2Q_STATUS_BYTES + (((size_t)count * 3 * sizeof(int) + 255) & ~(size_t)255);
}

extern "C" int pt2q_quantize_perchannel_group(int count, const void* const* W, int wdtype, int64_t ldw,
                                              const int* n, int m, const float* const* S1d, int max_iter,
                                              float* const* alpha, float* const* mu, void* const* T, int tdtype,
                                              int64_t* const* perm, int* const* iters_dev, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (count <= 0 || count > PT2Q_PC_GROUP_MAX || !W || !n || !alpha || !mu || !T || !perm || m <= 512 ||
      !dtype_ok(wdtype) || (tdtype != PT2Q_I8 && tdtype != PT2Q_F32) || max_iter < 0 || ldw < m)
    return PT2Q_E_ARG;
  for (int z = 0; z < count; ++z)
    if (!W[z] || n[z] <= 0 || !alpha[z] || !mu[z] || !T[z] || !perm[z]) return PT2Q_E_ARG;
  Carve c{(char*)workspace, workspace_bytes};
  int rc;
  int* status = take_status(c, st, rc);
  (void)status;  // no cross-workgroup waits here: the word stays 0
  if (rc != PT2Q_OK) return rc;
  int* ints = c.take<int>((size_t)count * 3);
  if (!c.ok) return PT2Q_E_WORKSPACE;
  PcLinear lin[PT2Q_PC_GROUP_MAX];
  for (int z = 0; z < count; ++z) {
    const float* s1 = S1d ? S1d[z] : nullptr;
    int* it = (iters_dev && iters_dev[z]) ? iters_dev[z] : ints + 2 * count + z;
    lin[z] = PcLinear{W[z], (long)ldw, n[z], s1, s1 ? s1 + m : nullptr, alpha[z], mu[z], T[z], (long)m, it,
                      ints + 2 * z, perm[z]};
  }
  return run_perchannel(count, lin, wdtype, m, max_iter, tdtype, st);
}

extern "C" size_t pt2q_quantize_blocks_group_workspace_bytes(int count, int n, int m, int b, int flags) {
  if (count <= 0 || n <= 0 || m <= 0 || b <= 0) return 0;
  return PT2Q_STATUS_BYTES + (size_t)count * group_slice_bytes(n, m, b, flags);
}

extern "C" int pt2q_quantize_blocks_group(int count, const void* const* W, int wdtype, int64_t ldw, int n,
                                          int m, int b, int flags, const float* const* A, int64_t lda,
                                          const float* const* Hinv, int64_t ldhi, int max_iter,
                                          float* const* alpha, float* const* mu, void* const* T, int tdtype,
                                          int64_t* const* perm, int* const* iters_dev, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int aga = flags & PT2Q_AGA_MASK;
  if (flags & PT2Q_FLAG_S1_GIVEN) return PT2Q_E_ARG;  // per-channel blocks only (pt2q_quantize_blocks)
  if (count <= 0 || count > PT2Q_GROUP_MAX || !W || !Hinv || !alpha || !mu || !T || !perm || n <= 0 ||
      m <= 0 || b <= 0 || !dtype_ok(wdtype) || (tdtype != PT2Q_I8 && tdtype != PT2Q_F32) || max_iter < 0 ||
      ldw < m || ldhi < m)
    return PT2Q_E_ARG;
  if (aga == PT2Q_AGA_ACT && (!A || lda < m)) return PT2Q_E_ARG;
  for (int z = 0; z < count; ++z)
    if (!W[z] || !Hinv[z] || !alpha[z] || !mu[z] || !T[z] || !perm[z] || (aga == PT2Q_AGA_ACT && !A[z]))
      return PT2Q_E_ARG;
  // grouped launches: blocks of at most 128 columns, several blocks (the error feedback runs),
  // variant M (S1/d in the ATQ launch) or no AGA, the fused w-bar, the EF kernel (group_ok)
  if (!group_ok(n, m, b, flags)) return PT2Q_E_UNSUPPORTED;
  Carve c{(char*)workspace, workspace_bytes};
  BlockWs w;
  int rc;
  w.status = take_status(c, st, rc);
  if (rc != PT2Q_OK) return rc;
  const size_t slice = group_slice_bytes(n, m, b, flags);
  char* base = c.p;
  if (!c.ok || !base || c.left < slice * count) return PT2Q_E_WORKSPACE;
  Carve s0{base, slice};
  if (!carve_blocks(s0, n, m, b, w, flags)) return PT2Q_E_WORKSPACE;
  int64_t* perm64 = s0.take<int64_t>((size_t)m);
  if (!s0.ok) return PT2Q_E_WORKSPACE;
  Grp g{};
  g.ws = (long)slice;
  g.count = count;
  for (int z = 0; z < count; ++z) {
    g.G[z] = aga == PT2Q_AGA_ACT ? A[z] : nullptr;
    g.Hinv[z] = Hinv[z];
  }
  return run_blocks(count, W, wdtype, ldw, n, m, b, flags, A, lda, Hinv, ldhi, max_iter, alpha, mu, T, tdtype,
                    perm, iters_dev, w, &g, perm64, st);
}

extern "C" int pt2q_quantize_layer(const void* W, int wdtype, int64_t ldw, int n, int m,
                                   const void* X, int xdtype, int64_t N, int64_t ldx, int b,
                                   int flags, float percdamp, int max_iter, float* alpha,
                                   float* mu, void* T, int tdtype, int64_t* perm, int* iters_dev,
                                   int* info_dev, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!W || !X || !info_dev || N <= 0 || N > INT_MAX || m <= 0 || n <= 0 || b <= 0 ||
      !dtype_ok(xdtype) || !dtype_ok(wdtype) || ldx < m || ldw < m || (flags & PT2Q_FLAG_S1_GIVEN) ||
      max_iter < 0)
    return PT2Q_E_ARG;
  Carve c{(char*)workspace, workspace_bytes};
  int rc;
  int* status = take_status(c, st, rc);
  if (rc != PT2Q_OK) return rc;
  float* G = c.take<float>((size_t)m * m);
  float* H = c.take<float>((size_t)m * m);
  float* Ui = c.take<float>((size_t)m * m);
  float* Hinv = c.take<float>((size_t)m * m);
  float* damp = c.take<float>(1);
  int* gflags = c.take<int>(pt2q_gram_flags_ints(m));
  BlockWs w;
  if (!c.ok || !carve_blocks(c, n, m, b, w)) return PT2Q_E_WORKSPACE;
  w.status = status;
  {
    GemmDesc g{};
    g.M = m; g.N = m; g.K = (int)N;
    g.A = X; g.lda = ldx; g.a_layout = LAY_KMAJOR;
    g.B = X; g.ldb = ldx; g.b_layout = LAY_KMAJOR;
    g.in_dtype = xdtype;
    g.C = G; g.ldc = m;
    g.mode = GEMM_STORE;
    g.upper = 1; g.mirror = 1;
    StageScope ts(PT2Q_TIMER_GRAM, st);
    if ((rc = pt2q_launch_gram(g, gflags, st, status)) != PT2Q_OK) return rc;
  }
  StageScope ts_inv(PT2Q_TIMER_INVERSE, st);
  // H is consumed in place as the Cholesky work matrix (variant M's AGA uses the raw Gram G), so
  // it is written in that form at once (strictly lower part zero; no separate copy pass).
  // Hinv only feeds the error feedback; a single block (per-channel, b >= m) has none, so the
  // factorisation would be dead work: skip it and report success.
  const bool upper = b < m && m <= SUMN_LDS_MAX;
  if ((rc = pt2q_launch_prepare_hessian(G, m, m, N, percdamp, H, m, damp, st, upper)) != PT2Q_OK) return rc;
  if (b < m) {
    if ((rc = pt2q_launch_cholesky_inverse(H, m, m, Hinv, m, H, Ui, info_dev, st, upper)) != PT2Q_OK)
      return rc;
  } else if (hipMemsetAsync(info_dev, 0, sizeof(int), st) != hipSuccess) {
    return PT2Q_E_HIP;
  }
  ts_inv.close();
  int f = (flags & ~PT2Q_AGA_MASK) | PT2Q_AGA_ACT;
  const float* Gc = G;
  const float* Hc = Hinv;
  return run_blocks(1, &W, wdtype, ldw, n, m, b, f, &Gc, m, &Hc, m, max_iter, &alpha, &mu, &T, tdtype,
                    &perm, &iters_dev, w, nullptr, nullptr, st);
}

extern "C" int pt2q_s1_from_gram(const float* S, int64_t lds, int b, float* S1, float* d_dev,
                                 void* stream) {
  if (!S || !S1 || !d_dev || b <= 0 || lds < b) return PT2Q_E_ARG;
  return pt2q_launch_s1(S, lds, nullptr, b, S1, d_dev, (hipStream_t)stream);
}

extern "C" int pt2q_s1_from_gram_batched(const float* S, int64_t lds, int m, int batch, int64_t item_stride,
                                         float* S1d, void* stream) {
  if (!S || !S1d || m <= 0 || batch < 0 || lds < m || (batch > 1 && item_stride < lds * m)) return PT2Q_E_ARG;
  if (batch == 0) return PT2Q_OK;
  StageScope ts(PT2Q_TIMER_ATQ, (hipStream_t)stream);  // the AGA's S1 / d (quantizer.py:215-218)
  return pt2q_launch_s1(S, lds, nullptr, m, S1d, S1d + m, (hipStream_t)stream, batch, item_stride, m + 1, S1_GRAMS);
}

extern "C" int pt2q_s1_from_upper_batched(const float* S, int64_t lds, int m, int batch, int64_t item_stride,
                                          float* S1d, void* stream) {
  if (!S || !S1d || m <= 0 || batch < 0 || lds < m || (batch > 1 && item_stride < lds * m)) return PT2Q_E_ARG;
  if (batch == 0) return PT2Q_OK;
  StageScope ts(PT2Q_TIMER_ATQ, (hipStream_t)stream);
  return pt2q_launch_s1(S, lds, nullptr, m, S1d, S1d + m, (hipStream_t)stream, batch, item_stride, m + 1,
                        S1_UPPER_GRAMS);
}

extern "C" int pt2q_ssr_select(const float* W, int64_t ldw, int n, int m, const int64_t* rem, int r,
                               int b, int64_t* blk, int64_t* newrem, float* sim, void* workspace,
                               size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!W || !rem || !blk || n <= 0 || m <= 0 || r <= 0 || r > m || b <= 0 || ldw < m) return PT2Q_E_ARG;
  if (r > b && !newrem) return PT2Q_E_ARG;
  Carve c{(char*)workspace, workspace_bytes};
  BlockWs w;
  int rc;
  w.status = take_status(c, st, rc);
  if (rc != PT2Q_OK) return rc;
  if (!carve_blocks(c, n, m, 128, w)) return PT2Q_E_WORKSPACE;
  if ((rc = pt2q_launch_transpose_to_f32(W, PT2Q_F32, ldw, n, m, w.Wt, w.ldw, st)) != PT2Q_OK) return rc;
  hipLaunchKernelGGL(i64_to_i32_kernel, dim3(ceil_div(r, 256)), dim3(256), 0, st, rem, r, w.rem[0]);
  PT2Q_LAUNCH_CHECK();
  const int bs = r < b ? r : b;
  // blk indices (int32) are staged in rem[1] (capacity m >= b); newrem in the Tt scratch
  int* blk32 = w.rem[1];
  int* nrem32 = (int*)w.Tt;  // m*ldw bytes >= 4m
  if (sim || r > b) {
    float* part = w.ssr;
    float* wn = part + (size_t)ceil_div(m, 128) * n;
    float* simb = sim ? sim : wn + n;
    int* cnt = w.counters + 4 * ceil_div(m, 128);
    if (hipMemsetAsync(cnt, 0, sizeof(int) * pt2q_ssr_counter_ints(n), st) != hipSuccess) return PT2Q_E_HIP;
    if ((rc = pt2q_launch_ssr_similarity(w.Wt, w.ldw, n, w.rem[0], r, part, wn, simb, st, cnt)) != PT2Q_OK)
      return rc;
    if (r > b) {
      if ((rc = pt2q_launch_ssr_topk(simb, w.rem[0], r, b, blk32, nrem32, nullptr, st)) != PT2Q_OK)
        return rc;
      hipLaunchKernelGGL(i32_to_i64_kernel, dim3(ceil_div(r - bs, 256)), dim3(256), 0, st, nrem32,
                         r - bs, newrem);
      PT2Q_LAUNCH_CHECK();
    }
  }
  if (r <= b) blk32 = w.rem[0];
  hipLaunchKernelGGL(i32_to_i64_kernel, dim3(ceil_div(bs, 256)), dim3(256), 0, st, blk32, bs, blk);
  PT2Q_LAUNCH_CHECK();
  return PT2Q_OK;
}

// ---- static reorder (reorder.py:15-33, :81-104)
extern "C" size_t pt2q_cosine_similarity_workspace_bytes(int n, int m) {
  if (n <= 0 || m <= 0) return 0;
  Carve c{nullptr, 0};
  c.dry = true;
  c.take<int>(PT2Q_STATUS_BYTES / sizeof(int));
  c.take<float>((size_t)m);                          // column norms
  c.take<float>((size_t)n * round_up(m, 4));         // Wn
  return c.used;
}

extern "C" int pt2q_cosine_similarity(const void* W, int wdtype, int64_t ldw, int n, int m, float* S,
                                      int64_t lds, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!W || !S || n <= 0 || m <= 0 || !dtype_ok(wdtype) || ldw < m || lds < m) return PT2Q_E_ARG;
  if (!workspace || workspace_bytes < pt2q_cosine_similarity_workspace_bytes(n, m)) return PT2Q_E_WORKSPACE;
  Carve c{(char*)workspace, workspace_bytes};
  int rc;
  take_status(c, st, rc);  // reserved (every Gram tile is one chain: nothing waits on another workgroup)
  if (rc != PT2Q_OK) return rc;
  const long ldn = round_up(m, 4);  // 16-byte rows: the Gram's vector loads apply when m % 4 == 0
  float* nrm = c.take<float>((size_t)m);
  float* Wn = c.take<float>((size_t)n * ldn);
  if (!c.ok) return PT2Q_E_WORKSPACE;
  if ((rc = pt2q_launch_colnorm_normalize(W, wdtype, ldw, n, m, nrm, Wn, ldn, st)) != PT2Q_OK) return rc;
  GemmDesc g{};
  g.M = m; g.N = m; g.K = n;
  g.A = Wn; g.lda = ldn; g.a_layout = LAY_KMAJOR;
  g.B = Wn; g.ldb = ldn; g.b_layout = LAY_KMAJOR;
  g.in_dtype = PT2Q_F32;
  g.C = S; g.ldc = lds;
  g.mode = GEMM_STORE;
  g.upper = 1; g.mirror = 1;
  return pt2q_launch_gram(g, nullptr, st);
}

extern "C" size_t pt2q_ssr_static_order_workspace_bytes(int m) {
  if (m <= 0) return 0;
  Carve c{nullptr, 0};
  c.dry = true;
  c.take<int>(PT2Q_STATUS_BYTES / sizeof(int));
  c.take<float>((size_t)m + 1);  // row sums, then their total (pt2q_s1_from_gram_batched's layout)
  return c.used;
}

extern "C" int pt2q_ssr_static_order(const float* S, int64_t lds, int m, int64_t* perm, int64_t* inv_perm,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!S || !perm || m <= 0 || lds < m) return PT2Q_E_ARG;
  if (m > PT2Q_STATIC_ORDER_MAX) return PT2Q_E_UNSUPPORTED;
  if (!workspace || workspace_bytes < pt2q_ssr_static_order_workspace_bytes(m)) return PT2Q_E_WORKSPACE;
  Carve c{(char*)workspace, workspace_bytes};
  int rc;
  take_status(c, st, rc);  // reserved (one workgroup: nothing waits on another)
  if (rc != PT2Q_OK) return rc;
  float* S1d = c.take<float>((size_t)m + 1);
  if (!c.ok) return PT2Q_E_WORKSPACE;
  if ((rc = pt2q_launch_s1(S, lds, nullptr, m, S1d, S1d + m, st, 1, 0, 0, S1_GRAMS)) != PT2Q_OK) return rc;
  return pt2q_launch_greedy_order(S, lds, m, S1d, perm, inv_perm, st);
}

// ---- standalone error feedback (main.py:187-214 / gptq.py:158-186 for one block)
extern "C" size_t pt2q_error_feedback_workspace_bytes(int n, int m, int bs) {
  if (n <= 0 || m <= 0 || bs <= 0) return 0;
  Carve c{nullptr, 0};
  c.dry = true;
  const long ldW = round_up(n, 64);
  c.take<int>(PT2Q_STATUS_BYTES / sizeof(int));
  c.take<float>((size_t)m * ldW);
  c.take<float>((size_t)bs * ldW);
  c.take<float>((size_t)bs * round_up(m, 4));
  c.take<int>((size_t)bs);
  c.take<int>((size_t)m);
  return c.used;
}

extern "C" int pt2q_error_feedback(float* W, int64_t ldw, int n, int m, const int64_t* blk, int bs,
                                   const int64_t* rem, int r, const float* E, int64_t lde,
                                   const float* Hinv, int64_t ldhi, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!W || !blk || !E || !Hinv || n <= 0 || m <= 0 || bs <= 0 || r < 0 || bs + r > m ||
      ldw < m || lde < bs || ldhi < m || (r > 0 && !rem))
    return PT2Q_E_ARG;
  if (r == 0) return PT2Q_OK;
  Carve c{(char*)workspace, workspace_bytes};
  int rc;
  take_status(c, st, rc);  // reserved (nothing in this call waits on another workgroup)
  if (rc != PT2Q_OK) return rc;
  const long ldW = round_up(n, 64), ldc = round_up(m, 4);
  float* Wt = c.take<float>((size_t)m * ldW);
  float* Et = c.take<float>((size_t)bs * ldW);
  float* Ck = c.take<float>((size_t)bs * ldc);
  int* blk32 = c.take<int>((size_t)bs);
  int* rem32 = c.take<int>((size_t)m);
  if (!c.ok) return PT2Q_E_WORKSPACE;
  // feature-major working copies: column gathers W[:, rem] become row gathers of Wt
  if ((rc = pt2q_launch_transpose_to_f32(W, PT2Q_F32, ldw, n, m, Wt, ldW, st)) != PT2Q_OK) return rc;
  if ((rc = pt2q_launch_transpose_to_f32(E, PT2Q_F32, lde, n, bs, Et, ldW, st)) != PT2Q_OK) return rc;
  hipLaunchKernelGGL(i64_to_i32_kernel, dim3(ceil_div(bs, 256)), dim3(256), 0, st, blk, bs, blk32);
  PT2Q_LAUNCH_CHECK();
  hipLaunchKernelGGL(i64_to_i32_kernel, dim3(ceil_div(r, 256)), dim3(256), 0, st, rem, r, rem32);
  PT2Q_LAUNCH_CHECK();
  // C[k][e] = Hinv[blk_k][rem_e] / clamp(Hinv[blk_k][blk_k], 1e-8)   (main.py:201-209)
  if ((rc = pt2q_launch_ef_coeffs(Hinv, ldhi, blk32, bs, rem32, r, Ck, ldc, st)) != PT2Q_OK) return rc;
  // W[:, rem] -= E @ C   (main.py:214: product rounded, then one subtraction)
  rc = pt2q_launch_ef(Ck, ldc, Et, Wt, ldW, m, rem32, r, bs, st);
  if (rc == PT2Q_E_UNSUPPORTED) {
    GemmDesc g{};
    g.M = r; g.N = n; g.K = bs;
    g.A = Ck; g.lda = ldc; g.a_layout = LAY_KMAJOR;
    g.B = Et; g.ldb = ldW; g.b_layout = LAY_KMAJOR;
    g.in_dtype = PT2Q_F32;
    g.C = Wt; g.ldc = ldW; g.crow = rem32;
    g.mode = GEMM_SUB;
    rc = pt2q_launch_gemm(g, st);
  }
  if (rc != PT2Q_OK) return rc;
  return pt2q_launch_transpose_f32(Wt, ldW, m, n, W, ldw, st);
}

// ---- per-layer error report from the Gram (quantizer.py:296-306 in Gram form; layer_report.hip)
namespace {

struct ReportCarve {
  int* blockof;
  float *At, *partw, *part, *rows, *tsc;
  long npad, R;
};

// rows: the A operand's data rows (n, or n D rows and n W rows at offset npad); `codes`: the
// residual path's block table and ew partials
ReportCarve report_carve(Carve& c, int n, int m, bool two, bool codes) {
  ReportCarve r{};
  r.npad = round_up(n, 128);
  r.R = two ? 2 * r.npad : r.npad;
  const size_t nch = (size_t)ceil_div(m, 32);
  if (codes) r.blockof = c.take<int>((size_t)m);
  r.At = c.take<float>((size_t)m * r.R);
  if (codes) r.partw = c.take<float>(nch * r.npad);
  r.part = c.take<float>(nch * r.R);
  r.rows = c.take<float>((size_t)3 * n);                      // stand-ins for NULL per-row outputs
  r.tsc = c.take<float>((size_t)3 * ceil_div(n, 32) + 4);     // totals scratch
  return r;
}

}  // namespace

extern "C" size_t pt2q_quadform_rows_workspace_bytes(int rows, int m) {
  if (rows <= 0 || m <= 0) return 0;
  Carve c{nullptr, 0};
  c.dry = true;
  c.take<int>(PT2Q_STATUS_BYTES / sizeof(int));
  report_carve(c, rows, m, false, false);
  return c.used;
}

extern "C" int pt2q_quadform_rows(const void* A, int adtype, int64_t lda, int rows, int m, const float* G,
                                  int64_t ldg, float* q, float* total, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!A || !G || rows <= 0 || m <= 0 || !dtype_ok(adtype) || lda < m || ldg < m) return PT2Q_E_ARG;
  if (!workspace || workspace_bytes < pt2q_quadform_rows_workspace_bytes(rows, m)) return PT2Q_E_WORKSPACE;
  Carve c{(char*)workspace, workspace_bytes};
  int rc;
  take_status(c, st, rc);  // reserved (nothing in this call waits on another workgroup)
  if (rc != PT2Q_OK) return rc;
  const ReportCarve w = report_carve(c, rows, m, false, false);
  if (!c.ok) return PT2Q_E_WORKSPACE;
  float* qv = q ? q : w.rows;
  if ((rc = pt2q_launch_report_residual(2, A, adtype, lda, rows, m, nullptr, PT2Q_I8, 0, nullptr, nullptr, 1,
                                        nullptr, w.At, w.R, w.R, 0, nullptr, 0, st)) != PT2Q_OK)
    return rc;
  if ((rc = pt2q_launch_quadform_rows(w.At, w.R, w.R, m, G, ldg, w.part, w.R, st)) != PT2Q_OK) return rc;
  if ((rc = pt2q_launch_rowtree_finish(w.part, w.R, m, 0, rows, qv, st)) != PT2Q_OK) return rc;
  if (total) return pt2q_launch_rowtree_totals(qv, nullptr, nullptr, 1, rows, w.tsc, total, st);
  return PT2Q_OK;
}

extern "C" size_t pt2q_layer_report_workspace_bytes(int n, int m, int flags) {
  if (n <= 0 || m <= 0) return 0;
  Carve c{nullptr, 0};
  c.dry = true;
  c.take<int>(PT2Q_STATUS_BYTES / sizeof(int));
  report_carve(c, n, m, (flags & PT2Q_REPORT_REF) != 0, true);
  return c.used;
}

extern "C" int pt2q_layer_report(const void* W, int wdtype, int64_t ldw, int n, int m, int b, const float* alpha,
                                 const float* mu, const void* T, int tdtype, int64_t ldt, const int64_t* perm,
                                 const float* G, int64_t ldg, int flags, float* ew, float* ex, float* ey,
                                 float* totals, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!W || !T || !alpha || !mu || n <= 0 || m <= 0 || b <= 0 || !dtype_ok(wdtype) ||
      (tdtype != PT2Q_I8 && tdtype != PT2Q_F32) || ldw < m || ldt < m || (G && ldg < m) ||
      (flags & ~PT2Q_REPORT_REF))
    return PT2Q_E_ARG;
  if (!workspace || workspace_bytes < pt2q_layer_report_workspace_bytes(n, m, flags)) return PT2Q_E_WORKSPACE;
  Carve c{(char*)workspace, workspace_bytes};
  int rc;
  take_status(c, st, rc);  // reserved (nothing in this call waits on another workgroup)
  if (rc != PT2Q_OK) return rc;
  const bool ref = (flags & PT2Q_REPORT_REF) && G;  // ey needs the Gram
  // the carve is the size function's (flags alone); without G the W half stays unused
  const ReportCarve w = report_carve(c, n, m, (flags & PT2Q_REPORT_REF) != 0, true);
  if (!c.ok) return PT2Q_E_WORKSPACE;
  const long R = ref ? 2 * w.npad : w.npad;
  const int B = (b < m) ? ceil_div(m, b) : 1, bb = (b < m) ? b : m;  // as pt2q_dequantize
  float* ewv = ew ? ew : w.rows;
  float* exv = ex ? ex : w.rows + n;
  float* eyv = ey ? ey : w.rows + 2 * (size_t)n;
  if ((rc = pt2q_launch_report_blockof(perm, m, bb, w.blockof, st)) != PT2Q_OK) return rc;
  if ((rc = pt2q_launch_report_residual(ref ? 1 : 0, W, wdtype, ldw, n, m, T, tdtype, ldt, alpha, mu, B, w.blockof,
                                        w.At, R, w.npad, w.npad, w.partw, w.npad, st)) != PT2Q_OK)
    return rc;
  if ((rc = pt2q_launch_rowtree_finish(w.partw, w.npad, m, 0, n, ewv, st)) != PT2Q_OK) return rc;
  if (G) {
    if ((rc = pt2q_launch_quadform_rows(w.At, R, R, m, G, ldg, w.part, R, st)) != PT2Q_OK) return rc;
    if ((rc = pt2q_launch_rowtree_finish(w.part, R, m, 0, n, exv, st)) != PT2Q_OK) return rc;
    if (ref && (rc = pt2q_launch_rowtree_finish(w.part, R, m, w.npad, n, eyv, st)) != PT2Q_OK) return rc;
  }
  if (totals)
    return pt2q_launch_rowtree_totals(ewv, G ? exv : nullptr, ref ? eyv : nullptr, 3, n, w.tsc, totals, st);
  return PT2Q_OK;
}
