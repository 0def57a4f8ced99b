// Development probes: the ONE switchboard.  Every probe is a compile-time mask, 0 in the library
// build, so each hook (`if constexpr (probe::...)`, PT2Q_TOPK_STAMP, ...) compiles to nothing and
// no kernel argument carries a switch.  A probe program under tools/ compiles the kernel source in
// with -D<MASK>=<bits>; a whole knock-out library comes from `make EXTRA_HIPFLAGS=-D<MASK>=<bits>`
// (tools/build_variant_lib.sh) and is timed against the release build with tools/lib_ab.sh.
// Results of a knock-out build are garbage: it is for timing only.
//
//   PT2Q_PROBE          1, 2    Gram: no DMA / no MFMA          tools/gram16_probe.hip
//                       4       top-k phase timestamps          tools/topk_probe.hip
//                       8       EF: Wt loads / stores dropped   tools/build_ef_probe.sh
//                       64      ef2 start / end clock stamps    tools/build_ef_probe.sh, build_ef2_clock.sh
//   PT2Q_EF2_KPROBE     1 no Wt traffic, 2 operand DMAs from one chunk, 4 no MFMAs, 8 old-value
//                       loads from L2-hot rows, 16 stores to them    tools/build_ef2_clock.sh
//   PT2Q_EF2_G0_EARLY   stages before a tile's last at which column group 0's old values are
//                       loaded (default 3)                      tools/ef2_g0_ab.sh, ef2_g0_lib_ab.sh
//   PT2Q_EF2_STORE_AUX  cache policy of the Wt stores (default 0)    tools/ef2_store_ab.sh
//   PT2Q_ATQ_KPROBE     block ATQ (atq.hip): 1 rows skip the S1 wait, 2 no coefficient workgroups,
//                       4 rows skip ITF, 8 / 128 / 256 no code / error-term / scale stores, 16 no
//                       S1 workgroups, 32 no row gathers, 64 idle rows; per-channel ATQ
//                       (atq_pc.hip): 1 no code stores, 2 AGA with S1 = 1 (no S1 loads), 4 ITF
//                       skipped                                 tools/build_variant_lib.sh
#pragma once

#ifndef PT2Q_PROBE
#define PT2Q_PROBE 0
#endif
#ifndef PT2Q_EF2_KPROBE
#define PT2Q_EF2_KPROBE 0
#endif
#ifndef PT2Q_EF2_G0_EARLY
#define PT2Q_EF2_G0_EARLY 3
#endif
#ifndef PT2Q_EF2_STORE_AUX
#define PT2Q_EF2_STORE_AUX 0
#endif
#ifndef PT2Q_ATQ_KPROBE
#define PT2Q_ATQ_KPROBE 0
#endif

namespace probe {
constexpr bool gram_no_dma = (PT2Q_PROBE & 1) != 0;   // tools/gram16_probe.hip: compute-only (stale LDS)
constexpr bool gram_no_mfma = (PT2Q_PROBE & 2) != 0;  // tools/gram16_probe.hip: fetch-only
constexpr bool topk_stamps = (PT2Q_PROBE & 4) != 0;   // tools/topk_probe.hip: phase timestamps
constexpr bool ef_drop_wt = (PT2Q_PROBE & 8) != 0;    // tools/ef_probe.hip: Wt loads / stores dropped
// block ATQ (atq.hip)
constexpr bool atq_no_s1_wait = (PT2Q_ATQ_KPROBE & 1) != 0;
constexpr bool atq_no_coeff = (PT2Q_ATQ_KPROBE & 2) != 0;
constexpr bool atq_no_itf = (PT2Q_ATQ_KPROBE & 4) != 0;
constexpr bool atq_no_codes = (PT2Q_ATQ_KPROBE & 8) != 0;
constexpr bool atq_no_s1_wgs = (PT2Q_ATQ_KPROBE & 16) != 0;
constexpr bool atq_no_gather = (PT2Q_ATQ_KPROBE & 32) != 0;
constexpr bool atq_idle_rows = (PT2Q_ATQ_KPROBE & 64) != 0;
constexpr bool atq_no_et = (PT2Q_ATQ_KPROBE & 128) != 0;
constexpr bool atq_no_scales = (PT2Q_ATQ_KPROBE & 256) != 0;
// per-channel ATQ (atq_pc.hip)
constexpr bool pc_no_codes = (PT2Q_ATQ_KPROBE & 1) != 0;
constexpr bool pc_s1_one = (PT2Q_ATQ_KPROBE & 2) != 0;
constexpr bool pc_no_itf = (PT2Q_ATQ_KPROBE & 4) != 0;
}  // namespace probe

#if (PT2Q_PROBE & 4) != 0
// thread 0 of each of the first 64 workgroups of the top-k launch: s_memtime at phase i
__device__ long long topk_stamps[64][16];
#define PT2Q_TOPK_STAMP(i) \
  if (threadIdx.x == 0 && blockIdx.x < 64) topk_stamps[blockIdx.x][i] = __builtin_amdgcn_s_memtime()
#else
#define PT2Q_TOPK_STAMP(i)
#endif

#if (PT2Q_PROBE & 64) != 0
// ef2_gemm_kernel: thread 0 of each workgroup, s_memtime (shader clock) and s_memrealtime
// (100 MHz) at the kernel's start (i = 0) and end (i = 1): the clock the launch ran at
__device__ long long ef2_clk[1024][4];
#define PT2Q_EF2_CLK(i)                                                  \
  if (threadIdx.x == 0 && blockIdx.x < 1024) {                           \
    ef2_clk[blockIdx.x][2 * (i)] = __builtin_amdgcn_s_memtime();         \
    ef2_clk[blockIdx.x][2 * (i) + 1] = __builtin_amdgcn_s_memrealtime(); \
  }
#else
#define PT2Q_EF2_CLK(i)
#endif
