// STFT kernel instantiations for ONE transform precision (SSR_TU_T) and ONE part of the variant space (SSR_TU_PART);
// included by the tu_stft_*.hip units.  Parts:
//   0  direct / Bluestein engines, (est, target) pairs of float32 signals
//   1  direct / Bluestein engines, pairs with float64 signals (IN64 = 1, 3)
//   2  direct / Bluestein engines, frame pairs of ONE signal (wav_to_spectrogram, FDomainHelper)
//   3  radix-3 engine: float32 pairs + single
//   4  radix-3 engine: pairs with float64 signals
#include "ssr_host.h"
#include "ssr_stft_r3.h"
#include "ssr_stft_wave.h"
#include "ssr_stft_rn_wave.h"
#include "ssr_stft_r3_rot.h"

typedef SSR_TU_T TT;
static_assert(SSR_W_N == SSR_WAVE_N && SSR_W_TWP == SSR_WAVE_TWP && SSR_W_WCS_OFF == SSR_WAVE_WCS_OFF, "ssr_tables.h appends what ssr_stft_wave.h reads");
static_assert(SSR_W24_N == SSR_WAVE24_N && SSR_W24_TWP == SSR_WAVE24_TWP, "ssr_tables.h appends what ssr_fft24.h reads");

// Minimum waves per SIMD asked of the register allocator.  The 2048-point direct kernel without running
// SISpec sums fits 128 VGPRs with no spill, which admits a 4th workgroup per CU (-4.5 % time, measured);
// the variant that carries the six sums would spill at 128, so it stays at 3.
constexpr int ssr_stft_min_waves(int logn, bool blu, bool sums) { return (logn == 11 && !blu && !sums) ? 4 : 1; }

#if SSR_TU_PART <= 2
// E64 (SSR_IN_EST64 / SSR_IN_BOTH64): float64 signals (pair mode only); their float64 epilogue needs more registers,
// so those variants are left to the allocator (min waves 1).
template <typename T, int LOGN, bool BLU, int MODE, bool SUMS, int E64>
__global__ __launch_bounds__((1 << LOGN) / ssr_stft_ppt(LOGN, BLU), E64 ? 1 : ssr_stft_min_waves(LOGN, BLU, SUMS))
void k_stft(SsrStftParams<T> p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  SsrBlk blk{(int)threadIdx.x};
  const int item = blockIdx.x / p.n_chunks, chunk = blockIdx.x % p.n_chunks;
  ssr_stft_body<T, LOGN, BLU, MODE, SUMS, ssr_stft_ppt(LOGN, BLU), E64>(p, blk, chunk, item, smem);
}

template <typename T, int LOGN, bool BLU, int MODE, bool SUMS, int E64 = 0>
static int launch_stft_mode(SsrStftParams<T>& p, int grid, hipStream_t s) {
  constexpr int PPT = ssr_stft_ppt(LOGN, BLU);
  const size_t lds = SsrStftLds<T, LOGN, PPT>::bytes();
  static thread_local SsrLdsSlot slot;
  if (int rc = ssr_allow_lds((const void*)k_stft<T, LOGN, BLU, MODE, SUMS, E64>, lds, &slot)) return rc;
  hipLaunchKernelGGL((k_stft<T, LOGN, BLU, MODE, SUMS, E64>), dim3(grid), dim3((1 << LOGN) / PPT), lds, s, p);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}

template <typename T, int LOGN, bool BLU> static int launch_stft_inst(SsrStftParams<T>& p, int grid, hipStream_t s) {
  const bool sums = p.metric_mask & (SSR_M_SISPEC | SSR_M_LOG_SISPEC);
  (void)sums;
#if SSR_TU_PART == 2
  return launch_stft_mode<T, LOGN, BLU, SSR_MODE_SINGLE, false>(p, grid, s);
#elif SSR_TU_PART == 1
  if (p.a64 && p.b64)
    return sums ? launch_stft_mode<T, LOGN, BLU, SSR_MODE_PAIR, true, SSR_IN_BOTH64>(p, grid, s)
                : launch_stft_mode<T, LOGN, BLU, SSR_MODE_PAIR, false, SSR_IN_BOTH64>(p, grid, s);
  return sums ? launch_stft_mode<T, LOGN, BLU, SSR_MODE_PAIR, true, SSR_IN_EST64>(p, grid, s)
              : launch_stft_mode<T, LOGN, BLU, SSR_MODE_PAIR, false, SSR_IN_EST64>(p, grid, s);
#else
  return sums ? launch_stft_mode<T, LOGN, BLU, SSR_MODE_PAIR, true>(p, grid, s)
              : launch_stft_mode<T, LOGN, BLU, SSR_MODE_PAIR, false>(p, grid, s);
#endif
}

#if SSR_TU_PART == 0
// Wave-autonomous engine (ssr_stft_wave.h) for the 2048-point direct pair transform: one wave per workgroup.
// SPLIT = false: 33 KB (float64) of LDS per wave -> 4 waves per CU, 1 per SIMD, register budget 512;
// SPLIT = true : 17 KB -> 8 waves per CU, 2 per SIMD, register budget 256 (the kernel fits it without a spill).
// Measured (1024 pairs, LSD + magnitudes): 3.8 ms at one wave per SIMD - every LDS / memory issue slot and wait is exposed -
// against 2.9 ms at two (profiles/r02_notes.md); the four-waves-per-frame engine it replaces: 3.3 ms.  The product launches
// SPLIT = true (the host emulation tests both layouts).
// Block mapping under interleaving (S = p.interleave > 1): logical workgroup L = item * n_chunks + chunk = G * S + j (group G,
// member j).  The S members of a group must share an L2 and run together: workgroups are dealt to the 8 XCDs round-robin by
// blockIdx, so group G takes blockIdx = ((G / 8) * S + j) * 8 + G % 8 - the same XCD for every j, dispatched back to back.
// The grid is padded to whole rounds of 8 groups (n_groups: the real count; the padding exits).
// Two waves per SIMD for float32 too: at three the float32 kernel spills (LSD 1.57 ms against 1.54, with magnitudes 2.42 against
// 2.14), at four far more (profiles/r06_notes.md).
template <typename T, bool SUMS, bool SPLIT, bool MAG>
__global__ __launch_bounds__(64, SPLIT ? 2 : 1) void k_stft_wave(SsrStftParams<T> p, int n_groups) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  SsrBlk blk{(int)threadIdx.x};
  int logical = (int)blockIdx.x;
  if (p.interleave > 1) {
    const int S = p.interleave, xcd = (int)blockIdx.x & 7, slot = (int)blockIdx.x >> 3;
    const int G = (slot / S) * 8 + xcd;
    if (G >= n_groups) return;
    logical = G * S + slot % S;
  }
  const int item = logical / p.n_chunks, chunk = logical % p.n_chunks;
  ssr_stft_wave_body<T, SUMS, SPLIT, MAG ? 1 : 0>(p, blk, chunk, item, smem);
}
template <typename T, bool SUMS> static int launch_stft_wave(SsrStftParams<T>& p, int grid, hipStream_t s) {
  const size_t lds = ssr_stft_wave_lds_bytes<T, true, SUMS>();
  int n_groups = grid;
  if (p.interleave > 1) {
    if (p.n_chunks % p.interleave) return ssr_fail(SSR_ERR_INVALID_ARG, "interleaved chunks: n_chunks must be a multiple of the group size");
    n_groups = grid / p.interleave;
    grid = ssr_ceil_div(n_groups, 8) * 8 * p.interleave;
  }
  if (p.out_kind == SSR_OUT_MAG) hipLaunchKernelGGL((k_stft_wave<T, SUMS, true, true>), dim3(grid), dim3(64), lds, s, p, n_groups);
  else hipLaunchKernelGGL((k_stft_wave<T, SUMS, true, false>), dim3(grid), dim3(64), lds, s, p, n_groups);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}
#endif

static int launch_stft_part(const ssr_plan* pl, SsrStftParams<TT>& p, int grid, hipStream_t s) {
#if SSR_TU_PART == 0
  if (ssr_stft_uses_wave_engine(pl, false)) {
    const bool sums = p.metric_mask & (SSR_M_SISPEC | SSR_M_LOG_SISPEC);
    return sums ? launch_stft_wave<TT, true>(p, grid, s) : launch_stft_wave<TT, false>(p, grid, s);
  }
#endif
#define CASE(L)                                                                   \
  case L:                                                                         \
    return pl->eng.bluestein ? launch_stft_inst<TT, L, true>(p, grid, s) : launch_stft_inst<TT, L, false>(p, grid, s);
  switch (pl->eng.logn) { CASE(8) CASE(9) CASE(10) CASE(11) CASE(12)
    case 13: return launch_stft_inst<TT, 13, true>(p, grid, s);
  }
#undef CASE
  return ssr_fail(SSR_ERR_UNSUPPORTED, "no kernel for this FFT length");
}

#if SSR_TU_PART == 0
template <> int ssr_launch_stft_pair<TT>(const ssr_plan* pl, SsrStftParams<TT>& p, int grid, hipStream_t s) { return launch_stft_part(pl, p, grid, s); }
#elif SSR_TU_PART == 1
template <> int ssr_launch_stft_pair64<TT>(const ssr_plan* pl, SsrStftParams<TT>& p, int grid, hipStream_t s) { return launch_stft_part(pl, p, grid, s); }
#else
template <> int ssr_launch_stft_single<TT>(const ssr_plan* pl, SsrStftParams<TT>& p, int grid, hipStream_t s) { return launch_stft_part(pl, p, grid, s); }
#endif

#else  // ---------------------------------------------------------------- radix-3 engine
template <typename T, int LOGN, int MODE, bool SUMS, int E64>
__global__ __launch_bounds__((1 << LOGN) / 8) void k_stft_r3(SsrStftParams<T> p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  SsrBlk blk{(int)threadIdx.x};
  const int item = blockIdx.x / p.n_chunks, chunk = blockIdx.x % p.n_chunks;
  ssr_stft_r3_body<T, LOGN, MODE, SUMS, E64>(p, blk, chunk, item, smem);
}

template <typename T, int LOGN, int MODE, bool SUMS, int E64 = 0>
static int launch_stft_r3_mode(SsrStftParams<T>& p, int grid, hipStream_t s) {
  const size_t lds = SsrStftR3Lds<T, LOGN>::bytes(p.n_fft / 3);
  // the LDS size depends on q = n_fft / 3: remember the largest size this (kernel, device) was opted into
  static thread_local SsrLdsSlot slot;
  if (int rc = ssr_allow_lds((const void*)k_stft_r3<T, LOGN, MODE, SUMS, E64>, lds, &slot)) return rc;
  hipLaunchKernelGGL((k_stft_r3<T, LOGN, MODE, SUMS, E64>), dim3(grid), dim3((1 << LOGN) / 8), lds, s, p);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}

template <typename T, int LOGN> static int launch_stft_r3_inst(SsrStftParams<T>& p, int grid, hipStream_t s) {
  const bool sums = p.metric_mask & (SSR_M_SISPEC | SSR_M_LOG_SISPEC);
  (void)sums;
#if SSR_TU_PART == 3
  if (p.mode != SSR_MODE_PAIR) return launch_stft_r3_mode<T, LOGN, SSR_MODE_SINGLE, false>(p, grid, s);
  return sums ? launch_stft_r3_mode<T, LOGN, SSR_MODE_PAIR, true>(p, grid, s)
              : launch_stft_r3_mode<T, LOGN, SSR_MODE_PAIR, false>(p, grid, s);
#else
  if (p.a64 && p.b64)
    return sums ? launch_stft_r3_mode<T, LOGN, SSR_MODE_PAIR, true, SSR_IN_BOTH64>(p, grid, s)
                : launch_stft_r3_mode<T, LOGN, SSR_MODE_PAIR, false, SSR_IN_BOTH64>(p, grid, s);
  return sums ? launch_stft_r3_mode<T, LOGN, SSR_MODE_PAIR, true, SSR_IN_EST64>(p, grid, s)
              : launch_stft_r3_mode<T, LOGN, SSR_MODE_PAIR, false, SSR_IN_EST64>(p, grid, s);
#endif
}

#if SSR_TU_PART == 3
// n_fft = R q over M = 2048 (P = 32 points per lane) or M = 1536 (P = 24; q <= 768), float32 pairs: R autonomous waves per
// workgroup (ssr_stft_rn_wave.h)
// (NQ = 4: sixteen rows of 64 per wave, q in 769 .. 1024 - no AudioMetrics(rate) size - need more than 256 float64 registers: those
// instances take one wave per SIMD instead of 18 registers of scratch)
template <typename T, bool SUMS, int NW, int NQ, int P>
__global__ __launch_bounds__(64 * NW, (NQ == 4 && sizeof(T) == 8) ? 1 : 2) void k_stft_rn_wave(SsrStftParams<T> p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  SsrBlk blk{(int)threadIdx.x};
  const int item = blockIdx.x / p.n_chunks, chunk = blockIdx.x % p.n_chunks;
  ssr_stft_rn_wave_body<T, SUMS, NW, NQ, P>(p, blk, chunk, item, smem);
}
template <typename T, bool SUMS, int NW, int NQ, int P> static int launch_stft_rn_wave(SsrStftParams<T>& p, int grid, hipStream_t s) {
  const size_t lds = ssr_stft_rn_wave_lds_bytes<T, NW, SUMS, P>();
  static thread_local SsrLdsSlot slot;
  if (int rc = ssr_allow_lds((const void*)k_stft_rn_wave<T, SUMS, NW, NQ, P>, lds, &slot)) return rc;
  hipLaunchKernelGGL((k_stft_rn_wave<T, SUMS, NW, NQ, P>), dim3(grid), dim3(64 * NW), lds, s, p);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}
template <typename T, int NW, int NQ, int P> static int launch_stft_rn_wave_sums(SsrStftParams<T>& p, int grid, hipStream_t s) {
  return (p.metric_mask & (SSR_M_SISPEC | SSR_M_LOG_SISPEC)) ? launch_stft_rn_wave<T, true, NW, NQ, P>(p, grid, s)
                                                             : launch_stft_rn_wave<T, false, NW, NQ, P>(p, grid, s);
}
// n_fft = 3 q, q <= 768 (AudioMetrics(48000): 2229): four waves rotating through the sub-sequence transforms (ssr_stft_r3_rot.h)
template <typename T, bool SUMS, int NQ, int P, int IN64 = 0>
__global__ __launch_bounds__(64 * SSR_R3ROT_WAVES, 2) void k_stft_r3_rot(SsrStftParams<T> p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  SsrBlk blk{(int)threadIdx.x};
  const int item = blockIdx.x / p.n_chunks, chunk = blockIdx.x % p.n_chunks;
  ssr_stft_r3_rot_body<T, SUMS, NQ, P, IN64>(p, blk, chunk, item, smem);
}
template <typename T, bool SUMS, int NQ, int P, int IN64 = 0> static int launch_stft_r3_rot(SsrStftParams<T>& p, int grid, hipStream_t s) {
  const size_t lds = SsrR3RotLds<T, P>::bytes(p.n_fft / 3);
  static thread_local SsrLdsSlot slot;
  if (int rc = ssr_allow_lds((const void*)k_stft_r3_rot<T, SUMS, NQ, P, IN64>, lds, &slot)) return rc;
  hipLaunchKernelGGL((k_stft_r3_rot<T, SUMS, NQ, P, IN64>), dim3(grid), dim3(64 * SSR_R3ROT_WAVES), lds, s, p);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}
template <> int ssr_launch_stft_rn_wave<TT>(const ssr_plan* pl, SsrStftParams<TT>& p, int grid, hipStream_t s) {
  const bool wide = pl->weng.q > 768;                 // sixteen rows of 64 per wave instead of twelve
  if (pl->weng.m == SSR_W24_N) {                      // q <= 768: the 1536-point transforms
    switch (ssr_stft_rn_wave_radix(pl)) {
      case 1: return launch_stft_rn_wave_sums<TT, 1, 3, 24>(p, grid, s);
      case 2: return launch_stft_rn_wave_sums<TT, 2, 3, 24>(p, grid, s);
      case 3: {
        if constexpr (sizeof(TT) == 8) {
          if (p.a64 != nullptr && p.b64 != nullptr)      // two float64 estimates, images only (ssr_pair_metrics_multi_est64)
            return launch_stft_r3_rot<TT, false, 3, 24, SSR_IN_EST64X2>(p, grid, s);
        }
        if (p.a64 != nullptr)             // float64 estimate, float32 target (ssr_launch_stft sends nothing else with a64 here)
          return (p.metric_mask & (SSR_M_SISPEC | SSR_M_LOG_SISPEC)) ? launch_stft_r3_rot<TT, true, 3, 24, SSR_IN_EST64>(p, grid, s)
                                                                     : launch_stft_r3_rot<TT, false, 3, 24, SSR_IN_EST64>(p, grid, s);
        return (p.metric_mask & (SSR_M_SISPEC | SSR_M_LOG_SISPEC)) ? launch_stft_r3_rot<TT, true, 3, 24>(p, grid, s)
                                                                   : launch_stft_r3_rot<TT, false, 3, 24>(p, grid, s);
      }
    }
    return ssr_fail(SSR_ERR_UNSUPPORTED, "no wave kernel for this n_fft");
  }
  switch (ssr_stft_rn_wave_radix(pl)) {
    case 1: return wide ? launch_stft_rn_wave_sums<TT, 1, 4, 32>(p, grid, s) : launch_stft_rn_wave_sums<TT, 1, 3, 32>(p, grid, s);
    case 2: return wide ? launch_stft_rn_wave_sums<TT, 2, 4, 32>(p, grid, s) : launch_stft_rn_wave_sums<TT, 2, 3, 32>(p, grid, s);
    case 3: return launch_stft_rn_wave_sums<TT, 3, 3, 32>(p, grid, s);
  }
  return ssr_fail(SSR_ERR_UNSUPPORTED, "no wave kernel for this n_fft");
}
#endif

static int launch_stft_r3_part(const ssr_plan* pl, SsrStftParams<TT>& p, int grid, hipStream_t s) {
  switch (pl->eng.logn) {
    case 8: return launch_stft_r3_inst<TT, 8>(p, grid, s);
    case 9: return launch_stft_r3_inst<TT, 9>(p, grid, s);
    case 10: return launch_stft_r3_inst<TT, 10>(p, grid, s);
    case 11: return launch_stft_r3_inst<TT, 11>(p, grid, s);
  }
  return ssr_fail(SSR_ERR_UNSUPPORTED, "no radix-3 kernel for this FFT length");
}
#if SSR_TU_PART == 3
template <> int ssr_launch_stft_r3<TT>(const ssr_plan* pl, SsrStftParams<TT>& p, int grid, hipStream_t s) { return launch_stft_r3_part(pl, p, grid, s); }
#else
template <> int ssr_launch_stft_r3_64<TT>(const ssr_plan* pl, SsrStftParams<TT>& p, int grid, hipStream_t s) { return launch_stft_r3_part(pl, p, grid, s); }
#endif
#endif
