// What the per-pair waveform metric families share (ssr_stoi.h, ssr_wave_metrics.h, ssr_quality.h, ssr_pitch.h, ssr_phase.h,
// ssr_mrstft.h, ssr_bss.h, ssr_coherence.h, ssr_spectrum.h, ssr_auditory.h, ssr_loudness.h, ssr_modulation.h, ssr_csii.h): estimate e
// is scored against target tgt_index[e], consecutive pairs that name one target form a run, and every
// grid is a prefix sum of per-item counts (tiles, frames, chunks) that a workgroup finds its item in.  ssr_run_geometry_body builds
// the prefixes of wave, quality, bss, coherence, spectrum (over its n_tgt + n_est signals) and csii; stoi, pitch, phase, mrstft,
// auditory, loudness (signals, no pairs) and modulation (through ssr_auditory.h) build their own and share ssr_prefix_find.
// Compiles on the device
// and under SSR_HOST_EMU (tests/emu/*_emu.cpp).  A new family uses these and re-implements none of them; what stays its own is
// its count function, its *Params struct (taken by value by its kernels: no common base) and its kernel bodies.
#pragma once
#include "ssr_block.h"
#include <type_traits>

#define SSR_PAIRS_NT 256                   // threads of the run-geometry workgroup

// largest s in [0, n) with off[s] <= g (off ascending, off[0] = 0): the item that owns grid block g.  Items with a count of
// zero repeat their successor's entry and are never returned for a g below off[n]
SSR_HD int ssr_prefix_find(const int64_t* off, int n, int64_t g) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// metrics selected by the bit mask `which`, and the output column of metric bit b (columns in bit order)
SSR_HD int ssr_which_count(int which) { return __builtin_popcount((unsigned)which); }
SSR_HD int ssr_which_col(int which, int bit) { return ssr_which_count(which & (bit - 1)); }

// the eight signal fields every per-pair parameter struct names alike
template <typename P>
SSR_HD void ssr_set_pair_sig(P& p, const void* tgt, const int64_t* tgt_off, const void* est, const int64_t* est_off,
                             const int32_t* tgt_len, const int32_t* tgt_index, int n_tgt, int n_est) {
  p.tgt = tgt; p.tgt_off = tgt_off; p.est = est; p.est_off = est_off; p.tgt_len = tgt_len; p.tgt_index = tgt_index;
  p.n_tgt = n_tgt; p.n_est = n_est;
}

// ---- run geometry: one workgroup of SSR_PAIRS_NT threads.  LDS: 3 * NT int64.
// count(len): the items (tiles, frames) of a target of len samples.  Writes run_start [n_runs + 1] (first pair of each run of
// consecutive pairs with one target; [n_runs] = n_est), run_pre [n_runs + 1] (item prefix over runs: a run's target is
// processed once), pair_pre [n_est + 1] (item prefix over pairs) and the frame window win [L],
// 0.5 (1 - cos(2 pi (i + 1) / (L + 1))).  Thread t owns pairs [t c, (t + 1) c), c = ceil(n_est / NT).
template <typename COUNT, typename BLK>
SSR_BODY void ssr_run_geometry_body(const int32_t* tgt_len, const int32_t* tgt_index, int n_est, COUNT count, int32_t* run_start,
                                    int64_t* run_pre, int64_t* pair_pre, double* win, int L, BLK& blk, int64_t* sums) {
  const int NT = SSR_PAIRS_NT, c = (n_est + NT - 1) / NT;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    int64_t runs = 0, rp = 0, pp = 0;
    for (int e = tid * c; e < n_est && e < (tid + 1) * c; ++e) {
      const int64_t m = count(tgt_len[tgt_index[e]]);
      if (e == 0 || tgt_index[e] != tgt_index[e - 1]) { ++runs; rp += m; }
      pp += m;
    }
    sums[tid] = runs; sums[NT + tid] = rp; sums[2 * NT + tid] = pp;
    for (int i = tid; i < L; i += NT) win[i] = 0.5 * (1.0 - cos(2.0 * M_PI * (double)(i + 1) / (double)(L + 1)));
  });
  SSR_PHASE(blk, regs, {
    if (tid < 3) {
      int64_t a = 0;
      for (int t = 0; t < NT; ++t) { const int64_t v = sums[tid * NT + t]; sums[tid * NT + t] = a; a += v; }
    }
  });
  SSR_PHASE(blk, regs, {
    int64_t r = sums[tid], rp = sums[NT + tid], pp = sums[2 * NT + tid];
    for (int e = tid * c; e < n_est && e < (tid + 1) * c; ++e) {
      const int64_t m = count(tgt_len[tgt_index[e]]);
      if (e == 0 || tgt_index[e] != tgt_index[e - 1]) {
        run_start[r] = e; run_pre[r] = rp;
        ++r; rp += m;
      }
      pair_pre[e] = pp;
      pp += m;
    }
    if (tid == NT - 1) { run_start[r] = n_est; run_pre[r] = rp; pair_pre[n_est] = pp; }   // (r = n_runs here)
  });
}

// f(std::integral_constant<int, LOGN>{}) for the LOGN in [LO, HI] that equals logn (the caller validated the range: HI otherwise)
template <int LO, int HI, typename F> inline auto ssr_dispatch_logn(int logn, F&& f) {
  if constexpr (LO < HI) {
    if (logn != LO) return ssr_dispatch_logn<LO + 1, HI>(logn, f);
  }
  return f(std::integral_constant<int, LO>{});
}
