// Host emulation of the delay stage's kernel bodies (ssr_eval_amd/csrc/ssr_align.h) for tests/test_align_host.py: every kernel of
// ssr_align run in launch order, one workgroup after another.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libalign_emu.so align_emu.cpp
#define SSR_HOST_EMU 1
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_align.h"

template <typename TT, typename TE> static void corr(SsrAlignParams& p, int64_t grid) {
  std::vector<double> xs(SSR_ALIGN_X_LDS), ys(SSR_ALIGN_Y_LDS), red(12);
  SsrBlk blk{SSR_ALIGN_NT};
  for (int64_t g = 0; g < grid; ++g) ssr_align_corr_body<TT, TE>(p, blk, g, xs.data(), ys.data(), red.data());
}

template <typename TE> static void shift(SsrAlignParams& p, int64_t grid) {
  std::vector<double> ysh(SSR_ALIGN_S_LDS), hs(SSR_ALIGN_TAPS);
  SsrBlk blk{SSR_ALIGN_NT};
  for (int64_t g = 0; g < grid; ++g) ssr_align_shift_body<TE>(p, blk, g, ysh.data(), hs.data());
}

// tgt / est: float32 or float64 signals at tgt + tgt_off[t] / est + est_off[e]; rows: [n_est][4]; shifted: the estimates' dtype at
// shifted + shifted_off[e], or null; c: [n_est][2 max_lag + 1] or null; taps_out: [n_est][33] or null
extern "C" int align_emu(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                         int est_f64, const int64_t* est_off, const int32_t* est_len, const int32_t* tgt_index, int n_est, int max_lag,
                         int subsample, double* rows, void* shifted, const int64_t* shifted_off, double* c, double* taps_out) {
  if (max_lag < 1 || max_lag > SSR_ALIGN_LAG_LIMIT) return -2;
  int64_t tiles = 0, outs = 0;
  for (int e = 0; e < n_est; ++e) { tiles += ssr_align_tiles(tgt_len[tgt_index[e]]); outs += ssr_align_out_tiles(est_len[e]); }
  const int NL = 2 * max_lag + 1;
  std::vector<int64_t> pt(n_est + 1, -1), po(n_est + 1, -1), sums(2 * SSR_ALIGN_NT);
  std::vector<double> cpart((size_t)tiles * NL + 1, -777.0), epart((size_t)tiles * 2 + 1, -777.0), taps((size_t)n_est * SSR_ALIGN_TAPS + 1, -777.0);
  SsrAlignParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, tgt_len, tgt_index, n_tgt, n_est);
  p.est_len = est_len; p.L = max_lag; p.subsample = subsample;
  p.pair_tile = pt.data(); p.pair_out = po.data(); p.cpart = cpart.data(); p.epart = epart.data(); p.taps = taps.data();
  p.rows = rows; p.c = c; p.out = shifted; p.out_off = shifted_off;
  SsrBlk blk{SSR_ALIGN_NT};
  ssr_align_geometry_body(p, blk, sums.data());
  if (pt[n_est] != tiles || po[n_est] != outs) return -1;
  const int64_t grid = tiles * ssr_align_lag_blocks(max_lag);
  const int kind = (tgt_f64 ? 2 : 0) + (est_f64 ? 1 : 0);
  if (kind == 0) corr<float, float>(p, grid);
  else if (kind == 1) corr<float, double>(p, grid);
  else if (kind == 2) corr<double, float>(p, grid);
  else corr<double, double>(p, grid);
  if (cpart.back() != -777.0 || epart.back() != -777.0) return -3;
  for (size_t i = 0; i + 1 < cpart.size(); ++i)
    if (cpart[i] == -777.0) return -4;                // every lag of every tile row is written
  std::vector<double> mx(128), hs(SSR_ALIGN_TAPS), st(8);
  SsrBlk wave{64};
  for (int e = 0; e < n_est; ++e) ssr_align_pick_body(p, wave, e, mx.data(), hs.data(), st.data());
  if (taps.back() != -777.0) return -5;
  if (shifted) {
    if (est_f64) shift<double>(p, outs); else shift<float>(p, outs);
  }
  if (taps_out)
    for (size_t i = 0; i + 1 < taps.size(); ++i) taps_out[i] = taps[i];
  return 0;
}
