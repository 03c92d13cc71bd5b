// Host emulation of the filter-invariant SDR kernel bodies (ssr_eval_amd/csrc/ssr_bss.h) for tests/test_bss_host.py: every kernel of
// ssr_bss_sdr run in launch order, one workgroup after another.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libbss_emu.so bss_emu.cpp
#define SSR_HOST_EMU 1
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_bss.h"

template <typename TT, typename TE> static void passes(SsrBssParams& p, int64_t run_tiles, int64_t pair_tiles) {
  SsrBlk blk{SSR_BSS_NT}, wave{64};
  std::vector<double> xs(SSR_BSS_RESID_LDS), ys(SSR_BSS_CORR_LDS), part(SSR_BSS_PART_LDS);
  std::vector<double> rr(SSR_BSS_MAX_TAPS), bb(SSR_BSS_MAX_TAPS), av(SSR_BSS_MAX_TAPS), cv(SSR_BSS_MAX_TAPS), red(8), st(4), mx(128);
  for (int64_t g = 0; g < run_tiles; ++g) ssr_bss_corr_body<TT, TE>(p, blk, g, xs.data(), ys.data(), part.data());
  for (int e = 0; e < p.n_est; ++e)
    ssr_bss_solve_body(p, wave, e, rr.data(), bb.data(), av.data(), cv.data(), red.data(), st.data(), mx.data());
  for (int64_t g = 0; g < pair_tiles; ++g) ssr_bss_resid_body<TT, TE>(p, blk, g, xs.data(), cv.data(), red.data());
  for (int e = 0; e < p.n_est; ++e) ssr_bss_finalize(p, e);
}

// tgt / est: float32 or float64 signals at tgt + tgt_off[t] / est + est_off[e]; out: [n_est][2]; filt: [n_est][taps] or null
extern "C" int bss_emu(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                       int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int taps, double* out, double* filt) {
  if (taps < 1 || taps > SSR_BSS_MAX_TAPS) return -2;
  int n_runs = 0;
  int64_t run_tiles = 0, pair_tiles = 0;
  for (int e = 0; e < n_est; ++e) {
    const int64_t nt = ssr_bss_tiles(tgt_len[tgt_index[e]]);
    if (e == 0 || tgt_index[e] != tgt_index[e - 1]) { ++n_runs; run_tiles += nt; }
    pair_tiles += nt;
  }
  // every area the kernels must write before they read it starts out as NaN (or a wild index)
  std::vector<int32_t> rs(n_runs + 1, -1), pr(n_est + 1, 0x7fffffff);
  std::vector<int64_t> rt(n_runs + 1, -1), pt(n_est + 1, -1), sums(3 * SSR_BSS_NT);
  std::vector<double> rp(run_tiles * taps + 1, NAN), bp(pair_tiles * taps + 1, NAN), c((int64_t)n_est * taps + 1, NAN),
      fin(n_est + 1, NAN), p2(pair_tiles * 2 + 1, NAN);
  SsrBssParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, tgt_len, tgt_index, n_tgt, n_est);
  p.n_runs = n_runs; p.L = taps;
  p.run_start = rs.data(); p.run_tile = rt.data(); p.pair_tile = pt.data(); p.pair_run = pr.data();
  p.rpart = rp.data(); p.bpart = bp.data(); p.c = c.data(); p.fin = fin.data(); p.part2 = p2.data(); p.out = out; p.filt = filt;
  SsrBlk blk{SSR_BSS_NT};
  ssr_bss_geometry_body(p, blk, sums.data());
  if (rt[n_runs] != run_tiles || pt[n_est] != pair_tiles || rs[n_runs] != n_est) return -1;
  const int kind = (tgt_f64 ? 2 : 0) + (est_f64 ? 1 : 0);
  if (kind == 0) passes<float, float>(p, run_tiles, pair_tiles);
  else if (kind == 1) passes<float, double>(p, run_tiles, pair_tiles);
  else if (kind == 2) passes<double, float>(p, run_tiles, pair_tiles);
  else passes<double, double>(p, run_tiles, pair_tiles);
  return 0;
}

extern "C" void bss_geometry(int64_t n, int64_t* res) { res[0] = SSR_BSS_TILE; res[1] = ssr_bss_tiles(n); }
