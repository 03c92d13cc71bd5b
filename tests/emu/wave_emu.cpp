// Host emulation of the waveform-metric kernel bodies (ssr_eval_amd/csrc/ssr_wave_metrics.h) for tests/test_wave_metrics_host.py:
// every kernel of ssr_wave_metrics run in launch order, one workgroup after another.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libwave_emu.so wave_emu.cpp
#define SSR_HOST_EMU 1
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_wave_metrics.h"

template <typename TT, typename TE> static void passes(SsrWaveParams& p, int64_t grid, SsrBlk& blk) {
  std::vector<double> red(16), tst(3), seg(8);
  for (int64_t g = 0; g < grid; ++g) ssr_wave_pass1_body<TT, TE>(p, blk, g, red.data(), tst.data(), seg.data());
  for (int e = 0; e < p.n_est; ++e) ssr_wave_finalize1(p, e);
  if (p.which & SSR_WAVE_SI_SDR) {
    for (int64_t g = 0; g < grid; ++g) ssr_wave_pass2_body<TT, TE>(p, blk, g, red.data());
    for (int e = 0; e < p.n_est; ++e) ssr_wave_finalize2(p, e);
  }
}

// tgt / est: float32 or float64 signals at tgt + tgt_off[t] / est + est_off[e]; out: [n_est][popcount(which)]
extern "C" int wave_emu(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                        int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int fs, int which, double* out) {
  int n_runs = 0;
  int64_t run_tiles = 0, pair_tiles = 0;
  for (int e = 0; e < n_est; ++e) {
    const int64_t nt = ssr_wave_tiles(tgt_len[tgt_index[e]], fs);
    if (e == 0 || tgt_index[e] != tgt_index[e - 1]) { ++n_runs; run_tiles += nt; }
    pair_tiles += nt;
  }
  std::vector<int32_t> rs(n_runs + 1);
  std::vector<int64_t> rt(n_runs + 1), pt(n_est + 1), sums(3 * SSR_WAVE_NT);
  std::vector<double> win(ssr_wave_frame_len(fs) + 1), p1(pair_tiles * SSR_WAVE_P1 + 1), p2(pair_tiles * SSR_WAVE_P2 + 1),
      fin(3 * n_est + 1);
  SsrWaveParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, tgt_len, tgt_index, n_tgt, n_est);
  p.n_runs = n_runs; p.which = which; p.fs = fs;
  p.L = ssr_wave_frame_len(fs); p.R = ssr_wave_hop(fs); p.fpt = ssr_wave_frames_per_tile(fs); p.tile = ssr_wave_tile_len(fs);
  p.run_start = rs.data(); p.run_tile = rt.data(); p.pair_tile = pt.data(); p.win = win.data();
  p.part1 = p1.data(); p.part2 = p2.data(); p.fin = fin.data(); p.out = out;
  SsrBlk blk{SSR_WAVE_NT};
  ssr_wave_geometry_body(p, blk, sums.data());
  if (rt[n_runs] != run_tiles || pt[n_est] != pair_tiles || rs[n_runs] != n_est) return -1;
  const int kind = (tgt_f64 ? 2 : 0) + (est_f64 ? 1 : 0);
  if (kind == 0) passes<float, float>(p, run_tiles, blk);
  else if (kind == 1) passes<float, double>(p, run_tiles, blk);
  else if (kind == 2) passes<double, float>(p, run_tiles, blk);
  else passes<double, double>(p, run_tiles, blk);
  return 0;
}

extern "C" void wave_geometry(int fs, int64_t n, int64_t* res) {
  res[0] = ssr_wave_frame_len(fs); res[1] = ssr_wave_hop(fs); res[2] = ssr_wave_frames(n, fs);
  res[3] = ssr_wave_tile_len(fs); res[4] = ssr_wave_tiles(n, fs);
}
