// Host emulation of the loudness kernel bodies (ssr_eval_amd/csrc/ssr_loudness.h) for tests/test_loudness_host.py: every kernel of
// ssr_loudness run in launch order, one workgroup after another.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libloudness_emu.so loudness_emu.cpp
#define SSR_HOST_EMU 1
#include <memory>
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_loudness.h"

template <typename X> static void sweeps_and_peaks(SsrLoudParams& p, int64_t n_seg, int64_t n_tiles) {
  SsrPitTile tile{};
  const int64_t lanes = (n_seg + 63) / 64 * 64;           // whole waves, as on the device
  for (int64_t l = 0; l < lanes; ++l) ssr_loud_filter_lane<X, false>(p, l, n_seg, tile);
  for (int i = 0; i < (p.n_sig + 63) / 64 * 64; ++i) ssr_loud_scan_signal(p, i);
  for (int64_t l = 0; l < lanes; ++l) ssr_loud_filter_lane<X, true>(p, l, n_seg, tile);
  auto lds = std::make_unique<SsrLoudPeakLds>();
  SsrBlk blk{SSR_LOUD_NT};
  for (int64_t g = 0; g < n_tiles; ++g) ssr_loud_peak_body<X>(p, blk, g, *lds);
}

// sig: float32 or float64 signals at sig + off[i]; out: [n_sig][6]; blocks_out: E[s] of signal i at blocks_out + blocks_off[i], or null
extern "C" int loudness_emu(const void* sig, int sig_f64, const int64_t* off, const int32_t* len, int n_sig, int rate, double* out,
                            const int64_t* blocks_off, double* blocks_out) {
  if (rate < SSR_LOUD_MIN_RATE || rate > SSR_LOUD_MAX_RATE) return -2;
  int64_t n_seg = 0, n_tiles = 0;
  for (int i = 0; i < n_sig; ++i) {
    if (ssr_loud_sub_blocks(len[i], rate) > SSR_LOUD_MAX_SUB) return -2;
    n_seg += ssr_loud_segments(len[i], rate);
    n_tiles += ssr_loud_tiles(len[i]);
  }
  std::vector<double> tab;
  ssr_loud_tables_host(rate, tab);
  std::vector<int64_t> sp(n_sig + 1, -1), tp(n_sig + 1, -1), sums(2 * SSR_LOUD_NT);
  std::vector<double> zend(n_seg * 4 + 1, -777.0), zin(n_seg * 4 + 1, -777.0), part(n_seg + 1, -777.0), peak(n_tiles * 2 + 1, -777.0);
  SsrLoudParams p{};
  p.sig = sig; p.off = off; p.len = len; p.n_sig = n_sig; p.rate = rate; p.h = ssr_loud_sub_len(rate);
  p.tab = tab.data(); p.seg_pre = sp.data(); p.tile_pre = tp.data();
  p.zend = zend.data(); p.zin = zin.data(); p.part = part.data(); p.peak = peak.data();
  p.out = out; p.blocks_off = blocks_off; p.blocks_out = blocks_out;
  SsrBlk blk{SSR_LOUD_NT};
  ssr_loud_geometry_body(p, blk, sums.data());
  if (sp[n_sig] != n_seg || tp[n_sig] != n_tiles) return -1;
  if (sig_f64) sweeps_and_peaks<double>(p, n_seg, n_tiles);
  else sweeps_and_peaks<float>(p, n_seg, n_tiles);
  if (zend.back() != -777.0 || zin.back() != -777.0 || part.back() != -777.0 || peak.back() != -777.0) return -3;
  auto lds = std::make_unique<SsrLoudGateLds>();
  for (int i = 0; i < n_sig; ++i) ssr_loud_gate_body(p, blk, i, *lds);
  return 0;
}

// the rate's table: c[2][5], the state map, the taps (SSR_LOUD_TAB_LEN doubles)
extern "C" void loudness_tables(int rate, double* tab) {
  std::vector<double> t;
  ssr_loud_tables_host(rate, t);
  for (int j = 0; j < SSR_LOUD_TAB_LEN; ++j) tab[j] = t[j];
}

// h, segments per sub-block, sub-block limit, tile, table length, offset of M, offset of the taps
extern "C" void loudness_geometry(int rate, int64_t* res) {
  res[0] = ssr_loud_sub_len(rate); res[1] = SSR_LOUD_G; res[2] = SSR_LOUD_MAX_SUB; res[3] = SSR_LOUD_TILE; res[4] = SSR_LOUD_TAB_LEN;
  res[5] = SSR_LOUD_TAB_M; res[6] = SSR_LOUD_TAB_TAPS;
}
