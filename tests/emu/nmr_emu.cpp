// Host emulation of the noise-to-mask kernel bodies (ssr_eval_amd/csrc/ssr_nmr.h) for tests/test_nmr_host.py: every kernel of ssr_nmr
// run in launch order, one workgroup after another.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libnmr_emu.so nmr_emu.cpp
#define SSR_HOST_EMU 1
#include <memory>
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_nmr.h"

template <typename TT, typename TE, int LOGN> static void transforms(SsrNmrParams& p, int64_t tchunks, int64_t chunks, double* es_out, int64_t cells) {
  auto lds = std::make_unique<SsrNmrLds<LOGN>>();
  SsrBlk blk{(1 << LOGN) / 8}, bt{SSR_NMR_BT};
  for (int64_t g = 0; g < tchunks; ++g) ssr_nmr_excite_body<TT, LOGN>(p, blk, g, *lds);
  if (es_out)
    for (int64_t i = 0; i < cells; ++i) es_out[i] = p.mask[i];
  for (int t = 0; t < p.n_tgt; ++t) ssr_nmr_mask_body(p, bt, t);
  for (int64_t g = 0; g < chunks; ++g) ssr_nmr_noise_body<TT, TE, LOGN>(p, blk, g, *lds);
}

template <typename TT, typename TE> static void passes(SsrNmrParams& p, int64_t tchunks, int64_t chunks, double* es_out, int64_t cells) {
  ssr_dispatch_logn<SSR_PHASE_LOGN_MIN, SSR_PHASE_LOGN_MAX>(ssr_phase_log2_nfft(p.N), [&](auto logn) {
    transforms<TT, TE, decltype(logn)::value>(p, tchunks, chunks, es_out, cells);
  });
}

// tgt / est: float32 or float64 signals at tgt + tgt_off[t] / est + est_off[e]; weights: [n_fft / 2 + 1]; bins: [n_bands][2]; table:
// [n_bands][SSR_NMR_TAB]; split: [n_est]; out: [n_est][SSR_NMR_COLS]; bands_out: [n_est][n_bands] or null; mask_out, es_out: [the
// frames of all targets][n_bands] or null (M, and Es before the mask kernel overwrote it); part_out: [the chunks of all pairs][n_bands
// + 2] or null; ratio_out: [the frames of all pairs][n_bands] or null (R of every frame, pair after pair)
extern "C" int nmr_emu(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est, int est_f64,
                       const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_fft, int n_bands, const double* weights,
                       const int32_t* bins, const double* table, const int32_t* split, double* out, double* bands_out, double* mask_out,
                       double* es_out, double* part_out, double* ratio_out) {
  if (ssr_phase_log2_nfft(n_fft) < 0 || n_bands < 1 || n_bands > SSR_NMR_MAX_BANDS) return -2;
  const int hop = n_fft / 2;
  int64_t chunks = 0, tchunks = 0, frames = 0;
  for (int e = 0; e < n_est; ++e) chunks += ssr_coh_chunks(tgt_len[tgt_index[e]], n_fft, hop);
  for (int t = 0; t < n_tgt; ++t) {
    frames += ssr_coh_segments(tgt_len[t], n_fft, hop);
    tchunks += ssr_coh_chunks(tgt_len[t], n_fft, hop);
  }
  std::vector<cx<double>> tw;
  ssr_phase_twiddles_host(n_fft, tw);
  std::vector<int32_t> rs(n_est + 1, -1);
  std::vector<int64_t> rc(n_est + 1, -1), co(n_est + 1, -1), so(n_tgt + 1, -1), to(n_tgt + 1, -1), sums(3 * SSR_NMR_NT);
  std::vector<double> mask((size_t)frames * n_bands + 1, -777.0), part((size_t)chunks * (n_bands + 2) + 1, -777.0);
  SsrNmrParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, tgt_len, tgt_index, n_tgt, n_est);
  p.N = n_fft; p.H = hop; p.n_bands = n_bands; p.split = split; p.bins = bins; p.tab = table; p.w2 = weights;
  p.tw = tw.data(); p.seg_off = so.data(); p.tchunk_off = to.data();
  p.run_start = rs.data(); p.run_chunk = rc.data(); p.chunk_off = co.data(); p.mask = mask.data(); p.part = part.data();
  p.out = out; p.bands_out = bands_out; p.mask_out = mask_out;
  std::vector<int64_t> ro(n_est + 1, 0);
  for (int e = 0; e < n_est; ++e) ro[e + 1] = ro[e] + ssr_coh_segments(tgt_len[tgt_index[e]], n_fft, hop);
  p.ratio_off = ro.data(); p.ratio_out = ratio_out;
  SsrBlk blk{SSR_NMR_NT};
  ssr_nmr_geometry_body(p, blk, sums.data());
  if (co[n_est] != chunks || so[n_tgt] != frames || to[n_tgt] != tchunks) return -1;
  const int kind = (tgt_f64 ? 2 : 0) + (est_f64 ? 1 : 0);
  const int64_t cells = frames * n_bands;
  if (kind == 0) passes<float, float>(p, tchunks, chunks, es_out, cells);
  else if (kind == 1) passes<float, double>(p, tchunks, chunks, es_out, cells);
  else if (kind == 2) passes<double, float>(p, tchunks, chunks, es_out, cells);
  else passes<double, double>(p, tchunks, chunks, es_out, cells);
  if (mask.back() != -777.0 || part.back() != -777.0) return -3;
  for (int64_t i = 0; i < cells; ++i)
    if (mask[i] == -777.0) return -4;             // every frame of every target has its mask
  for (size_t i = 0; i + 1 < part.size(); ++i)
    if (part[i] == -777.0) return -5;             // every chunk row is written whole
  auto lds = std::make_unique<SsrNmrScoreLds>();
  SsrBlk bt{SSR_NMR_BT};
  for (int e = 0; e < n_est; ++e) ssr_nmr_score_body(p, bt, e, *lds);
  if (part_out)
    for (size_t i = 0; i + 1 < part.size(); ++i) part_out[i] = part[i];
  return 0;
}
