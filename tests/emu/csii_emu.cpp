// Host emulation of the CSII kernel bodies (ssr_eval_amd/csrc/ssr_csii.h) for tests/test_csii_host.py: every kernel of ssr_csii run
// in launch order, one workgroup after another.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libcsii_emu.so csii_emu.cpp
#define SSR_HOST_EMU 1
#include <memory>
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_csii.h"

template <typename TT, typename TE, int LOGN> static void spectra(SsrCsiiParams& p, int64_t grid) {
  auto lds = std::make_unique<SsrCohLds<LOGN>>();
  SsrBlk blk{(1 << LOGN) / 8};
  for (int64_t g = 0; g < grid; ++g) ssr_csii_spectra_body<TT, TE, LOGN>(p, blk, g, *lds);
}

template <typename TT, typename TE> static void passes(SsrCsiiParams& p, int64_t grid) {
  SsrCsiiLevelsLds lv;
  SsrBlk blk{SSR_CSII_NT};
  for (int t = 0; t < p.n_tgt; ++t) ssr_csii_levels_body<TT>(p, blk, t, lv);
  ssr_dispatch_logn<SSR_PHASE_LOGN_MIN, SSR_PHASE_LOGN_MAX>(ssr_phase_log2_nfft(p.N),
                                                            [&](auto logn) { spectra<TT, TE, decltype(logn)::value>(p, grid); });
}

// tgt / est: float32 or float64 signals at tgt + tgt_off[t] / est + est_off[e]; weights: [n_bands][n_fft / 2 + 1]; importance:
// [n_bands]; split: [n_est]; out: [n_est][SSR_CSII_COLS]; bands_out: [n_est][4][n_bands] or null; cls_out: the class of every
// segment of every target, target after target (the sum of their K bytes), or null
extern "C" int csii_emu(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                        int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_fft, int hop, int n_bands,
                        const double* weights, const double* importance, const int32_t* split, double* out, double* bands_out,
                        int8_t* cls_out) {
  if (ssr_phase_log2_nfft(n_fft) < 0 || n_bands < 1 || n_bands > SSR_CSII_MAX_BANDS) return -2;
  int64_t chunks = 0, segs = 0;
  for (int e = 0; e < n_est; ++e) chunks += ssr_coh_chunks(tgt_len[tgt_index[e]], n_fft, hop);
  for (int t = 0; t < n_tgt; ++t) segs += ssr_coh_segments(tgt_len[t], n_fft, hop);
  std::vector<cx<double>> tw;
  ssr_phase_twiddles_host(n_fft, tw);
  std::vector<int32_t> rs(n_est + 1, -1);
  std::vector<int64_t> rc(n_est + 1, -1), co(n_est + 1, -1), so(n_tgt + 1, -1), sums(3 * SSR_CSII_NT);
  std::vector<int8_t> cls((size_t)segs + 1, 99);
  std::vector<double> part((size_t)chunks * SSR_CSII_SETS * (n_fft / 2 + 1) * 4 + 1, -777.0);
  SsrCsiiParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, tgt_len, tgt_index, n_tgt, n_est);
  p.N = n_fft; p.H = hop; p.n_bands = n_bands; p.split = split; p.weights = weights; p.importance = importance;
  p.tw = tw.data(); p.seg_off = so.data(); p.cls = cls.data();
  p.run_start = rs.data(); p.run_chunk = rc.data(); p.chunk_off = co.data(); p.part = part.data();
  p.out = out; p.bands_out = bands_out;
  SsrBlk blk{SSR_CSII_NT};
  ssr_csii_geometry_body(p, blk, sums.data());
  if (co[n_est] != chunks || so[n_tgt] != segs) return -1;
  const int kind = (tgt_f64 ? 2 : 0) + (est_f64 ? 1 : 0);
  if (kind == 0) passes<float, float>(p, chunks);
  else if (kind == 1) passes<float, double>(p, chunks);
  else if (kind == 2) passes<double, float>(p, chunks);
  else passes<double, double>(p, chunks);
  if (part.back() != -777.0 || cls.back() != 99) return -3;
  for (int64_t i = 0; i < segs; ++i)
    if (cls[i] == 99) return -4;                // every segment of every target is classified
  auto lds = std::make_unique<SsrCsiiBandsLds>();
  for (int e = 0; e < n_est; ++e) ssr_csii_bands_body(p, blk, e, *lds);
  if (cls_out)
    for (int64_t i = 0; i < segs; ++i) cls_out[i] = cls[i];
  return 0;
}
