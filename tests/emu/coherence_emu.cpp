// Host emulation of the coherence kernel bodies (ssr_eval_amd/csrc/ssr_coherence.h) for tests/test_coherence_host.py: every kernel
// of ssr_coherence run in launch order, one workgroup after another.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libcoherence_emu.so coherence_emu.cpp
#define SSR_HOST_EMU 1
#include <memory>
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_coherence.h"

template <typename TT, typename TE, int LOGN> static void spectra(SsrCohParams& p, int64_t grid) {
  auto lds = std::make_unique<SsrCohLds<LOGN>>();
  SsrBlk blk{(1 << LOGN) / 8};
  for (int64_t g = 0; g < grid; ++g) ssr_coh_spectra_body<TT, TE, LOGN>(p, blk, g, *lds);
}

template <typename TT, typename TE> static void passes(SsrCohParams& p, int64_t grid) {
  ssr_dispatch_logn<SSR_PHASE_LOGN_MIN, SSR_PHASE_LOGN_MAX>(ssr_phase_log2_nfft(p.N),
                                                            [&](auto logn) { spectra<TT, TE, decltype(logn)::value>(p, grid); });
}

// tgt / est: float32 or float64 signals at tgt + tgt_off[t] / est + est_off[e]; bands: [n_est][n_bands][2]; out: [n_est][n_bands][3];
// msc_out: [n_est][n_fft / 2 + 1] or null
extern "C" int coherence_emu(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                             int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_fft, int hop, int n_bands,
                             const int32_t* bands, double thr, double* out, double* msc_out) {
  if (ssr_phase_log2_nfft(n_fft) < 0 || n_bands < 1 || n_bands > SSR_COH_MAX_BANDS) return -2;
  int64_t chunks = 0;
  for (int e = 0; e < n_est; ++e) chunks += ssr_coh_chunks(tgt_len[tgt_index[e]], n_fft, hop);
  std::vector<cx<double>> tw;
  ssr_phase_twiddles_host(n_fft, tw);
  std::vector<int32_t> rs(n_est + 1, -1);
  std::vector<int64_t> rc(n_est + 1, -1), co(n_est + 1, -1), sums(3 * SSR_COH_NT);
  std::vector<double> part((size_t)chunks * (n_fft / 2 + 1) * 4 + 1, -777.0);
  SsrCohParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, tgt_len, tgt_index, n_tgt, n_est);
  p.N = n_fft; p.H = hop; p.n_bands = n_bands; p.thr = thr; p.bands = bands;
  p.tw = tw.data(); p.run_start = rs.data(); p.run_chunk = rc.data(); p.chunk_off = co.data(); p.part = part.data();
  p.out = out; p.msc_out = msc_out;
  SsrBlk blk{SSR_COH_NT};
  ssr_coh_geometry_body(p, blk, sums.data());
  if (co[n_est] != chunks) return -1;
  const int kind = (tgt_f64 ? 2 : 0) + (est_f64 ? 1 : 0);
  if (kind == 0) passes<float, float>(p, chunks);
  else if (kind == 1) passes<float, double>(p, chunks);
  else if (kind == 2) passes<double, float>(p, chunks);
  else passes<double, double>(p, chunks);
  if (part.back() != -777.0) return -3;
  auto lds = std::make_unique<SsrCohBandsLds>();
  for (int e = 0; e < n_est; ++e) ssr_coh_bands_body(p, blk, e, *lds);
  return 0;
}

// K, chunks, segments per chunk
extern "C" void coherence_geometry(int n, int n_fft, int hop, int64_t* res) {
  res[0] = ssr_coh_segments(n, n_fft, hop); res[1] = ssr_coh_chunks(n, n_fft, hop); res[2] = SSR_COH_FR;
}
