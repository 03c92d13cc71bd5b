// Host emulation of the phase-distance kernel bodies (ssr_eval_amd/csrc/ssr_phase.h) for tests/test_phase_host.py: every kernel
// of ssr_phase_metrics run in launch order, one workgroup after another.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libphase_emu.so phase_emu.cpp
#define SSR_HOST_EMU 1
#include <memory>
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_phase.h"

template <typename TT, typename TE, int LOGN> static void dist(SsrPhaseParams& p, int64_t grid) {
  auto lds = std::make_unique<SsrPhaseLds<LOGN>>();
  SsrBlk blk{(1 << LOGN) / 8};
  for (int64_t g = 0; g < grid; ++g) ssr_phase_dist_body<TT, TE, LOGN>(p, blk, g, *lds);
}

template <typename TT, typename TE> static void passes(SsrPhaseParams& p, int64_t grid) {
  ssr_dispatch_logn<SSR_PHASE_LOGN_MIN, SSR_PHASE_LOGN_MAX>(ssr_phase_log2_nfft(p.N),
                                                            [&](auto logn) { dist<TT, TE, decltype(logn)::value>(p, grid); });
}

// tgt / est: float32 or float64 signals at tgt + tgt_off[t] / est + est_off[e]; out: [n_est][popcount(which)]
extern "C" int phase_emu(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                         int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_fft, int hop, int bin_lo,
                         int bin_hi, int which, double* out) {
  if (ssr_phase_log2_nfft(n_fft) < 0) return -2;
  int64_t chunks = 0;
  for (int e = 0; e < n_est; ++e) chunks += ssr_phase_chunks(tgt_len[tgt_index[e]], n_fft, hop);
  std::vector<cx<double>> tw;
  ssr_phase_twiddles_host(n_fft, tw);
  std::vector<int64_t> co(n_est + 1, -1), sums(SSR_PHASE_NT);
  std::vector<double> part(3 * chunks + 1, -777.0);
  SsrPhaseParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, tgt_len, tgt_index, n_tgt, n_est);
  p.which = which; p.N = n_fft; p.H = hop; p.k_lo = bin_lo; p.k_hi = bin_hi;
  p.tw = tw.data(); p.chunk_off = co.data(); p.part = part.data(); p.out = out;
  SsrBlk blk{SSR_PHASE_NT};
  ssr_phase_geometry_body(p, blk, sums.data());
  if (co[n_est] != chunks) return -1;
  const int kind = (tgt_f64 ? 2 : 0) + (est_f64 ? 1 : 0);
  if (kind == 0) passes<float, float>(p, chunks);
  else if (kind == 1) passes<float, double>(p, chunks);
  else if (kind == 2) passes<double, float>(p, chunks);
  else passes<double, double>(p, chunks);
  SsrBlk fin{SSR_PHASE_FIN_NT};
  for (int b = 0; b < (n_est + SSR_PHASE_FIN_NT - 1) / SSR_PHASE_FIN_NT; ++b) ssr_phase_finalize_body(p, fin, b);
  return 0;
}

// T, chunks, frames per chunk
extern "C" void phase_geometry(int n, int n_fft, int hop, int64_t* res) {
  res[0] = ssr_phase_frames(n, n_fft, hop); res[1] = ssr_phase_chunks(n, n_fft, hop); res[2] = SSR_PHASE_FR;
}
