// Host emulation of the spectrum kernel bodies (ssr_eval_amd/csrc/ssr_spectrum.h) for tests/test_spectrum_host.py: every kernel of
// ssr_spectrum run in launch order, one workgroup after another.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libspectrum_emu.so spectrum_emu.cpp
#define SSR_HOST_EMU 1
#include <memory>
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_spectrum.h"

template <typename T, int LOGN> static void ltas(SsrSpecParams& p, int64_t g0, int64_t g1) {
  auto lds = std::make_unique<SsrSpecLds<LOGN>>();
  SsrBlk blk{(1 << LOGN) / 8};
  for (int64_t g = g0; g < g1; ++g) ssr_spec_ltas_body<T, LOGN>(p, blk, g, *lds);
}

template <typename T> static void side(SsrSpecParams& p, int64_t g0, int64_t g1) {
  ssr_dispatch_logn<SSR_PHASE_LOGN_MIN, SSR_PHASE_LOGN_MAX>(ssr_phase_log2_nfft(p.N), [&](auto logn) { ltas<T, decltype(logn)::value>(p, g0, g1); });
}

// the arguments of ssr_spectrum up to ltas_out; pa_out: [n_tgt + n_est][n_fft / 2 + 1][2], the chunk rows of P and A added in chunk
// order (the debug row), or null
extern "C" int spectrum_emu(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                            int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_fft, int hop, int lo, int hi,
                            double rho, double drop_db, int n_bands, const int32_t* bands, const int32_t* split, double* sig_out,
                            double* pair_out, double* ltas_out, double* pa_out) {
  if (ssr_phase_log2_nfft(n_fft) < 0 || n_bands < 1 || n_bands > SSR_SPEC_MAX_BANDS) return -2;
  const int n_sig = n_tgt + n_est, NB = n_fft / 2 + 1;
  int64_t ct = 0, ce = 0;
  for (int t = 0; t < n_tgt; ++t) ct += ssr_spec_chunks(tgt_len[t], n_fft, hop);
  for (int e = 0; e < n_est; ++e) ce += ssr_spec_chunks(tgt_len[tgt_index[e]], n_fft, hop);
  std::vector<cx<double>> tw;
  ssr_phase_twiddles_host(n_fft, tw);
  std::vector<int32_t> si(n_sig + 1, -1), rs(n_sig + 1, -1);
  std::vector<int64_t> rc(n_sig + 1, -1), co(n_sig + 1, -1), sums(3 * SSR_SPEC_NT);
  std::vector<double> part((size_t)(ct + ce) * NB * 2 + 1, -777.0), cp((size_t)n_sig * NB + 1, -777.0), sig((size_t)n_sig * 4 + 1, -777.0),
      lev((size_t)n_sig * n_bands + 1, -777.0);
  SsrSpecParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, tgt_len, tgt_index, n_tgt, n_est);
  p.N = n_fft; p.H = hop; p.lo = lo; p.hi = hi; p.n_bands = n_bands; p.rho = rho; p.thr_lin = pow(10.0, -drop_db / 10.0);
  p.bands = bands; p.split = split; p.tw = tw.data();
  p.sig_index = si.data(); p.run_start = rs.data(); p.run_chunk = rc.data(); p.chunk_off = co.data();
  p.part = part.data(); p.cp = cp.data(); p.sig = sig.data(); p.lev = lev.data();
  p.sig_out = sig_out; p.pair_out = pair_out; p.ltas_out = ltas_out;
  SsrBlk blk{SSR_SPEC_NT};
  ssr_spec_geometry_body(p, blk, sums.data());
  if (co[n_sig] != ct + ce || (n_tgt > 0 && co[n_tgt] != ct)) return -1;
  if (tgt_f64) side<double>(p, 0, ct); else side<float>(p, 0, ct);
  if (est_f64) side<double>(p, ct, ct + ce); else side<float>(p, ct, ct + ce);
  if (part.back() != -777.0) return -3;
  auto lds = std::make_unique<SsrSpecSignalLds>();
  for (int s = 0; s < n_sig; ++s) ssr_spec_signal_body(p, blk, s, *lds);
  auto pl = std::make_unique<SsrSpecPairLds>();
  for (int e = 0; e < n_est; ++e) ssr_spec_pair_body(p, blk, e, *pl);
  if (cp.back() != -777.0 || sig.back() != -777.0 || lev.back() != -777.0 || si[n_sig] != -1) return -3;
  if (pa_out)
    for (int s = 0; s < n_sig; ++s)
      for (int k = 0; k < NB; ++k) {
        double pk = 0.0, ak = 0.0;
        for (int64_t c = co[s]; c < co[s + 1]; ++c) { pk += part[(c * NB + k) * 2]; ak += part[(c * NB + k) * 2 + 1]; }
        pa_out[((size_t)s * NB + k) * 2] = pk; pa_out[((size_t)s * NB + k) * 2 + 1] = ak;
      }
  return 0;
}

// K, chunks, segments per chunk, the band limit
extern "C" void spectrum_geometry(int n, int n_fft, int hop, int64_t* res) {
  res[0] = ssr_spec_segments(n, n_fft, hop); res[1] = ssr_spec_chunks(n, n_fft, hop); res[2] = SSR_SPEC_FR; res[3] = SSR_SPEC_MAX_BANDS;
}
