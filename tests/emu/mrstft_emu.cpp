// Host emulation of the multi-resolution STFT distance kernel bodies (ssr_eval_amd/csrc/ssr_mrstft.h) for
// tests/test_mrstft_host.py: every kernel of ssr_mrstft_metrics run in launch order, one workgroup after another.  Test
// infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libmrstft_emu.so mrstft_emu.cpp
#define SSR_HOST_EMU 1
#include <memory>
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_mrstft.h"

template <typename TT, typename TE, int LOGN> static void dist(const SsrMrstftSig& p, const SsrMrstftRes& q, double eps, int64_t grid) {
  auto lds = std::make_unique<SsrMrstftLds<LOGN>>();
  SsrBlk blk{(1 << LOGN) / 8};
  for (int64_t g = 0; g < grid; ++g) ssr_mrstft_dist_body<TT, TE, LOGN>(p, q, eps, blk, g, *lds);
}

template <typename TT, typename TE> static void passes(const SsrMrstftSig& p, const SsrMrstftRes& q, double eps, int64_t grid) {
  ssr_dispatch_logn<SSR_PHASE_LOGN_MIN, SSR_PHASE_LOGN_MAX>(
      ssr_phase_log2_nfft(q.N), [&](auto logn) { dist<TT, TE, decltype(logn)::value>(p, q, eps, grid); });
}

// tgt / est: float32 or float64 signals at tgt + tgt_off[t] / est + est_off[e]; out: [n_est][n_res + 1][2]
extern "C" int mrstft_emu(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                          int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_res, const int32_t* n_fft,
                          const int32_t* hop, const int32_t* win, const int32_t* bin_lo, const int32_t* bin_hi, double eps,
                          double* out) {
  if (n_res < 1 || n_res > SSR_MRSTFT_MAX_RES) return -2;
  SsrMrstftSig p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, tgt_len, tgt_index, n_tgt, n_est);
  SsrMrstftAll a{};
  a.n_res = n_res; a.out = out;
  std::vector<std::vector<cx<double>>> tw(n_res);
  std::vector<std::vector<double>> wn(n_res), part(n_res);
  std::vector<std::vector<int64_t>> co(n_res);
  std::vector<int64_t> sums(SSR_PHASE_NT);
  const int kind = (tgt_f64 ? 2 : 0) + (est_f64 ? 1 : 0);
  for (int r = 0; r < n_res; ++r) {
    if (ssr_phase_log2_nfft(n_fft[r]) < 0 || win[r] < 2 || win[r] > n_fft[r]) return -2;
    int64_t chunks = 0;
    for (int e = 0; e < n_est; ++e) chunks += ssr_phase_chunks(tgt_len[tgt_index[e]], n_fft[r], hop[r]);
    ssr_phase_twiddles_host(n_fft[r], tw[r]);
    ssr_mrstft_window_host(n_fft[r], win[r], wn[r]);
    co[r].assign(n_est + 1, -1);
    part[r].assign(3 * chunks + 1, -777.0);
    SsrMrstftRes& q = a.res[r];
    q.N = n_fft[r]; q.H = hop[r]; q.k_lo = bin_lo[r]; q.k_hi = bin_hi[r];
    q.tw = tw[r].data(); q.win = wn[r].data(); q.chunk_off = co[r].data(); q.part = part[r].data();
    SsrBlk blk{SSR_PHASE_NT};
    const SsrPhaseParams g = ssr_mrstft_geometry_params(p, q);
    ssr_phase_geometry_body(g, blk, sums.data());
    if (co[r][n_est] != chunks) return -1;
    if (kind == 0) passes<float, float>(p, q, eps, chunks);
    else if (kind == 1) passes<float, double>(p, q, eps, chunks);
    else if (kind == 2) passes<double, float>(p, q, eps, chunks);
    else passes<double, double>(p, q, eps, chunks);
  }
  SsrBlk fin{SSR_PHASE_FIN_NT};
  for (int b = 0; b < (n_est + SSR_PHASE_FIN_NT - 1) / SSR_PHASE_FIN_NT; ++b) ssr_mrstft_finalize_body(p, a, fin, b);
  return 0;
}

// the window table of (n_fft, win): [n_fft]
extern "C" void mrstft_window(int n_fft, int win, double* out) {
  std::vector<double> w;
  ssr_mrstft_window_host(n_fft, win, w);
  for (int i = 0; i < n_fft; ++i) out[i] = w[i];
}
