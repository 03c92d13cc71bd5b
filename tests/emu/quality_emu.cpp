// Host emulation of the quality-measure kernel bodies (ssr_eval_amd/csrc/ssr_quality.h) for tests/test_quality_host.py: every
// kernel of ssr_quality_metrics run in launch order, one workgroup after another.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libquality_emu.so quality_emu.cpp
#define SSR_HOST_EMU 1
#include <memory>
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_quality.h"

template <typename TT, typename TE, int LOGN> static void bands(SsrQualParams& p, int64_t grid) {
  auto lds = std::make_unique<SsrQualBandLds<LOGN>>();
  SsrBlk blk{(1 << LOGN) / 8};
  for (int64_t g = 0; g < grid; ++g) ssr_qual_bands_body<TT, TE, LOGN>(p, blk, g, *lds);
}

template <typename TT, typename TE> static void passes(SsrQualParams& p, int64_t run_frames) {
  if (p.which & (SSR_QUAL_LLR | SSR_QUAL_CEP)) {
    auto lds = std::make_unique<SsrQualLpcLds>();
    SsrBlk blk{64};
    for (int64_t g = 0; g < run_frames; ++g) ssr_qual_lpc_body<TT, TE>(p, blk, g, *lds);
  }
  if (p.which & (SSR_QUAL_WSS | SSR_QUAL_FWSEG))
    ssr_dispatch_logn<9, 12>(ssr_qual_log2_nfft(p.fs), [&](auto logn) { bands<TT, TE, decltype(logn)::value>(p, run_frames); });
}

// tgt / est: float32 or float64 signals at tgt + tgt_off[t] / est + est_off[e]; out: [n_est][popcount(which)]
extern "C" int quality_emu(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                           int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int fs, int lpc_order, int which,
                           double* out) {
  int n_runs = 0;
  int64_t run_frames = 0, pair_frames = 0;
  for (int e = 0; e < n_est; ++e) {
    const int64_t M = ssr_qual_frames(tgt_len[tgt_index[e]], fs);
    if (e == 0 || tgt_index[e] != tgt_index[e - 1]) { ++n_runs; run_frames += M; }
    pair_frames += M;
  }
  SsrQualTables t;
  ssr_qual_tables_host(fs, t);
  std::vector<int32_t> rs(n_runs + 1);
  std::vector<int64_t> rf(n_runs + 1), pf(n_est + 1), sums(3 * SSR_QUAL_NT);
  std::vector<double> win(ssr_qual_frame_len(fs) + 1), val(4 * pair_frames + 1, -777.0);
  SsrQualParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, tgt_len, tgt_index, n_tgt, n_est);
  p.n_runs = n_runs; p.which = which; p.fs = fs;
  p.L = ssr_qual_frame_len(fs); p.R = ssr_qual_hop(fs); p.P = lpc_order ? lpc_order : ssr_qual_default_order(fs); p.N = t.N;
  p.run_start = rs.data(); p.run_frame = rf.data(); p.pair_frame = pf.data(); p.win = win.data();
  p.tw = t.tw.data(); p.fw = t.packed.data();
  for (int b = 0; b < SSR_QUAL_BANDS; ++b) { p.band_lo[b] = t.lo[b]; p.band_hi[b] = t.hi[b]; p.band_off[b] = t.off[b]; }
  p.val = val.data(); p.n_val = pair_frames; p.out = out;
  SsrBlk blk{SSR_QUAL_NT};
  ssr_qual_geometry_body(p, blk, sums.data());
  if (rf[n_runs] != run_frames || pf[n_est] != pair_frames || rs[n_runs] != n_est) return -1;
  const int kind = (tgt_f64 ? 2 : 0) + (est_f64 ? 1 : 0);
  if (kind == 0) passes<float, float>(p, run_frames);
  else if (kind == 1) passes<float, double>(p, run_frames);
  else if (kind == 2) passes<double, float>(p, run_frames);
  else passes<double, double>(p, run_frames);
  SsrQualFinLds fl;
  for (int e = 0; e < n_est; ++e) ssr_qual_finalize_body(p, blk, e, fl);
  return 0;
}

// L, R, M, N, default P, K of the trimmed mean
extern "C" void quality_geometry(int fs, int64_t n, int64_t* res) {
  const int64_t M = ssr_qual_frames(n, fs);
  res[0] = ssr_qual_frame_len(fs); res[1] = ssr_qual_hop(fs); res[2] = M; res[3] = 1 << ssr_qual_log2_nfft(fs);
  res[4] = ssr_qual_default_order(fs); res[5] = ssr_qual_trim_count(M);
}

// the trimmed mean of the finalize body on one pair's frame values v[0 .. M) (metric slot 0)
extern "C" double quality_trimmed_mean(const double* v, int64_t M) {
  const int fs = 16000;
  const int L = ssr_qual_frame_len(fs), R = ssr_qual_hop(fs);
  const int32_t len = (int32_t)(L + M * R), idx = 0;
  int64_t pf[2] = {0, M};
  std::vector<double> val(4 * M + 1);
  for (int64_t i = 0; i < M; ++i) val[i] = v[i];
  double out = -777.0;
  SsrQualParams p{};
  p.tgt_len = &len; p.tgt_index = &idx; p.n_tgt = 1; p.n_est = 1; p.which = SSR_QUAL_LLR; p.fs = fs;
  p.pair_frame = pf; p.val = val.data(); p.n_val = M; p.out = &out;
  SsrBlk blk{SSR_QUAL_NT};
  SsrQualFinLds fl;
  ssr_qual_finalize_body(p, blk, 0, fl);
  return out;
}

extern "C" void quality_levinson(const double* r, int P, double* a) {
  double alpha[SSR_QUAL_PMAX + 1], tmp[SSR_QUAL_PMAX + 1];
  ssr_qual_levinson(r, a, alpha, tmp, P);
}
