// Host emulation of the auditory kernel bodies (ssr_eval_amd/csrc/ssr_auditory.h) for tests/test_auditory_host.py: every kernel of
// ssr_auditory run in launch order, one workgroup after another.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libauditory_emu.so auditory_emu.cpp
#define SSR_HOST_EMU 1
#include <memory>
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_auditory.h"

template <typename X> static void sweeps(SsrAudParams& p, int64_t g0, int64_t g1, bool second) {
  auto lds = std::make_unique<SsrAudSweepLds>();
  SsrBlk blk{SSR_AUD_NT};
  for (int64_t g = g0; g < g1; ++g) {
    if (second) ssr_aud_sweep_body<X, true>(p, blk, g, *lds);
    else ssr_aud_sweep_body<X, false>(p, blk, g, *lds);
  }
}

// the arguments of ssr_auditory up to image_out; power_out: [rows][n_bands], P of every signal's image in signal order (the debug
// image, from the block sums), or null
extern "C" int auditory_emu(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                            int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int hop, int n_bands,
                            const double* coef, double range_db, int match_level, const int32_t* split_band, double* pair_out,
                            double* band_out, double* image_out, double* power_out) {
  if (hop < 1 || n_bands < SSR_AUD_MIN_BANDS || n_bands > SSR_AUD_MAX_BANDS) return -2;
  const int n_sig = n_tgt + n_est, C = n_bands, cp = ssr_aud_lanes(C);
  int64_t segs = 0, wt = 0, we = 0, rows = 0;
  for (int s = 0; s < n_sig; ++s) {
    const int n = tgt_len[s < n_tgt ? s : tgt_index[s - n_tgt]];
    if (ssr_aud_blocks(n, hop) > SSR_AUD_MAX_BLOCKS) return -2;
    segs += ssr_aud_segments(n, hop); rows += ssr_aud_rows(n, hop);
    (s < n_tgt ? wt : we) += ssr_aud_wgs(n, hop, cp);
  }
  std::vector<double> tab;
  ssr_aud_tables_host(coef, C, hop, tab);
  std::vector<int32_t> si(n_sig + 1, -1);
  std::vector<int64_t> so(n_sig + 1, -1), wo(n_sig + 1, -1), ro(n_sig + 1, -1), sums(3 * SSR_AUD_NT);
  std::vector<double> state((size_t)segs * C * 8 + 1, -777.0), bl((size_t)segs * SSR_AUD_SEG * C + 1, -777.0), stat((size_t)n_sig * 2 + 1, -777.0),
      gimg((size_t)rows * C + 1, -777.0);
  SsrAudParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, tgt_len, tgt_index, n_tgt, n_est);
  p.hop = hop; p.C = C; p.CP = cp; p.range_db = range_db; p.match = match_level != 0;
  p.tab = tab.data(); p.split = split_band; p.sig_index = si.data(); p.seg_off = so.data(); p.wg_off = wo.data(); p.row_off = ro.data();
  p.state = state.data(); p.blk = bl.data(); p.stat = stat.data(); p.gimg = gimg.data();
  p.pair_out = pair_out; p.band_out = band_out; p.image_out = image_out;
  SsrBlk blk{SSR_AUD_NT};
  ssr_aud_geometry_body(p, blk, sums.data());
  if (so[n_sig] != segs || wo[n_sig] != wt + we || ro[n_sig] != rows || (n_tgt > 0 && wo[n_tgt] != wt)) return -1;
  for (int second = 0; second < 2; ++second) {
    if (tgt_f64) sweeps<double>(p, 0, wt, second); else sweeps<float>(p, 0, wt, second);
    if (est_f64) sweeps<double>(p, wt, wt + we, second); else sweeps<float>(p, wt, wt + we, second);
    if (!second)
      for (int64_t id = 0; id < ((int64_t)n_sig * C + 63) / 64 * 64; ++id) ssr_aud_scan_lane(p, id);      // whole waves, as on the device
  }
  if (state.back() != -777.0 || bl.back() != -777.0) return -3;
  auto il = std::make_unique<SsrAudImageLds>();
  for (int s = 0; s < n_sig; ++s) ssr_aud_image_body(p, blk, s, *il);
  auto sl = std::make_unique<SsrAudScoreLds>();
  for (int e = 0; e < n_est; ++e) ssr_aud_score_body(p, blk, e, *sl);
  if (stat.back() != -777.0 || gimg.back() != -777.0 || si[n_sig] != -1) return -3;
  if (power_out)
    for (int s = 0; s < n_sig; ++s) {
      const int T = (int)(ro[s + 1] - ro[s]);
      const double* B = bl.data() + so[s] * SSR_AUD_SEG * C;
      for (int i = 0; i < T * C; ++i) power_out[ro[s] * C + i] = (B[i] + B[i + C]) / (2.0 * (2.0 * (double)hop));
    }
  return 0;
}

// blocks, rows, segments, sweep workgroups of a signal of n samples; then hop-blocks per segment, the block limit, lanes per row
extern "C" void auditory_geometry(int n, int hop, int n_bands, int64_t* res) {
  const int cp = ssr_aud_lanes(n_bands);
  res[0] = ssr_aud_blocks(n, hop); res[1] = ssr_aud_rows(n, hop); res[2] = ssr_aud_segments(n, hop); res[3] = ssr_aud_wgs(n, hop, cp);
  res[4] = SSR_AUD_SEG; res[5] = SSR_AUD_MAX_BLOCKS; res[6] = cp;
}

// the table of a call: [n_bands][12] = Re a, Im a, g, -, a^L binom(L - 1 + d, d) for d = 0 .. 3
extern "C" void auditory_tables(const double* coef, int n_bands, int hop, double* tab) {
  std::vector<double> t;
  ssr_aud_tables_host(coef, n_bands, hop, t);
  for (size_t j = 0; j < t.size(); ++j) tab[j] = t[j];
}
