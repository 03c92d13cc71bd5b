// Host emulation of the modulation kernel bodies (ssr_eval_amd/csrc/ssr_modulation.h on the sweeps of ssr_auditory.h) for
// tests/test_modulation_host.py: every kernel of ssr_modulation run in launch order, one workgroup after another.  Test
// infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libmodulation_emu.so modulation_emu.cpp
#define SSR_HOST_EMU 1
#include <memory>
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_modulation.h"

template <typename X> static void sweeps(SsrAudParams& p, int64_t g0, int64_t g1, bool second) {
  auto lds = std::make_unique<SsrAudSweepLds>();
  SsrBlk blk{SSR_AUD_NT};
  for (int64_t g = g0; g < g1; ++g) {
    if (second) ssr_aud_sweep_body<X, true>(p, blk, g, *lds);
    else ssr_aud_sweep_body<X, false>(p, blk, g, *lds);
  }
}

// the arguments of ssr_modulation up to spectrum_out.  The block sums behind a signal's last block and the unused table entries hold
// NaN, as a poisoned workspace would
extern "C" int modulation_emu(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                              int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int hop, int n_bands,
                              const double* coef, const double* mod, int S, const int32_t* kstar, double range_db, const int32_t* split_band,
                              double* signal_out, double* pair_out, double* spectrum_out) {
  if (hop < 1 || n_bands < SSR_AUD_MIN_BANDS || n_bands > SSR_AUD_MAX_BANDS || S < 1 || S > SSR_MOD_MAX_S) return -2;
  const int n_sig = n_tgt + n_est, C = n_bands, cp = ssr_aud_lanes(C);
  int64_t segs = 0, wt = 0, we = 0;
  for (int s = 0; s < n_sig; ++s) {
    const int n = tgt_len[s < n_tgt ? s : tgt_index[s - n_tgt]];
    if (ssr_aud_blocks(n, hop) > SSR_AUD_MAX_BLOCKS) return -2;
    segs += ssr_aud_segments(n, hop);
    (s < n_tgt ? wt : we) += ssr_aud_wgs(n, hop, cp);
  }
  std::vector<double> tab, mtab;
  ssr_aud_tables_host(coef, C, hop, tab);
  ssr_mod_tables_host(mod, S, mtab);
  mtab.resize((size_t)SSR_MOD_TAB + 4 * SSR_MOD_MAX_S, (double)NAN);
  std::vector<int32_t> si(n_sig + 1, -1);
  std::vector<int64_t> so(n_sig + 1, -1), wo(n_sig + 1, -1), ro(n_sig + 1, -1), sums(3 * SSR_AUD_NT);
  std::vector<double> state((size_t)segs * C * 8 + 1, -777.0), bl((size_t)segs * SSR_AUD_SEG * C + 1, (double)NAN),
      emod((size_t)n_sig * C * SSR_MOD_K + 1, -777.0);
  bl.back() = -777.0;
  SsrAudParams a{};
  ssr_set_pair_sig(a, tgt, tgt_off, est, est_off, tgt_len, tgt_index, n_tgt, n_est);
  a.hop = hop; a.C = C; a.CP = cp;
  a.tab = tab.data(); a.sig_index = si.data(); a.seg_off = so.data(); a.wg_off = wo.data(); a.row_off = ro.data();
  a.state = state.data(); a.blk = bl.data();
  SsrBlk blk{SSR_AUD_NT};
  ssr_aud_geometry_body(a, blk, sums.data());
  if (so[n_sig] != segs || wo[n_sig] != wt + we || (n_tgt > 0 && wo[n_tgt] != wt)) return -1;
  for (int second = 0; second < 2; ++second) {
    if (tgt_f64) sweeps<double>(a, 0, wt, second); else sweeps<float>(a, 0, wt, second);
    if (est_f64) sweeps<double>(a, wt, wt + we, second); else sweeps<float>(a, wt, wt + we, second);
    if (!second)
      for (int64_t id = 0; id < ((int64_t)n_sig * C + 63) / 64 * 64; ++id) ssr_aud_scan_lane(a, id);      // whole waves, as on the device
  }
  if (state.back() != -777.0 || bl.back() != -777.0) return -3;
  SsrModParams p{};
  p.tgt_len = tgt_len; p.tgt_index = tgt_index; p.n_tgt = n_tgt; p.n_est = n_est;
  p.hop = hop; p.C = C; p.S = S; p.range_db = range_db;
  p.sig_index = si.data(); p.seg_off = so.data(); p.blk = bl.data();
  p.tab = mtab.data(); p.kstar = kstar; p.split = split_band; p.emod = emod.data();
  p.signal_out = signal_out; p.pair_out = pair_out; p.spectrum_out = spectrum_out;
  auto bank = std::make_unique<SsrModBankLds>();
  for (int s = 0; s < n_sig; ++s) {
    if (C > 32) ssr_mod_bank_body<true>(p, blk, s, *bank);
    else ssr_mod_bank_body<false>(p, blk, s, *bank);
  }
  auto sl = std::make_unique<SsrModSignalLds>();
  for (int s = 0; s < n_sig; ++s) ssr_mod_signal_body(p, blk, s, *sl);
  auto pl = std::make_unique<SsrModPairLds>();
  for (int e = 0; e < n_est; ++e) ssr_mod_pair_body(p, blk, e, *pl);
  if (emod.back() != -777.0 || si[n_sig] != -1) return -3;
  return 0;
}

// blocks, frames, segments, sweep workgroups of a signal of n samples; then hop-blocks per segment, segments per sweep workgroup, the
// rows of the bank's staging tile, the block limit, the largest S
extern "C" void modulation_geometry(int n, int hop, int n_bands, int S, int64_t* res) {
  const int cp = ssr_aud_lanes(n_bands);
  res[0] = ssr_aud_blocks(n, hop); res[1] = ssr_mod_frames((int)res[0], S); res[2] = ssr_aud_segments(n, hop); res[3] = ssr_aud_wgs(n, hop, cp);
  res[4] = SSR_AUD_SEG; res[5] = SSR_AUD_NT / cp; res[6] = SSR_MOD_TILE; res[7] = SSR_AUD_MAX_BLOCKS; res[8] = SSR_MOD_MAX_S;
}

// the table of a call: [40 + 4 S] = the biquads, then the window
extern "C" void modulation_tables(const double* mod, int S, double* tab) {
  std::vector<double> t;
  ssr_mod_tables_host(mod, S, t);
  for (size_t j = 0; j < t.size(); ++j) tab[j] = t[j];
}
