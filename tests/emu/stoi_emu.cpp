// Host emulation of the STOI / ESTOI kernel bodies (ssr_eval_amd/csrc/ssr_stoi.h) for tests/test_stoi_host.py: every kernel of
// ssr_stoi run in launch order, one workgroup after another.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -DSSR_HOST_EMU -o libstoi_emu.so stoi_emu.cpp
#define SSR_HOST_EMU 1
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_stoi.h"

extern "C" void stoi_band_edges(int* lo, int* hi) { ssr_stoi_band_edges_host(lo, hi); }

// tgt / est: packed 10 kHz float64 signals; len: [n_tgt + n_est]; out: [n_est][n_out]
extern "C" int stoi_emu(const double* tgt, const int64_t* tgt_off, const double* est, const int64_t* est_off, const int32_t* len,
                        const int32_t* tgt_index, int n_tgt, int n_est, int which, double* out) {
  const int S = n_tgt + n_est;
  int64_t tgt_frames = 0, all_frames = 0, tiles = 0;
  for (int s = 0; s < S; ++s) {
    const int f = ssr_stoi_frames(len[s]);
    all_frames += f;
    if (s < n_tgt) tgt_frames += f;
    else tiles += ssr_stoi_seg_tiles(f);
  }
  std::vector<int64_t> fr(S + 1), st(n_est + 1), sums(2 * SSR_STOI_NT);
  std::vector<double> win(SSR_STOI_FRAME), energy(tgt_frames + 1), tob(all_frames * SSR_STOI_BANDS + 1), part(2 * tiles + 2);
  std::vector<int32_t> kept(tgt_frames + 1), n_kept(n_tgt + 1);
  SsrStoiParams p{};
  p.tgt = tgt; p.tgt_off = tgt_off; p.est = est; p.est_off = est_off; p.len = len; p.tgt_index = tgt_index;
  p.n_tgt = n_tgt; p.n_est = n_est; p.which = which;
  p.fr_off = fr.data(); p.st_off = st.data(); p.win = win.data(); p.energy = energy.data(); p.kept = kept.data();
  p.n_kept = n_kept.data(); p.tob = tob.data(); p.part = part.data(); p.out = out;
  ssr_stoi_band_edges_host(p.band_lo, p.band_hi);
  SsrBlk blk{SSR_STOI_NT};
  ssr_stoi_geometry_body(p, blk, sums.data());
  if (fr[S] != all_frames || st[n_est] != tiles) return -1;
  for (int64_t g = 0; g < tgt_frames; ++g) ssr_stoi_energy(p, g);
  std::vector<double> red(SSR_STOI_NT);
  std::vector<int> cnt(SSR_STOI_NT);
  for (int t = 0; t < n_tgt; ++t) ssr_stoi_vad_body(p, blk, t, red.data(), cnt.data());
  std::vector<double> re(SSR_STOI_NFFT), im(SSR_STOI_NFFT), twr(256), twi(256), pw(257);
  for (int64_t g = 0; g < all_frames; ++g) ssr_stoi_bands_body(p, blk, g, re.data(), im.data(), twr.data(), twi.data(), pw.data());
  SsrBlk wave{SSR_STOI_SEG};
  std::vector<double> X(SSR_STOI_SEG_ROWS * SSR_STOI_BANDS), Y(SSR_STOI_SEG_ROWS * SSR_STOI_BANDS), rs(4 * SSR_STOI_BANDS * SSR_STOI_SEG),
      r2(2 * SSR_STOI_SEG);
  for (int64_t g = 0; g < tiles; ++g) ssr_stoi_segments_body(p, wave, g, X.data(), Y.data(), rs.data(), r2.data());
  for (int e = 0; e < n_est; ++e) ssr_stoi_finalize(p, e);
  return 0;
}
