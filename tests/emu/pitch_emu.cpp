// Host emulation of the pitch kernel bodies (ssr_eval_amd/csrc/ssr_pitch.h) for tests/test_pitch_host.py: every kernel of
// ssr_f0_track / ssr_f0_metrics run in launch order, one workgroup after another.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libpitch_emu.so pitch_emu.cpp
#define SSR_HOST_EMU 1
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_pitch.h"

static void tracks(SsrPitchParams& p) {
  const int n = p.n_a + p.n_b;
  SsrBlk blk{SSR_PITCH_NT};
  std::vector<int64_t> sums(2 * SSR_PITCH_NT);
  ssr_pitch_geometry_body(p, blk, sums.data());
  std::vector<double> xs(SSR_PITCH_XS), d(SSR_PITCH_F * SSR_PITCH_TAU_MAX), wsum(SSR_PITCH_NT), wpart(SSR_PITCH_NT),
      wmin(SSR_PITCH_NT), red(SSR_PITCH_NT + 1);
  std::vector<int> wtau(SSR_PITCH_NT), wcand(SSR_PITCH_NT), wfirst(SSR_PITCH_NT / 64);
  for (int64_t g = 0; g < p.tile_pre[n]; ++g)
    ssr_pitch_track_body(p, blk, g, xs.data(), d.data(), wsum.data(), wpart.data(), wmin.data(), wtau.data(), wcand.data(),
                         wfirst.data());
  for (int i = 0; i < n; ++i) ssr_pitch_voicing_body(p, blk, i, red.data());
}

// sig: float64 16 kHz signals at sig + off[i]; outputs at frame_off[i] = the frames of the signals before i
extern "C" int pitch_track_emu(const double* sig, const int64_t* off, const int32_t* len, int n, double fmin, double fmax,
                               double* f0, double* ap, double* en, uint8_t* voiced) {
  std::vector<int64_t> tp(n + 1), fp(n + 1);
  SsrPitchParams p{};
  p.sig_a = sig; p.off_a = off; p.len_a = len; p.n_a = n; p.n_b = 0;
  p.tau_lo = ssr_pitch_tau_lo(fmax); p.tau_hi = ssr_pitch_tau_hi(fmin); p.nb = ssr_pitch_runs(p.tau_hi);
  p.tile_pre = tp.data(); p.frame_pre = fp.data(); p.frame_off = fp.data();
  p.f0 = f0; p.ap = ap; p.en = en; p.voiced = voiced;
  tracks(p);
  return 0;
}

// out: [n_est][popcount(which)]
extern "C" int pitch_metrics_emu(const double* tgt, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const double* est,
                                 const int64_t* est_off, const int32_t* tgt_index, int n_est, double fmin, double fmax, int which,
                                 double* out) {
  int64_t frames = 0;
  for (int i = 0; i < n_tgt; ++i) frames += ssr_pitch_frames(tgt_len[i]);
  for (int e = 0; e < n_est; ++e) frames += ssr_pitch_frames(tgt_len[tgt_index[e]]);
  std::vector<int64_t> tp(n_tgt + n_est + 1), fp(n_tgt + n_est + 1);
  std::vector<double> f0(frames + 1), ap(frames + 1), en(frames + 1);
  std::vector<uint8_t> vo(frames + 1);
  SsrPitchParams p{};
  p.sig_a = tgt; p.off_a = tgt_off; p.sig_b = est; p.off_b = est_off; p.len_a = tgt_len; p.idx_b = tgt_index;
  p.n_a = n_tgt; p.n_b = n_est;
  p.tau_lo = ssr_pitch_tau_lo(fmax); p.tau_hi = ssr_pitch_tau_hi(fmin); p.nb = ssr_pitch_runs(p.tau_hi);
  p.tile_pre = tp.data(); p.frame_pre = fp.data(); p.frame_off = fp.data();
  p.f0 = f0.data(); p.ap = ap.data(); p.en = en.data(); p.voiced = vo.data();
  p.which = which; p.out = out;
  tracks(p);
  if (fp[n_tgt + n_est] != frames) return -1;
  SsrBlk blk{SSR_PITCH_NT};
  std::vector<double> red(5 * SSR_PITCH_NT), mm(4 * SSR_PITCH_NT), tot(12);
  std::vector<int64_t> cnt(3 * SSR_PITCH_NT);
  for (int e = 0; e < n_est; ++e) ssr_pitch_pair_body(p, blk, e, red.data(), cnt.data(), mm.data(), tot.data());
  return 0;
}

extern "C" void pitch_geometry(double fmin, double fmax, int64_t n, int64_t* res) {
  res[0] = ssr_pitch_tau_lo(fmax); res[1] = ssr_pitch_tau_hi(fmin); res[2] = ssr_pitch_frames(n); res[3] = ssr_pitch_tiles(n);
  res[4] = ssr_pitch_runs((int)res[1]);
}
