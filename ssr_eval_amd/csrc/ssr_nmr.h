// Kernel bodies of the noise-to-mask family (Total NMR and Relative Disturbed Frames on the FFT ear model of ITU-R BS.1387 as laid out
// by Kabal 2002; no conformance is claimed), restated in DESIGN §28.  Target x, estimate y, float32 or float64 signals read in their
// own dtype; all arithmetic is float64.  Framing (hop N / 2), the packing of two frames of ONE signal into one complex transform and
// the live / silent rule are the CSII family's (ssr_csii.h), the chunk geometry is the coherence family's;
// what is new is the ear model, the masking threshold with its recursion over time and the noise pattern.
//
//   power      Px[t][k] = w2[k] |X|^2 with w2 = G W2 the host's table (level and ear weighting, w2[0] = 0); Pd[t][k] = w2[k] (|X| -
//              |Y|)^2 with literal square roots
//   bands      band i covers bins k_lo .. k_hi with weight u_lo on the first, u_hi on the last and 1 between them (k_lo == k_hi:
//              u_lo alone): Eb[i] = sum + Ein[i], Pn[i] = sum
//   spreading  over frequency, the target only.  Source band l: L = 10 log10 Eb[l], upper slope s = c_up[l] + 0.2 L dB / Bark, r =
//              10^(s dz / 10); the column sum A[l] = sum_{j = 0}^{Nc - 1 - l} r^j (a running product, no closed form: it has no
//              pole at r = 1) + ad[l], the host's sum of the fixed lower slope.  THE FORM USED: in log2 - lp[l] = 0.4 log2(Eb[l] /
//              A[l]), lq[l] = 0.4 log2 r - a lane per band i adds exp2(lp[l] + (i - l) lq[l]) over l = 0 .. i in that order (one
//              exp2 per term and no cross-lane hand-off; the geometric form by running products needs a barrier per step or a
//              serial lane), and the fixed lower slope over l = i + 1 .. Nc - 1 by a running product of q_d = 10^(-0.27).  Es[i] =
//              T^2.5 / Bs[i], T^2.5 = T T sqrt(T).  The oracle's direct `** 0.4` form is met within 1e-9 relative
//   time       Ef[t] = a Ef[t - 1] + (1 - a) Es[t] from Ef[-1] = 0, M[t] = max(Ef[t], Es[t]) mgain: a lane per band walks the frames
//   values     R = Pn / M (M > 0: Ein > 0 is checked on the host); per chunk and band the sum of R over the chunk's frames, the sum
//              of 10 log10 max(mean_i R, 1e-20) over them and the frames with max_i R >= 10^0.15; a value at or under the floor is
//              -200 exactly, no logarithm
//
//   geometry   one workgroup: ssr_run_geometry_body on chunks of SSR_COH_FR frames per pair, then the frame and the chunk prefix
//              over the targets
//   excite     a workgroup of N / 8 threads per (target, chunk): Es of the chunk's frames into the mask area
//   mask       a workgroup of SSR_NMR_BT threads per target: Es -> M in place (a target shared by K estimates is done once)
//   noise      a workgroup of N / 8 threads per (pair, chunk): the target's and the estimate's frame pairs through separate
//              transforms (never one signal per part: y == x gives Pn == 0 exactly, and a mask does not see the estimates), one
//              partial row [n_bands + 2] per chunk
//   score      a workgroup of SSR_NMR_BT threads per pair: the chunk rows in chunk order, the split, the NaN and floor rules
//
// The chunking of a signal depends on its own length only and every sum has a fixed order: a pair has the same bits alone, in any
// batch and at any position.  There are no atomics.  All bodies compile on the host too (SSR_HOST_EMU, tests/emu/nmr_emu.cpp).
#pragma once
#include "ssr_csii.h"

#define SSR_NMR_NT 256                     // threads of the geometry workgroup
#define SSR_NMR_BT 128                     // threads of the mask and of the score workgroup
#define SSR_NMR_MAX_BANDS 128              // 109 bands of a quarter Bark reach 18 kHz
#define SSR_NMR_COLS 6                     // nmr, nmr_seg, rdf, nmr_hf, nmr_lf, frames
#define SSR_NMR_TAB 8                      // per band: u_lo, u_hi, Ein, c_up, ad, 1 / Bs, a, mgain
#define SSR_NMR_DZ 0.25                    // Bark per band
#define SSR_NMR_FLOOR 1e-20
#define SSR_NMR_RDF 1.4125375446227544     // 10^0.15: a frame is disturbed where max_i R reaches 1.5 dB
static_assert(SSR_NMR_NT == SSR_PAIRS_NT, "the geometry workgroup is ssr_run_geometry_body's");

struct SsrNmrParams {
  const void* tgt;              // targets, float32 or float64
  const int64_t* tgt_off;       // [n_tgt] device
  const void* est;              // estimates, float32 or float64
  const int64_t* est_off;       // [n_est] device
  const int32_t* tgt_len;       // [n_tgt] (workspace copy)
  const int32_t* tgt_index;     // [n_est] (workspace copy)
  int n_tgt, n_est;
  int N, H, n_bands;
  const int32_t* split;         // [n_est] first band of the upper part, in [0, n_bands]; -1: no split (workspace copy)
  const int32_t* bins;          // [n_bands][2] k_lo <= k_hi in [0, N / 2] (workspace copy)
  const double* tab;            // [n_bands][SSR_NMR_TAB] (workspace copy)
  const double* w2;             // [N / 2 + 1] G W2
  const cx<double>* tw;         // [N] exp(-2 pi i k / N); the window is 0.5 - 0.5 Re tw
  int64_t* seg_off;             // [n_tgt + 1] frame prefix over the targets
  int64_t* tchunk_off;          // [n_tgt + 1] chunk prefix over the targets (the excite grid)
  int32_t* run_start;           // [n_est + 1] ssr_run_geometry_body's runs (not used further)
  int64_t* run_chunk;           // [n_est + 1]
  int64_t* chunk_off;           // [n_est + 1] chunk prefix over pairs (the noise grid)
  double* mask;                 // [seg_off[n_tgt]][n_bands] Es, then M
  double* part;                 // [chunk_off[n_est]][n_bands + 2] per band the sum of R, then the dB sum and the disturbed frames
  double* out;                  // [n_est][SSR_NMR_COLS]
  double* bands_out;            // [n_est][n_bands] mean_t R, or null
  double* mask_out;             // [seg_off[n_tgt]][n_bands] a copy of M, or null
#ifdef SSR_HOST_EMU
  const int64_t* ratio_off;     // [n_est] frame prefix over the pairs (the emulation's view of every frame; the device has no such row)
  double* ratio_out;            // [ratio_off's total][n_bands] R of every frame of every pair, or null
#endif
};

// 10 log10 max(v, floor); at or under the floor -200 exactly
SSR_DEV double ssr_nmr_db(double v) { return v > SSR_NMR_FLOOR ? 10.0 * log10(v) : -200.0; }

// sum_k U[i][k] pw[k] of one band
SSR_DEV double ssr_nmr_group(const double* pw, int k_lo, int k_hi, double u_lo, double u_hi) {
  double a = u_lo * pw[k_lo];
  for (int k = k_lo + 1; k < k_hi; ++k) a += pw[k];
  if (k_hi > k_lo) a += u_hi * pw[k_hi];
  return a;
}

// ---- geometry: one workgroup of SSR_NMR_NT threads.  LDS: 3 * NT int64.  The chunk prefix over the pairs, then the frame and the
// chunk prefix over the targets: thread t owns targets [t c, (t + 1) c), c = ceil(n_tgt / NT)
template <typename BLK> SSR_BODY void ssr_nmr_geometry_body(const SsrNmrParams& p, BLK& blk, int64_t* sums) {
  ssr_run_geometry_body(p.tgt_len, p.tgt_index, p.n_est, [&](int32_t n) { return (int64_t)ssr_coh_chunks(n, p.N, p.H); }, p.run_start,
                        p.run_chunk, p.chunk_off, (double*)nullptr, 0, blk, sums);
  constexpr int NT = SSR_NMR_NT;
  const int c = (p.n_tgt + NT - 1) / NT;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    int64_t a = 0, b = 0;
    for (int t = tid * c; t < p.n_tgt && t < (tid + 1) * c; ++t) {
      a += ssr_coh_segments(p.tgt_len[t], p.N, p.H);
      b += ssr_coh_chunks(p.tgt_len[t], p.N, p.H);
    }
    sums[tid] = a;
    sums[NT + tid] = b;
  });
  SSR_PHASE(blk, regs, {
    if (tid < 2) {
      int64_t a = 0;
      for (int t = 0; t < NT; ++t) { const int64_t v = sums[tid * NT + t]; sums[tid * NT + t] = a; a += v; }
      (tid == 0 ? p.seg_off : p.tchunk_off)[p.n_tgt] = a;
    }
  });
  SSR_PHASE(blk, regs, {
    int64_t a = sums[tid], b = sums[NT + tid];
    for (int t = tid * c; t < p.n_tgt && t < (tid + 1) * c; ++t) {
      p.seg_off[t] = a;
      p.tchunk_off[t] = b;
      a += ssr_coh_segments(p.tgt_len[t], p.N, p.H);
      b += ssr_coh_chunks(p.tgt_len[t], p.N, p.H);
    }
  });
}

// LDS of the excite and of the noise body
template <int LOGN> struct SsrNmrLds {
  SsrCohLds<LOGN> f;                                   // the transform and the live flags of its two frames
  double pw[2][(1 << LOGN) / 2 + 1];                   // Px (excite) or Pd (noise) of the two frames in flight
  double lp[2][SSR_NMR_MAX_BANDS];                     // excite: 0.4 log2(Eb / A) per source band; noise: R of the two frames
  double lq[2][SSR_NMR_MAX_BANDS];                     // excite: 0.4 log2 r
  double P[2][SSR_NMR_MAX_BANDS];                      // excite: exp2(lp)
  double bsum[SSR_NMR_MAX_BANDS];                      // noise: per band the sum of R over the chunk's frames
  double seg[2], cnt[2];                               // noise: dB sum and disturbed frames of the even and of the odd frames
};

struct SsrNmrRegs {
  cx<double> v[8];
  double w[8];                              // the window at this thread's eight first-pass samples (the same in every frame)
  double g[5];                              // w2 at bins 4 tid .. 4 tid + 3, and at bin N / 2 on the last thread
  double xa[5], xb[5];                      // noise: the target's magnitudes of the two frames in flight at this thread's bins
};

// one windowed frame pair of one signal through the transform, natural order in S.f.re / S.f.im, the live flags in S.f.live
#define SSR_NMR_TRANSFORM(sig, t)                                                                                   \
  do {                                                                                                              \
    ssr_launder(blk);     /* (per-pass LDS addresses are recomputed where used, not hoisted across the frame loop) */ \
    SSR_PHASE(blk, regs, {                                                                                          \
      ssr_csii_load_pair<LOGN>(tid, R.w, sig, (t) * H, ((t) + 1) * H, two, R.v);                                    \
      bool la = false, lb = false;                                                                                  \
      SSR_UNROLL for (int r = 0; r < 8; ++r) { la = la || R.v[r].x != 0.0; lb = lb || R.v[r].y != 0.0; }            \
      SSR_WAVE_ANY_STORE(tid, la, S.f.live[0]);                                                                     \
      SSR_WAVE_ANY_STORE(tid, lb, S.f.live[1]);                                                                     \
      ssr_fft_compute<double, LOGN, 0>(tid, R.v, tw);                                                               \
      ssr_fft_store<double, LOGN, 0>(tid, S.f.re, S.f.im, R.v);                                                     \
    });                                                                                                             \
    ssr_fft_finish_natural<LOGN>(blk, regs, S.f.re, S.f.im, tw);                                                    \
  } while (0)

// ---- excite: grid block g = (target ti, chunk c), N / 8 threads
template <typename TT, int LOGN, typename BLK> SSR_BODY void ssr_nmr_excite_body(const SsrNmrParams& p, BLK& blk, int64_t g, SsrNmrLds<LOGN>& S) {
  using PL = SsrFftPlan<LOGN>;
  constexpr int N = PL::N, NT = PL::NT, NW = (NT + 63) / 64;
  const int ti = ssr_prefix_find(p.tchunk_off, p.n_tgt, g);
  const int ch = (int)(g - p.tchunk_off[ti]);
  const int H = p.H, Nc = p.n_bands;
  const int K = ssr_coh_segments(p.tgt_len[ti], N, H);
  const int t0 = ch * SSR_COH_FR, t1 = t0 + SSR_COH_FR < K ? t0 + SSR_COH_FR : K;
  const TT* x = (const TT*)p.tgt + p.tgt_off[ti];
  const cx<double>* tw = p.tw;
  const double* tab = p.tab;
  double* es = p.mask + p.seg_off[ti] * Nc;
  const double kq = 0.1 * SSR_NMR_DZ * 3.321928094887362;      // log2 r = s dz / 10 * log2(10)
  const double qd = 0.537031796370253;                         // 10^(-2.7 dz * 0.4): the lower slope per band, to the power 0.4
  SSR_REGS(SsrNmrRegs, regs, blk);
  SSR_PHASE(blk, regs, {
    SSR_UNROLL for (int r = 0; r < 8; ++r) R.w[r] = 0.5 - 0.5 * tw[ssr_fft_first_index<LOGN>(tid, r)].x;
    SSR_UNROLL for (int j = 0; j < 5; ++j) R.g[j] = (j < 4 || tid == NT - 1) ? p.w2[4 * tid + j] : 0.0;
  });
  for (int t = t0; t < t1; t += 2) {
    const bool two = t + 1 < t1;
    SSR_NMR_TRANSFORM(x, t);
    SSR_PHASE(blk, regs, {
      int live_a = 0, live_b = 0;
      for (int q = 0; q < NW; ++q) { live_a |= S.f.live[0][q]; live_b |= S.f.live[1][q]; }
      SSR_UNROLL for (int j = 0; j < 5; ++j) {
        if (j < 4 || tid == NT - 1) {
          cx<double> A, B;
          ssr_csii_split<N>(S.f.re, S.f.im, 4 * tid + j, live_a, live_b, A, B);
          S.pw[0][4 * tid + j] = R.g[j] * (A.x * A.x + A.y * A.y);
          S.pw[1][4 * tid + j] = R.g[j] * (B.x * B.x + B.y * B.y);
        }
      }
    });
    // source role: a lane per (frame, band l)
    SSR_PHASE(blk, regs, {
      for (int m = tid; m < 2 * Nc; m += NT) {
        const int f = m >= Nc ? 1 : 0, l = m - f * Nc;
        if (f == 0 || two) {
          const double* row = tab + l * SSR_NMR_TAB;
          const double eb = ssr_nmr_group(S.pw[f], p.bins[2 * l], p.bins[2 * l + 1], row[0], row[1]) + row[2];
          const double lr = (row[3] + 0.2 * (10.0 * log10(eb))) * kq;
          const double r = exp2(lr);
          double a = 0.0, gq = 1.0;
          for (int j = 0; j < Nc - l; ++j) { a += gq; gq *= r; }
          a += row[4];
          const double lp = 0.4 * log2(eb / a);
          S.lp[f][l] = lp;
          S.lq[f][l] = 0.4 * lr;
          S.P[f][l] = exp2(lp);
        }
      }
    });
    // target role: a lane per (frame, band i)
    SSR_PHASE(blk, regs, {
      for (int m = tid; m < 2 * Nc; m += NT) {
        const int f = m >= Nc ? 1 : 0, i = m - f * Nc;
        if (f == 0 || two) {
          double T = 0.0;
          for (int l = 0; l <= i; ++l) T += exp2(S.lp[f][l] + (double)(i - l) * S.lq[f][l]);
          double gq = qd;
          for (int l = i + 1; l < Nc; ++l) { T += S.P[f][l] * gq; gq *= qd; }
          es[(int64_t)(t + f) * Nc + i] = T * T * sqrt(T) * tab[i * SSR_NMR_TAB + 5];
        }
      }
    });
  }
}

// ---- mask: workgroup ti walks the frames of target ti, SSR_NMR_BT threads, a lane per band
template <typename BLK> SSR_BODY void ssr_nmr_mask_body(const SsrNmrParams& p, BLK& blk, int ti) {
  constexpr int NT = SSR_NMR_BT;
  const int Nc = p.n_bands;
  const int K = ssr_coh_segments(p.tgt_len[ti], p.N, p.H);
  double* m = p.mask + p.seg_off[ti] * Nc;
  double* mo = p.mask_out ? p.mask_out + p.seg_off[ti] * Nc : nullptr;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    for (int i = tid; i < Nc; i += NT) {
      const double a = p.tab[i * SSR_NMR_TAB + 6], mg = p.tab[i * SSR_NMR_TAB + 7];
      double ef = 0.0;
      for (int t = 0; t < K; ++t) {
        const double e = m[(int64_t)t * Nc + i];
        ef = a * ef + (1.0 - a) * e;
        const double v = (ef > e ? ef : e) * mg;
        m[(int64_t)t * Nc + i] = v;
        if (mo) mo[(int64_t)t * Nc + i] = v;
      }
    }
  });
}

// ---- noise: grid block g = (pair e, chunk c), N / 8 threads
template <typename TT, typename TE, int LOGN, typename BLK>
SSR_BODY void ssr_nmr_noise_body(const SsrNmrParams& p, BLK& blk, int64_t g, SsrNmrLds<LOGN>& S) {
  using PL = SsrFftPlan<LOGN>;
  constexpr int N = PL::N, NT = PL::NT, NW = (NT + 63) / 64;
  const int e = ssr_prefix_find(p.chunk_off, p.n_est, g);
  const int ch = (int)(g - p.chunk_off[e]);
  const int ti = p.tgt_index[e];
  const int H = p.H, Nc = p.n_bands;
  const int K = ssr_coh_segments(p.tgt_len[ti], N, H);
  const int t0 = ch * SSR_COH_FR, t1 = t0 + SSR_COH_FR < K ? t0 + SSR_COH_FR : K;
  const TT* x = (const TT*)p.tgt + p.tgt_off[ti];
  const TE* y = (const TE*)p.est + p.est_off[e];
  const cx<double>* tw = p.tw;
  const double* tab = p.tab;
  const double* M = p.mask + p.seg_off[ti] * Nc;
  SSR_REGS(SsrNmrRegs, regs, blk);
  SSR_PHASE(blk, regs, {
    SSR_UNROLL for (int r = 0; r < 8; ++r) R.w[r] = 0.5 - 0.5 * tw[ssr_fft_first_index<LOGN>(tid, r)].x;
    SSR_UNROLL for (int j = 0; j < 5; ++j) R.g[j] = (j < 4 || tid == NT - 1) ? p.w2[4 * tid + j] : 0.0;
    for (int i = tid; i < Nc; i += NT) S.bsum[i] = 0.0;
    if (tid < 2) { S.seg[tid] = 0.0; S.cnt[tid] = 0.0; }
  });
  for (int t = t0; t < t1; t += 2) {
    const bool two = t + 1 < t1;
    SSR_NMR_TRANSFORM(x, t);
    SSR_PHASE(blk, regs, {
      int live_a = 0, live_b = 0;
      for (int q = 0; q < NW; ++q) { live_a |= S.f.live[0][q]; live_b |= S.f.live[1][q]; }
      SSR_UNROLL for (int j = 0; j < 5; ++j) {
        if (j < 4 || tid == NT - 1) {
          cx<double> A, B;
          ssr_csii_split<N>(S.f.re, S.f.im, 4 * tid + j, live_a, live_b, A, B);
          R.xa[j] = sqrt(A.x * A.x + A.y * A.y);
          R.xb[j] = sqrt(B.x * B.x + B.y * B.y);
        }
      }
    });
    SSR_NMR_TRANSFORM(y, t);
    SSR_PHASE(blk, regs, {
      int live_a = 0, live_b = 0;
      for (int q = 0; q < NW; ++q) { live_a |= S.f.live[0][q]; live_b |= S.f.live[1][q]; }
      SSR_UNROLL for (int j = 0; j < 5; ++j) {
        if (j < 4 || tid == NT - 1) {
          cx<double> A, B;
          ssr_csii_split<N>(S.f.re, S.f.im, 4 * tid + j, live_a, live_b, A, B);
          const double da = R.xa[j] - sqrt(A.x * A.x + A.y * A.y), db = R.xb[j] - sqrt(B.x * B.x + B.y * B.y);
          S.pw[0][4 * tid + j] = R.g[j] * (da * da);
          S.pw[1][4 * tid + j] = R.g[j] * (db * db);
        }
      }
    });
    SSR_PHASE(blk, regs, {
      for (int m = tid; m < 2 * Nc; m += NT) {
        const int f = m >= Nc ? 1 : 0, i = m - f * Nc;
        if (f == 0 || two) {
          const double* row = tab + i * SSR_NMR_TAB;
          S.lp[f][i] = ssr_nmr_group(S.pw[f], p.bins[2 * i], p.bins[2 * i + 1], row[0], row[1]) / M[(int64_t)(t + f) * Nc + i];
#ifdef SSR_HOST_EMU
          if (p.ratio_out) p.ratio_out[(p.ratio_off[e] + t + f) * Nc + i] = S.lp[f][i];
#endif
        }
      }
    });
    SSR_PHASE(blk, regs, {
      for (int i = tid; i < Nc; i += NT) {
        double a = S.bsum[i] + S.lp[0][i];
        if (two) a += S.lp[1][i];
        S.bsum[i] = a;
      }
      if (tid == 0 || (tid == 1 && two)) {      // a lane per frame: the bands in order
        double a = 0.0, mx = 0.0;
        for (int i = 0; i < Nc; ++i) { const double v = S.lp[tid][i]; a += v; mx = v > mx ? v : mx; }
        S.seg[tid] += ssr_nmr_db(a / (double)Nc);
        S.cnt[tid] += mx >= SSR_NMR_RDF ? 1.0 : 0.0;
      }
    });
  }
  SSR_PHASE(blk, regs, {
    double* row = p.part + g * (Nc + 2);
    for (int i = tid; i < Nc; i += NT) row[i] = S.bsum[i];
    if (tid == 0) { row[Nc] = S.seg[0] + S.seg[1]; row[Nc + 1] = S.cnt[0] + S.cnt[1]; }
  });
}

// LDS of the score body
struct SsrNmrScoreLds {
  double tot[SSR_NMR_MAX_BANDS];
};

// ---- score: workgroup e scores pair e, SSR_NMR_BT threads
template <typename BLK> SSR_BODY void ssr_nmr_score_body(const SsrNmrParams& p, BLK& blk, int e, SsrNmrScoreLds& S) {
  constexpr int NT = SSR_NMR_BT;
  const int Nc = p.n_bands;
  const int K = ssr_coh_segments(p.tgt_len[p.tgt_index[e]], p.N, p.H);
  const int64_t c0 = p.chunk_off[e], c1 = p.chunk_off[e + 1];
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    for (int i = tid; i < Nc; i += NT) {
      double a = 0.0;
      for (int64_t c = c0; c < c1; ++c) a += p.part[c * (Nc + 2) + i];
      S.tot[i] = a;
      if (p.bands_out) p.bands_out[(int64_t)e * Nc + i] = K > 0 ? a / (double)K : (double)NAN;
    }
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      double* o = p.out + (int64_t)e * SSR_NMR_COLS;
      const int sp = p.split[e];
      double all = 0.0, hf = 0.0, lf = 0.0, seg = 0.0, cnt = 0.0;
      for (int i = 0; i < Nc; ++i) all += S.tot[i];
      for (int i = 0; i < Nc; ++i) {
        if (sp >= 0 && i >= sp) hf += S.tot[i];
        else if (sp >= 0) lf += S.tot[i];
      }
      for (int64_t c = c0; c < c1; ++c) { seg += p.part[c * (Nc + 2) + Nc]; cnt += p.part[c * (Nc + 2) + Nc + 1]; }
      const double k = (double)K;
      o[0] = K > 0 ? ssr_nmr_db(all / (k * (double)Nc)) : (double)NAN;
      o[1] = K > 0 ? seg / k : (double)NAN;
      o[2] = K > 0 ? cnt / k : (double)NAN;
      o[3] = K > 0 && sp >= 0 && sp < Nc ? ssr_nmr_db(hf / (k * (double)(Nc - sp))) : (double)NAN;
      o[4] = K > 0 && sp > 0 ? ssr_nmr_db(lf / (k * (double)sp)) : (double)NAN;
      o[5] = k;
    }
  });
}
