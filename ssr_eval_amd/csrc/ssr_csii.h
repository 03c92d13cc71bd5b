// Kernel bodies of the coherence speech intelligibility index (CSII and the fitted I3: Kates & Arehart 2005), restated in DESIGN
// §26.  Target x, estimate y, float32 or float64 signals read in their own dtype; all arithmetic is float64.  Framing, the packing of
// two real signals into one complex transform, the live / silent rule, the zero rule and the clamp of g2 and the chunk geometry are
// the coherence family's (ssr_coherence.h); what is new is the level class of a target segment, one accumulator set per
// class and the critical-band stage.
//
//   level      ms_t = the mean square of the N unwindowed target samples of segment t, ms_all = that of all n samples; class high
//              (3) where ms_t >= ms_all, mid (2) where ms_t >= 0.1 ms_all, low (1) where ms_t >= 0.001 ms_all, else dropped (0);
//              ms_t == 0 is dropped; ms_all == 0 marks every segment -1: every value of such a target is NaN.  No logarithm
//   sets       all = every one of the K segments, low, mid, high = the segments of that class: Sxx, Syy, Sxy summed over the set's
//              segments in segment order, g2 by §20's rule; a set of fewer than 2 segments is NaN
//   bands      W [n_bands][N / 2 + 1], a dense table the host built (rounded-exponential weights of the critical bands, W[j][0] =
//              0); num_j = sum_k W g2 Syy, den_j = sum_k W (1 - g2) Syy; T_j = 0 where num + den == 0 or num == 0, 1 where den ==
//              0, else (clip(10 log10(num / den), -15, 15) + 15) / 30
//   outputs    CSII_S = sum_j I_j T_j with the importance I (sum 1); above a split band s the same over j >= s with the importance
//              renormalised (NaN for s < 0 or s >= n_bands); i3 = 1 / (1 + exp(-(-3.47 + 1.84 CSII_low + 9.99 CSII_mid)))
//
//   levels     workgroup t of SSR_CSII_NT threads classifies target t: lane sums of squares over samples tid, tid + NT, ... with
//              fused multiply-adds, a wave sum, the waves in order; then a lane per segment, its N squares summed in sample order
//   spectra    §20's spectra geometry - a workgroup of N / 8 threads per (pair, chunk of 32 segments), two real frames per complex
//              transform - with four accumulator sets in registers: a segment's class is the same in every lane, so a segment
//              adds to `all` and, under a uniform branch, to at most one class set.  The two frames of a transform are segments t
//              and t + 1 of ONE signal, not the target and the estimate of one segment: the same number of transforms, and the
//              estimate's gain cannot reach the target's rounding.  One partial row [set][bin][4] per chunk
//   bands      workgroup e of SSR_CSII_NT threads scores pair e: per set the chunk partials in chunk order, g2, then per band lane
//              sums in bin order, a wave reduction, the waves in order; the class counts the same way; lane 0 writes the columns
//
// A target's classes depend on the target alone, a transform holds one segment of one pair and the chunking of a pair depends on its
// own length only: a pair has the same bits alone, in any batch and at any position.  There are no atomics.  All bodies compile on
// the host too (SSR_HOST_EMU, tests/emu/csii_emu.cpp).
#pragma once
#include "ssr_coherence.h"

#define SSR_CSII_NT 256                    // threads of the levels and of the bands workgroup
#define SSR_CSII_MAX_BANDS 21              // the critical bands of ANSI S3.5-1997
#define SSR_CSII_SETS 4                    // all, low, mid, high
#define SSR_CSII_COLS 13                   // csii, csii_low, csii_mid, csii_high, i3, the four sets' _hf values, the four segment counts
static_assert(SSR_CSII_NT == SSR_PAIRS_NT, "the geometry workgroup is ssr_run_geometry_body's");

#ifdef SSR_HOST_EMU
static inline int ssr_csii_uniform(int v) { return v; }
#else
// a value every lane of the wave holds alike, as a scalar: the branch on it is a scalar branch
SSR_DEV int ssr_csii_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
#endif

struct SsrCsiiParams {
  const void* tgt;              // targets, float32 or float64
  const int64_t* tgt_off;       // [n_tgt] device
  const void* est;              // estimates, float32 or float64
  const int64_t* est_off;       // [n_est] device
  const int32_t* tgt_len;       // [n_tgt] (workspace copy)
  const int32_t* tgt_index;     // [n_est] (workspace copy)
  int n_tgt, n_est;
  int N, H, n_bands;
  const int32_t* split;         // [n_est] first band of the upper part, in [0, n_bands]; -1: no split (workspace copy)
  const double* weights;        // [n_bands][N / 2 + 1] W
  const double* importance;     // [n_bands] I, sum 1 (workspace copy)
  const cx<double>* tw;         // [N] exp(-2 pi i k / N); the window is 0.5 - 0.5 Re tw
  int64_t* seg_off;             // [n_tgt + 1] segment prefix over the targets (the geometry kernel writes it)
  int8_t* cls;                  // [seg_off[n_tgt]] class of every segment of every target
  int32_t* run_start;           // [n_est + 1] ssr_run_geometry_body's runs (not used further)
  int64_t* run_chunk;           // [n_est + 1]
  int64_t* chunk_off;           // [n_est + 1] chunk prefix over pairs (the spectra grid)
  double* part;                 // [chunk_off[n_est]][4][N / 2 + 1][4] chunk sums per set: Sxx, Syy, Re Sxy, Im Sxy
  double* out;                  // [n_est][SSR_CSII_COLS]
  double* bands_out;            // [n_est][4][n_bands] T_j per set, or null
};

// ---- geometry: one workgroup of SSR_CSII_NT threads.  LDS: 3 * NT int64.  The chunk prefix over the pairs, then the segment
// prefix over the targets: thread t owns targets [t c, (t + 1) c), c = ceil(n_tgt / NT)
template <typename BLK> SSR_BODY void ssr_csii_geometry_body(const SsrCsiiParams& p, BLK& blk, int64_t* sums) {
  ssr_run_geometry_body(p.tgt_len, p.tgt_index, p.n_est, [&](int32_t n) { return (int64_t)ssr_coh_chunks(n, p.N, p.H); }, p.run_start,
                        p.run_chunk, p.chunk_off, (double*)nullptr, 0, blk, sums);
  constexpr int NT = SSR_CSII_NT;
  const int c = (p.n_tgt + NT - 1) / NT;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    int64_t a = 0;
    for (int t = tid * c; t < p.n_tgt && t < (tid + 1) * c; ++t) a += ssr_coh_segments(p.tgt_len[t], p.N, p.H);
    sums[tid] = a;
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      int64_t a = 0;
      for (int t = 0; t < NT; ++t) { const int64_t v = sums[t]; sums[t] = a; a += v; }
      p.seg_off[p.n_tgt] = a;
    }
  });
  SSR_PHASE(blk, regs, {
    int64_t a = sums[tid];
    for (int t = tid * c; t < p.n_tgt && t < (tid + 1) * c; ++t) { p.seg_off[t] = a; a += ssr_coh_segments(p.tgt_len[t], p.N, p.H); }
  });
}

struct SsrCsiiLevelsLds {
  double ws[SSR_CSII_NT / 64];              // per wave: the sum of squares of its lanes' samples
};

// ---- levels: workgroup t classifies the segments of target t, SSR_CSII_NT threads
template <typename TT, typename BLK> SSR_BODY void ssr_csii_levels_body(const SsrCsiiParams& p, BLK& blk, int t, SsrCsiiLevelsLds& S) {
  constexpr int NT = SSR_CSII_NT, NW = NT / 64;
  const int n = p.tgt_len[t], N = p.N, H = p.H;
  const int K = ssr_coh_segments(n, N, H);
  const TT* x = (const TT*)p.tgt + p.tgt_off[t];
  int8_t* cls = p.cls + p.seg_off[t];
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    double a = 0.0;
    for (int i = tid; i < n; i += NT) { const double v = (double)x[i]; a = ssr_fma(v, v, a); }
    SSR_WAVE_SUM_STORE(tid, NT, a, S.ws);
  });
  SSR_PHASE(blk, regs, {
    double all = 0.0;
    for (int q = 0; q < NW; ++q) all += S.ws[q];
    const double ms_all = all / (double)n;      // (K >= 1 below: n >= N > 0)
    for (int s = tid; s < K; s += NT) {
      double a = 0.0;
      for (int i = 0; i < N; ++i) { const double v = (double)x[s * H + i]; a = ssr_fma(v, v, a); }
      const double ms = a / (double)N;
      int c = 0;
      if (!(ms_all > 0.0)) c = -1;
      else if (ms > 0.0) c = ms >= ms_all ? 3 : (ms >= 0.1 * ms_all ? 2 : (ms >= 0.001 * ms_all ? 1 : 0));
      cls[s] = (int8_t)c;
    }
  });
}

struct SsrCsiiRegs {
  cx<double> v[8];
  double w[8];                              // the window at this thread's eight first-pass samples (the same in every segment)
  cx<double> xa[5], xb[5];                  // the target's spectra of the two segments in flight at this thread's bins
  double s[SSR_CSII_SETS][5][4];            // per set: Sxx, Syy, Re Sxy, Im Sxy of bins 4 tid .. 4 tid + 3, and of bin N / 2 on the last thread
};

SSR_DEV void ssr_csii_add(double (&s)[5][4], int j, const double* d) {
  s[j][0] += d[0]; s[j][1] += d[1]; s[j][2] += d[2]; s[j][3] += d[3];
}

// Segments a and b of ONE signal packed into one complex frame, in first-pass register order (two: segment b exists)
template <int LOGN, typename T>
SSR_DEV void ssr_csii_load_pair(int tid, const double* w, const T* x, int base_a, int base_b, bool two, cx<double>* v) {
  SSR_UNROLL for (int r = 0; r < 8; ++r) {
    const int i = ssr_fft_first_index<LOGN>(tid, r);
    v[r] = {w[r] * (double)x[base_a + i], two ? w[r] * (double)x[base_b + i] : 0.0};
  }
}

// A[k], B[k] of the two real frames behind Z = A + i B: A = (Z[k] + conj(Z[N - k])) / 2, B = (Z[k] - conj(Z[N - k])) / (2 i); a
// digitally silent frame has its exact value, zero, and the other is taken from Z alone (§20's live / silent rule)
template <int N> SSR_DEV void ssr_csii_split(const double* re, const double* im, int k, int live_a, int live_b, cx<double>& A, cx<double>& B) {
  const int kc = (N - k) & (N - 1);
  const double zr = re[ssr_pad(k)], zi = im[ssr_pad(k)];
  A = {0.0, 0.0};
  B = {0.0, 0.0};
  if (live_a && live_b) {
    const double cr = re[ssr_pad(kc)], ci = im[ssr_pad(kc)];
    A = {0.5 * (zr + cr), 0.5 * (zi - ci)};
    B = {0.5 * (zi + ci), 0.5 * (cr - zr)};
  } else if (live_a) {
    A = {zr, zi};
  } else if (live_b) {
    B = {zi, -zr};
  }
}

// one segment's |X|^2, |Y|^2 and Y conj(X) at bin slot j into `all` and, c = 1, 2, 3 (the same in every lane), into that class set
#define SSR_CSII_ACCUM(s, j, c, X, Y)                                                     \
  do {                                                                                   \
    const cx<double> m_ = ssr_phase_mulc(Y, X);                                          \
    double d_[4];                                                                        \
    d_[0] = (X).x * (X).x + (X).y * (X).y;                                               \
    d_[1] = (Y).x * (Y).x + (Y).y * (Y).y;                                               \
    d_[2] = m_.x;                                                                        \
    d_[3] = m_.y;                                                                        \
    ssr_csii_add((s)[0], j, d_);                                                         \
    if ((c) == 1) ssr_csii_add((s)[1], j, d_);                                           \
    else if ((c) == 2) ssr_csii_add((s)[2], j, d_);                                      \
    else if ((c) == 3) ssr_csii_add((s)[3], j, d_);                                      \
  } while (0)

// ---- spectra: grid block g = (pair e, chunk c), N / 8 threads
template <typename TT, typename TE, int LOGN, typename BLK>
SSR_BODY void ssr_csii_spectra_body(const SsrCsiiParams& p, BLK& blk, int64_t g, SsrCohLds<LOGN>& S) {
  using PL = SsrFftPlan<LOGN>;
  constexpr int N = PL::N, NT = PL::NT, NW = (NT + 63) / 64, NB = N / 2 + 1;
  const int e = ssr_prefix_find(p.chunk_off, p.n_est, g);
  const int ch = (int)(g - p.chunk_off[e]);
  const int ti = p.tgt_index[e];
  const int n = p.tgt_len[ti], H = p.H;
  const int K = ssr_coh_segments(n, N, H);
  const int t0 = ch * SSR_COH_FR, t1 = t0 + SSR_COH_FR < K ? t0 + SSR_COH_FR : K;
  const TT* x = (const TT*)p.tgt + p.tgt_off[ti];
  const TE* y = (const TE*)p.est + p.est_off[e];
  const int8_t* cls = p.cls + p.seg_off[ti];
  const cx<double>* tw = p.tw;
  SSR_REGS(SsrCsiiRegs, regs, blk);
  SSR_PHASE(blk, regs, {
    SSR_UNROLL for (int r = 0; r < 8; ++r) R.w[r] = 0.5 - 0.5 * tw[ssr_fft_first_index<LOGN>(tid, r)].x;
    SSR_UNROLL for (int q = 0; q < SSR_CSII_SETS; ++q) {
      SSR_UNROLL for (int j = 0; j < 5; ++j) { R.s[q][j][0] = R.s[q][j][1] = R.s[q][j][2] = R.s[q][j][3] = 0.0; }
    }
  });
  // Two segments per round, t and t + 1: one complex transform holds the two target segments, a second one the two estimate
  // segments.  A transform never mixes the two signals, so a power-of-two gain on the estimate scales its transform exactly and
  // changes no bit of g2 (§20 packs target and estimate into one transform; there the estimate's level enters the target's rounding)
  for (int t = t0; t < t1; t += 2) {
    const bool two = t + 1 < t1;
    ssr_launder(blk);     // (per-pass LDS addresses are recomputed where used, not hoisted across the segment loop)
    SSR_PHASE(blk, regs, {
      ssr_csii_load_pair<LOGN>(tid, R.w, x, t * H, (t + 1) * H, two, R.v);
      bool la = false, lb = false;
      SSR_UNROLL for (int r = 0; r < 8; ++r) { la = la || R.v[r].x != 0.0; lb = lb || R.v[r].y != 0.0; }
      SSR_WAVE_ANY_STORE(tid, la, S.live[0]);
      SSR_WAVE_ANY_STORE(tid, lb, S.live[1]);
      ssr_fft_compute<double, LOGN, 0>(tid, R.v, tw);
      ssr_fft_store<double, LOGN, 0>(tid, S.re, S.im, R.v);
    });
    ssr_fft_finish_natural<LOGN>(blk, regs, S.re, S.im, tw);
    SSR_PHASE(blk, regs, {
      int live_a = 0, live_b = 0;
      for (int q = 0; q < NW; ++q) { live_a |= S.live[0][q]; live_b |= S.live[1][q]; }
      SSR_UNROLL for (int j = 0; j < 5; ++j) {
        if (j < 4 || tid == NT - 1) ssr_csii_split<N>(S.re, S.im, 4 * tid + j, live_a, live_b, R.xa[j], R.xb[j]);
      }
    });
    ssr_launder(blk);
    SSR_PHASE(blk, regs, {
      ssr_csii_load_pair<LOGN>(tid, R.w, y, t * H, (t + 1) * H, two, R.v);
      bool la = false, lb = false;
      SSR_UNROLL for (int r = 0; r < 8; ++r) { la = la || R.v[r].x != 0.0; lb = lb || R.v[r].y != 0.0; }
      SSR_WAVE_ANY_STORE(tid, la, S.live[0]);
      SSR_WAVE_ANY_STORE(tid, lb, S.live[1]);
      ssr_fft_compute<double, LOGN, 0>(tid, R.v, tw);
      ssr_fft_store<double, LOGN, 0>(tid, S.re, S.im, R.v);
    });
    ssr_fft_finish_natural<LOGN>(blk, regs, S.re, S.im, tw);
    SSR_PHASE(blk, regs, {
      int live_a = 0, live_b = 0;
      for (int q = 0; q < NW; ++q) { live_a |= S.live[0][q]; live_b |= S.live[1][q]; }
      // (the same in every lane: the two segments' classes)
      const int ca = ssr_csii_uniform((int)cls[t]), cb = two ? ssr_csii_uniform((int)cls[t + 1]) : 0;
      SSR_UNROLL for (int j = 0; j < 5; ++j) {
        if (j < 4 || tid == NT - 1) {
          cx<double> Ya, Yb;
          ssr_csii_split<N>(S.re, S.im, 4 * tid + j, live_a, live_b, Ya, Yb);
          SSR_CSII_ACCUM(R.s, j, ca, R.xa[j], Ya);
          if (two) SSR_CSII_ACCUM(R.s, j, cb, R.xb[j], Yb);
        }
      }
    });
  }
  SSR_PHASE(blk, regs, {
    SSR_UNROLL for (int q = 0; q < SSR_CSII_SETS; ++q) {
      double* row = p.part + (((int64_t)g * SSR_CSII_SETS + q) * NB + 4 * tid) * 4;
      SSR_UNROLL for (int j = 0; j < 4; ++j) {
        SSR_UNROLL for (int m = 0; m < 4; ++m) row[4 * j + m] = R.s[q][j][m];
      }
      if (tid == NT - 1) {
        SSR_UNROLL for (int m = 0; m < 4; ++m) row[16 + m] = R.s[q][4][m];
      }
    }
  });
}

// LDS of the bands body
struct SsrCsiiBandsLds {
  double g2[SSR_COH_MAX_BINS], syy[SSR_COH_MAX_BINS];
  double ws[2][SSR_CSII_NT / 64];           // per wave: a band's num and den
  double wc[3][SSR_CSII_NT / 64];           // per wave: the segments of class low, mid, high
  double T[SSR_CSII_SETS][SSR_CSII_MAX_BANDS];
  int silent;                               // the target is digitally silent (ms_all == 0)
};

// ---- bands: workgroup e scores pair e, SSR_CSII_NT threads
template <typename BLK> SSR_BODY void ssr_csii_bands_body(const SsrCsiiParams& p, BLK& blk, int e, SsrCsiiBandsLds& S) {
  constexpr int NT = SSR_CSII_NT, NW = NT / 64;
  const int NB = p.N / 2 + 1, J = p.n_bands;
  const int ti = p.tgt_index[e];
  const int K = ssr_coh_segments(p.tgt_len[ti], p.N, p.H);
  const int8_t* cls = p.cls + p.seg_off[ti];
  const int64_t c0 = p.chunk_off[e], c1 = p.chunk_off[e + 1];
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    double n1 = 0.0, n2 = 0.0, n3 = 0.0;
    for (int s = tid; s < K; s += NT) {
      const int c = cls[s];
      n1 += c == 1 ? 1.0 : 0.0; n2 += c == 2 ? 1.0 : 0.0; n3 += c == 3 ? 1.0 : 0.0;
    }
    SSR_WAVE_SUM_STORE(tid, NT, n1, S.wc[0]);
    SSR_WAVE_SUM_STORE(tid, NT, n2, S.wc[1]);
    SSR_WAVE_SUM_STORE(tid, NT, n3, S.wc[2]);
    if (tid == 0) S.silent = K > 0 && cls[0] < 0;
  });
  for (int q = 0; q < SSR_CSII_SETS; ++q) {
    SSR_PHASE(blk, regs, {
      for (int k = tid; k < NB; k += NT) {
        double sxx = 0.0, syy = 0.0, cr = 0.0, ci = 0.0;
        for (int64_t c = c0; c < c1; ++c) {
          const double* r = p.part + ((c * SSR_CSII_SETS + q) * NB + k) * 4;
          sxx += r[0]; syy += r[1]; cr += r[2]; ci += r[3];
        }
        const double den = sxx * syy;
        double g2 = den == 0.0 ? 0.0 : (cr * cr + ci * ci) / den;
        if (g2 > 1.0) g2 = 1.0;
        S.g2[k] = g2;
        S.syy[k] = syy;
      }
    });
    for (int j = 0; j < J; ++j) {
      const double* W = p.weights + (int64_t)j * NB;
      SSR_PHASE(blk, regs, {
        double a0 = 0.0, a1 = 0.0;
        for (int k = tid; k < NB; k += NT) {
          const double g2 = S.g2[k], wsy = W[k] * S.syy[k];
          a0 += g2 * wsy;
          a1 += (1.0 - g2) * wsy;
        }
        SSR_WAVE_SUM_STORE(tid, NT, a0, S.ws[0]);
        SSR_WAVE_SUM_STORE(tid, NT, a1, S.ws[1]);
      });
      SSR_PHASE(blk, regs, {
        if (tid == 0) {
          double num = 0.0, den = 0.0;
          for (int w = 0; w < NW; ++w) { num += S.ws[0][w]; den += S.ws[1][w]; }
          double T;
          if (num + den == 0.0 || num == 0.0) T = 0.0;
          else if (den == 0.0) T = 1.0;
          else {
            double db = 10.0 * log10(num / den);
            db = db < -15.0 ? -15.0 : (db > 15.0 ? 15.0 : db);
            T = (db + 15.0) / 30.0;
          }
          S.T[q][j] = T;
        }
      });
    }
  }
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      double cnt[SSR_CSII_SETS] = {(double)K, 0.0, 0.0, 0.0};
      for (int m = 0; m < 3; ++m)
        for (int w = 0; w < NW; ++w) cnt[1 + m] += S.wc[m][w];
      const int sp = p.split[e];
      double* o = p.out + (int64_t)e * SSR_CSII_COLS;
      double v[SSR_CSII_SETS];
      for (int q = 0; q < SSR_CSII_SETS; ++q) {
        const bool ok = cnt[q] >= 2.0 && !S.silent;
        // (each sum over its own importance sum, added in the same order: band values of 1 give 1 exactly)
        double a = 0.0, ai = 0.0, h = 0.0, hi = 0.0;
        for (int j = 0; j < J; ++j) {
          a += p.importance[j] * S.T[q][j];
          ai += p.importance[j];
          if (sp >= 0 && j >= sp) { h += p.importance[j] * S.T[q][j]; hi += p.importance[j]; }
        }
        v[q] = ok ? a / ai : (double)NAN;
        o[q] = v[q];
        o[5 + q] = ok && sp >= 0 && sp < J ? h / hi : (double)NAN;
        o[9 + q] = cnt[q];
        if (p.bands_out)
          for (int j = 0; j < J; ++j) p.bands_out[((int64_t)e * SSR_CSII_SETS + q) * J + j] = ok ? S.T[q][j] : (double)NAN;
      }
      o[4] = 1.0 / (1.0 + exp(-(-3.47 + 1.84 * v[1] + 9.99 * v[2])));      // (NaN where either is)
    }
  });
}
