// Kernel bodies of the magnitude-squared coherence family (Welch-averaged MSC and the signal-to-distortion ratio derived from it:
// Kates 1992; Kates & Arehart 2005, the front end of CSII), restated in DESIGN §20.  Target x, estimate y, float32 or float64
// signals read in their own dtype; all arithmetic is float64.
//
//   framing    N = n_fft in {256 .. 2048}, hop H in [1, N], periodic Hann window w[i] = 0.5 - 0.5 cos(2 pi i / N); no padding, no
//              centring, no detrending (SciPy's Welch framing): K = 1 + (n - N) / H segments for n >= N, else 0; segment t covers
//              samples [t H, t H + N); X[t][k], Y[t][k] its N-point DFTs, 0 <= k <= N / 2
//   spectra    Sxx[k] = sum_t |X|^2, Syy[k] = sum_t |Y|^2, Sxy[k] = sum_t Y conj(X); every bin counts once (no one-sided doubling,
//              no density scaling: only ratios are used)
//   coherence  g2[k] = min(1, |Sxy|^2 / (Sxx Syy)), and 0 where Sxx Syy == 0: digital silence is incoherent, not NaN
//   per band   (bins lo <= k <= hi)  msc = mean of g2;  coh_sdr = 10 log10((sum g2 Syy + EPS) / (sum (1 - g2) Syy + EPS)), EPS =
//              DBL_EPSILON - the estimate's power that is a linear function of the target over the power that is not;  coh_bins =
//              the bins with g2 >= thr
//   NaN        K < 2 (one segment gives g2 = 1 identically) and an empty band (lo > hi): all three
//
//   geometry   one workgroup: ssr_run_geometry_body on chunks of SSR_COH_FR segments per pair, their prefix sum over the pairs
//   spectra    one workgroup of N / 8 threads per (pair, chunk): per segment the windowed target goes to the real part and the
//              windowed estimate to the imaginary part of ONE complex N-point transform (the phase family's, ssr_fft.h in LDS;
//              the window comes from the twiddle table); X[k], Y[k] are split from Z[k] and conj(Z[N - k]); a thread owns bins
//              4 tid .. 4 tid + 3 (bin N / 2: the last thread) and keeps their Sxx, Syy, Re Sxy, Im Sxy in registers across the
//              chunk's segments, in segment order; a segment in which one signal is digitally silent has that signal's spectrum
//              set to its exact value, zero, and the other's taken from Z alone (the split would return the loud one's rounding
//              error for it).  One partial row [bin][4] per chunk
//   bands      one workgroup of SSR_COH_NT threads per pair: per bin the chunk partials in chunk order, g2 with the zero rule and
//              the clamp, the optional msc_out row; per band lane sums in bin order, a wave reduction, the waves in order
//
// A transform holds one segment of one pair, the chunking of a pair depends on its own length only and a band's sums start at
// the band's own first bin, so a pair has the same bits alone, in any batch and at any position, and a band's row does not
// depend on the other bands.  There are no atomics.  All bodies compile on the host too (SSR_HOST_EMU, tests/emu/coherence_emu.cpp).
#pragma once
#include "ssr_pairs.h"
#include "ssr_fft.h"
#include "ssr_phase.h"                     // ssr_phase_log2_nfft, ssr_phase_mulc, SSR_PHASE_LOGN_MIN / _MAX: the same transform sizes

#define SSR_COH_FR 32                      // segments per chunk (no warm-up frame: longer than the phase family's 16)
#define SSR_COH_NT 256                     // threads of the geometry and of the bands workgroup
#define SSR_COH_MAX_BANDS 8                // SSR_MAX_BANDS
#define SSR_COH_MAX_BINS ((1 << SSR_PHASE_LOGN_MAX) / 2 + 1)
#define SSR_COH_EPS 2.220446049250313e-16  // DBL_EPSILON
static_assert(SSR_COH_NT == SSR_PAIRS_NT, "the geometry workgroup is ssr_run_geometry_body's");

SSR_HD int ssr_coh_segments(int n, int N, int H) { return n >= N ? 1 + (n - N) / H : 0; }
SSR_HD int ssr_coh_chunks(int n, int N, int H) { return (ssr_coh_segments(n, N, H) + SSR_COH_FR - 1) / SSR_COH_FR; }

struct SsrCohParams {
  const void* tgt;              // targets, float32 or float64
  const int64_t* tgt_off;       // [n_tgt] device
  const void* est;              // estimates, float32 or float64
  const int64_t* est_off;       // [n_est] device
  const int32_t* tgt_len;       // [n_tgt] (workspace copy)
  const int32_t* tgt_index;     // [n_est] (workspace copy)
  int n_tgt, n_est;
  int N, H, n_bands;
  double thr;                   // a bin counts into coh_bins where g2 >= thr
  const int32_t* bands;         // [n_est][n_bands][2] inclusive (lo, hi); lo > hi: the empty band (workspace copy)
  const cx<double>* tw;         // [N] exp(-2 pi i k / N); the window is 0.5 - 0.5 Re tw
  int32_t* run_start;           // [n_est + 1] ssr_run_geometry_body's runs (not used further)
  int64_t* run_chunk;           // [n_est + 1]
  int64_t* chunk_off;           // [n_est + 1] chunk prefix over pairs (the spectra grid)
  double* part;                 // [chunk_off[n_est]][N / 2 + 1][4] chunk sums: Sxx, Syy, Re Sxy, Im Sxy
  double* out;                  // [n_est][n_bands][3]: msc, coh_sdr, coh_bins
  double* msc_out;              // [n_est][N / 2 + 1] g2, or null
};

// ---- geometry: one workgroup of SSR_COH_NT threads.  LDS: 3 * NT int64.
template <typename BLK> SSR_BODY void ssr_coh_geometry_body(const SsrCohParams& p, BLK& blk, int64_t* sums) {
  ssr_run_geometry_body(p.tgt_len, p.tgt_index, p.n_est, [&](int32_t n) { return (int64_t)ssr_coh_chunks(n, p.N, p.H); }, p.run_start,
                        p.run_chunk, p.chunk_off, (double*)nullptr, 0, blk, sums);
}

// LDS of the spectra body
template <int LOGN> struct SsrCohLds {
  double re[ssr_padded_len(1 << LOGN)], im[ssr_padded_len(1 << LOGN)];
  int live[2][4];                           // per wave: the segment has a non-zero windowed sample of the target / of the estimate
};

struct SsrCohRegs {
  cx<double> v[8];
  double w[8];                              // the window at this thread's eight first-pass samples (the same in every segment)
  double s[5][4];                           // Sxx, Syy, Re Sxy, Im Sxy of bins 4 tid .. 4 tid + 3, and of bin N / 2 on the last thread
};

// Two real signals packed into one complex frame, in first-pass register order: the N samples from `base` of x times the window
// into the real parts, of y into the imaginary parts (no padding: the caller's segment lies inside the signal)
template <int LOGN, typename TT, typename TE>
SSR_DEV void ssr_coh_load_segment(int tid, const double* w, const TT* x, const TE* y, int base, cx<double>* v) {
  SSR_UNROLL for (int r = 0; r < 8; ++r) {
    const int i = base + ssr_fft_first_index<LOGN>(tid, r);
    v[r] = {w[r] * (double)x[i], w[r] * (double)y[i]};
  }
}

// ---- spectra: grid block g = (pair e, chunk c), N / 8 threads
template <typename TT, typename TE, int LOGN, typename BLK>
SSR_BODY void ssr_coh_spectra_body(const SsrCohParams& p, BLK& blk, int64_t g, SsrCohLds<LOGN>& S) {
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
  const cx<double>* tw = p.tw;
  SSR_REGS(SsrCohRegs, regs, blk);
  SSR_PHASE(blk, regs, {
    SSR_UNROLL for (int r = 0; r < 8; ++r) R.w[r] = 0.5 - 0.5 * tw[ssr_fft_first_index<LOGN>(tid, r)].x;
    SSR_UNROLL for (int j = 0; j < 5; ++j) { R.s[j][0] = R.s[j][1] = R.s[j][2] = R.s[j][3] = 0.0; }
  });
  for (int t = t0; t < t1; ++t) {
    ssr_launder(blk);     // (per-pass LDS addresses are recomputed where used, not hoisted across the segment loop)
    SSR_PHASE(blk, regs, {
      ssr_coh_load_segment<LOGN>(tid, R.w, x, y, t * H, R.v);
      bool lx = false, ly = false;
      SSR_UNROLL for (int r = 0; r < 8; ++r) { lx = lx || R.v[r].x != 0.0; ly = ly || R.v[r].y != 0.0; }
      SSR_WAVE_ANY_STORE(tid, lx, S.live[0]);
      SSR_WAVE_ANY_STORE(tid, ly, S.live[1]);
      ssr_fft_compute<double, LOGN, 0>(tid, R.v, tw);
      ssr_fft_store<double, LOGN, 0>(tid, S.re, S.im, R.v);
    });
    ssr_fft_finish_natural<LOGN>(blk, regs, S.re, S.im, tw);
    SSR_PHASE(blk, regs, {
      // X[k] = (Z[k] + conj(Z[N - k])) / 2, Y[k] = (Z[k] - conj(Z[N - k])) / (2 i) (at k = 0 and k = N / 2: Re Z[k] and Im Z[k]);
      // with the target silent Z = i Y, with the estimate silent Z = X
      int live_x = 0, live_y = 0;
      for (int q = 0; q < NW; ++q) { live_x |= S.live[0][q]; live_y |= S.live[1][q]; }
      SSR_UNROLL for (int j = 0; j < 5; ++j) {
        const int k = 4 * tid + j, kc = (N - k) & (N - 1);
        if (j < 4 || tid == NT - 1) {
          const double zr = S.re[ssr_pad(k)], zi = S.im[ssr_pad(k)];
          if (live_x && live_y) {
            const double cr = S.re[ssr_pad(kc)], ci = S.im[ssr_pad(kc)];
            const cx<double> X = {0.5 * (zr + cr), 0.5 * (zi - ci)}, Y = {0.5 * (zi + ci), 0.5 * (cr - zr)};
            const cx<double> c = ssr_phase_mulc(Y, X);
            R.s[j][0] += X.x * X.x + X.y * X.y;
            R.s[j][1] += Y.x * Y.x + Y.y * Y.y;
            R.s[j][2] += c.x;
            R.s[j][3] += c.y;
          } else if (live_x) {
            R.s[j][0] += zr * zr + zi * zi;
          } else if (live_y) {
            R.s[j][1] += zr * zr + zi * zi;
          }
        }
      }
    });
  }
  SSR_PHASE(blk, regs, {
    double* row = p.part + ((int64_t)g * NB + 4 * tid) * 4;
    SSR_UNROLL for (int j = 0; j < 4; ++j) {
      SSR_UNROLL for (int q = 0; q < 4; ++q) row[4 * j + q] = R.s[j][q];
    }
    if (tid == NT - 1) {
      SSR_UNROLL for (int q = 0; q < 4; ++q) row[16 + q] = R.s[4][q];
    }
  });
}

// LDS of the bands body
struct SsrCohBandsLds {
  double g2[SSR_COH_MAX_BINS], syy[SSR_COH_MAX_BINS];
  double ws[4][SSR_COH_NT / 64];            // per wave: a band's sums of g2, g2 Syy, (1 - g2) Syy and its count of g2 >= thr
};

// ---- bands: workgroup e scores pair e, SSR_COH_NT threads
template <typename BLK> SSR_BODY void ssr_coh_bands_body(const SsrCohParams& p, BLK& blk, int e, SsrCohBandsLds& S) {
  constexpr int NT = SSR_COH_NT, NW = NT / 64;
  const int NB = p.N / 2 + 1;
  const int K = ssr_coh_segments(p.tgt_len[p.tgt_index[e]], p.N, p.H);
  const int64_t c0 = p.chunk_off[e], c1 = p.chunk_off[e + 1];
  const double thr = p.thr;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    for (int k = tid; k < NB; k += NT) {
      double sxx = 0.0, syy = 0.0, cr = 0.0, ci = 0.0;
      for (int64_t c = c0; c < c1; ++c) {
        const double* q = p.part + (c * NB + k) * 4;
        sxx += q[0]; syy += q[1]; cr += q[2]; ci += q[3];
      }
      const double den = sxx * syy;
      double g2 = den == 0.0 ? 0.0 : (cr * cr + ci * ci) / den;
      if (g2 > 1.0) g2 = 1.0;
      S.g2[k] = g2;
      S.syy[k] = syy;
      if (p.msc_out) p.msc_out[(int64_t)e * NB + k] = K >= 2 ? g2 : (double)NAN;
    }
  });
  for (int b = 0; b < p.n_bands; ++b) {
    const int32_t* edge = p.bands + ((int64_t)e * p.n_bands + b) * 2;
    const int lo = edge[0], hi = edge[1];
    SSR_PHASE(blk, regs, {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      if (lo <= hi) {      // (the empty band's edges are any lo > hi: never added to)
        for (int k = lo + tid; k <= hi; k += NT) {
          const double g2 = S.g2[k], sy = S.syy[k];
          a0 += g2;
          a1 += g2 * sy;
          a2 += (1.0 - g2) * sy;
          a3 += g2 >= thr ? 1.0 : 0.0;
        }
      }
      SSR_WAVE_SUM_STORE(tid, NT, a0, S.ws[0]);
      SSR_WAVE_SUM_STORE(tid, NT, a1, S.ws[1]);
      SSR_WAVE_SUM_STORE(tid, NT, a2, S.ws[2]);
      SSR_WAVE_SUM_STORE(tid, NT, a3, S.ws[3]);
    });
    SSR_PHASE(blk, regs, {
      if (tid < 3) {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        for (int m = 0; m < 4; ++m)
          for (int q = 0; q < NW; ++q) a[m] += S.ws[m][q];
        double v = (double)NAN;
        if (K >= 2 && lo <= hi) {
          if (tid == 0) v = a[0] / (double)(hi - lo + 1);
          else if (tid == 1) v = 10.0 * log10((a[1] + SSR_COH_EPS) / (a[2] + SSR_COH_EPS));
          else v = a[3];
        }
        p.out[((int64_t)e * p.n_bands + b) * 3 + tid] = v;
      }
    });
  }
}
