// Kernel bodies of STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) on 10 kHz float64 signals, as pystoi 0.3.x computes
// them (restated in DESIGN §9; no pinned copy of pystoi was available).  The resampling to 10 kHz runs before these bodies, in
// ssr_resample_poly_f64 with the Octave-compatible taps (backend.StoiResamplePlan).
//
//   geometry   one workgroup: frame / segment-tile prefix sums of the ragged batch, the analysis window
//   energy     one thread per target frame: 20 log10(|w x_frame| + EPS)
//   vad        one workgroup per target: max energy, mask (max - 40 - e < 0), ordered compaction into a kept-frame list
//   bands      one workgroup per (signal, output frame): the frame of the silence-removed signal straight from three kept frames
//              (the overlap-added signal is never stored), window, 512-point FFT in LDS, 15 one-third-octave band magnitudes
//   segments   one wave per (pair, 64 segments): band rows + 29-frame halo in LDS, one segment per lane; STOI (scale, clip,
//              correlate per band) and / or ESTOI (row then column normalisation); a fixed-order partial per tile
//   finalize   one thread per pair: the tile partials in ascending order, / (J * 15) or / (J * 30); 1e-5 below 30 frames
//
// Every sum has a fixed order (no atomics): results are identical from run to run and independent of the batch they are in.
// All bodies compile on the host too (SSR_HOST_EMU, tests/emu/stoi_emu.cpp).
#pragma once
#include "ssr_pairs.h"

#define SSR_STOI_FRAME 256           // N_FRAME
#define SSR_STOI_HOP 128
#define SSR_STOI_NFFT 512
#define SSR_STOI_BANDS 15            // NUMBAND
#define SSR_STOI_N 30                // frames per segment
#define SSR_STOI_DYN_RANGE 40.0
#define SSR_STOI_CLIP 5.623413251903491   // 10^(-BETA / 20), BETA = -15
#define SSR_STOI_EPS 2.220446049250313e-16 // np.finfo(float).eps
#define SSR_STOI_SHORT 1e-5          // pystoi's value when fewer than N frames remain
#define SSR_STOI_NT 256              // threads of the geometry / vad / bands workgroups
#define SSR_STOI_SEG 64              // segments per wave of the segment kernel
#define SSR_STOI_SEG_ROWS (SSR_STOI_SEG + SSR_STOI_N - 1)

// frames of a signal of `len` samples: range(0, len - 256, 128)
SSR_HD int ssr_stoi_frames(int64_t len) { return len > SSR_STOI_FRAME ? (int)((len - SSR_STOI_FRAME + SSR_STOI_HOP - 1) / SSR_STOI_HOP) : 0; }
// segment tiles of a pair whose target has `frames` frames: at most frames - 1 - (N - 1) segments (all frames kept)
SSR_HD int ssr_stoi_seg_tiles(int frames) {
  const int j = frames - SSR_STOI_N;
  return j > 0 ? (j + SSR_STOI_SEG - 1) / SSR_STOI_SEG : 0;
}

struct SsrStoiParams {
  const double* tgt;            // 10 kHz targets (clean), float64
  const int64_t* tgt_off;       // [n_tgt]
  const double* est;            // 10 kHz estimates (processed), float64
  const int64_t* est_off;       // [n_est]
  const int32_t* len;           // [n_tgt + n_est]: the targets' lengths, then the estimates'
  const int32_t* tgt_index;     // [n_est]
  int n_tgt, n_est;
  int which;                    // bit 0: STOI, bit 1: ESTOI
  int64_t* fr_off;              // [n_tgt + n_est + 1] frame prefix: targets, then estimates
  int64_t* st_off;              // [n_est + 1] segment-tile prefix
  double* win;                  // [256] np.hanning(258)[1:-1]
  double* energy;               // [fr_off[n_tgt]] target frame energies (dB)
  int32_t* kept;                // [fr_off[n_tgt]] kept frame indices of each target, ascending
  int32_t* n_kept;              // [n_tgt]
  double* tob;                  // [fr_off[n_tgt + n_est]][15] band magnitudes of kept-frame STFT frames
  double* part;                 // [st_off[n_est]][2] per-tile sums (STOI, ESTOI)
  int band_lo[SSR_STOI_BANDS], band_hi[SSR_STOI_BANDS];   // bins [lo, hi) of each band (pystoi.utils.thirdoct)
  double* out;                  // [n_est][n_out], n_out = popcount(which): STOI first
};

// pystoi.utils.thirdoct(10000, 512, 15, 150): band k spans [150 2^((2k-1)/6), 150 2^((2k+1)/6)) Hz, each edge snapped to the
// nearest bin of linspace(0, 10000, 513)[:257] (the first one on a tie, np.argmin)
static inline void ssr_stoi_band_edges_host(int* lo, int* hi) {
  const double step = 10000.0 / SSR_STOI_NFFT;
  auto nearest = [&](double f) {
    int best = 0;
    double bd = 1e300;
    for (int b = 0; b <= SSR_STOI_NFFT / 2; ++b) {
      const double d = (b * step - f) * (b * step - f);
      if (d < bd) { bd = d; best = b; }
    }
    return best;
  };
  for (int k = 0; k < SSR_STOI_BANDS; ++k) {
    lo[k] = nearest(150.0 * pow(2.0, (2.0 * k - 1.0) / 6.0));
    hi[k] = nearest(150.0 * pow(2.0, (2.0 * k + 1.0) / 6.0));
  }
}

SSR_HD int ssr_stoi_target_of(const SsrStoiParams& p, int s) { return s < p.n_tgt ? s : p.tgt_index[s - p.n_tgt]; }

// ---- geometry: one workgroup of SSR_STOI_NT threads.  LDS: 2 * NT int64.
template <typename BLK> SSR_BODY void ssr_stoi_geometry_body(const SsrStoiParams& p, BLK& blk, int64_t* sums) {
  const int S = p.n_tgt + p.n_est, NT = SSR_STOI_NT;
  const int cf = (S + NT - 1) / NT, cs = (p.n_est + NT - 1) / NT;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    int64_t a = 0, b = 0;
    for (int s = tid * cf; s < S && s < (tid + 1) * cf; ++s) a += ssr_stoi_frames(p.len[s]);
    for (int e = tid * cs; e < p.n_est && e < (tid + 1) * cs; ++e) b += ssr_stoi_seg_tiles(ssr_stoi_frames(p.len[p.n_tgt + e]));
    sums[tid] = a;
    sums[NT + tid] = b;
    // the window: np.hanning(258)[1:-1] = 0.5 + 0.5 cos(pi (2k - 257) / 257), k = 1 .. 256
    p.win[tid] = 0.5 + 0.5 * cos(M_PI * (double)(2 * (tid + 1) - 257) / 257.0);
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      int64_t a = 0, b = 0;
      for (int t = 0; t < NT; ++t) {
        const int64_t va = sums[t], vb = sums[NT + t];
        sums[t] = a; sums[NT + t] = b;
        a += va; b += vb;
      }
    }
  });
  SSR_PHASE(blk, regs, {
    int64_t a = sums[tid], b = sums[NT + tid];
    for (int s = tid * cf; s < S && s < (tid + 1) * cf; ++s) { p.fr_off[s] = a; a += ssr_stoi_frames(p.len[s]); }
    for (int e = tid * cs; e < p.n_est && e < (tid + 1) * cs; ++e) {
      p.st_off[e] = b;
      b += ssr_stoi_seg_tiles(ssr_stoi_frames(p.len[p.n_tgt + e]));
    }
    if (tid == NT - 1) { p.fr_off[S] = a; p.st_off[p.n_est] = b; }
  });
}

// ---- energy of target frame g (g < fr_off[n_tgt])
SSR_HD void ssr_stoi_energy(const SsrStoiParams& p, int64_t g) {
  const int t = ssr_prefix_find(p.fr_off, p.n_tgt, g);
  const int64_t i = g - p.fr_off[t];
  const double* x = p.tgt + p.tgt_off[t] + i * SSR_STOI_HOP;
  double s = 0.0;
  for (int m = 0; m < SSR_STOI_FRAME; ++m) {
    const double v = p.win[m] * x[m];
    s += v * v;
  }
  p.energy[g] = 20.0 * log10(sqrt(s) + SSR_STOI_EPS);
}

// ---- voice-activity mask and compaction of target t: one workgroup of SSR_STOI_NT threads.  LDS: NT doubles + NT ints.
template <typename BLK> SSR_BODY void ssr_stoi_vad_body(const SsrStoiParams& p, BLK& blk, int t, double* red, int* cnt) {
  const int NT = SSR_STOI_NT;
  const int64_t base = p.fr_off[t];
  const int F = (int)(p.fr_off[t + 1] - base), c = (F + NT - 1) / NT;
  const double* e = p.energy + base;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    double m = -1e300;
    for (int i = tid * c; i < F && i < (tid + 1) * c; ++i) m = e[i] > m ? e[i] : m;
    red[tid] = m;
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      double m = -1e300;
      for (int k = 0; k < NT; ++k) m = red[k] > m ? red[k] : m;
      red[0] = m;
    }
  });
  SSR_PHASE(blk, regs, {
    const double thr = red[0] - SSR_STOI_DYN_RANGE;
    int n = 0;
    for (int i = tid * c; i < F && i < (tid + 1) * c; ++i) n += (thr - e[i] < 0.0) ? 1 : 0;
    cnt[tid] = n;
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      int a = 0;
      for (int k = 0; k < NT; ++k) { const int v = cnt[k]; cnt[k] = a; a += v; }
      p.n_kept[t] = a;
    }
  });
  SSR_PHASE(blk, regs, {
    const double thr = red[0] - SSR_STOI_DYN_RANGE;
    int o = cnt[tid];
    for (int i = tid * c; i < F && i < (tid + 1) * c; ++i)
      if (thr - e[i] < 0.0) p.kept[base + o++] = i;
  });
}

SSR_HD unsigned ssr_stoi_bitrev9(unsigned n) {
  unsigned r = 0;
  for (int b = 0; b < 9; ++b) r |= ((n >> b) & 1u) << (8 - b);
  return r;
}

// ---- band magnitudes of STFT frame t of the silence-removed signal s (s < n_tgt: target s, else estimate s - n_tgt).
// One workgroup of SSR_STOI_NT threads; LDS: re[512], im[512], twr[256], twi[256], pw[257] doubles.
// With hop = frame / 2 the overlap-added signal's frame t is [f_t[0:128] + f_{t-1}[128:256], f_{t+1}[0:128] + f_t[128:256]],
// f_j = w * (kept frame j), f_{-1} = 0; t < K - 1 (K kept frames) so f_{t+1} exists.
template <typename BLK> SSR_BODY void ssr_stoi_bands_body(const SsrStoiParams& p, BLK& blk, int64_t g, double* re, double* im,
                                                         double* twr, double* twi, double* pw) {
  const int S = p.n_tgt + p.n_est;
  const int s = ssr_prefix_find(p.fr_off, S, g);
  const int t = (int)(g - p.fr_off[s]);
  const int tt = ssr_stoi_target_of(p, s);
  if (t >= p.n_kept[tt] - 1) return;                    // (uniform over the workgroup)
  const double* x = s < p.n_tgt ? p.tgt + p.tgt_off[s] : p.est + p.est_off[s - p.n_tgt];
  const int32_t* kept = p.kept + p.fr_off[tt];
  const double* w = p.win;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    const int n = tid, m = n & (SSR_STOI_HOP - 1), b = t + (n >> 7);
    double v = w[m] * x[(int64_t)kept[b] * SSR_STOI_HOP + m];
    if (b > 0) v += w[m + SSR_STOI_HOP] * x[(int64_t)kept[b - 1] * SSR_STOI_HOP + m + SSR_STOI_HOP];
    const unsigned r0 = ssr_stoi_bitrev9((unsigned)n), r1 = ssr_stoi_bitrev9((unsigned)n + 256u);
    re[r0] = w[n] * v; im[r0] = 0.0;
    re[r1] = 0.0; im[r1] = 0.0;                         // rfft(n = 512) zero-pads the 256 samples
    twr[tid] = cos(M_PI * (double)tid / 256.0);         // exp(-2 pi i k / 512)
    twi[tid] = -sin(M_PI * (double)tid / 256.0);
  });
  // radix-2 decimation in time, in place: pass h pairs (i, i + h), one butterfly per thread
  for (int h = 1; h < SSR_STOI_NFFT; h <<= 1) {
    SSR_PHASE(blk, regs, {
      const int pos = tid & (h - 1), i0 = ((tid - pos) << 1) + pos, i1 = i0 + h;
      const int k = pos * (256 / h);
      const double wr = twr[k], wi = twi[k];
      const double br = re[i1] * wr - im[i1] * wi, bi = re[i1] * wi + im[i1] * wr;
      const double ar = re[i0], ai = im[i0];
      re[i0] = ar + br; im[i0] = ai + bi;
      re[i1] = ar - br; im[i1] = ai - bi;
    });
  }
  SSR_PHASE(blk, regs, {
    pw[tid] = re[tid] * re[tid] + im[tid] * im[tid];
    if (tid == 0) pw[256] = re[256] * re[256] + im[256] * im[256];
  });
  SSR_PHASE(blk, regs, {
    if (tid < SSR_STOI_BANDS) {
      double a = 0.0;
      for (int k = p.band_lo[tid]; k < p.band_hi[tid]; ++k) a += pw[k];
      p.tob[(p.fr_off[s] + t) * SSR_STOI_BANDS + tid] = sqrt(a);
    }
  });
}

// ---- per-segment scores.  X / Y: band magnitudes [frame][15] of the segment's 30 frames.
// STOI: sum over bands of the correlation of the row of X with the scaled, clipped row of Y.
SSR_HD double ssr_stoi_segment(const double* X, const double* Y) {
  double acc = 0.0;
  for (int j = 0; j < SSR_STOI_BANDS; ++j) {
    double nx = 0.0, ny = 0.0;
    for (int n = 0; n < SSR_STOI_N; ++n) {
      const double a = X[n * SSR_STOI_BANDS + j], b = Y[n * SSR_STOI_BANDS + j];
      nx += a * a; ny += b * b;
    }
    const double alpha = sqrt(nx) / (sqrt(ny) + SSR_STOI_EPS);
    double mx = 0.0, my = 0.0;
    for (int n = 0; n < SSR_STOI_N; ++n) {
      const double a = X[n * SSR_STOI_BANDS + j], b = alpha * Y[n * SSR_STOI_BANDS + j], c = a * (1.0 + SSR_STOI_CLIP);
      mx += a; my += b < c ? b : c;
    }
    mx /= SSR_STOI_N; my /= SSR_STOI_N;
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int n = 0; n < SSR_STOI_N; ++n) {
      const double a = X[n * SSR_STOI_BANDS + j], b = alpha * Y[n * SSR_STOI_BANDS + j], c = a * (1.0 + SSR_STOI_CLIP);
      const double u = a - mx, v = (b < c ? b : c) - my;
      sxx += u * u; syy += v * v; sxy += u * v;
    }
    acc += sxy / ((sqrt(sxx) + SSR_STOI_EPS) * (sqrt(syy) + SSR_STOI_EPS));
  }
  return acc;
}

// ESTOI: rows (bands) normalised over the 30 frames, then columns (frames) over the 15 bands; the sum of the products.
// rs: 4 * 15 doubles of row statistics at stride `rstride` (LDS, one lane's column).
SSR_HD double ssr_estoi_segment(const double* X, const double* Y, double* rs, int rstride) {
  for (int j = 0; j < SSR_STOI_BANDS; ++j) {
    double mx = 0.0, my = 0.0;
    for (int n = 0; n < SSR_STOI_N; ++n) { mx += X[n * SSR_STOI_BANDS + j]; my += Y[n * SSR_STOI_BANDS + j]; }
    mx /= SSR_STOI_N; my /= SSR_STOI_N;
    double sx = 0.0, sy = 0.0;
    for (int n = 0; n < SSR_STOI_N; ++n) {
      const double u = X[n * SSR_STOI_BANDS + j] - mx, v = Y[n * SSR_STOI_BANDS + j] - my;
      sx += u * u; sy += v * v;
    }
    rs[(4 * j + 0) * rstride] = mx;
    rs[(4 * j + 1) * rstride] = 1.0 / (sqrt(sx) + SSR_STOI_EPS);
    rs[(4 * j + 2) * rstride] = my;
    rs[(4 * j + 3) * rstride] = 1.0 / (sqrt(sy) + SSR_STOI_EPS);
  }
  double acc = 0.0;
  for (int n = 0; n < SSR_STOI_N; ++n) {
    double cx = 0.0, cy = 0.0;
    for (int j = 0; j < SSR_STOI_BANDS; ++j) {
      cx += (X[n * SSR_STOI_BANDS + j] - rs[(4 * j + 0) * rstride]) * rs[(4 * j + 1) * rstride];
      cy += (Y[n * SSR_STOI_BANDS + j] - rs[(4 * j + 2) * rstride]) * rs[(4 * j + 3) * rstride];
    }
    cx /= SSR_STOI_BANDS; cy /= SSR_STOI_BANDS;
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int j = 0; j < SSR_STOI_BANDS; ++j) {
      const double u = (X[n * SSR_STOI_BANDS + j] - rs[(4 * j + 0) * rstride]) * rs[(4 * j + 1) * rstride] - cx;
      const double v = (Y[n * SSR_STOI_BANDS + j] - rs[(4 * j + 2) * rstride]) * rs[(4 * j + 3) * rstride] - cy;
      sxx += u * u; syy += v * v; sxy += u * v;
    }
    acc += sxy / ((sqrt(sxx) + SSR_STOI_EPS) * (sqrt(syy) + SSR_STOI_EPS));
  }
  return acc;
}

// ---- segment tile g (g < st_off[n_est]): one wave of SSR_STOI_SEG lanes.
// LDS: X, Y [SEG_ROWS][15], rs [60][SEG], red [2][SEG] doubles.
template <typename BLK> SSR_BODY void ssr_stoi_segments_body(const SsrStoiParams& p, BLK& blk, int64_t g, double* X, double* Y,
                                                            double* rs, double* red) {
  const int e = ssr_prefix_find(p.st_off, p.n_est, g);
  const int k = (int)(g - p.st_off[e]);
  const int tt = p.tgt_index[e];
  const int T = p.n_kept[tt] - 1, J = T - (SSR_STOI_N - 1);
  const int f0 = k * SSR_STOI_SEG;
  int nf = T - f0;
  nf = nf < 0 ? 0 : (nf > SSR_STOI_SEG_ROWS ? SSR_STOI_SEG_ROWS : nf);
  const double* xs = p.tob + (p.fr_off[tt] + f0) * SSR_STOI_BANDS;
  const double* ys = p.tob + (p.fr_off[p.n_tgt + e] + f0) * SSR_STOI_BANDS;
  SSR_REGS(int, regs, blk);
  SSR_WPHASE(blk, regs, {
    for (int i = tid; i < nf * SSR_STOI_BANDS; i += SSR_STOI_SEG) { X[i] = xs[i]; Y[i] = ys[i]; }
  });
  SSR_WPHASE(blk, regs, {
    const int j = f0 + tid;
    const bool live = j < J;
    red[tid] = (live && (p.which & 1)) ? ssr_stoi_segment(X + tid * SSR_STOI_BANDS, Y + tid * SSR_STOI_BANDS) : 0.0;
    red[SSR_STOI_SEG + tid] = (live && (p.which & 2))
                                  ? ssr_estoi_segment(X + tid * SSR_STOI_BANDS, Y + tid * SSR_STOI_BANDS, rs + tid, SSR_STOI_SEG) : 0.0;
  });
  SSR_WPHASE(blk, regs, {
    if (tid < 2) {
      double a = 0.0;
      for (int l = 0; l < SSR_STOI_SEG; ++l) a += red[tid * SSR_STOI_SEG + l];
      p.part[g * 2 + tid] = a;
    }
  });
}

// ---- pair e: the tile sums in ascending order
SSR_HD void ssr_stoi_finalize(const SsrStoiParams& p, int e) {
  const int T = p.n_kept[p.tgt_index[e]] - 1, J = T - (SSR_STOI_N - 1);
  const int n_out = ((p.which & 1) ? 1 : 0) + ((p.which & 2) ? 1 : 0);
  int o = 0;
  for (int m = 0; m < 2; ++m) {
    if (!(p.which & (1 << m))) continue;
    double v = SSR_STOI_SHORT;
    if (T >= SSR_STOI_N) {
      double a = 0.0;
      for (int64_t g = p.st_off[e]; g < p.st_off[e + 1]; ++g) a += p.part[g * 2 + m];
      v = a / ((double)J * (m == 0 ? SSR_STOI_BANDS : SSR_STOI_N));
    }
    p.out[(int64_t)e * n_out + o++] = v;
  }
}
