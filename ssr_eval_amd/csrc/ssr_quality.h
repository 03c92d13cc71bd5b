// Kernel bodies of the objective quality measures of Loizou (Speech Enhancement: Theory and Practice, §11.1-11.2; Hu & Loizou
// 2008), restated in DESIGN §12: the log-likelihood ratio (LLR), the LPC cepstral distance, Klatt's weighted spectral slope (WSS)
// and the frequency-weighted segmental SNR (fwSNRseg), on float32 or float64 targets and estimates read in their own dtype.
// Every sample gets EPS added, frames are those of §10 (L = 30 ms, hop L / 4, Loizou's Hann window), all arithmetic is float64.
//
//   geometry   one workgroup (ssr_pairs.h): runs of consecutive pairs that name one target; frame prefix sums over runs and
//              over pairs; the window
//   lpc        one wave per (run, frame): the P + 1 lags of the target's frame by fixed-order wave reductions, Levinson-Durbin and
//              the cepstrum on one lane; then the same for each estimate of the run, and its LLR and cepstral distance
//   bands      one workgroup of N / 8 threads per (run, frame): the N-point transform of the real frame (ssr_fft.h in LDS), its
//              25 band powers and band magnitudes; the target's products (band energies, slopes, weights, normalised bands) once
//              per run, then each estimate's WSS and fwSNRseg frame values against them
//   finalize   one workgroup per pair: the mean of the 95 % smallest frame values (LLR, cepstral distance, WSS) by a radix
//              select on order-preserving keys, the plain mean (fwSNRseg)
//
// Every transform holds one frame of one signal, so a pair's values depend on the pair alone: the same bits alone, in any batch
// and through the multi path; y == x gives the target's bits for the estimate.  Every float sum has a fixed order; the
// only atomics are the integer histogram counts of the select.  All bodies compile on the host too (SSR_HOST_EMU,
// tests/emu/quality_emu.cpp).
#pragma once
#include "ssr_pairs.h"
#include "ssr_fft.h"
#include <vector>

#define SSR_QUAL_LLR 1
#define SSR_QUAL_CEP 2
#define SSR_QUAL_WSS 4
#define SSR_QUAL_FWSEG 8
#define SSR_QUAL_NT 256                    // threads of the geometry and finalize workgroups
static_assert(SSR_QUAL_NT == SSR_PAIRS_NT, "the geometry workgroup is ssr_run_geometry_body's");
#define SSR_QUAL_BANDS 25
#define SSR_QUAL_PMAX 32                   // largest LPC order
#define SSR_QUAL_FS_MIN 8000
#define SSR_QUAL_FS_MAX 48000
#define SSR_QUAL_LMAX 1440                 // frame length at SSR_QUAL_FS_MAX
#define SSR_QUAL_EPS 2.220446049250313e-16 // np.finfo(np.float64).eps
#define SSR_QUAL_LLR_CLIP 2.0
#define SSR_QUAL_CEP_CLIP 10.0
#define SSR_QUAL_FW_LO -10.0
#define SSR_QUAL_FW_HI 35.0

// frames of §10: L = 30 ms rounded half up, hop R = L // 4, M = max(0, (n - L) // R)
SSR_HD int ssr_qual_frame_len(int fs) { return (int)((3 * (int64_t)fs + 50) / 100); }
SSR_HD int ssr_qual_hop(int fs) { return ssr_qual_frame_len(fs) / 4; }
SSR_HD int64_t ssr_qual_frames(int64_t n, int fs) {
  const int L = ssr_qual_frame_len(fs), R = ssr_qual_hop(fs);
  return (R > 0 && n >= L) ? (n - L) / R : 0;
}
// transform size N = 2^ceil(log2(2 L)), as log2
SSR_HD int ssr_qual_log2_nfft(int fs) {
  const int L2 = 2 * ssr_qual_frame_len(fs);
  int g = 0;
  while ((1 << g) < L2) ++g;
  return g;
}
SSR_HD int ssr_qual_default_order(int fs) { return fs < 10000 ? 10 : 16; }
// frames averaged by the trimmed mean: MATLAB's round(0.95 M)
SSR_HD int64_t ssr_qual_trim_count(int64_t M) { return (int64_t)floor(0.95 * (double)M + 0.5); }

struct SsrQualParams {
  const void* tgt;              // targets (clean), float32 or float64
  const int64_t* tgt_off;       // [n_tgt] device
  const void* est;              // estimates, float32 or float64
  const int64_t* est_off;       // [n_est] device
  const int32_t* tgt_len;       // [n_tgt] (workspace copy)
  const int32_t* tgt_index;     // [n_est] (workspace copy)
  int n_tgt, n_est, n_runs;
  int which, fs, L, R, P, N;    // P: LPC order, N: transform size
  int32_t* run_start;           // [n_runs + 1] first pair of each run; [n_runs] = n_est
  int64_t* run_frame;           // [n_runs + 1] frame prefix over runs (the lpc and bands grids)
  int64_t* pair_frame;          // [n_est + 1] frame prefix over pairs (the frame values)
  double* win;                  // [L] 0.5 (1 - cos(2 pi (i + 1) / (L + 1)))
  const cx<double>* tw;         // [N] exp(-2 pi i k / N)
  const double* fw;             // band b's filter weights on bins [band_lo[b], band_hi[b]) at fw + band_off[b]
  int band_lo[SSR_QUAL_BANDS], band_hi[SSR_QUAL_BANDS], band_off[SSR_QUAL_BANDS];
  double* val;                  // [4][pair_frame[n_est]] frame values: LLR, cepstral distance, WSS, fwSNRseg
  int64_t n_val;                // pair_frame[n_est]
  double* out;                  // [n_est][popcount(which)]
};

// ---- geometry: ssr_run_geometry_body on the frames of each target
template <typename BLK> SSR_BODY void ssr_qual_geometry_body(const SsrQualParams& p, BLK& blk, int64_t* sums) {
  ssr_run_geometry_body(p.tgt_len, p.tgt_index, p.n_est, [&](int32_t n) { return ssr_qual_frames(n, p.fs); },
                        p.run_start, p.run_frame, p.pair_frame, p.win, p.L, blk, sums);
}

// ---- LPC analysis (one lane; a, alpha, tmp: P + 1 doubles each)
// Levinson-Durbin from the lags r[0..P]: a = [1, -alpha_1, .., -alpha_P].  Guard: the recursion stops at the first order whose
// prediction error E_{i-1} is not finite and positive; the coefficients above it stay zero.
SSR_HD void ssr_qual_levinson(const double* r, double* a, double* alpha, double* tmp, int P) {
  for (int m = 0; m <= P; ++m) alpha[m] = 0.0;
  double E = r[0];
  for (int i = 1; i <= P; ++i) {
    if (!(E > 0.0) || !isfinite(E)) break;
    double acc = r[i];
    for (int m = 1; m < i; ++m) acc -= alpha[m] * r[i - m];
    const double k = acc / E;
    for (int m = 1; m < i; ++m) tmp[m] = alpha[m] - k * alpha[i - m];
    for (int m = 1; m < i; ++m) alpha[m] = tmp[m];
    alpha[i] = k;
    E = (1.0 - k * k) * E;
  }
  a[0] = 1.0;
  for (int m = 1; m <= P; ++m) a[m] = -alpha[m];
}

// a^T T(r) a, T(r) the (P + 1) x (P + 1) Toeplitz matrix of the lags
SSR_HD double ssr_qual_toeplitz_form(const double* r, const double* a, int P) {
  double q = 0.0;
  for (int i = 0; i <= P; ++i) {
    double s = 0.0;
    for (int j = 0; j <= P; ++j) s += a[j] * r[i > j ? i - j : j - i];
    q += a[i] * s;
  }
  return q;
}

// LPC cepstrum c[1..P] of a[0..P]: c_1 = -a_1, c_k = -(a_k + (1 / k) Σ_{i<k} i c_i a_{k-i})
SSR_HD void ssr_qual_cepstrum(const double* a, double* c, int P) {
  c[0] = 0.0;
  for (int k = 1; k <= P; ++k) {
    double s = 0.0;
    for (int i = 1; i < k; ++i) s += (double)i * c[i] * a[k - i];
    c[k] = -(a[k] + s / (double)k);
  }
}

SSR_HD bool ssr_qual_pos_finite(double v) { return v > 0.0 && isfinite(v); }

// LLR of a frame: min(2, ln(a_y^T R_x a_y / a_x^T R_x a_x)); 2 where a form or the ratio is not finite and positive
SSR_HD double ssr_qual_llr_frame(const double* rx, const double* ax, const double* ay, int P) {
  const double num = ssr_qual_toeplitz_form(rx, ay, P), den = ssr_qual_toeplitz_form(rx, ax, P);
  if (!ssr_qual_pos_finite(num) || !ssr_qual_pos_finite(den)) return SSR_QUAL_LLR_CLIP;
  const double q = num / den;
  if (!ssr_qual_pos_finite(q)) return SSR_QUAL_LLR_CLIP;
  const double v = log(q);
  return v < SSR_QUAL_LLR_CLIP ? v : SSR_QUAL_LLR_CLIP;
}

// cepstral distance of a frame: min(10, (10 sqrt(2) / ln 10) ||c_x - c_y||)
SSR_HD double ssr_qual_cep_frame(const double* cx_, const double* cy_, int P) {
  double d = 0.0;
  for (int k = 1; k <= P; ++k) { const double u = cx_[k] - cy_[k]; d += u * u; }
  const double v = 10.0 * sqrt(2.0) / log(10.0) * sqrt(d);
  return v < SSR_QUAL_CEP_CLIP ? v : SSR_QUAL_CEP_CLIP;
}

// LDS of the lpc body (one wave)
struct SsrQualLpcLds {
  double f[SSR_QUAL_LMAX];                  // the windowed frame
  double rx[SSR_QUAL_PMAX + 1], ax[SSR_QUAL_PMAX + 1], cx[SSR_QUAL_PMAX + 1];   // the target's lags, coefficients, cepstrum
  double ry[SSR_QUAL_PMAX + 1], ay[SSR_QUAL_PMAX + 1], cy[SSR_QUAL_PMAX + 1];   // an estimate's
  double alpha[SSR_QUAL_PMAX + 1], tmp[SSR_QUAL_PMAX + 1];
};

// the P + 1 lags of frame s[0 .. L) (EPS added, windowed): lane l takes samples l, l + 64, ..; one wave sum per lag
template <typename T, typename BLK, typename REGS>
SSR_BODY void ssr_qual_lags(const SsrQualParams& p, BLK& blk, REGS& regs, const T* s, double* f, double* r) {
  SSR_WPHASE(blk, regs, {
    for (int i = tid; i < p.L; i += 64) f[i] = p.win[i] * ((double)s[i] + SSR_QUAL_EPS);
  });
  SSR_WPHASE(blk, regs, {
    for (int k = 0; k <= p.P; ++k) {
      double a = 0.0;
      for (int i = tid; i < p.L - k; i += 64) a += f[i] * f[i + k];
      SSR_WAVE_SUM_STORE(tid, 64, a, r + k);
    }
  });
}

// ---- lpc: grid block g = (run, frame j), one wave of 64 lanes
template <typename TT, typename TE, typename BLK>
SSR_BODY void ssr_qual_lpc_body(const SsrQualParams& p, BLK& blk, int64_t g, SsrQualLpcLds& S) {
  const int r = ssr_prefix_find(p.run_frame, p.n_runs, g);
  const int64_t j = g - p.run_frame[r];
  const int e0 = p.run_start[r], e1 = p.run_start[r + 1];
  const int P = p.P;
  const TT* x = (const TT*)p.tgt + p.tgt_off[p.tgt_index[e0]] + j * p.R;
  SSR_REGS(int, regs, blk);
  ssr_qual_lags<TT>(p, blk, regs, x, S.f, S.rx);
  SSR_WPHASE(blk, regs, {
    if (tid == 0) {
      ssr_qual_levinson(S.rx, S.ax, S.alpha, S.tmp, P);
      ssr_qual_cepstrum(S.ax, S.cx, P);
    }
  });
  for (int e = e0; e < e1; ++e) {
    const TE* y = (const TE*)p.est + p.est_off[e] + j * p.R;
    ssr_qual_lags<TE>(p, blk, regs, y, S.f, S.ry);
    SSR_WPHASE(blk, regs, {
      if (tid == 0) {
        ssr_qual_levinson(S.ry, S.ay, S.alpha, S.tmp, P);
        const int64_t o = p.pair_frame[e] + j;
        if (p.which & SSR_QUAL_LLR) p.val[o] = ssr_qual_llr_frame(S.rx, S.ax, S.ay, P);
        if (p.which & SSR_QUAL_CEP) {
          ssr_qual_cepstrum(S.ay, S.cy, P);
          p.val[p.n_val + o] = ssr_qual_cep_frame(S.cx, S.cy, P);
        }
      }
    });
  }
}

// ---- critical-band products of one frame (one lane; LDS rows)
// WSS: band energies E (dB) from the band powers, slopes S, weights W (Klatt: K_max = 20, K_locmax = 1).  The nearest peak walks
// uphill from band b: right while the slope is positive (p_b = E_n), else left while it is not (p_b = E_{n+1}); p_b >= E_b.
SSR_HD void ssr_qual_wss_products(const double* pw, double* E, double* S, double* W) {
  double emax = -1e300;
  for (int b = 0; b < SSR_QUAL_BANDS; ++b) {
    E[b] = 10.0 * log10(pw[b] > 1e-10 ? pw[b] : 1e-10);
    emax = E[b] > emax ? E[b] : emax;
  }
  for (int b = 0; b < SSR_QUAL_BANDS - 1; ++b) S[b] = E[b + 1] - E[b];
  for (int b = 0; b < SSR_QUAL_BANDS - 1; ++b) {
    double pk;
    if (S[b] > 0.0) {
      int n = b;
      while (n <= SSR_QUAL_BANDS - 2 && S[n] > 0.0) ++n;
      pk = E[n];
    } else {
      int n = b;
      while (n >= 0 && S[n] <= 0.0) --n;
      pk = E[n + 1];
    }
    W[b] = 20.0 / (20.0 + emax - E[b]) * (1.0 / (1.0 + pk - E[b]));
  }
}

// WSS frame value: Σ W̄ (S_x - S_y)² / Σ W̄, W̄ the mean of the two signals' weights
SSR_HD double ssr_qual_wss_frame(const double* Sx, const double* Wx, const double* Sy, const double* Wy) {
  double num = 0.0, den = 0.0;
  for (int b = 0; b < SSR_QUAL_BANDS - 1; ++b) {
    const double w = 0.5 * (Wx[b] + Wy[b]), d = Sx[b] - Sy[b];
    num += w * d * d;
    den += w;
  }
  return num / den;
}

// fwSNRseg frame value from the normalised band magnitudes; bands with B_x = 0 are skipped, none left: -10
SSR_HD double ssr_qual_fwseg_frame(const double* Bx, const double* By) {
  double num = 0.0, den = 0.0;
  for (int b = 0; b < SSR_QUAL_BANDS; ++b) {
    if (!(Bx[b] != 0.0)) continue;
    const double w = pow(Bx[b], 0.2), d = Bx[b] - By[b], dd = d * d;
    num += w * (10.0 * log10(Bx[b] * Bx[b] / (dd > SSR_QUAL_EPS ? dd : SSR_QUAL_EPS)));
    den += w;
  }
  double v = den > 0.0 ? num / den : SSR_QUAL_FW_LO;
  v = v < SSR_QUAL_FW_LO ? SSR_QUAL_FW_LO : (v > SSR_QUAL_FW_HI ? SSR_QUAL_FW_HI : v);
  return v;
}

// LDS of the bands body
template <int LOGN> struct SsrQualBandLds {
  double re[ssr_padded_len(1 << LOGN)], im[ssr_padded_len(1 << LOGN)];
  double bs[2][SSR_QUAL_BANDS];             // [power, magnitude][band] band sums
  double msum[8];                           // per wave: Σ |X_k| over the half spectrum
  double tot;
  double tE[SSR_QUAL_BANDS], tS[SSR_QUAL_BANDS], tW[SSR_QUAL_BANDS], tB[SSR_QUAL_BANDS];   // the target's products
  double eE[SSR_QUAL_BANDS], eS[SSR_QUAL_BANDS], eW[SSR_QUAL_BANDS], eB[SSR_QUAL_BANDS];   // an estimate's
};

struct SsrQualBandRegs {
  cx<double> v[8];
  double pw[4];                             // the power spectrum at bins tid + q NT
};

// band sums of the frame s[0 .. L) (EPS added, windowed): one N-point transform of the real frame.  (Two real frames packed into
// one complex transform would halve the work, but a frame of digital silence next to a loud one then loses its spectrum to the
// loud one's rounding: fwSNRseg reads the silent frame's upper bands at about 1e-8 of its total.)
template <typename T, int LOGN, typename BLK, typename REGS>
SSR_BODY void ssr_qual_band_sums(const SsrQualParams& p, BLK& blk, REGS& regs, SsrQualBandLds<LOGN>& S, const T* s, bool pw, bool mag) {
  using PL = SsrFftPlan<LOGN>;
  constexpr int NT = PL::NT, NW = (NT + 63) / 64;
  const double* w = p.win;
  const cx<double>* tw = p.tw;
  const int L = p.L;
  ssr_launder(blk);     // (per-pass LDS addresses are recomputed where used, not hoisted across the estimate loop)
  SSR_PHASE(blk, regs, {
    SSR_UNROLL for (int r = 0; r < 8; ++r) {
      const int m = ssr_fft_first_index<LOGN>(tid, r);
      R.v[r] = {m < L ? w[m] * ((double)s[m] + SSR_QUAL_EPS) : 0.0, 0.0};
    }
    ssr_fft_compute<double, LOGN, 0>(tid, R.v, tw);
    ssr_fft_store<double, LOGN, 0>(tid, S.re, S.im, R.v);
  });
  ssr_fft_finish_natural<LOGN>(blk, regs, S.re, S.im, tw);
  SSR_PHASE(blk, regs, {
    double ma = 0.0;
    SSR_UNROLL for (int q = 0; q < 4; ++q) {
      const int k = tid + q * NT;
      const double zr = S.re[ssr_pad(k)], zi = S.im[ssr_pad(k)];
      R.pw[q] = zr * zr + zi * zi;
      ma += sqrt(R.pw[q]);
    }
    SSR_WAVE_SUM_STORE(tid, NT, ma, S.msum);
  });
  SSR_PHASE(blk, regs, {
    SSR_UNROLL for (int q = 0; q < 4; ++q) S.re[tid + q * NT] = R.pw[q];   // (unpadded: bins 0 .. N/2 - 1)
  });
  SSR_PHASE(blk, regs, {
    for (int t = tid; t < 2 * SSR_QUAL_BANDS; t += NT) {
      const int kind = t / SSR_QUAL_BANDS, b = t % SSR_QUAL_BANDS;
      if ((kind == 0 && !pw) || (kind == 1 && !mag)) continue;
      const double* fw = p.fw + p.band_off[b] - p.band_lo[b];
      double a = 0.0;
      for (int k = p.band_lo[b]; k < p.band_hi[b]; ++k) a += (kind ? sqrt(S.re[k]) : S.re[k]) * fw[k];
      S.bs[kind][b] = a;
    }
    if (tid == 0) {
      double a = 0.0;
      for (int q = 0; q < NW; ++q) a += S.msum[q];
      S.tot = a;
    }
  });
}

// ---- bands: grid block g = (run, frame j), N / 8 threads
template <typename TT, typename TE, int LOGN, typename BLK>
SSR_BODY void ssr_qual_bands_body(const SsrQualParams& p, BLK& blk, int64_t g, SsrQualBandLds<LOGN>& S) {
  const int r = ssr_prefix_find(p.run_frame, p.n_runs, g);
  const int64_t j = g - p.run_frame[r];
  const int e0 = p.run_start[r], e1 = p.run_start[r + 1];
  const bool wss = (p.which & SSR_QUAL_WSS) != 0, fws = (p.which & SSR_QUAL_FWSEG) != 0;
  const TT* x = (const TT*)p.tgt + p.tgt_off[p.tgt_index[e0]] + j * p.R;
  SSR_REGS(SsrQualBandRegs, regs, blk);
  ssr_qual_band_sums<TT, LOGN>(p, blk, regs, S, x, wss, fws);
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      if (wss) ssr_qual_wss_products(S.bs[0], S.tE, S.tS, S.tW);
      if (fws)
        for (int b = 0; b < SSR_QUAL_BANDS; ++b) S.tB[b] = S.bs[1][b] / S.tot;
    }
  });
  for (int e = e0; e < e1; ++e) {
    const TE* y = (const TE*)p.est + p.est_off[e] + j * p.R;
    ssr_qual_band_sums<TE, LOGN>(p, blk, regs, S, y, wss, fws);
    SSR_PHASE(blk, regs, {
      if (tid == 0) {
        const int64_t o = p.pair_frame[e] + j;
        if (wss) {
          ssr_qual_wss_products(S.bs[0], S.eE, S.eS, S.eW);
          p.val[2 * p.n_val + o] = ssr_qual_wss_frame(S.tS, S.tW, S.eS, S.eW);
        }
        if (fws) {
          for (int b = 0; b < SSR_QUAL_BANDS; ++b) S.eB[b] = S.bs[1][b] / S.tot;
          p.val[3 * p.n_val + o] = ssr_qual_fwseg_frame(S.tB, S.eB);
        }
      }
    });
  }
}

// ---- finalize: pair e, one workgroup of SSR_QUAL_NT threads
// order-preserving key of a double (non-NaN): a < b  <=>  key(a) < key(b)
SSR_HD uint64_t ssr_qual_key(double v) {
  uint64_t u;
  memcpy(&u, &v, 8);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
SSR_HD double ssr_qual_unkey(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  memcpy(&v, &u, 8);
  return v;
}
#ifdef SSR_HOST_EMU
#define SSR_QUAL_COUNT(p) (++*(p))
#else
#define SSR_QUAL_COUNT(p) atomicAdd((p), 1)
#endif

struct SsrQualFinLds {
  int hist[256];
  double ps[SSR_QUAL_NT];
  int64_t pc[SSR_QUAL_NT];
  uint64_t st[3];                           // key prefix, key mask, rank left
};

// mean of the K = round(0.95 M) smallest values (metric slot m < 3) or of all M (m = 3).  The K-th smallest value v is selected
// radix by radix (8 bits, most significant first, integer counts); then the values < v are added in frame order and
// (K - count) v on top: the sorted-prefix sum without a sort.
template <typename BLK> SSR_BODY void ssr_qual_finalize_body(const SsrQualParams& p, BLK& blk, int e, SsrQualFinLds& S) {
  const int NT = SSR_QUAL_NT;
  const int64_t M = ssr_qual_frames(p.tgt_len[p.tgt_index[e]], p.fs);
  const int n_out = ssr_which_count(p.which);
  const int64_t c = (M + NT - 1) / NT;
  SSR_REGS(int, regs, blk);
  for (int m = 0; m < 4; ++m) {
    if (!(p.which & (1 << m))) continue;
    double* o = p.out + (int64_t)e * n_out + ssr_which_col(p.which, 1 << m);
    if (M == 0) {
      SSR_PHASE(blk, regs, { if (tid == 0) *o = (double)NAN; });
      continue;
    }
    const double* v = p.val + m * p.n_val + p.pair_frame[e];
    if (m == 3) {
      SSR_PHASE(blk, regs, {
        double a = 0.0;
        for (int64_t i = tid * c; i < M && i < (tid + 1) * c; ++i) a += v[i];
        S.ps[tid] = a;
      });
      SSR_PHASE(blk, regs, {
        if (tid == 0) {
          double a = 0.0;
          for (int t = 0; t < NT; ++t) a += S.ps[t];
          *o = a / (double)M;
        }
      });
      continue;
    }
    const int64_t K = ssr_qual_trim_count(M);
    SSR_PHASE(blk, regs, { if (tid == 0) { S.st[0] = 0; S.st[1] = 0; S.st[2] = (uint64_t)K; } });
    for (int d = 7; d >= 0; --d) {
      SSR_PHASE(blk, regs, { S.hist[tid] = 0; });
      SSR_PHASE(blk, regs, {
        const uint64_t pre = S.st[0], msk = S.st[1];
        for (int64_t i = tid * c; i < M && i < (tid + 1) * c; ++i) {
          const uint64_t k = ssr_qual_key(v[i]);
          if ((k & msk) == pre) SSR_QUAL_COUNT(&S.hist[(int)((k >> (8 * d)) & 255u)]);
        }
      });
      SSR_PHASE(blk, regs, {
        if (tid == 0) {
          const uint64_t left = S.st[2];
          uint64_t cum = 0;
          for (int b = 0; b < 256; ++b) {
            const uint64_t h = (uint64_t)S.hist[b];
            if (cum + h >= left) {
              S.st[0] |= (uint64_t)b << (8 * d);
              S.st[1] |= (uint64_t)255 << (8 * d);
              S.st[2] = left - cum;
              break;
            }
            cum += h;
          }
        }
      });
    }
    SSR_PHASE(blk, regs, {
      const uint64_t kk = S.st[0];
      double a = 0.0;
      int64_t n = 0;
      for (int64_t i = tid * c; i < M && i < (tid + 1) * c; ++i)
        if (ssr_qual_key(v[i]) < kk) { a += v[i]; ++n; }
      S.ps[tid] = a;
      S.pc[tid] = n;
    });
    SSR_PHASE(blk, regs, {
      if (tid == 0) {
        double a = 0.0;
        int64_t n = 0;
        for (int t = 0; t < NT; ++t) { a += S.ps[t]; n += S.pc[t]; }
        const double vk = ssr_qual_unkey(S.st[0]);
        *o = (a + (double)(K - n) * vk) / (double)K;
      }
    });
  }
}

// ---- host tables: Loizou's 25 critical bands (comp_wss.m / comp_fwseg.m), their Gaussian-shaped filters on bins 0 .. N/2 - 1
// (float64), the transform's twiddles (long double, rounded once)
static const double SSR_QUAL_CENT[SSR_QUAL_BANDS] = {
    50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72,
    1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63};
static const double SSR_QUAL_BW[SSR_QUAL_BANDS] = {
    70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154,
    183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136};

struct SsrQualTables {
  int N = 0;
  int lo[SSR_QUAL_BANDS], hi[SSR_QUAL_BANDS], off[SSR_QUAL_BANDS];
  std::vector<double> dense;                // [25][N / 2]
  std::vector<double> packed;               // the non-zero range of each filter, band after band
  std::vector<cx<double>> tw;               // [N]
};

static inline void ssr_qual_tables_host(int fs, SsrQualTables& t) {
  t.N = 1 << ssr_qual_log2_nfft(fs);
  const int N2 = t.N / 2;
  const double half = (double)fs / 2.0, thr = exp(-30.0 / (2.0 * 2.303));
  t.dense.assign((size_t)SSR_QUAL_BANDS * N2, 0.0);
  t.packed.clear();
  for (int b = 0; b < SSR_QUAL_BANDS; ++b) {
    const double f0 = SSR_QUAL_CENT[b] / half * (double)N2, bwb = SSR_QUAL_BW[b] / half * (double)N2;
    int lo = -1, hi = -1;
    for (int j = 0; j < N2; ++j) {
      const double u = ((double)j - floor(f0)) / bwb;
      const double w = exp(-11.0 * (u * u) + log(SSR_QUAL_BW[0]) - log(SSR_QUAL_BW[b]));
      if (w > thr) {
        t.dense[(size_t)b * N2 + j] = w;
        if (lo < 0) lo = j;
        hi = j + 1;
      }
    }
    if (lo < 0) lo = hi = 0;
    t.lo[b] = lo; t.hi[b] = hi; t.off[b] = (int)t.packed.size();
    for (int j = lo; j < hi; ++j) t.packed.push_back(t.dense[(size_t)b * N2 + j]);
  }
  ssr_phase_twiddles_host(t.N, t.tw);
}
