// Kernel bodies of the spectrum family (bandwidth, spectral edge, centroid, HF level and LTAS distance of a signal from its long-term
// average spectrum; the rolloff is the reference's BasicTestee._find_cutoff made a metric), restated in DESIGN §22.  Signals are the
// n_tgt targets followed by the n_est estimates, float32 or float64 read in their own dtype; all arithmetic is float64.
//
//   framing    N = n_fft in {256 .. 2048}, hop H in [1, N], periodic Hann window w[i] = 0.5 - 0.5 cos(2 pi i / N); no padding, no
//              centring, no detrending (ssr_coherence.h's framing): K = 1 + (n - N) / H segments for n >= N, else 0
//   spectra    P[k] = sum_t |X_t[k]|^2, A[k] = sum_t |X_t[k]|, 0 <= k <= N / 2, in segment order; c[k] = 1 at k = 0 and N / 2, else 2
//   band       bins lo .. hi (lo > hi: the empty band); E_tot = sum c P over it
//   rolloff    the smallest r in the band with sum_{lo..r} A >= rho sum_{lo..hi} A
//   edge       the highest e in the band with P[e] >= max_band(P) thr_lin   (thr_lin = 10^(-drop_db / 10), from the host)
//   centroid   sum k c P / sum c P over the band, in bins
//   levels     L_b = 10 log10(max(E_b / E_tot, EPS)), E_b = sum c P over analysis band b (disjoint ascending inclusive bin ranges)
//   per pair   hf_db = 10 log10(max(E_hi / E_tot, EPS)) of both signals, E_hi = sum c P over bins max(split, lo) .. hi (split < 0 or
//              no such bin: NaN); the differences estimate - target; ltas_dist = sqrt(mean_b d_b^2), ltas_max = max_b |d_b|,
//              d_b = L_b(y) - L_b(x)
//   NaN        K == 0, the empty band or E_tot == 0 (digital silence): every value of the signal and of every pair that uses it
//
//   geometry   one workgroup: the signal -> target-length map, then ssr_run_geometry_body on chunks of SSR_SPEC_FR segments per signal
//   ltas       one workgroup of N / 8 threads per (signal, chunk): ONE complex N-point transform (ssr_fft.h in LDS, the phase family's)
//              carries TWO consecutive segments of the same signal - segment 2 j in the real parts, 2 j + 1 in the imaginary parts;
//              their spectra are split from Z[k] and conj(Z[N - k]) as ssr_coh_spectra_body splits target and estimate, with its
//              live rule (a digitally silent half is exactly zero and the other is taken from Z alone); an odd last segment is a
//              transform with an empty imaginary half.  A thread keeps P and A of bins 4 tid .. 4 tid + 3 (bin N / 2: the last
//              thread) in registers across the chunk, in segment order.  One partial row [bin][2] per chunk
//   signal     one workgroup of SSR_SPEC_NT threads per signal: the chunk rows in chunk order into LDS; max P, E_tot, sum A and
//              sum k c P with every thread on a contiguous run of the band's bins, a wave reduction, the waves in order; the rolloff
//              from the same runs - a scan of the lane sums in lane order, the waves in order, then each thread walks its run; the
//              edge; one thread per analysis band for its level
//   pair       one workgroup of SSR_SPEC_NT threads per estimate: E_hi of both signals from their stored c P rows, the sums starting
//              at the pair's own first bin; the differences and the two LTAS distances from the stored rows
//
// The chunking of a signal depends on its own length only and every sum starts at the signal's (the pair's) own first bin, so a
// signal and a pair have the same bits alone, in any batch and at any position.  There are no atomics.  All bodies compile on the
// host too (SSR_HOST_EMU, tests/emu/spectrum_emu.cpp).
#pragma once
#include "ssr_pairs.h"
#include "ssr_fft.h"
#include "ssr_phase.h"                     // ssr_phase_log2_nfft, SSR_PHASE_LOGN_MIN / _MAX: the same transform sizes

#define SSR_SPEC_FR 32                      // segments per chunk: 16 transforms of two segments
#define SSR_SPEC_NT 256                     // threads of the geometry, the signal and the pair workgroup
#define SSR_SPEC_MAX_BANDS 40               // analysis bands of the LTAS distance
#define SSR_SPEC_MAX_BINS ((1 << SSR_PHASE_LOGN_MAX) / 2 + 1)
#define SSR_SPEC_EPS 2.220446049250313e-16  // DBL_EPSILON
#define SSR_SPEC_SIG_COLS 3                 // rolloff bin, edge bin, centroid in bins
#define SSR_SPEC_PAIR_COLS 8                // hf_db of the estimate and of the target, bw / edge / centroid diff in bins, hf_diff, ltas_dist, ltas_max
static_assert(SSR_SPEC_NT == SSR_PAIRS_NT, "the geometry workgroup is ssr_run_geometry_body's");
static_assert(SSR_SPEC_FR % 2 == 0, "a transform holds two segments of one chunk");

SSR_HD int ssr_spec_segments(int n, int N, int H) { return n >= N ? 1 + (n - N) / H : 0; }
SSR_HD int ssr_spec_chunks(int n, int N, int H) { return (ssr_spec_segments(n, N, H) + SSR_SPEC_FR - 1) / SSR_SPEC_FR; }

struct SsrSpecParams {
  const void* tgt;              // targets, float32 or float64
  const int64_t* tgt_off;       // [n_tgt] device
  const void* est;              // estimates, float32 or float64
  const int64_t* est_off;       // [n_est] device
  const int32_t* tgt_len;       // [n_tgt] (workspace copy)
  const int32_t* tgt_index;     // [n_est] (workspace copy)
  int n_tgt, n_est;
  int N, H, lo, hi, n_bands;
  double rho, thr_lin;
  const int32_t* bands;         // [n_bands][2] inclusive (lo, hi) (workspace copy)
  const int32_t* split;         // [n_est] first bin of the pair's upper part, < 0: none (workspace copy)
  const cx<double>* tw;         // [N] exp(-2 pi i k / N); the window is 0.5 - 0.5 Re tw
  int32_t* sig_index;           // [n_tgt + n_est] signal -> the target that gives its length
  int32_t* run_start;           // [n_sig + 1] ssr_run_geometry_body's runs (not used further)
  int64_t* run_chunk;           // [n_sig + 1]
  int64_t* chunk_off;           // [n_sig + 1] chunk prefix over signals (the ltas grid)
  double* part;                 // [chunk_off[n_sig]][N / 2 + 1][2] chunk sums: P, A
  double* cp;                   // [n_sig][N / 2 + 1] c P
  double* sig;                  // [n_sig][4] rolloff bin, edge bin, centroid, E_tot (NaN rows: see above)
  double* lev;                  // [n_sig][n_bands] L_b
  double* sig_out;              // [n_sig][SSR_SPEC_SIG_COLS]
  double* pair_out;             // [n_est][SSR_SPEC_PAIR_COLS]
  double* ltas_out;             // [n_sig][N / 2 + 1] c P / K, or null
};

// ---- geometry: one workgroup of SSR_SPEC_NT threads.  LDS: 3 * NT int64.
template <typename BLK> SSR_BODY void ssr_spec_geometry_body(const SsrSpecParams& p, BLK& blk, int64_t* sums) {
  const int n_sig = p.n_tgt + p.n_est;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    for (int s = tid; s < n_sig; s += SSR_SPEC_NT) p.sig_index[s] = s < p.n_tgt ? s : p.tgt_index[s - p.n_tgt];
  });
#ifndef SSR_HOST_EMU
  __syncthreads();                          // (sig_index is global memory: the LDS-only barrier of a phase does not order it)
#endif
  ssr_run_geometry_body(p.tgt_len, p.sig_index, n_sig, [&](int32_t n) { return (int64_t)ssr_spec_chunks(n, p.N, p.H); }, p.run_start,
                        p.run_chunk, p.chunk_off, (double*)nullptr, 0, blk, sums);
}

// LDS of the ltas body
template <int LOGN> struct SsrSpecLds {
  double re[ssr_padded_len(1 << LOGN)], im[ssr_padded_len(1 << LOGN)];
  int live[2][4];                           // per wave: the even / the odd segment of the transform has a non-zero windowed sample
};

struct SsrSpecRegs {
  cx<double> v[8];
  double w[8];                              // the window at this thread's eight first-pass samples (the same in every segment)
  double s[5][2];                           // P, A of bins 4 tid .. 4 tid + 3, and of bin N / 2 on the last thread
};

// ---- ltas: grid block g = (signal s, chunk c) of the side T reads (side 0: targets, 1: estimates), N / 8 threads
template <typename T, int LOGN, typename BLK>
SSR_BODY void ssr_spec_ltas_body(const SsrSpecParams& p, BLK& blk, int64_t g, SsrSpecLds<LOGN>& S) {
  using PL = SsrFftPlan<LOGN>;
  constexpr int N = PL::N, NT = PL::NT, NW = (NT + 63) / 64, NB = N / 2 + 1;
  const int n_sig = p.n_tgt + p.n_est;
  const int s = ssr_prefix_find(p.chunk_off, n_sig, g);
  const int ch = (int)(g - p.chunk_off[s]);
  const int n = p.tgt_len[p.sig_index[s]], H = p.H;
  const int K = ssr_spec_segments(n, N, H);
  const int t0 = ch * SSR_SPEC_FR, t1 = t0 + SSR_SPEC_FR < K ? t0 + SSR_SPEC_FR : K;
  const T* x = s < p.n_tgt ? (const T*)p.tgt + p.tgt_off[s] : (const T*)p.est + p.est_off[s - p.n_tgt];
  const cx<double>* tw = p.tw;
  SSR_REGS(SsrSpecRegs, regs, blk);
  SSR_PHASE(blk, regs, {
    SSR_UNROLL for (int r = 0; r < 8; ++r) R.w[r] = 0.5 - 0.5 * tw[ssr_fft_first_index<LOGN>(tid, r)].x;
    SSR_UNROLL for (int j = 0; j < 5; ++j) { R.s[j][0] = R.s[j][1] = 0.0; }
  });
  for (int t = t0; t < t1; t += 2) {
    ssr_launder(blk);     // (per-pass LDS addresses are recomputed where used, not hoisted across the segment loop)
    const bool two = t + 1 < t1;            // (the odd last segment of a chunk: an empty imaginary half)
    SSR_PHASE(blk, regs, {
      SSR_UNROLL for (int r = 0; r < 8; ++r) {
        const int i = t * H + ssr_fft_first_index<LOGN>(tid, r);
        R.v[r] = {R.w[r] * (double)x[i], two ? R.w[r] * (double)x[i + H] : 0.0};
      }
      bool lx = false, ly = false;
      SSR_UNROLL for (int r = 0; r < 8; ++r) { lx = lx || R.v[r].x != 0.0; ly = ly || R.v[r].y != 0.0; }
      SSR_WAVE_ANY_STORE(tid, lx, S.live[0]);
      SSR_WAVE_ANY_STORE(tid, ly, S.live[1]);
      ssr_fft_compute<double, LOGN, 0>(tid, R.v, tw);
      ssr_fft_store<double, LOGN, 0>(tid, S.re, S.im, R.v);
    });
    ssr_fft_finish_natural<LOGN>(blk, regs, S.re, S.im, tw);
    SSR_PHASE(blk, regs, {
      // X[k] = (Z[k] + conj(Z[N - k])) / 2, Y[k] = (Z[k] - conj(Z[N - k])) / (2 i); with the even segment silent Z = i Y, with
      // the odd one silent Z = X.  The even segment is added first: segment order
      int live_x = 0, live_y = 0;
      for (int q = 0; q < NW; ++q) { live_x |= S.live[0][q]; live_y |= S.live[1][q]; }
      SSR_UNROLL for (int j = 0; j < 5; ++j) {
        const int k = 4 * tid + j, kc = (N - k) & (N - 1);
        if (j < 4 || tid == NT - 1) {
          const double zr = S.re[ssr_pad(k)], zi = S.im[ssr_pad(k)];
          if (live_x && live_y) {
            const double cr = S.re[ssr_pad(kc)], ci = S.im[ssr_pad(kc)];
            const double xr = 0.5 * (zr + cr), xi = 0.5 * (zi - ci), yr = 0.5 * (zi + ci), yi = 0.5 * (cr - zr);
            const double px = xr * xr + xi * xi, py = yr * yr + yi * yi;
            R.s[j][0] += px; R.s[j][1] += sqrt(px);
            R.s[j][0] += py; R.s[j][1] += sqrt(py);
          } else if (live_x || live_y) {
            const double pz = zr * zr + zi * zi;
            R.s[j][0] += pz; R.s[j][1] += sqrt(pz);
          }
        }
      }
    });
  }
  SSR_PHASE(blk, regs, {
    double* row = p.part + ((int64_t)g * NB + 4 * tid) * 2;
    SSR_UNROLL for (int j = 0; j < 4; ++j) { row[2 * j] = R.s[j][0]; row[2 * j + 1] = R.s[j][1]; }
    if (tid == NT - 1) { row[8] = R.s[4][0]; row[9] = R.s[4][1]; }
  });
}

// LDS of the signal body
struct SsrSpecSignalLds {
  double p[SSR_SPEC_MAX_BINS], a[SSR_SPEC_MAX_BINS];      // c P and A of every bin
  double run[SSR_SPEC_NT];                                // a thread's sum of A over its run, then the exclusive prefix inside its wave
  double pm[SSR_SPEC_NT];                                 // a thread's largest P over its run
  double ws[4][SSR_SPEC_NT / 64];                         // per wave: E_tot, sum A, sum k c P; [3]: max P and E_tot of the signal
  int wi[2][SSR_SPEC_NT];                                 // a thread's rolloff and edge candidates
};

SSR_HD double ssr_spec_level(double e, double e_tot) {
  const double q = e / e_tot;
  return 10.0 * log10(q > SSR_SPEC_EPS ? q : SSR_SPEC_EPS);
}

// ---- signal: workgroup s finishes signal s, SSR_SPEC_NT threads
template <typename BLK> SSR_BODY void ssr_spec_signal_body(const SsrSpecParams& p, BLK& blk, int s, SsrSpecSignalLds& S) {
  constexpr int NT = SSR_SPEC_NT, NW = NT / 64;
  const int NB = p.N / 2 + 1;
  const int K = ssr_spec_segments(p.tgt_len[p.sig_index[s]], p.N, p.H);
  const int64_t c0 = p.chunk_off[s], c1 = p.chunk_off[s + 1];
  const int lo = p.lo, hi = p.hi;
  const int nb = lo <= hi ? hi - lo + 1 : 0, per = (nb + NT - 1) / NT;      // a thread's run: bins lo + tid per .. + per - 1
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    for (int k = tid; k < NB; k += NT) {
      double pk = 0.0, ak = 0.0;
      for (int64_t c = c0; c < c1; ++c) {
        const double* q = p.part + (c * NB + k) * 2;
        pk += q[0]; ak += q[1];
      }
      const double cpk = (k == 0 || k == NB - 1) ? pk : 2.0 * pk;
      S.p[k] = cpk;
      S.a[k] = ak;
      p.cp[(int64_t)s * NB + k] = cpk;
      if (p.ltas_out) p.ltas_out[(int64_t)s * NB + k] = K > 0 ? cpk / (double)K : (double)NAN;
    }
  });
  SSR_PHASE(blk, regs, {
    double e = 0.0, a = 0.0, m = 0.0, pm = 0.0;
    const int k0 = lo + tid * per;
    for (int k = k0; k < k0 + per && k <= hi; ++k) {
      const double cpk = S.p[k], pk = (k == 0 || k == NB - 1) ? cpk : 0.5 * cpk;      // (P = c P / c, exactly)
      e += cpk; a += S.a[k]; m += (double)k * cpk;
      pm = pk > pm ? pk : pm;
    }
    S.run[tid] = a;
    S.pm[tid] = pm;
    SSR_WAVE_SUM_STORE(tid, NT, e, S.ws[0]);
    SSR_WAVE_SUM_STORE(tid, NT, a, S.ws[1]);
    SSR_WAVE_SUM_STORE(tid, NT, m, S.ws[2]);
  });
  // the exclusive scan of the lane sums in lane order (one thread per wave), the max of P over the band (a thread of another wave)
  SSR_PHASE(blk, regs, {
    if (tid < NW) {
      double acc = 0.0;
      for (int l = 0; l < 64; ++l) { const double v = S.run[tid * 64 + l]; S.run[tid * 64 + l] = acc; acc += v; }
    } else if (tid == 64) {
      double pm = 0.0;
      for (int t = 0; t < NT; ++t) pm = S.pm[t] > pm ? S.pm[t] : pm;
      S.ws[3][0] = pm;
    }
  });
  SSR_PHASE(blk, regs, {
    double a_tot = 0.0, before = 0.0;
    for (int q = 0; q < NW; ++q) { if (q == (tid >> 6)) before = a_tot; a_tot += S.ws[1][q]; }
    const double want = p.rho * a_tot, floor_p = S.ws[3][0] * p.thr_lin;
    double cum = before + S.run[tid];
    int r = hi + 1, e = lo - 1;
    const int k0 = lo + tid * per;
    for (int k = k0; k < k0 + per && k <= hi; ++k) {
      cum += S.a[k];
      if (r > hi && cum >= want) r = k;
      const double pk = (k == 0 || k == NB - 1) ? S.p[k] : 0.5 * S.p[k];
      if (pk >= floor_p) e = k;
    }
    S.wi[0][tid] = r;
    S.wi[1][tid] = e;
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      double e_tot = 0.0, m = 0.0;
      for (int q = 0; q < NW; ++q) { e_tot += S.ws[0][q]; m += S.ws[2][q]; }
      int r = hi, e = lo;                   // (no crossing found - rho a_tot rounded above the last sum: the band's last bin)
      for (int t = NT - 1; t >= 0; --t) if (S.wi[0][t] <= hi) r = S.wi[0][t];
      for (int t = 0; t < NT; ++t) if (S.wi[1][t] >= lo) e = S.wi[1][t];
      const bool ok = K > 0 && nb > 0 && e_tot > 0.0;
      double* row = p.sig + (int64_t)s * 4;
      row[0] = ok ? (double)r : (double)NAN;
      row[1] = ok ? (double)e : (double)NAN;
      row[2] = ok ? m / e_tot : (double)NAN;
      row[3] = ok ? e_tot : (double)NAN;
      SSR_UNROLL for (int q = 0; q < SSR_SPEC_SIG_COLS; ++q) p.sig_out[(int64_t)s * SSR_SPEC_SIG_COLS + q] = row[q];
      S.ws[3][1] = ok ? e_tot : (double)NAN;
    }
  });
  SSR_PHASE(blk, regs, {
    if (tid < p.n_bands) {
      const int b0 = p.bands[2 * tid], b1 = p.bands[2 * tid + 1];
      const double e_tot = S.ws[3][1];
      double e = 0.0;
      for (int k = b0; k <= b1; ++k) e += S.p[k];
      p.lev[(int64_t)s * p.n_bands + tid] = e_tot == e_tot ? ssr_spec_level(e, e_tot) : (double)NAN;
    }
  });
}

// LDS of the pair body
struct SsrSpecPairLds {
  double ws[2][SSR_SPEC_NT / 64];           // per wave: E_hi of the estimate and of the target
};

// ---- pair: workgroup e scores estimate e against its target, SSR_SPEC_NT threads
template <typename BLK> SSR_BODY void ssr_spec_pair_body(const SsrSpecParams& p, BLK& blk, int e, SsrSpecPairLds& S) {
  constexpr int NT = SSR_SPEC_NT, NW = NT / 64;
  const int NB = p.N / 2 + 1;
  const int sy = p.n_tgt + e, sx = p.tgt_index[e];
  const int sp = p.split[e];
  const int k_lo = sp > p.lo ? sp : p.lo, hi = p.hi;
  const bool upper = sp >= 0 && k_lo <= hi;
  const int nb = upper ? hi - k_lo + 1 : 0, per = (nb + NT - 1) / NT;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    double ey = 0.0, ex = 0.0;
    const int k0 = k_lo + tid * per;
    for (int k = k0; k < k0 + per && k <= hi; ++k) {
      ey += p.cp[(int64_t)sy * NB + k];
      ex += p.cp[(int64_t)sx * NB + k];
    }
    SSR_WAVE_SUM_STORE(tid, NT, ey, S.ws[0]);
    SSR_WAVE_SUM_STORE(tid, NT, ex, S.ws[1]);
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      const double* ry = p.sig + (int64_t)sy * 4;
      const double* rx = p.sig + (int64_t)sx * 4;
      double ey = 0.0, ex = 0.0;
      for (int q = 0; q < NW; ++q) { ey += S.ws[0][q]; ex += S.ws[1][q]; }
      // (a NaN E_tot - the signal's NaN rule - makes its hf_db NaN by the same test)
      const double hy = upper && ry[3] == ry[3] ? ssr_spec_level(ey, ry[3]) : (double)NAN;
      const double hx = upper && rx[3] == rx[3] ? ssr_spec_level(ex, rx[3]) : (double)NAN;
      double sq = 0.0, mx = 0.0;
      for (int b = 0; b < p.n_bands; ++b) {
        const double d = p.lev[(int64_t)sy * p.n_bands + b] - p.lev[(int64_t)sx * p.n_bands + b];
        sq += d * d;
        const double ad = fabs(d);
        mx = ad > mx || ad != ad ? ad : mx;
      }
      const bool ok = ry[3] == ry[3] && rx[3] == rx[3];
      double* out = p.pair_out + (int64_t)e * SSR_SPEC_PAIR_COLS;
      out[0] = hy;
      out[1] = hx;
      out[2] = ry[0] - rx[0];
      out[3] = ry[1] - rx[1];
      out[4] = ry[2] - rx[2];
      out[5] = hy - hx;
      out[6] = ok ? sqrt(sq / (double)p.n_bands) : (double)NAN;
      out[7] = ok ? mx : (double)NAN;
    }
  });
}
