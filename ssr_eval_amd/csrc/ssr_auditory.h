// Kernel bodies of the auditory family (neurogram similarity, NSIM, of gammatone spectrograms: Hines & Harte 2012, the core of ViSQOL),
// restated in DESIGN §23.  Signals are the n_tgt targets followed by the n_est estimates, float32 or float64 read in their own dtype;
// all arithmetic is float64.
//
//   filterbank  Hohmann's complex all-pole gammatone of order 4; band c has a = lambda exp(i 2 pi f_c / fs), |a| < 1, and the gain g
//               (designed on the host): y_0[n] = g x[n], y_s[n] = y_{s-1}[n] + a y_s[n - 1], s = 1 .. 4, from the zero state; z = y_4
//   image       win = 2 hop, no padding: NB = len / hop hop-blocks for len >= win (else 0), T = NB - 1 rows;
//               B[j][c] = sum |z_c[n]|^2 over block j in sample order; P[t][c] = (B[t][c] + B[t + 1][c]) / (2 win)
//   level       match: the estimate's P times sum P_target / sum P_estimate (1 where sum P_estimate = 0)
//   dB          top = max P_target, floor_db = 10 log10(top) - R; D = max(10 log10 P, floor_db), G = D - floor_db
//   nsim        3 x 3 window w = g3 g3^T, g3 = (e^-2, 1, e^-2) / (1 + 2 e^-2), cells 1 <= t <= T - 2, 1 <= c <= C - 2, centred form
//   NaN         T < 3 or top = 0: every value; a level factor that is not finite (sum P_estimate denormal): every value of that pair
//
//   geometry   one workgroup: the signal -> target-length map and the prefix sums over the signals of their segments, sweep
//              workgroups and image rows
//   sweeps     PARALLEL IN TIME as §21: a signal is cut into segments of SSR_AUD_SEG hop-blocks.  A workgroup of SSR_AUD_NT threads
//              holds NT / CP consecutive segments of one signal with the bands across CP lanes (CP: the power of two >= C); the
//              samples of its segments are staged once for all bands in an LDS tile (a lane group reads one address: a broadcast).
//              Sweep 1 filters a segment from the zero state and keeps the 4 complex end states; the scan (one lane per signal and
//              band) hands the state on, s_in[k + 1] = a^L M s_in[k] + s_end[k] with M[k][j] = binom(L - 1 + k - j, k - j), j <= k,
//              L the samples of a segment - in place, the end states become the start states; sweep 2 filters again from the
//              start state and sums |z|^2 per hop-block in sample order.  The signal is read twice, z is never written
//   image      one workgroup per signal (the targets' launch first): sum and max of P with fixed shapes, then D and G
//   score      one workgroup per estimate: NSIM per valid cell from the two G images, a band's cells summed by NT / CP lanes in
//              strides and those in order; the band means, nsim, nsim_hf, nsim_lf
//
// Segments and sum shapes depend on the signal's own length, hop and the band count only: a signal and a pair give the same bits
// alone, in any batch and at any position.  No atomics.  All bodies compile on the host too (SSR_HOST_EMU, tests/emu/auditory_emu.cpp).
#pragma once
#include <vector>
#include "ssr_pairs.h"

#define SSR_AUD_NT 256                     // threads of every workgroup of the family
#define SSR_AUD_SEG 8                      // hop-blocks per segment
#define SSR_AUD_TILE 2048                  // samples of the staging tile: NT / CP rows of 8 CP samples
#define SSR_AUD_MIN_BANDS 3
#define SSR_AUD_MAX_BANDS 64
#define SSR_AUD_MAX_BLOCKS 65536           // hop-blocks per signal
#define SSR_AUD_TAB 12                     // a band's table: Re a, Im a, g, -, then t_d = a^L binom(L - 1 + d, d), d = 0 .. 3 (re, im)
#define SSR_AUD_PAIR_COLS 3                // nsim, nsim_hf, nsim_lf
static_assert(SSR_AUD_NT == SSR_PAIRS_NT, "the scan of the geometry workgroup is ssr_run_geometry_body's shape");

SSR_HD int ssr_aud_blocks(int n, int hop) { return (int64_t)n >= 2 * (int64_t)hop ? n / hop : 0; }
SSR_HD int ssr_aud_rows(int n, int hop) { const int nb = ssr_aud_blocks(n, hop); return nb >= 2 ? nb - 1 : 0; }
SSR_HD int ssr_aud_segments(int n, int hop) { return (ssr_aud_blocks(n, hop) + SSR_AUD_SEG - 1) / SSR_AUD_SEG; }
// lanes per segment row: the power of two >= C, at least 4
SSR_HD int ssr_aud_lanes(int C) { int cp = 4; while (cp < C) cp <<= 1; return cp; }
SSR_HD int ssr_aud_wgs(int n, int hop, int cp) { const int r = SSR_AUD_NT / cp; return (ssr_aud_segments(n, hop) + r - 1) / r; }

// ---- host: the table of a call, float64 ------------------------------------------------------------------------------------------
// coef [C][3] = Re a, Im a, g -> tab [C][SSR_AUD_TAB]; a^L by squaring, L = SSR_AUD_SEG hop samples
inline void ssr_aud_tables_host(const double* coef, int C, int hop, std::vector<double>& tab) {
  tab.assign((size_t)C * SSR_AUD_TAB, 0.0);
  const int64_t L = (int64_t)SSR_AUD_SEG * hop;
  const double Ld = (double)L;
  const double bin[4] = {1.0, Ld, Ld * (Ld + 1.0) / 2.0, Ld * (Ld + 1.0) * (Ld + 2.0) / 6.0};
  for (int c = 0; c < C; ++c) {
    double* t = tab.data() + (size_t)c * SSR_AUD_TAB;
    t[0] = coef[3 * c]; t[1] = coef[3 * c + 1]; t[2] = coef[3 * c + 2];
    double pr = 1.0, pi = 0.0, br = t[0], bi = t[1];
    for (int64_t e = L; e > 0; e >>= 1) {
      if (e & 1) { const double r = pr * br - pi * bi; pi = pr * bi + pi * br; pr = r; }
      const double r = br * br - bi * bi; bi = 2.0 * br * bi; br = r;
    }
    for (int d = 0; d < 4; ++d) { t[4 + 2 * d] = pr * bin[d]; t[5 + 2 * d] = pi * bin[d]; }
  }
}

struct SsrAudParams {
  const void* tgt;              // targets, float32 or float64
  const int64_t* tgt_off;       // [n_tgt] device
  const void* est;              // estimates, float32 or float64
  const int64_t* est_off;       // [n_est] device
  const int32_t* tgt_len;       // [n_tgt] (workspace copy)
  const int32_t* tgt_index;     // [n_est] (workspace copy)
  int n_tgt, n_est;
  int hop, C, CP;               // CP = ssr_aud_lanes(C)
  double range_db;
  int match;
  const double* tab;            // [C][SSR_AUD_TAB] (workspace copy)
  const int32_t* split;         // [n_est] first interior band of the pair's upper part, C - 1: none above, -1: no split (workspace copy)
  int32_t* sig_index;           // [n_sig] signal -> the target that gives its length
  int64_t* seg_off;             // [n_sig + 1] segment prefix over signals
  int64_t* wg_off;              // [n_sig + 1] sweep workgroup prefix over signals (the sweep grid)
  int64_t* row_off;             // [n_sig + 1] image row prefix over signals
  double* state;                // [segments][C][8] end states of sweep 1, then the start states of sweep 2
  double* blk;                  // [segments][SSR_AUD_SEG][C] block sums B
  double* stat;                 // [n_sig][2] sum P, max P
  double* gimg;                 // [rows][C] G
  double* pair_out;             // [n_est][SSR_AUD_PAIR_COLS]
  double* band_out;             // [n_est][C] or null
  double* image_out;            // [rows][C] D, or null
};

// ---- geometry: one workgroup of SSR_AUD_NT threads; thread t owns signals [t c, (t + 1) c).  LDS: 3 * NT int64.
template <typename BLK> SSR_BODY void ssr_aud_geometry_body(const SsrAudParams& p, BLK& blk, int64_t* sums) {
  const int NT = SSR_AUD_NT, n_sig = p.n_tgt + p.n_est, per = (n_sig + NT - 1) / NT;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    int64_t a = 0, b = 0, c = 0;
    for (int i = tid * per; i < n_sig && i < (tid + 1) * per; ++i) {
      const int ti = i < p.n_tgt ? i : p.tgt_index[i - p.n_tgt];
      const int n = p.tgt_len[ti];
      p.sig_index[i] = ti;
      a += ssr_aud_segments(n, p.hop); b += ssr_aud_wgs(n, p.hop, p.CP); c += ssr_aud_rows(n, p.hop);
    }
    sums[tid] = a; sums[NT + tid] = b; sums[2 * NT + tid] = c;
  });
  SSR_PHASE(blk, regs, {
    if (tid < 3) {
      int64_t a = 0;
      for (int t = 0; t < NT; ++t) { const int64_t v = sums[tid * NT + t]; sums[tid * NT + t] = a; a += v; }
    }
  });
  SSR_PHASE(blk, regs, {
    int64_t a = sums[tid], b = sums[NT + tid], c = sums[2 * NT + tid];
    for (int i = tid * per; i < n_sig && i < (tid + 1) * per; ++i) {
      const int n = p.tgt_len[i < p.n_tgt ? i : p.tgt_index[i - p.n_tgt]];
      p.seg_off[i] = a; p.wg_off[i] = b; p.row_off[i] = c;
      a += ssr_aud_segments(n, p.hop); b += ssr_aud_wgs(n, p.hop, p.CP); c += ssr_aud_rows(n, p.hop);
    }
    if (tid == NT - 1) { p.seg_off[n_sig] = a; p.wg_off[n_sig] = b; p.row_off[n_sig] = c; }
  });
}

// LDS of a sweep: NT / CP rows of 8 CP samples, a row one sample longer than that (rows on different banks)
struct SsrAudSweepLds { double x[SSR_AUD_TILE + SSR_AUD_NT / 4]; };
struct SsrAudSweepRegs {
  double ar, ai, g;
  double z[8];                              // y_1 .. y_4 (re, im)
  double acc;                               // sum |z|^2 of the hop-block under way
};

// one sample through the cascade; -> |y_4|^2
SSR_DEV double ssr_aud_step(double v, double ar, double ai, double g, double* z) {
  double ur = g * v, ui = 0.0;
  SSR_UNROLL for (int s = 0; s < 4; ++s) {
    const double zr = z[2 * s], zi = z[2 * s + 1];
    ur = (ur + ar * zr) - ai * zi;
    ui = (ui + ar * zi) + ai * zr;
    z[2 * s] = ur; z[2 * s + 1] = ui;
  }
  return ur * ur + ui * ui;
}

// ---- sweeps: grid block g = (signal s, workgroup w of its segments) of the side X reads.  SECOND = false: from the zero state, the
// end state only.  SECOND = true: from the start state, the block sums.
template <typename X, bool SECOND, typename BLK>
SSR_BODY void ssr_aud_sweep_body(const SsrAudParams& p, BLK& blk, int64_t g, SsrAudSweepLds& S) {
  constexpr int NT = SSR_AUD_NT, SEG = SSR_AUD_SEG;
  const int n_sig = p.n_tgt + p.n_est;
  const int s = ssr_prefix_find(p.wg_off, n_sig, g);
  const int w = (int)(g - p.wg_off[s]);
  const int hop = p.hop, C = p.C, CP = p.CP;
  const int NB = ssr_aud_blocks(p.tgt_len[p.sig_index[s]], hop), n_seg = (NB + SEG - 1) / SEG;
  const int rows = NT / CP, TS = SSR_AUD_TILE / rows, ts_shift = __builtin_ctz((unsigned)TS), pitch = TS + 1;
  const int64_t seg0 = p.seg_off[s];
  const X* x = s < p.n_tgt ? (const X*)p.tgt + p.tgt_off[s] : (const X*)p.est + p.est_off[s - p.n_tgt];
  SSR_REGS(SsrAudSweepRegs, regs, blk);
  SSR_PHASE(blk, regs, {
    const int c = tid & (CP - 1), seg = w * rows + tid / CP;
    const bool live = c < C && seg < n_seg;
    const double* t = p.tab + (live ? c : 0) * SSR_AUD_TAB;
    R.ar = t[0]; R.ai = t[1]; R.g = t[2]; R.acc = 0.0;
    SSR_UNROLL for (int j = 0; j < 8; ++j) R.z[j] = (SECOND && live) ? p.state[((seg0 + seg) * C + c) * 8 + j] : 0.0;
  });
  for (int b = 0; b < SEG; ++b) {
    for (int t0 = 0; t0 < hop; t0 += TS) {
      const int tn = hop - t0 < TS ? hop - t0 : TS;
      SSR_PHASE(blk, regs, {
        for (int idx = tid; idx < rows * TS; idx += NT) {
          const int rr = idx >> ts_shift, i = idx & (TS - 1);
          const int64_t jb = (int64_t)(w * rows + rr) * SEG + b;         // the hop-block of row rr: inside the signal where jb < NB
          if (jb < NB && i < tn) S.x[rr * pitch + i] = (double)x[jb * hop + t0 + i];
        }
      });
      SSR_PHASE(blk, regs, {
        const int c = tid & (CP - 1), r = tid / CP, seg = w * rows + r;
        if (c < C && (int64_t)seg * SEG + b < NB) {
          const double* xs = S.x + r * pitch;
          double acc = R.acc;
          for (int i = 0; i < tn; ++i) {
            const double e = ssr_aud_step(xs[i], R.ar, R.ai, R.g, R.z);
            if (SECOND) acc += e;
          }
          R.acc = acc;
          if (SECOND && t0 + TS >= hop) {
            p.blk[((seg0 + seg) * SEG + b) * C + c] = acc;
            R.acc = 0.0;
          }
        }
      });
    }
  }
  if (!SECOND) {
    SSR_PHASE(blk, regs, {
      const int c = tid & (CP - 1), seg = w * rows + tid / CP;
      if (c < C && seg < n_seg) {
        SSR_UNROLL for (int j = 0; j < 8; ++j) p.state[((seg0 + seg) * C + c) * 8 + j] = R.z[j];
      }
    });
  }
}

// ---- scan: lane id = (signal, band).  s_in[0] = 0, s_in[k + 1] = a^L M s_in[k] + s_end[k], in place
SSR_DEV void ssr_aud_scan_lane(const SsrAudParams& p, int64_t id) {
  const int C = p.C;
  if (id >= (int64_t)(p.n_tgt + p.n_est) * C) return;
  const int s = (int)(id / C), c = (int)(id % C);
  const int64_t k0 = p.seg_off[s], k1 = p.seg_off[s + 1];
  double t[8], z[8], e[8], nz[8];
  SSR_UNROLL for (int j = 0; j < 8; ++j) { t[j] = p.tab[c * SSR_AUD_TAB + 4 + j]; z[j] = 0.0; }
  for (int64_t k = k0; k < k1; ++k) {
    double* q = p.state + (k * C + c) * 8;
    SSR_UNROLL for (int j = 0; j < 8; ++j) { e[j] = q[j]; q[j] = z[j]; }
    SSR_UNROLL for (int r = 0; r < 4; ++r) {
      double ar = 0.0, ai = 0.0;
      SSR_UNROLL for (int j = 0; j <= r; ++j) {         // t_{r - j} z_j, from the stage furthest back
        const double tr = t[2 * (r - j)], ti = t[2 * (r - j) + 1];
        ar += tr * z[2 * j] - ti * z[2 * j + 1];
        ai += tr * z[2 * j + 1] + ti * z[2 * j];
      }
      nz[2 * r] = ar + e[2 * r]; nz[2 * r + 1] = ai + e[2 * r + 1];
    }
    SSR_UNROLL for (int j = 0; j < 8; ++j) z[j] = nz[j];
  }
}

// LDS of the image and the score body
struct SsrAudImageLds { double sc[2][SSR_AUD_NT], mid[2][16], res[2]; };
struct SsrAudScoreLds { double part[SSR_AUD_NT], bs[SSR_AUD_MAX_BANDS]; };

// ---- image: workgroup s finishes signal s (every target before any estimate), SSR_AUD_NT threads
template <typename BLK> SSR_BODY void ssr_aud_image_body(const SsrAudParams& p, BLK& blk, int s, SsrAudImageLds& S) {
  constexpr int NT = SSR_AUD_NT;
  const int C = p.C, ti = p.sig_index[s];
  const int T = ssr_aud_rows(p.tgt_len[ti], p.hop), cells = T * C;
  const double* B = p.blk + p.seg_off[s] * SSR_AUD_SEG * C;
  const double den = 2.0 * (2.0 * (double)p.hop);         // 2 win
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    double sum = 0.0, mx = 0.0;
    for (int i = tid; i < cells; i += NT) {
      const double pw = (B[i] + B[i + C]) / den;          // cell i = (t, c): B[t][c] = B[i], B[t + 1][c] = B[i + C]
      sum += pw;
      mx = pw > mx || pw != pw ? pw : mx;
    }
    S.sc[0][tid] = sum; S.sc[1][tid] = mx;
  });
  SSR_PHASE(blk, regs, {
    if (tid < 32) {
      const int q = tid >> 4, l = tid & 15;
      double a = S.sc[q][l];
      for (int t = l + 16; t < NT; t += 16) { const double v = S.sc[q][t]; a = q == 0 ? a + v : (v > a || v != v ? v : a); }
      S.mid[q][l] = a;
    }
  });
  SSR_PHASE(blk, regs, {
    if (tid < 2) {
      double a = S.mid[tid][0];
      for (int l = 1; l < 16; ++l) { const double v = S.mid[tid][l]; a = tid == 0 ? a + v : (v > a || v != v ? v : a); }
      S.res[tid] = a;
      p.stat[(int64_t)s * 2 + tid] = a;
    }
  });
  SSR_PHASE(blk, regs, {
    const bool is_est = s >= p.n_tgt;
    const double top = is_est ? p.stat[(int64_t)ti * 2 + 1] : S.res[1];
    double f = 1.0;
    if (is_est && p.match && S.res[0] != 0.0) f = p.stat[(int64_t)ti * 2] / S.res[0];
    // (a level factor that overflowed - sum P_estimate denormal - is the estimate's NaN rule: no infinity leaves the kernel)
    const bool ok = top > 0.0 && f <= 1.7976931348623157e308;
    const double floor_db = 10.0 * log10(top) - p.range_db;
    const int64_t r0 = p.row_off[s] * C;
    for (int i = tid; i < cells; i += NT) {
      const double pw = (B[i] + B[i + C]) / den * f;
      const double d = 10.0 * log10(pw);
      const double D = d > floor_db ? d : floor_db;       // (P = 0: -inf -> the floor; NaN stays NaN)
      p.gimg[r0 + i] = ok ? (d != d ? d : D - floor_db) : (double)NAN;
      if (p.image_out) p.image_out[r0 + i] = ok ? (d != d ? d : D) : (double)NAN;
    }
  });
}

// NSIM of the cell whose 3 x 3 neighbourhood starts at x / y (row pitch C); w: the window, c1, c3: the constants
SSR_DEV double ssr_aud_nsim_cell(const double* x, const double* y, int C, const double* w, double c1, double c3) {
  double gx[9], gy[9], mx = 0.0, my = 0.0;
  SSR_UNROLL for (int i = 0; i < 3; ++i) {
    SSR_UNROLL for (int j = 0; j < 3; ++j) { gx[3 * i + j] = x[i * C + j]; gy[3 * i + j] = y[i * C + j]; }
  }
  SSR_UNROLL for (int k = 0; k < 9; ++k) { mx += w[k] * gx[k]; my += w[k] * gy[k]; }
  double vx = 0.0, vy = 0.0, cov = 0.0;
  SSR_UNROLL for (int k = 0; k < 9; ++k) {
    const double dx = gx[k] - mx, dy = gy[k] - my;
    vx += w[k] * (dx * dx); vy += w[k] * (dy * dy); cov += w[k] * (dx * dy);
  }
  return (2.0 * mx * my + c1) / (mx * mx + my * my + c1) * ((cov + c3) / (sqrt(vx * vy) + c3));
}

// ---- score: workgroup e scores estimate e against its target, SSR_AUD_NT threads
template <typename BLK> SSR_BODY void ssr_aud_score_body(const SsrAudParams& p, BLK& blk, int e, SsrAudScoreLds& S) {
  constexpr int NT = SSR_AUD_NT;
  const int C = p.C, CP = p.CP, Q = NT / CP;
  const int sy = p.n_tgt + e, sx = p.tgt_index[e];
  const int T = ssr_aud_rows(p.tgt_len[sx], p.hop);
  const bool ok = T >= 3 && p.stat[(int64_t)sx * 2 + 1] > 0.0;
  const double* gx = p.gimg + p.row_off[sx] * C;
  const double* gy = p.gimg + p.row_off[sy] * C;
  const double c1 = (0.01 * p.range_db) * (0.01 * p.range_db), c3 = (0.03 * p.range_db) * (0.03 * p.range_db) / 2.0;
  const double e2 = exp(-2.0), g3[3] = {e2 / (1.0 + 2.0 * e2), 1.0 / (1.0 + 2.0 * e2), e2 / (1.0 + 2.0 * e2)};
  double w[9];
  SSR_UNROLL for (int i = 0; i < 3; ++i) {
    SSR_UNROLL for (int j = 0; j < 3; ++j) w[3 * i + j] = g3[i] * g3[j];
  }
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    const int c = tid & (CP - 1), q = tid / CP;
    double acc = 0.0;
    if (ok && c >= 1 && c <= C - 2) {
      for (int t = 1 + q; t <= T - 2; t += Q) {
        const int64_t at = (int64_t)(t - 1) * C + (c - 1);
        acc += ssr_aud_nsim_cell(gx + at, gy + at, C, w, c1, c3);
      }
    }
    S.part[tid] = acc;
  });
  SSR_PHASE(blk, regs, {
    if (tid < C) {
      double a = 0.0;
      for (int q = 0; q < Q; ++q) a += S.part[q * CP + tid];
      S.bs[tid] = a;
      if (p.band_out) p.band_out[(int64_t)e * C + tid] = (ok && tid >= 1 && tid <= C - 2) ? a / (double)(T - 2) : (double)NAN;
    }
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      const int sp = p.split[e];
      double all = 0.0, lf = 0.0, hf = 0.0;
      for (int c = 1; c <= C - 2; ++c) {
        all += S.bs[c];
        if (c < sp) lf += S.bs[c]; else hf += S.bs[c];
      }
      const int n_lf = sp >= 1 ? sp - 1 : 0, n_hf = sp >= 1 ? C - 1 - sp : 0;
      const double rows = (double)(T - 2);
      double* out = p.pair_out + (int64_t)e * SSR_AUD_PAIR_COLS;
      out[0] = ok ? all / (rows * (double)(C - 2)) : (double)NAN;
      out[1] = ok && n_hf > 0 ? hf / (rows * (double)n_hf) : (double)NAN;
      out[2] = ok && n_lf > 0 ? lf / (rows * (double)n_lf) : (double)NAN;
    }
  });
}
