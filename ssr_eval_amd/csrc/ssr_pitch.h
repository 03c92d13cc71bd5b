// Kernel bodies of the pitch metrics: YIN F0 tracking (de Cheveigné & Kawahara, JASA 2002) on 16 kHz float64
// signals, and the pair statistics F0 RMSE (cents), F0 correlation, GPE, VDE (Nakatani et al. 2008) and FFE (Chu & Alwan 2009).
//
//   geometry  one workgroup: frames and tracker tiles of every signal, prefix sums over the signals in a fixed order
//   track     one workgroup per tile of SSR_PITCH_F consecutive frames of one signal.  The tile's samples, (F-1) H + W + the
//             largest lag, are staged in LDS.  Each lane sums d_t(tau) = Σ_j (x[s+j] - x[s+j+tau])^2 in the direct form for a run
//             of SSR_PITCH_R consecutive lags of one frame, j ascending: x[s+j] is a broadcast read, the lagged samples slide
//             through a register ring, so one LDS read serves the whole run.  R is odd: the 32 lanes of a half-wave read
//             ds_read_b64 addresses 2 R dwords apart, gcd(2 R, 64) = 2, and cover the 64 banks once (no conflict).  d stays in
//             LDS; then one wave per frame forms the cumulative-mean-normalised d' (prefix over tau in a fixed order), finds
//             the first trough below 0.1 (ballot), else the first minimum, refines it by the parabola and sums E_t.  Only
//             f0, the aperiodicity d'(tau*) and E are written.
//   voicing   one workgroup per signal: max E (exact in any order), then the voiced flags
//   pairs     one workgroup per pair: exact integer counts, cents^2 and the Pearson moments as float64 sums in a fixed order
//             (means first, then centred sums), then [n_est][popcount(which)] in bit order
//
// Every sum has a fixed order and there are no atomics: a signal's track, and a pair's values, are the same bits alone, in any
// batch and through the multi path.  All bodies compile on the host too (SSR_HOST_EMU, tests/emu/pitch_emu.cpp).
#pragma once
#include "ssr_pairs.h"

#define SSR_PITCH_F0_RMSE 1
#define SSR_PITCH_F0_CORR 2
#define SSR_PITCH_GPE 4
#define SSR_PITCH_VDE 8
#define SSR_PITCH_FFE 16
#define SSR_PITCH_FS 16000                // the rate every signal is tracked at
#define SSR_PITCH_HOP 160                 // H: 10 ms
#define SSR_PITCH_WIN 400                 // W: 25 ms integration window
#define SSR_PITCH_TAU_MAX 400             // ceil(16000 / 40): the largest tau_hi the options allow
#define SSR_PITCH_NT 256                  // threads of every workgroup (4 waves)
#define SSR_PITCH_F 8                     // frames per tracker tile (two per wave in the per-frame steps)
#define SSR_PITCH_R 5                     // consecutive lags per lane in the difference sums (odd: see above)
#define SSR_PITCH_RUN 7                   // consecutive lags per lane in the per-frame wave: 64 * 7 >= SSR_PITCH_TAU_MAX
#define SSR_PITCH_XS ((SSR_PITCH_F - 1) * SSR_PITCH_HOP + SSR_PITCH_WIN + SSR_PITCH_TAU_MAX + SSR_PITCH_R - 1)   // staged samples
#define SSR_PITCH_TROUGH 0.1              // absolute threshold of the trough search
#define SSR_PITCH_VOICED 0.2              // a frame is voiced when its aperiodicity is below this (and it is loud enough)
#define SSR_PITCH_SILENCE 1e-4            // ... and E_t >= 1e-4 max E (within 40 dB of the loudest frame)
#define SSR_PITCH_GROSS 0.2               // gross error: |f_y / f_x - 1| > 0.2

// lag range of the options (validated on the host: 40 <= fmin < fmax <= 1000, tau_hi - tau_lo >= 2)
SSR_HD int ssr_pitch_tau_lo(double fmax) { return (int)floor((double)SSR_PITCH_FS / fmax); }
SSR_HD int ssr_pitch_tau_hi(double fmin) { return (int)ceil((double)SSR_PITCH_FS / fmin); }
SSR_HD int ssr_pitch_runs(int tau_hi) { return (tau_hi + SSR_PITCH_R - 1) / SSR_PITCH_R; }     // lag runs of one frame
// frames of a 16 kHz signal of n samples: frame t is centred on sample t H
SSR_HD int64_t ssr_pitch_frames(int64_t n) { return n > 0 ? n / SSR_PITCH_HOP + 1 : 0; }
SSR_HD int64_t ssr_pitch_tiles(int64_t n) { return (ssr_pitch_frames(n) + SSR_PITCH_F - 1) / SSR_PITCH_F; }

#ifdef SSR_HOST_EMU
// inside a phase: dst = the first lane of this wave where pred holds, -1 if none (host: lanes run in ascending order)
#define SSR_PITCH_FIRST_LANE(tid, pred, dst)                \
  do {                                                      \
    if (((tid) & 63) == 0) (dst) = -1;                      \
    if ((pred) && (dst) < 0) (dst) = (tid) & 63;            \
  } while (0)
#else
#define SSR_PITCH_FIRST_LANE(tid, pred, dst)                                          \
  do {                                                                                \
    const unsigned long long m_ = __builtin_amdgcn_ballot_w64(pred);  /* whole wave */ \
    if (((tid) & 63) == 0) (dst) = m_ ? __builtin_ctzll(m_) : -1;                     \
  } while (0)
#endif

struct SsrPitchParams {
  const double* sig_a;          // signals 0 .. n_a - 1 (the targets, or every signal of a track call)
  const int64_t* off_a;         // [n_a] device sample offsets
  const double* sig_b;          // signals n_a .. n_a + n_b - 1 (the estimates of a metrics call)
  const int64_t* off_b;         // [n_b]
  const int32_t* len_a;         // [n_a] (workspace copy)
  const int32_t* idx_b;         // [n_b] estimate k is as long as signal idx_b[k] (workspace copy)
  int n_a, n_b;
  int tau_lo, tau_hi, nb;       // nb: lag runs of SSR_PITCH_R per frame
  int64_t* tile_pre;            // [n_a + n_b + 1] tracker tiles before each signal
  int64_t* frame_pre;           // [n_a + n_b + 1] frames before each signal
  const int64_t* frame_off;     // [n_a + n_b] first frame of each signal in f0 / ap / en / voiced (the caller's, or frame_pre)
  double* f0;                   // per frame: Hz (NaN where E = 0)
  double* ap;                   // per frame: d'(tau*)
  double* en;                   // per frame: E_t
  uint8_t* voiced;              // per frame: 0 / 1
  int which;
  double* out;                  // [n_b][popcount(which)]
};

SSR_HD int64_t ssr_pitch_len(const SsrPitchParams& p, int i) { return i < p.n_a ? p.len_a[i] : p.len_a[p.idx_b[i - p.n_a]]; }
SSR_HD const double* ssr_pitch_sig(const SsrPitchParams& p, int i) {
  return i < p.n_a ? p.sig_a + p.off_a[i] : p.sig_b + p.off_b[i - p.n_a];
}

// ---- geometry: one workgroup of SSR_PITCH_NT threads.  LDS: 2 * NT int64.
template <typename BLK> SSR_BODY void ssr_pitch_geometry_body(const SsrPitchParams& p, BLK& blk, int64_t* sums) {
  const int NT = SSR_PITCH_NT, n = p.n_a + p.n_b, c = (n + NT - 1) / NT;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    int64_t tl = 0, fr = 0;
    for (int i = tid * c; i < n && i < (tid + 1) * c; ++i) {
      const int64_t m = ssr_pitch_len(p, i);
      tl += ssr_pitch_tiles(m); fr += ssr_pitch_frames(m);
    }
    sums[tid] = tl; sums[NT + tid] = fr;
  });
  SSR_PHASE(blk, regs, {
    if (tid < 2) {
      int64_t a = 0;
      for (int t = 0; t < NT; ++t) { const int64_t v = sums[tid * NT + t]; sums[tid * NT + t] = a; a += v; }
    }
  });
  SSR_PHASE(blk, regs, {
    int64_t tl = sums[tid], fr = sums[NT + tid];
    for (int i = tid * c; i < n && i < (tid + 1) * c; ++i) {
      const int64_t m = ssr_pitch_len(p, i);
      p.tile_pre[i] = tl; p.frame_pre[i] = fr;
      tl += ssr_pitch_tiles(m); fr += ssr_pitch_frames(m);
    }
    if (tid == NT - 1) { p.tile_pre[n] = tl; p.frame_pre[n] = fr; }
  });
}

// ---- tracker, grid block g.  LDS: xs [SSR_PITCH_XS], d [F][SSR_PITCH_TAU_MAX] doubles; per wave 64 each of wsum, wpart, wmin
// (double) and wtau, wcand (int); wfirst [4] int.
template <typename BLK>
SSR_BODY void ssr_pitch_track_body(const SsrPitchParams& p, BLK& blk, int64_t g, double* xs, double* d, double* wsum,
                                   double* wpart, double* wmin, int* wtau, int* wcand, int* wfirst) {
  const int NT = SSR_PITCH_NT, H = SSR_PITCH_HOP, W = SSR_PITCH_WIN, F = SSR_PITCH_F, NR = SSR_PITCH_R, RUN = SSR_PITCH_RUN;
  const int i = ssr_prefix_find(p.tile_pre, p.n_a + p.n_b, g);
  const int64_t n = ssr_pitch_len(p, i), T = ssr_pitch_frames(n), t0 = (g - p.tile_pre[i]) * F;
  const int nf = (int)(T - t0 < F ? T - t0 : F), nb = p.nb, tau_lo = p.tau_lo, tau_hi = p.tau_hi;
  const double* x = ssr_pitch_sig(p, i);
  const int64_t s0 = t0 * H - W / 2;                        // frame t0 starts at t0 H - W / 2; zeros outside [0, n)
  const int span = (nf - 1) * H + W + nb * NR;               // <= SSR_PITCH_XS
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    for (int k = tid; k < span; k += NT) {
      const int64_t q = s0 + k;
      xs[k] = (q >= 0 && q < n) ? x[q] : 0.0;
    }
  });
  // d_f(tau) for tau = 1 + b NR .. b NR + NR: item (f, b).  ring[m % NR] holds x[s + j + tau0 + m] for the NR values of m in use.
  SSR_PHASE(blk, regs, {
    for (int it = tid; it < nf * nb; it += NT) {
      const int f = it / nb, b = it - f * nb;
      const double* xf = xs + f * H;
      const double* xl = xf + 1 + b * NR;
      double acc[NR], ring[NR];
      SSR_UNROLL for (int r = 0; r < NR; ++r) acc[r] = 0.0;
      SSR_UNROLL for (int m = 0; m < NR - 1; ++m) ring[m] = xl[m];
      for (int j = 0; j < W; j += NR) {
        SSR_UNROLL for (int u = 0; u < NR; ++u) {
          ring[(u + NR - 1) % NR] = xl[j + u + NR - 1];
          const double xj = xf[j + u];
          SSR_UNROLL for (int r = 0; r < NR; ++r) {
            const double e = xj - ring[(u + r) % NR];
            acc[r] = fma(e, e, acc[r]);
          }
        }
      }
      double* df = d + f * SSR_PITCH_TAU_MAX;             // df[tau - 1] = d_f(tau)
      SSR_UNROLL for (int r = 0; r < NR; ++r) {
        const int tau = 1 + b * NR + r;
        if (tau <= tau_hi) df[tau - 1] = acc[r];
      }
    }
  });
  // one wave per frame: wave w takes frames w, w + 4; lane l holds lags 1 + RUN l .. RUN l + RUN
  for (int k = 0; k < F / 4; ++k) {
    SSR_WPHASE(blk, regs, {
      const int w = tid >> 6, l = tid & 63, f = w + 4 * k;
      if (f < nf) {
        const double* df = d + f * SSR_PITCH_TAU_MAX;
        const int a = 1 + RUN * l, z = RUN * l + RUN < tau_hi ? RUN * l + RUN : tau_hi;
        double s = 0.0;
        for (int tau = a; tau <= z; ++tau) s += df[tau - 1];
        wsum[tid] = s;
        const double* xf = xs + f * H;
        double e = 0.0;
        for (int j = l; j < W; j += 64) e = fma(xf[j], xf[j], e);
        wpart[tid] = e;
      }
    });
    // the cumulative sums: lanes below l in ascending order, then the lane's own lags; d -> d' in place
    SSR_WPHASE(blk, regs, {
      const int w = tid >> 6, l = tid & 63, f = w + 4 * k;
      if (f < nf) {
        double* df = d + f * SSR_PITCH_TAU_MAX;
        const int a = 1 + RUN * l, z = RUN * l + RUN < tau_hi ? RUN * l + RUN : tau_hi;
        double pre = 0.0;
        for (int q = 0; q < l; ++q) pre += wsum[(w << 6) + q];
        for (int tau = a; tau <= z; ++tau) {
          const double v = df[tau - 1];
          pre += v;
          df[tau - 1] = pre > 0.0 ? (double)tau * v / pre : 1.0;
        }
      }
    });
    // troughs in [tau_lo, tau_hi]: the lane's first one below the threshold, and its first minimum
    SSR_WPHASE(blk, regs, {
      const int w = tid >> 6, l = tid & 63, f = w + 4 * k;
      int c = -1;
      if (f < nf) {
        const double* df = d + f * SSR_PITCH_TAU_MAX;
        const int a = 1 + RUN * l > tau_lo ? 1 + RUN * l : tau_lo, z = RUN * l + RUN < tau_hi ? RUN * l + RUN : tau_hi;
        double mv = 1e300;
        int mt = 0x7fffffff;
        for (int tau = a; tau <= z; ++tau) {
          const double v = df[tau - 1];
          const bool trough = tau == tau_lo ? v < df[tau] : (tau == tau_hi ? v < df[tau - 2] : (v < df[tau - 2] && v <= df[tau]));
          if (c < 0 && trough && v < SSR_PITCH_TROUGH) c = tau;
          if (v < mv) { mv = v; mt = tau; }
        }
        wcand[tid] = c; wmin[tid] = mv; wtau[tid] = mt;
      }
      SSR_PITCH_FIRST_LANE(tid, f < nf && c >= 0, wfirst[w]);
    });
    // lane 0: tau*, the parabola, f0, d'(tau*) and E
    SSR_WPHASE(blk, regs, {
      const int w = tid >> 6, l = tid & 63, f = w + 4 * k;
      if (f < nf && l == 0) {
        const double* df = d + f * SSR_PITCH_TAU_MAX;
        const int base = w << 6;
        int ts;
        if (wfirst[w] >= 0) {
          ts = wcand[base + wfirst[w]];
        } else {                                            // the smallest tau with the minimum (lanes hold ascending lags)
          double mv = wmin[base];
          ts = wtau[base];
          for (int q = 1; q < 64; ++q)
            if (wmin[base + q] < mv) { mv = wmin[base + q]; ts = wtau[base + q]; }
        }
        const double v = df[ts - 1];
        double delta = 0.0;
        if (ts > tau_lo && ts < tau_hi) {
          const double v0 = df[ts - 2], v2 = df[ts];
          const double den = 2.0 * (v0 - 2.0 * v + v2);
          if (den > 0.0) {
            const double dl = (v0 - v2) / den;
            if (fabs(dl) <= 1.0) delta = dl;
          }
        }
        double e = 0.0;
        for (int q = 0; q < 64; ++q) e += wpart[base + q];
        const int64_t o = p.frame_off[i] + t0 + f;
        p.en[o] = e;
        p.ap[o] = v;
        p.f0[o] = e > 0.0 ? (double)SSR_PITCH_FS / ((double)ts + delta) : __builtin_nan("");
      }
    });
  }
}

// ---- voicing of signal i.  LDS: NT + 1 doubles.
template <typename BLK> SSR_BODY void ssr_pitch_voicing_body(const SsrPitchParams& p, BLK& blk, int i, double* red) {
  const int NT = SSR_PITCH_NT;
  const int64_t T = ssr_pitch_frames(ssr_pitch_len(p, i)), o = p.frame_off[i];
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    double m = 0.0;
    for (int64_t t = tid; t < T; t += NT) m = fmax(m, p.en[o + t]);
    red[tid] = m;
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      double m = 0.0;
      for (int q = 0; q < NT; ++q) m = fmax(m, red[q]);
      red[NT] = m;
    }
  });
  SSR_PHASE(blk, regs, {
    const double thr = SSR_PITCH_SILENCE * red[NT];
    for (int64_t t = tid; t < T; t += NT) {
      const double e = p.en[o + t];
      p.voiced[o + t] = (e > 0.0 && e >= thr && p.ap[o + t] < SSR_PITCH_VOICED) ? 1 : 0;
    }
  });
}

// ---- pair e: estimate n_a + e against target idx_b[e].  LDS: red [5][NT] doubles, cnt [3][NT] int64, mm [4][NT] doubles,
// tot [12] doubles.
template <typename BLK>
SSR_BODY void ssr_pitch_pair_body(const SsrPitchParams& p, BLK& blk, int e, double* red, int64_t* cnt, double* mm, double* tot) {
  const int NT = SSR_PITCH_NT;
  const int ti = p.idx_b[e];
  const int64_t T = ssr_pitch_frames(p.len_a[ti]), ox = p.frame_off[ti], oy = p.frame_off[p.n_a + e];
  const double* fx = p.f0 + ox;
  const double* fy = p.f0 + oy;
  const uint8_t* vx = p.voiced + ox;
  const uint8_t* vy = p.voiced + oy;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    int64_t nbth = 0, nv = 0, ng = 0;
    double sc = 0.0, sx = 0.0, sy = 0.0, lx = 1e300, hx = -1e300, ly = 1e300, hy = -1e300;
    for (int64_t t = tid; t < T; t += NT) {
      if (vx[t] != vy[t]) {
        ++nv;
      } else if (vx[t]) {
        const double a = fx[t], b = fy[t], r = b / a;
        ++nbth;
        if (fabs(r - 1.0) > SSR_PITCH_GROSS) ++ng;
        const double c = 1200.0 * log2(r);
        sc += c * c; sx += a; sy += b;
        lx = fmin(lx, a); hx = fmax(hx, a); ly = fmin(ly, b); hy = fmax(hy, b);
      }
    }
    cnt[tid] = nbth; cnt[NT + tid] = nv; cnt[2 * NT + tid] = ng;
    red[tid] = sc; red[NT + tid] = sx; red[2 * NT + tid] = sy;
    mm[tid] = lx; mm[NT + tid] = hx; mm[2 * NT + tid] = ly; mm[3 * NT + tid] = hy;
  });
  SSR_PHASE(blk, regs, {
    if (tid < 3) {
      int64_t a = 0;
      double s = 0.0;
      for (int q = 0; q < NT; ++q) { a += cnt[tid * NT + q]; s += red[tid * NT + q]; }
      tot[tid] = (double)a; tot[3 + tid] = s;
    } else if (tid < 7) {
      const int k = tid - 3;
      double m = mm[k * NT];
      for (int q = 1; q < NT; ++q) m = (k & 1) ? fmax(m, mm[k * NT + q]) : fmin(m, mm[k * NT + q]);
      tot[6 + k] = m;
    }
  });
  // centred moments about the means over B
  SSR_PHASE(blk, regs, {
    const double nbd = tot[0], mx = tot[4] / nbd, my = tot[5] / nbd;
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
    if (nbd > 0.0)
      for (int64_t t = tid; t < T; t += NT)
        if (vx[t] && vy[t]) {
          const double a = fx[t] - mx, b = fy[t] - my;
          sxx += a * a; syy += b * b; sxy += a * b;
        }
    red[tid] = sxx; red[NT + tid] = syy; red[2 * NT + tid] = sxy;
  });
  SSR_PHASE(blk, regs, {
    if (tid < 3) {
      double s = 0.0;
      for (int q = 0; q < NT; ++q) s += red[tid * NT + q];
      red[3 * NT + tid] = s;
    }
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      const double nan = __builtin_nan("");
      const double nbd = tot[0], nv = tot[1], ng = tot[2], Td = (double)T;
      const double sxx = red[3 * NT], syy = red[3 * NT + 1], sxy = red[3 * NT + 2];
      const bool flat = !(tot[6] < tot[7]) || !(tot[8] < tot[9]);      // every f_x, or every f_y, of B is the same
      double v[5];
      v[0] = nbd > 0.0 ? sqrt(tot[3] / nbd) : nan;
      v[1] = (nbd >= 2.0 && !flat) ? sxy / sqrt(sxx * syy) : nan;
      v[2] = nbd > 0.0 ? ng / nbd : nan;
      v[3] = T > 0 ? nv / Td : nan;
      v[4] = T > 0 ? (nv + ng) / Td : nan;
      double* o = p.out + (int64_t)e * ssr_which_count(p.which);
      int c = 0;
      for (int b = 0; b < 5; ++b)
        if (p.which & (1 << b)) o[c++] = v[b];
    }
  });
}
