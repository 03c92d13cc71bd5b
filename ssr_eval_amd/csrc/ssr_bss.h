// Kernel bodies of the filter-invariant SDR: the SDR of BSS Eval (Vincent, Gribonval & Févotte, "Performance measurement
// in blind audio source separation", IEEE TASLP 14(4), 2006) for one source with a causal L-tap allowed distortion, 1 <= L <= 512.
// x = target, y = estimate, both of length n and widened to float64; EPS = DBL_EPSILON:
//
//   r[k] = Σ_{t=0}^{n-1-k} x[t] x[t+k],  b[k] = Σ_{t=0}^{n-1-k} x[t] y[t+k]        k = 0 .. L-1 (terms with t + k >= n do not exist)
//   Toeplitz(r) c = b                                                             no diagonal loading
//   p[t] = Σ_k c[k] x[t-k],  e[t] = y[t] - p[t]                                   t = 0 .. n+L-2, y zero beyond n
//   sdr = 10 log10((Σp² + EPS) / (Σe² + EPS)),  sdr_lag = the smallest k with |c[k]| maximal
//   n = 0 or r[0] = 0: both NaN (and c = 0)
//
// The system is solved by Levinson's recursion for a general right-hand side.  If the prediction error E_m of order m is <= 0 or
// not finite (m = 0: E_0 = r[0]), the recursion stops there: the taps from m on are 0.
//
//   geometry   one workgroup (ssr_pairs.h): runs of consecutive pairs that name one target, tile prefix sums over runs and pairs
//   corr       one workgroup per (run, tile of SSR_BSS_TILE samples): the tile's share of r once, then of b for each estimate of
//              the run.  SSR_BSS_SUB samples and their L-sample halo are staged in LDS per round; a lane owns 8 consecutive lags in
//              registers and a share of the round's samples, eight at a time: 8 broadcast x, 8 new window values, 64 FMAs.
//   solve      one wave per pair: the tile partials in tile order, Levinson's recursion (vectors in LDS, the two dot products of
//              an order as whole-wave sums), c, sdr_lag
//   resid      one workgroup per (pair, tile): p and e sample by sample, a lane owns 8 consecutive outputs and slides the x window
//              through registers; the last tile of a pair also takes the L - 1 samples past n
//   finalize   one thread per pair: the resid tiles in ascending order, sdr
//
// Tiles, rounds and the lanes' shares depend on the pair's own length and L only, every sum has a fixed order and there are no
// atomics: a pair gives the same bits alone, in any batch and in any run.  All bodies compile on the host too (SSR_HOST_EMU,
// tests/emu/bss_emu.cpp).
#pragma once
#include "ssr_pairs.h"

#ifndef SSR_BSS_MAX_TAPS
#define SSR_BSS_MAX_TAPS 512
#endif
#define SSR_BSS_NT 256                     // threads of the geometry, corr and resid workgroups
static_assert(SSR_BSS_NT == SSR_PAIRS_NT, "the geometry workgroup is ssr_run_geometry_body's");
#define SSR_BSS_TILE 16384                 // samples of a tile: one partial row of r / b, one partial (Σp², Σe²)
#define SSR_BSS_SUB 1024                   // corr: samples staged per round (+ the SSR_BSS_MAX_TAPS halo)
#define SSR_BSS_RSUB 2048                  // resid: outputs per round, 8 per thread (+ the SSR_BSS_MAX_TAPS samples before them)
#define SSR_BSS_EPS 2.220446049250313e-16  // DBL_EPSILON
static_assert(SSR_BSS_TILE % SSR_BSS_SUB == 0 && SSR_BSS_TILE % SSR_BSS_RSUB == 0 && SSR_BSS_RSUB == 8 * SSR_BSS_NT, "rounds");

// LDS index of staged sample i: one spare double per 8, so that lanes whose windows start 8 samples apart read 9 doubles apart
// (18 banks: no two of 32 lanes share one) and a window of 8 from a multiple of 8 stays contiguous
SSR_HD constexpr int ssr_bss_pad(int i) { return i + (i >> 3); }
#define SSR_BSS_CORR_LDS (ssr_bss_pad(SSR_BSS_SUB + SSR_BSS_MAX_TAPS - 1) + 1)      // doubles of a staged corr array
#define SSR_BSS_RESID_LDS (ssr_bss_pad(SSR_BSS_RSUB + SSR_BSS_MAX_TAPS - 1) + 1)    // doubles of the staged resid array
#define SSR_BSS_PART_LDS (SSR_BSS_NT * 8)                                            // corr: the lanes' 8 sums each

SSR_HD int64_t ssr_bss_tiles(int64_t n) { return (n + SSR_BSS_TILE - 1) / SSR_BSS_TILE; }

struct SsrBssParams {
  const void* tgt;              // targets, float32 or float64
  const int64_t* tgt_off;       // [n_tgt] device
  const void* est;              // estimates, float32 or float64
  const int64_t* est_off;       // [n_est] device
  const int32_t* tgt_len;       // [n_tgt] (workspace copy)
  const int32_t* tgt_index;     // [n_est] (workspace copy)
  int n_tgt, n_est, n_runs;
  int L;                        // taps
  int32_t* run_start;           // [n_runs + 1] first pair of each run of consecutive pairs with one target; [n_runs] = n_est
  int64_t* run_tile;            // [n_runs + 1] tile prefix over runs (the corr grid, the rows of rpart)
  int64_t* pair_tile;           // [n_est + 1] tile prefix over pairs (the resid grid, the rows of bpart and part2)
  int32_t* pair_run;            // [n_est] the run of a pair (written by corr for targets with n > 0, read for those only)
  double* rpart;                // [run_tile[n_runs]][L]
  double* bpart;                // [pair_tile[n_est]][L]
  double* c;                    // [n_est][L]
  double* fin;                  // [n_est] 1: the pair has a score, 0: NaN
  double* part2;                // [pair_tile[n_est]][2] Σp², Σe²
  double* out;                  // [n_est][2] sdr, sdr_lag
  double* filt;                 // [n_est][L] or null
};

// ---- geometry: ssr_run_geometry_body on the tiles of each target (no frame window)
template <typename BLK> SSR_BODY void ssr_bss_geometry_body(const SsrBssParams& p, BLK& blk, int64_t* sums) {
  ssr_run_geometry_body(p.tgt_len, p.tgt_index, p.n_est, [&](int32_t n) { return ssr_bss_tiles(n); }, p.run_start, p.run_tile,
                        p.pair_tile, (double*)nullptr, 0, blk, sums);
}

// lags 8 g .. 8 g + 7 against the samples 8 q0 .. 8 q1 - 1 of the round: acc[j] += Σ_t xs[t] ws[t + 8 g + j]
struct SsrBssAcc { double a[8]; };
SSR_DEV void ssr_bss_corr_run(const double* xs, const double* ws, int q0, int q1, int g, double (&acc)[8]) {
  double w[16];
  const int w0 = ssr_bss_pad(8 * q0 + 8 * g);
  SSR_UNROLL
  for (int j = 0; j < 8; ++j) w[j] = ws[w0 + j];
  for (int q = q0; q < q1; ++q) {
    const int xi = ssr_bss_pad(8 * q), wn = ssr_bss_pad(8 * q + 8 * g + 8);
    double xv[8];
    SSR_UNROLL
    for (int j = 0; j < 8; ++j) { xv[j] = xs[xi + j]; w[8 + j] = ws[wn + j]; }
    SSR_UNROLL
    for (int i = 0; i < 8; ++i) {
      SSR_UNROLL
      for (int j = 0; j < 8; ++j) acc[j] += xv[i] * w[i + j];
    }
    SSR_UNROLL
    for (int j = 0; j < 8; ++j) w[j] = w[8 + j];
  }
}

// ---- corr for grid block gidx.  LDS: xs, ys [SSR_BSS_CORR_LDS], part [SSR_BSS_PART_LDS] doubles.
// The ceil(L / 8) lag groups times S = NT / groups sample shares are the threads; a share is Q blocks of 8 samples of the round.
template <typename TT, typename TE, typename BLK>
SSR_BODY void ssr_bss_corr_body(const SsrBssParams& p, BLK& blk, int64_t gidx, double* xs, double* ys, double* part) {
  const int NT = SSR_BSS_NT, L = p.L;
  const int r = ssr_prefix_find(p.run_tile, p.n_runs, gidx);
  const int64_t k = gidx - p.run_tile[r];
  const int e0 = p.run_start[r], e1 = p.run_start[r + 1], t = p.tgt_index[e0];
  const int64_t n = p.tgt_len[t], a = k * SSR_BSS_TILE, b = (n - a < SSR_BSS_TILE) ? n : a + SSR_BSS_TILE;
  const TT* x = (const TT*)p.tgt + p.tgt_off[t];
  const int G = (L + 7) / 8, S = NT / G, QN = SSR_BSS_SUB / 8, Q = (QN + S - 1) / S;
  SSR_REGS(SsrBssAcc, regs, blk);
  for (int e = e0 - 1; e < e1; ++e) {                  // e0 - 1: the target against itself (r), then b of each estimate
    const bool est = e >= e0;
    const TE* y = (const TE*)p.est + (est ? p.est_off[e] : 0);
    const double* ws = est ? ys : xs;
    SSR_PHASE(blk, regs, {
      SSR_UNROLL
      for (int j = 0; j < 8; ++j) R.a[j] = 0.0;
      if (!est && k == 0)
        for (int i = e0 + tid; i < e1; i += NT) p.pair_run[i] = r;
    });
    for (int64_t s0 = a; s0 < b; s0 += SSR_BSS_SUB) {
      SSR_PHASE(blk, regs, {
        for (int i = tid; i < SSR_BSS_SUB + SSR_BSS_MAX_TAPS; i += NT) {
          const int64_t u = s0 + i;
          xs[ssr_bss_pad(i)] = u < n ? (double)x[u] : 0.0;
          if (est) ys[ssr_bss_pad(i)] = u < n ? (double)y[u] : 0.0;
        }
      });
      SSR_PHASE(blk, regs, {
        const int g = tid % G, s = tid / G, q0 = s * Q, q1 = (q0 + Q < QN) ? q0 + Q : QN;
        if (s < S && q0 < q1) ssr_bss_corr_run(xs, ws, q0, q1, g, R.a);
      });
    }
    SSR_PHASE(blk, regs, {
      const int g = tid % G, s = tid / G;
      if (s < S) {
        SSR_UNROLL
        for (int j = 0; j < 8; ++j) part[(s * G + g) * 8 + j] = R.a[j];
      }
    });
    SSR_PHASE(blk, regs, {
      double* o = est ? p.bpart + (p.pair_tile[e] + k) * L : p.rpart + (p.run_tile[r] + k) * L;
      for (int kk = tid; kk < L; kk += NT) {
        double v = 0.0;
        for (int s = 0; s < S; ++s) v += part[(s * G + (kk >> 3)) * 8 + (kk & 7)];
        o[kk] = v;
      }
    });
  }
}

// ---- solve for pair e: one wave.  LDS: rr, bb, av, cv [SSR_BSS_MAX_TAPS], red [2], st [4], mx [128] doubles.
// st[m & 1]: the prediction error after order m, st[2]: the order's gain on c, st[3]: 1 once the recursion has stopped
template <typename BLK>
SSR_BODY void ssr_bss_solve_body(const SsrBssParams& p, BLK& blk, int e, double* rr, double* bb, double* av, double* cv, double* red,
                                 double* st, double* mx) {
  const int L = p.L, t = p.tgt_index[e];
  const int64_t n = p.tgt_len[t], nt = p.pair_tile[e + 1] - p.pair_tile[e];
  const double* rp = n > 0 ? p.rpart + p.run_tile[p.pair_run[e]] * L : nullptr;
  const double* bp = p.bpart + p.pair_tile[e] * L;
  SSR_REGS(int, regs, blk);
  SSR_WPHASE(blk, regs, {
    for (int k = tid; k < L; k += 64) {
      double r = 0.0, b = 0.0;
      for (int64_t q = 0; q < nt; ++q) { r += rp[q * L + k]; b += bp[q * L + k]; }
      rr[k] = r; bb[k] = b; av[k] = k == 0 ? 1.0 : 0.0; cv[k] = 0.0;
    }
    if (tid == 0) st[3] = 1.0;
  });
  const bool ok = n > 0 && rr[0] != 0.0;
  if (ok) {
    SSR_WPHASE(blk, regs, {
      if (tid == 0) {
        const double E = rr[0];
        const bool good = E > 0.0 && E < (double)INFINITY;
        st[0] = E; st[3] = good ? 0.0 : 1.0;
        if (good) cv[0] = bb[0] / E;
      }
    });
    for (int m = 1; m < L && st[3] == 0.0; ++m) {
      // Σ_{i<m} a[i] r[m-i] (a[0] = 1) and Σ_{i<m} c[i] r[m-i]
      SSR_WPHASE(blk, regs, {
        double sa = 0.0, sc = 0.0;
        for (int i = tid; i < m; i += 64) { const double rv = rr[m - i]; sa += av[i] * rv; sc += cv[i] * rv; }
        SSR_WAVE_SUM_STORE(tid, 64, sa, red);
        SSR_WAVE_SUM_STORE(tid, 64, sc, red + 1);
      });
      // the predictor of order m: a[i] += kk a[m-i], each lane its own (i, m - i) pairs
      SSR_WPHASE(blk, regs, {
        const double E = st[(m - 1) & 1], kk = -red[0] / E, En = E * (1.0 - kk * kk);
        for (int i = 1 + tid; 2 * i <= m; i += 64) {
          const int j = m - i;
          const double ai = av[i], aj = av[j];
          av[i] = ai + kk * aj;
          if (j != i) av[j] = aj + kk * ai;
        }
        if (tid == 0) {
          const bool good = En > 0.0 && En < (double)INFINITY;
          av[m] = kk;
          st[m & 1] = En; st[3] = good ? 0.0 : 1.0;
          st[2] = good ? (bb[m] - red[1]) / En : 0.0;
        }
      });
      // c[i] += gain a[m-i], c[m] = gain
      SSR_WPHASE(blk, regs, {
        if (st[3] == 0.0) {
          const double gain = st[2];
          for (int i = tid; i <= m; i += 64) cv[i] += gain * av[m - i];
        }
      });
    }
  }
  SSR_WPHASE(blk, regs, {
    double best = -1.0;
    int bk = 0;
    for (int k = tid; k < L; k += 64) {
      const double v = fabs(cv[k]);
      if (v > best) { best = v; bk = k; }
      p.c[(int64_t)e * L + k] = cv[k];
      if (p.filt) p.filt[(int64_t)e * L + k] = cv[k];
    }
    mx[tid] = best; mx[64 + tid] = (double)bk;
  });
  SSR_WPHASE(blk, regs, {
    if (tid == 0) {
      double best = -1.0, bk = 0.0;
      for (int l = 0; l < 64; ++l)
        if (mx[l] > best || (mx[l] == best && mx[64 + l] < bk)) { best = mx[l]; bk = mx[64 + l]; }
      p.out[2 * (int64_t)e + 1] = ok ? bk : (double)NAN;
      p.fin[e] = ok ? 1.0 : 0.0;
    }
  });
}

// outputs i0 - SSR_BSS_MAX_TAPS .. + 7 of the round (i0: their staged index, a multiple of 8): pv[j] += Σ_k cs[k] xs[i0 + j - k]
SSR_DEV void ssr_bss_fir_run(const double* xs, const double* cs, int i0, int L8, double (&pv)[8]) {
  double w[16];
  const int hi = ssr_bss_pad(i0);
  SSR_UNROLL
  for (int u = 0; u < 8; ++u) w[8 + u] = xs[hi + u];
  for (int kb = 0; kb < L8; kb += 8) {
    const int lo = ssr_bss_pad(i0 - kb - 8);
    double cq[8];
    SSR_UNROLL
    for (int u = 0; u < 8; ++u) { w[u] = xs[lo + u]; cq[u] = cs[kb + u]; }
    SSR_UNROLL
    for (int kk = 0; kk < 8; ++kk) {
      SSR_UNROLL
      for (int j = 0; j < 8; ++j) pv[j] += cq[kk] * w[j - kk + 8];
    }
    SSR_UNROLL
    for (int u = 0; u < 8; ++u) w[8 + u] = w[u];
  }
}

// ---- resid for grid block gidx.  LDS: xs [SSR_BSS_RESID_LDS], cs [SSR_BSS_MAX_TAPS], red [8] doubles.
struct SsrBssRes { double sp, se; };
template <typename TT, typename TE, typename BLK>
SSR_BODY void ssr_bss_resid_body(const SsrBssParams& p, BLK& blk, int64_t gidx, double* xs, double* cs, double* red) {
  const int NT = SSR_BSS_NT, L = p.L, L8 = (L + 7) & ~7;
  const int e = ssr_prefix_find(p.pair_tile, p.n_est, gidx);
  const int64_t k = gidx - p.pair_tile[e], nt = p.pair_tile[e + 1] - p.pair_tile[e];
  const int t = p.tgt_index[e];
  const int64_t n = p.tgt_len[t], a = k * SSR_BSS_TILE, b = (k == nt - 1) ? n + L - 1 : a + SSR_BSS_TILE;
  const TT* x = (const TT*)p.tgt + p.tgt_off[t];
  const TE* y = (const TE*)p.est + p.est_off[e];
  SSR_REGS(SsrBssRes, regs, blk);
  SSR_PHASE(blk, regs, {
    R.sp = 0.0; R.se = 0.0;
    for (int i = tid; i < SSR_BSS_MAX_TAPS; i += NT) cs[i] = i < L ? p.c[(int64_t)e * L + i] : 0.0;
  });
  for (int64_t s0 = a; s0 < b; s0 += SSR_BSS_RSUB) {
    SSR_PHASE(blk, regs, {
      for (int i = tid; i < SSR_BSS_RSUB + SSR_BSS_MAX_TAPS; i += NT) {
        const int64_t u = s0 - SSR_BSS_MAX_TAPS + i;
        xs[ssr_bss_pad(i)] = (u >= 0 && u < n) ? (double)x[u] : 0.0;
      }
    });
    SSR_PHASE(blk, regs, {
      const int64_t t0 = s0 + 8 * tid;
      if (t0 < b) {
        double pv[8];
        SSR_UNROLL
        for (int j = 0; j < 8; ++j) pv[j] = 0.0;
        ssr_bss_fir_run(xs, cs, 8 * tid + SSR_BSS_MAX_TAPS, L8, pv);
        SSR_UNROLL
        for (int j = 0; j < 8; ++j) {
          if (t0 + j < b) {
            const double yv = t0 + j < n ? (double)y[t0 + j] : 0.0, ev = yv - pv[j];
            R.sp += pv[j] * pv[j]; R.se += ev * ev;
          }
        }
      }
    });
  }
  SSR_PHASE(blk, regs, {
    SSR_WAVE_SUM_STORE(tid, NT, R.sp, red);
    SSR_WAVE_SUM_STORE(tid, NT, R.se, red + 4);
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      double* o = p.part2 + gidx * 2;
      o[0] = red[0] + red[1] + red[2] + red[3];
      o[1] = red[4] + red[5] + red[6] + red[7];
    }
  });
}

// ---- finalize: pair e, the resid tiles in ascending order
SSR_HD void ssr_bss_finalize(const SsrBssParams& p, int e) {
  const int64_t n = p.tgt_len[p.tgt_index[e]];
  double sp = 0.0, se = 0.0;
  for (int64_t g = p.pair_tile[e]; g < p.pair_tile[e + 1]; ++g) { sp += p.part2[2 * g]; se += p.part2[2 * g + 1]; }
  p.out[2 * (int64_t)e] = (n > 0 && p.fin[e] != 0.0) ? 10.0 * log10((sp + SSR_BSS_EPS) / (se + SSR_BSS_EPS)) : (double)NAN;
}
