// Kernel bodies of the delay stage: a bounded, two-sided, float64 delay search per (target, estimate) pair and the
// compensation of the delay found.  x = target of n_x samples, y = estimate of n_y samples, both widened to float64; 1 <= L <= 4096:
//
//   c[d] = Σ_t x[t] y[t + d]        over the t with 0 <= t < n_x and 0 <= t + d < n_y,  d = -L .. L (no such t: 0)
//   Ex = Σ x², Ey = Σ y²
//   d*   = the d of the largest c[d]; among equal values the smallest |d|, among those the non-negative one
//   δ    = 0.5 (c[d*-1] - c[d*+1]) / (c[d*-1] - 2 c[d*] + c[d*+1]) clamped to [-0.5, 0.5]; 0 where |d*| = L (edge = 1), or where the
//          denominator is 0 or not finite
//   corr = c[d*] / sqrt(Ex Ey)
//   Ex = 0, Ey = 0, n_x = 0, n_y = 0 or not c[d*] > 0:  d* = 0, δ = 0, edge = 0, corr = NaN
//   z[t] = y[t + d*] (0 outside y), or with subsample and δ != 0:  z[t] = Σ_{m=-16..16} h[m] y[t + d* + m],
//   h[m] = s(u) w(u) / Σ_m s(u) w(u),  u = m - δ,  s(u) = (-1)^(m+1) sin(π δ) / (π u),  w(u) = 0.5 (1 + cos(π u / 17))
//
//   geometry   one workgroup: the prefix over pairs of the corr tiles (of n_x) and of the shift tiles (of n_y)
//   corr       one workgroup per (pair, tile of SSR_ALIGN_TILE target samples, block of SSR_ALIGN_LAGS lags): ssr_bss.h's scheme - a
//              round stages SSR_ALIGN_SUB target samples and the estimate's window with its lag halo in LDS as doubles, a lane owns 8
//              consecutive lags in registers and a share of the round's samples; one partial row of c per tile.  The blocks hold the
//              lags -L .. L - 1; the block of the lowest lags also sums the tile's share of lag +L, of Ex and of Ey as lane sums
//              (the last tile takes the estimate's samples past the target's end)
//   pick       one wave per pair: the tile partials in tile order, the tie-ruled peak, δ, corr, edge, the 33 taps
//   shift      one workgroup per (pair, SSR_ALIGN_OUT outputs): d* and the taps come from device memory; a copy with zero fill
//              (16-byte accesses where both sides allow), or the 33-tap filter on samples staged in LDS, 8 outputs per lane
//
// Tiles, rounds, shares and sum orders depend on the pair's own lengths and L only and there are no atomics: a pair gives the same
// bits alone, in any batch, at any position and in any run.  All bodies compile on the host too (SSR_HOST_EMU, tests/emu/align_emu.cpp).
#pragma once
#include "ssr_bss.h"

#define SSR_ALIGN_LAG_LIMIT 4096           // the largest max_lag (SSR_ALIGN_MAX_LAG of the C ABI)
#define SSR_ALIGN_NT 256                   // threads of the geometry, corr and shift workgroups
#define SSR_ALIGN_TILE 16384               // target samples of a tile: one partial row of c, one partial (Ex, Ey)
#define SSR_ALIGN_SUB 1024                 // corr: target samples staged per round
#define SSR_ALIGN_LAGS (8 * SSR_ALIGN_NT)  // corr: lags of a block, 8 per lane
#define SSR_ALIGN_HALF 16                  // shift: taps on either side of the centre one
#define SSR_ALIGN_TAPS (2 * SSR_ALIGN_HALF + 1)
#define SSR_ALIGN_OUT (8 * SSR_ALIGN_NT)   // shift: outputs of a workgroup, 8 per lane
#define SSR_ALIGN_COLS 4                   // delay, frac, corr, edge
static_assert(SSR_ALIGN_TILE % SSR_ALIGN_SUB == 0 && SSR_ALIGN_SUB % 8 == 0, "rounds");

// staged arrays use ssr_bss_pad: lanes whose windows start 8 samples apart read 9 doubles (18 banks) apart
#define SSR_ALIGN_X_LDS (ssr_bss_pad(SSR_ALIGN_SUB - 1) + 1)                                      // doubles of the staged target samples
#define SSR_ALIGN_Y_LDS (ssr_bss_pad(SSR_ALIGN_SUB + SSR_ALIGN_LAGS - 1) + 1)                      // ... of the estimate's window
#define SSR_ALIGN_S_LDS (ssr_bss_pad(SSR_ALIGN_OUT + 2 * SSR_ALIGN_HALF - 1) + 1)                  // ... of the shift's staged samples
static_assert(SSR_ALIGN_Y_LDS >= SSR_ALIGN_NT * 8, "the lanes' sums reuse the window array");

SSR_HD int64_t ssr_align_tiles(int64_t n_x) { return (n_x + SSR_ALIGN_TILE - 1) / SSR_ALIGN_TILE; }
SSR_HD int64_t ssr_align_out_tiles(int64_t n_y) { return (n_y + SSR_ALIGN_OUT - 1) / SSR_ALIGN_OUT; }
// the lags -L .. L - 1 go in blocks of SSR_ALIGN_LAGS; lag +L rides with the first block (a power-of-two L fills its blocks)
SSR_HD int ssr_align_lag_blocks(int L) { return (2 * L + SSR_ALIGN_LAGS - 1) / SSR_ALIGN_LAGS; }

struct SsrAlignParams {
  const void* tgt;              // targets, float32 or float64
  const int64_t* tgt_off;       // [n_tgt] device
  const void* est;              // estimates, float32 or float64
  const int64_t* est_off;       // [n_est] device
  const int32_t* tgt_len;       // [n_tgt] (workspace copy)
  const int32_t* tgt_index;     // [n_est] (workspace copy)
  int n_tgt, n_est;
  const int32_t* est_len;       // [n_est] (workspace copy)
  int L;                        // the largest lag searched
  int subsample;                // shift: apply δ
  int64_t* pair_tile;           // [n_est + 1] corr tile prefix over pairs (the rows of cpart and epart)
  int64_t* pair_out;            // [n_est + 1] shift tile prefix over pairs (the shift grid)
  double* cpart;                // [pair_tile[n_est]][2 L + 1]
  double* epart;                // [pair_tile[n_est]][2] Ex, Ey
  double* taps;                 // [n_est][SSR_ALIGN_TAPS]
  double* rows;                 // [n_est][SSR_ALIGN_COLS] delay, frac, corr, edge
  double* c;                    // [n_est][2 L + 1] or null
  void* out;                    // the compensated estimates, in the estimates' dtype, or null
  const int64_t* out_off;       // [n_est] device
};

// ---- geometry: one workgroup of SSR_ALIGN_NT threads.  LDS: 2 * NT int64.  Thread t owns pairs [t c, (t + 1) c), c = ceil(n_est / NT)
template <typename BLK> SSR_BODY void ssr_align_geometry_body(const SsrAlignParams& p, BLK& blk, int64_t* sums) {
  const int NT = SSR_ALIGN_NT, c = (p.n_est + NT - 1) / NT;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    int64_t a = 0, b = 0;
    for (int e = tid * c; e < p.n_est && e < (tid + 1) * c; ++e) {
      a += ssr_align_tiles(p.tgt_len[p.tgt_index[e]]);
      b += ssr_align_out_tiles(p.est_len[e]);
    }
    sums[tid] = a; sums[NT + tid] = b;
  });
  SSR_PHASE(blk, regs, {
    if (tid < 2) {
      int64_t a = 0;
      for (int t = 0; t < NT; ++t) { const int64_t v = sums[tid * NT + t]; sums[tid * NT + t] = a; a += v; }
    }
  });
  SSR_PHASE(blk, regs, {
    int64_t a = sums[tid], b = sums[NT + tid];
    for (int e = tid * c; e < p.n_est && e < (tid + 1) * c; ++e) {
      p.pair_tile[e] = a; p.pair_out[e] = b;
      a += ssr_align_tiles(p.tgt_len[p.tgt_index[e]]);
      b += ssr_align_out_tiles(p.est_len[e]);
    }
    if (tid == NT - 1) { p.pair_tile[p.n_est] = a; p.pair_out[p.n_est] = b; }
  });
}

// ---- corr for grid block gidx = (pair tile) * lag blocks + lag block.  LDS: xs [SSR_ALIGN_X_LDS], ys [SSR_ALIGN_Y_LDS], red [12].
// The block's G = ceil(lags / 8) lag groups times S = NT / G sample shares are the threads; a share is Q blocks of 8 samples of the
// round.  Lag d0 + l of the block reads the window sample i + l for target sample i of the round: the window starts at s0 + d0.
template <typename TT, typename TE, typename BLK>
SSR_BODY void ssr_align_corr_body(const SsrAlignParams& p, BLK& blk, int64_t gidx, double* xs, double* ys, double* red) {
  const int NT = SSR_ALIGN_NT, L = p.L, NL = 2 * L + 1, NB = ssr_align_lag_blocks(L);
  const int64_t unit = gidx / NB;
  const int lb = (int)(gidx - unit * NB);
  const int e = ssr_prefix_find(p.pair_tile, p.n_est, unit);
  const int64_t k = unit - p.pair_tile[e];
  const int t = p.tgt_index[e];
  const int64_t nx = p.tgt_len[t], ny = p.est_len[e], a = k * SSR_ALIGN_TILE, b = (nx - a < SSR_ALIGN_TILE) ? nx : a + SSR_ALIGN_TILE;
  const TT* x = (const TT*)p.tgt + p.tgt_off[t];
  const TE* y = (const TE*)p.est + p.est_off[e];
  const int l0 = lb * SSR_ALIGN_LAGS, nl = (NL - 1 - l0 < SSR_ALIGN_LAGS) ? NL - 1 - l0 : SSR_ALIGN_LAGS, d0 = l0 - L;
  const int G = (nl + 7) / 8, S = NT / G, QN = SSR_ALIGN_SUB / 8, Q = (QN + S - 1) / S;
  double* part = ys;                                   // the lanes' 8 sums each, once the rounds are over
  SSR_REGS(SsrBssAcc, regs, blk);
  SSR_PHASE(blk, regs, {
    SSR_UNROLL
    for (int j = 0; j < 8; ++j) R.a[j] = 0.0;
  });
  for (int64_t s0 = a; s0 < b; s0 += SSR_ALIGN_SUB) {
    SSR_PHASE(blk, regs, {
      for (int i = tid; i < SSR_ALIGN_SUB; i += NT) {
        const int64_t u = s0 + i;
        xs[ssr_bss_pad(i)] = u < b ? (double)x[u] : 0.0;
      }
      for (int i = tid; i < SSR_ALIGN_SUB + 8 * G; i += NT) {
        const int64_t u = s0 + d0 + i;
        ys[ssr_bss_pad(i)] = (u >= 0 && u < ny) ? (double)y[u] : 0.0;
      }
    });
    SSR_PHASE(blk, regs, {
      const int g = tid % G, s = tid / G, q0 = s * Q, q1 = (q0 + Q < QN) ? q0 + Q : QN;
      if (s < S && q0 < q1) ssr_bss_corr_run(xs, ys, q0, q1, g, R.a);
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
    double* o = p.cpart + unit * NL + l0;
    for (int kk = tid; kk < nl; kk += NT) {
      double v = 0.0;
      for (int s = 0; s < S; ++s) v += part[(s * G + (kk >> 3)) * 8 + (kk & 7)];
      o[kk] = v;
    }
  });
  if (lb == 0) {
    // the tile's share of lag +L and of the energies: the estimate's samples past the target's end belong to the target's last tile
    const int64_t by = (k == ssr_align_tiles(nx) - 1) ? ny : ((ny < a + SSR_ALIGN_TILE) ? ny : a + SSR_ALIGN_TILE);
    SSR_PHASE(blk, regs, {
      double ex = 0.0, ey = 0.0, cl = 0.0;
      for (int64_t u = a + tid; u < b; u += NT) {
        const double v = (double)x[u];
        ex = ssr_fma(v, v, ex);
        if (u + L < ny) cl = ssr_fma(v, (double)y[u + L], cl);
      }
      for (int64_t u = a + tid; u < by; u += NT) { const double v = (double)y[u]; ey = ssr_fma(v, v, ey); }
      SSR_WAVE_SUM_STORE(tid, NT, ex, red);
      SSR_WAVE_SUM_STORE(tid, NT, ey, red + 4);
      SSR_WAVE_SUM_STORE(tid, NT, cl, red + 8);
    });
    SSR_PHASE(blk, regs, {
      if (tid == 0) {
        p.epart[2 * unit] = red[0] + red[1] + red[2] + red[3];
        p.epart[2 * unit + 1] = red[4] + red[5] + red[6] + red[7];
        p.cpart[unit * NL + NL - 1] = red[8] + red[9] + red[10] + red[11];
      }
    });
  }
}

// the place of lag index i (lag i - L) in the scan order 0, +1, -1, +2, -2, ...
SSR_HD int ssr_align_rank(int i, int L) { const int d = i - L; return d > 0 ? 2 * d - 1 : -2 * d; }

// c of lag index i of a pair: its nt tile partials from row pt on, in tile order
SSR_HD double ssr_align_lag_sum(const double* cpart, int64_t pt, int64_t nt, int NL, int i) {
  double v = 0.0;
  for (int64_t q = 0; q < nt; ++q) v += cpart[(pt + q) * NL + i];
  return v;
}

// ---- pick for pair e: one wave.  LDS: mx [128], hs [SSR_ALIGN_TAPS], st [8] doubles.
// st[0]: the peak's lag index, st[1..3]: c at the lags around it, st[4], st[5]: Ex, Ey, st[6]: δ, st[7]: Σ s w
template <typename BLK> SSR_BODY void ssr_align_pick_body(const SsrAlignParams& p, BLK& blk, int e, double* mx, double* hs, double* st) {
  const int L = p.L, NL = 2 * L + 1;
  const int64_t nx = p.tgt_len[p.tgt_index[e]], ny = p.est_len[e], pt = p.pair_tile[e], nt = p.pair_tile[e + 1] - pt;
  SSR_REGS(int, regs, blk);
  SSR_WPHASE(blk, regs, {
    double best = -(double)INFINITY;
    int bi = L, br = 0x7fffffff;
    for (int i = tid; i < NL; i += 64) {
      const double v = ssr_align_lag_sum(p.cpart, pt, nt, NL, i);
      const int r = ssr_align_rank(i, L);
      if (v > best || (v == best && r < br)) { best = v; bi = i; br = r; }
      if (p.c) p.c[(int64_t)e * NL + i] = v;
    }
    mx[tid] = best; mx[64 + tid] = (double)bi;
  });
  SSR_WPHASE(blk, regs, {
    if (tid == 0) {
      double best = -(double)INFINITY;
      int bi = L, br = 0x7fffffff;
      for (int l = 0; l < 64; ++l) {
        const int i = (int)mx[64 + l], r = ssr_align_rank(i, L);
        if (mx[l] > best || (mx[l] == best && r < br)) { best = mx[l]; bi = i; br = r; }
      }
      st[0] = (double)bi;
    }
  });
  SSR_WPHASE(blk, regs, {
    const int bi = (int)st[0];
    if (tid < 3) {
      const int i = bi - 1 + tid;
      st[1 + tid] = (i >= 0 && i < NL) ? ssr_align_lag_sum(p.cpart, pt, nt, NL, i) : 0.0;
    } else if (tid < 5) {
      double v = 0.0;
      for (int64_t q = 0; q < nt; ++q) v += p.epart[2 * (pt + q) + (tid - 3)];
      st[1 + tid] = v;
    }
  });
  SSR_WPHASE(blk, regs, {
    if (tid == 0) {
      const int bi = (int)st[0];
      const double cm = st[1], c0 = st[2], cp = st[3], ex = st[4], ey = st[5];
      const bool ok = nx > 0 && ny > 0 && ex != 0.0 && ey != 0.0 && c0 > 0.0;
      const bool edge = ok && (bi == 0 || bi == NL - 1);
      double delta = 0.0;
      if (ok && !edge) {
        const double den = (cm - 2.0 * c0) + cp, v = 0.5 * (cm - cp) / den;
        if (den != 0.0 && den - den == 0.0 && v == v) delta = v < -0.5 ? -0.5 : (v > 0.5 ? 0.5 : v);
      }
      double* o = p.rows + (int64_t)e * SSR_ALIGN_COLS;
      o[0] = ok ? (double)(bi - L) : 0.0;
      o[1] = delta;
      o[2] = ok ? c0 / sqrt(ex * ey) : (double)NAN;
      o[3] = edge ? 1.0 : 0.0;
      st[6] = delta;
    }
  });
  SSR_WPHASE(blk, regs, {
    if (tid < SSR_ALIGN_TAPS) {
      const double delta = st[6];
      const int m = tid - SSR_ALIGN_HALF;
      if (delta == 0.0) {
        hs[tid] = m == 0 ? 1.0 : 0.0;
      } else {
        const double u = (double)m - delta, s = ((m & 1) ? 1.0 : -1.0) * sin(M_PI * delta) / (M_PI * u);
        hs[tid] = s * (0.5 * (1.0 + cos(M_PI * u / (double)(SSR_ALIGN_HALF + 1))));
      }
    }
  });
  SSR_WPHASE(blk, regs, {
    if (tid == 0) {
      double v = 0.0;
      for (int m = 0; m < SSR_ALIGN_TAPS; ++m) v += hs[m];
      st[7] = v;
    }
  });
  SSR_WPHASE(blk, regs, {
    if (tid < SSR_ALIGN_TAPS) p.taps[(int64_t)e * SSR_ALIGN_TAPS + tid] = hs[tid] / st[7];
  });
}

// 16 bytes from / to a 16-byte aligned address
template <typename E> struct SsrAlignV16 { E v[16 / sizeof(E)]; };
template <typename E> SSR_DEV bool ssr_align_is16(const E* q) { return ((uintptr_t)q & 15) == 0; }

// ---- shift for grid block gidx.  LDS: ysh [SSR_ALIGN_S_LDS], hs [SSR_ALIGN_TAPS] doubles.  `out` does not overlap the estimates.
template <typename TE, typename BLK> SSR_BODY void ssr_align_shift_body(const SsrAlignParams& p, BLK& blk, int64_t gidx, double* ysh, double* hs) {
  const int NT = SSR_ALIGN_NT, V = 16 / (int)sizeof(TE);
  const int e = ssr_prefix_find(p.pair_out, p.n_est, gidx);
  const int64_t ny = p.est_len[e], w0 = (gidx - p.pair_out[e]) * SSR_ALIGN_OUT;
  const int64_t d = (int64_t)p.rows[(int64_t)e * SSR_ALIGN_COLS];
  const bool frac = p.subsample && p.rows[(int64_t)e * SSR_ALIGN_COLS + 1] != 0.0;
  const TE* y = (const TE*)p.est + p.est_off[e];
  TE* z = (TE*)p.out + p.out_off[e];
  SSR_REGS(int, regs, blk);
  if (!frac) {
    SSR_PHASE(blk, regs, {
      const int64_t t0 = w0 + 8 * tid, s0 = t0 + d;
      if (t0 < ny) {
        TE v[8];
        const bool whole = t0 + 8 <= ny;
        if (whole && s0 >= 0 && s0 + 8 <= ny && ssr_align_is16(y + s0)) {
          SSR_UNROLL
          for (int j = 0; j < 8; j += V) {
            SsrAlignV16<TE> q;
            memcpy(&q, __builtin_assume_aligned(y + s0 + j, 16), 16);
            SSR_UNROLL
            for (int i = 0; i < V; ++i) v[j + i] = q.v[i];
          }
        } else {
          SSR_UNROLL
          for (int j = 0; j < 8; ++j) v[j] = (s0 + j >= 0 && s0 + j < ny) ? y[s0 + j] : (TE)0;
        }
        if (whole && ssr_align_is16(z + t0)) {
          SSR_UNROLL
          for (int j = 0; j < 8; j += V) {
            SsrAlignV16<TE> q;
            SSR_UNROLL
            for (int i = 0; i < V; ++i) q.v[i] = v[j + i];
            memcpy(__builtin_assume_aligned(z + t0 + j, 16), &q, 16);
          }
        } else {
          SSR_UNROLL
          for (int j = 0; j < 8; ++j)
            if (t0 + j < ny) z[t0 + j] = v[j];
        }
      }
    });
    return;
  }
  // staged sample i is y[w0 + d - SSR_ALIGN_HALF + i]: output j of the lane reads i = 8 tid + j + mm for tap mm = m + SSR_ALIGN_HALF
  SSR_PHASE(blk, regs, {
    for (int i = tid; i < SSR_ALIGN_OUT + 2 * SSR_ALIGN_HALF; i += NT) {
      const int64_t u = w0 + d - SSR_ALIGN_HALF + i;
      ysh[ssr_bss_pad(i)] = (u >= 0 && u < ny) ? (double)y[u] : 0.0;
    }
    if (tid < SSR_ALIGN_TAPS) hs[tid] = p.taps[(int64_t)e * SSR_ALIGN_TAPS + tid];
  });
  SSR_PHASE(blk, regs, {
    const int64_t t0 = w0 + 8 * tid;
    if (t0 < ny) {
      double w[8 + 2 * SSR_ALIGN_HALF];
      double acc[8];
      SSR_UNROLL
      for (int g = 0; g < (8 + 2 * SSR_ALIGN_HALF) / 8; ++g) {
        const int at = ssr_bss_pad(8 * tid + 8 * g);
        SSR_UNROLL
        for (int j = 0; j < 8; ++j) w[8 * g + j] = ysh[at + j];
      }
      SSR_UNROLL
      for (int j = 0; j < 8; ++j) acc[j] = 0.0;
      SSR_UNROLL
      for (int mm = 0; mm < SSR_ALIGN_TAPS; ++mm) {
        const double h = hs[mm];
        SSR_UNROLL
        for (int j = 0; j < 8; ++j) acc[j] = ssr_fma(h, w[j + mm], acc[j]);
      }
      SSR_UNROLL
      for (int j = 0; j < 8; ++j)
        if (t0 + j < ny) z[t0 + j] = (TE)acc[j];
    }
  });
}
