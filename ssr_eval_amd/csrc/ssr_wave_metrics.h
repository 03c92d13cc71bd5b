// Kernel bodies of the waveform metrics: SNR, SI-SDR (Le Roux et al. 2019, zero-mean) and segmental SNR (Loizou,
// Speech Enhancement, §11.1, comp_snr.m), on the signals as they lie - float32 or float64 targets and estimates, read in their
// own dtype and accumulated in float64.
//
//   geometry   one workgroup (ssr_pairs.h): runs of consecutive pairs that name the same target, tile prefix sums over runs and
//              over pairs, the frame window
//   pass 1     one workgroup per (run, tile): the target's tile sums once, then for each estimate of the run Σy, the centred
//              co-moment and Σ(x - y)^2 about the tile means, and seg_j of the frames that start in the tile (a frame's L - R halo
//              is read past the tile); one partial record per (pair, tile)
//   finalize 1 one thread per pair: the tiles in ascending order, means and co-moments by Chan et al.'s pairwise update;
//              snr, seg_snr, and the pair's means and alpha for pass 2
//   pass 2     (SI-SDR only) one workgroup per (run, tile): alpha x0 - y0 sample by sample, Σ(alpha x0)^2 and Σ(alpha x0 - y0)^2
//   finalize 2 one thread per pair: the pass-2 tiles in ascending order, si_sdr
//
// The tile partition depends on the pair's own length (and fs) only, every sum has a fixed order and there are no atomics: a
// pair gives the same bits alone, in any batch and in any run.  All bodies compile on the host too (SSR_HOST_EMU,
// tests/emu/wave_emu.cpp).
#pragma once
#include "ssr_pairs.h"

#define SSR_WAVE_SNR 1
#define SSR_WAVE_SI_SDR 2
#define SSR_WAVE_SEG_SNR 4
#define SSR_WAVE_NT 256                    // threads of every workgroup
static_assert(SSR_WAVE_NT == SSR_PAIRS_NT, "the geometry workgroup is ssr_run_geometry_body's");
#define SSR_WAVE_TILE_MIN 4096             // a tile is the smallest whole number of hops with at least this many samples
#define SSR_WAVE_EPS 2.220446049250313e-16 // np.finfo(np.float64).eps
#define SSR_WAVE_SEG_LO -10.0
#define SSR_WAVE_SEG_HI 35.0
#define SSR_WAVE_P1 7                      // doubles of a pass-1 record: Σx, Σy, Σ(x-x̄)², Σ(x-x̄)(y-ȳ), Σx², Σ(x-y)², Σseg
#define SSR_WAVE_P2 2                      // doubles of a pass-2 record: Σs², Σ(s-y0)²

// frame length L = 30 ms rounded half up, hop R = L // 4, tile = whole hops
SSR_HD int ssr_wave_frame_len(int fs) { return (int)((3 * (int64_t)fs + 50) / 100); }
SSR_HD int ssr_wave_hop(int fs) { return ssr_wave_frame_len(fs) / 4; }
SSR_HD int ssr_wave_frames_per_tile(int fs) {
  const int R = ssr_wave_hop(fs);
  return R > 0 ? (SSR_WAVE_TILE_MIN + R - 1) / R : 0;
}
SSR_HD int64_t ssr_wave_tile_len(int fs) {
  const int R = ssr_wave_hop(fs);
  return R > 0 ? (int64_t)ssr_wave_frames_per_tile(fs) * R : SSR_WAVE_TILE_MIN;
}
SSR_HD int64_t ssr_wave_tiles(int64_t n, int fs) { const int64_t T = ssr_wave_tile_len(fs); return (n + T - 1) / T; }
// frames of a signal of n samples: max(0, (n - L) // R), one fewer than the number of whole frames (comp_snr.m's loop count)
SSR_HD int64_t ssr_wave_frames(int64_t n, int fs) {
  const int L = ssr_wave_frame_len(fs), R = ssr_wave_hop(fs);
  return (R > 0 && n >= L) ? (n - L) / R : 0;
}

struct SsrWaveParams {
  const void* tgt;              // targets (clean), float32 or float64
  const int64_t* tgt_off;       // [n_tgt] device
  const void* est;              // estimates, float32 or float64
  const int64_t* est_off;       // [n_est] device
  const int32_t* tgt_len;       // [n_tgt] (workspace copy)
  const int32_t* tgt_index;     // [n_est] (workspace copy)
  int n_tgt, n_est, n_runs;
  int which, fs, L, R, fpt;     // fpt: frames per tile
  int64_t tile;                 // samples per tile
  int32_t* run_start;           // [n_runs + 1] first pair of each run of consecutive pairs with one target; [n_runs] = n_est
  int64_t* run_tile;            // [n_runs + 1] tile prefix over runs (the pass grids)
  int64_t* pair_tile;           // [n_est + 1] tile prefix over pairs (the partial records)
  double* win;                  // [L] 0.5 (1 - cos(2 pi (i + 1) / (L + 1)))
  double* part1;                // [pair_tile[n_est]][SSR_WAVE_P1]
  double* part2;                // [pair_tile[n_est]][SSR_WAVE_P2]
  double* fin;                  // [n_est][3] x̄, ȳ, alpha
  double* out;                  // [n_est][popcount(which)]
};

// ---- geometry: ssr_run_geometry_body on the tiles of each target
template <typename BLK> SSR_BODY void ssr_wave_geometry_body(const SsrWaveParams& p, BLK& blk, int64_t* sums) {
  ssr_run_geometry_body(p.tgt_len, p.tgt_index, p.n_est, [&](int32_t n) { return ssr_wave_tiles(n, p.fs); },
                        p.run_start, p.run_tile, p.pair_tile, p.win, p.L, blk, sums);
}

// (run, tile k) of pass-grid block g, its target and the tile's samples [a, a + m)
struct SsrWaveTile { int r, e0, e1, t; int64_t k, a, m, n; };
SSR_HD SsrWaveTile ssr_wave_tile_of(const SsrWaveParams& p, int64_t g) {
  SsrWaveTile w;
  w.r = ssr_prefix_find(p.run_tile, p.n_runs, g);
  w.k = g - p.run_tile[w.r];
  w.e0 = p.run_start[w.r]; w.e1 = p.run_start[w.r + 1];
  w.t = p.tgt_index[w.e0];
  w.n = p.tgt_len[w.t];
  w.a = w.k * p.tile;
  w.m = (w.n - w.a < p.tile) ? w.n - w.a : p.tile;
  return w;
}

// ---- pass 1 for grid block g.  LDS: red[4][4], tst[3], seg[2][4] doubles (wave-indexed).
template <typename TT, typename TE, typename BLK>
SSR_BODY void ssr_wave_pass1_body(const SsrWaveParams& p, BLK& blk, int64_t g, double* red, double* tst, double* seg) {
  const int NT = SSR_WAVE_NT;
  const SsrWaveTile w = ssr_wave_tile_of(p, g);
  const TT* x = (const TT*)p.tgt + p.tgt_off[w.t];
  const int64_t a = w.a, b = w.a + w.m;
  const double inv_m = 1.0 / (double)w.m;
  const bool mom = (p.which & SSR_WAVE_SI_SDR) != 0, frames = (p.which & SSR_WAVE_SEG_SNR) != 0;
  const int64_t j0 = w.k * p.fpt, M = ssr_wave_frames(w.n, p.fs);
  const int64_t j1 = (j0 + p.fpt < M) ? j0 + p.fpt : M;
  const int rounds = frames ? (p.fpt + 3) / 4 : 0;
  SSR_REGS(int, regs, blk);
  // the target's tile: Σx, Σx², then Σ(x - x̄_tile)²
  SSR_PHASE(blk, regs, {
    double s = 0.0, s2 = 0.0;
    for (int64_t i = a + tid; i < b; i += NT) { const double v = (double)x[i]; s += v; s2 += v * v; }
    SSR_WAVE_SUM_STORE(tid, NT, s, red);
    SSR_WAVE_SUM_STORE(tid, NT, s2, red + 4);
  });
  SSR_PHASE(blk, regs, {
    const double mx = (red[0] + red[1] + red[2] + red[3]) * inv_m;
    double c = 0.0;
    if (mom)
      for (int64_t i = a + tid; i < b; i += NT) { const double v = (double)x[i] - mx; c += v * v; }
    SSR_WAVE_SUM_STORE(tid, NT, c, red + 8);
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      tst[0] = red[0] + red[1] + red[2] + red[3];
      tst[1] = red[4] + red[5] + red[6] + red[7];
      tst[2] = red[8] + red[9] + red[10] + red[11];
    }
  });
  for (int e = w.e0; e < w.e1; ++e) {
    const TE* y = (const TE*)p.est + p.est_off[e];
    SSR_PHASE(blk, regs, {
      double s = 0.0;
      if (mom)
        for (int64_t i = a + tid; i < b; i += NT) s += (double)y[i];
      SSR_WAVE_SUM_STORE(tid, NT, s, red);
      if ((tid & 63) == 0) seg[ssr_wave_of(tid)] = 0.0;
    });
    SSR_PHASE(blk, regs, {
      const double mx = tst[0] * inv_m, my = (red[0] + red[1] + red[2] + red[3]) * inv_m;
      double cxy = 0.0, dd = 0.0;
      for (int64_t i = a + tid; i < b; i += NT) {
        const double xv = (double)x[i], yv = (double)y[i], d = xv - yv;
        if (mom) cxy += (xv - mx) * (yv - my);
        dd += d * d;
      }
      SSR_WAVE_SUM_STORE(tid, NT, cxy, red + 4);
      SSR_WAVE_SUM_STORE(tid, NT, dd, red + 8);
    });
    // frames j0 + 4 q + wave: S_j = Σ (w x)², N_j = Σ (w (x - y))² over [jR, jR + L), one wave per frame
    for (int q = 0; q < rounds; ++q) {
      SSR_WPHASE(blk, regs, {
        const int64_t j = j0 + 4 * q + ssr_wave_of(tid);
        double s = 0.0, nn = 0.0;
        if (j < j1) {
          const TT* xf = x + j * p.R;
          const TE* yf = y + j * p.R;
          for (int i = tid & 63; i < p.L; i += 64) {
            const double xv = (double)xf[i], wv = p.win[i];
            const double u = wv * xv, v = wv * (xv - (double)yf[i]);
            s += u * u; nn += v * v;
          }
        }
        SSR_WAVE_SUM_STORE(tid, 64, s, red + 12);
        SSR_WAVE_SUM_STORE(tid, 64, nn, seg + 4);
      });
      SSR_WPHASE(blk, regs, {
        const int wv = ssr_wave_of(tid);
        if ((tid & 63) == 0 && j0 + 4 * q + wv < j1) {
          double v = 10.0 * log10(red[12 + wv] / (seg[4 + wv] + SSR_WAVE_EPS) + SSR_WAVE_EPS);
          v = v < SSR_WAVE_SEG_LO ? SSR_WAVE_SEG_LO : (v > SSR_WAVE_SEG_HI ? SSR_WAVE_SEG_HI : v);
          seg[wv] += v;
        }
      });
    }
    // the frame rounds synchronise their own wave only: every wave's seg[] is complete past this barrier
    SSR_PHASE(blk, regs, {});
    SSR_PHASE(blk, regs, {
      if (tid == 0) {
        double* o = p.part1 + (p.pair_tile[e] + w.k) * SSR_WAVE_P1;
        o[0] = tst[0];
        o[1] = red[0] + red[1] + red[2] + red[3];
        o[2] = tst[2];
        o[3] = red[4] + red[5] + red[6] + red[7];
        o[4] = tst[1];
        o[5] = red[8] + red[9] + red[10] + red[11];
        o[6] = seg[0] + seg[1] + seg[2] + seg[3];
      }
    });
  }
}

// ---- finalize 1: pair e.  Chan, Golub & LeVeque's pairwise update, tile after tile.
SSR_HD void ssr_wave_finalize1(const SsrWaveParams& p, int e) {
  const int64_t n = p.tgt_len[p.tgt_index[e]];
  const int n_out = ssr_which_count(p.which);
  double* out = p.out + (int64_t)e * n_out;
  double na = 0.0, mx = 0.0, my = 0.0, m2x = 0.0, cxy = 0.0, sxx = 0.0, sdd = 0.0, sseg = 0.0;
  const int64_t nt = p.pair_tile[e + 1] - p.pair_tile[e];
  for (int64_t k = 0; k < nt; ++k) {
    const double* r = p.part1 + (p.pair_tile[e] + k) * SSR_WAVE_P1;
    const int64_t a = k * p.tile;
    const double nb = (double)((n - a < p.tile) ? n - a : p.tile);
    const double mxb = r[0] / nb, myb = r[1] / nb;
    const double nn = na + nb, dx = mxb - mx, dy = myb - my, f = na * nb / nn;
    mx += dx * (nb / nn); my += dy * (nb / nn);
    m2x += r[2] + dx * dx * f;
    cxy += r[3] + dx * dy * f;
    na = nn;
    sxx += r[4]; sdd += r[5]; sseg += r[6];
  }
  const int64_t M = ssr_wave_frames(n, p.fs);
  if (p.which & SSR_WAVE_SNR)
    out[ssr_which_col(p.which, SSR_WAVE_SNR)] = n > 0 ? 10.0 * log10((sxx + SSR_WAVE_EPS) / (sdd + SSR_WAVE_EPS)) : (double)NAN;
  if (p.which & SSR_WAVE_SEG_SNR) out[ssr_which_col(p.which, SSR_WAVE_SEG_SNR)] = M > 0 ? sseg / (double)M : (double)NAN;
  if (p.which & SSR_WAVE_SI_SDR) {
    p.fin[3 * (int64_t)e + 0] = mx;
    p.fin[3 * (int64_t)e + 1] = my;
    p.fin[3 * (int64_t)e + 2] = (cxy + SSR_WAVE_EPS) / (m2x + SSR_WAVE_EPS);
  }
}

// ---- pass 2 (SI-SDR) for grid block g: s = alpha x0, Σs² and Σ(s - y0)², the residual formed sample by sample.
// LDS: red[2][4] doubles.
template <typename TT, typename TE, typename BLK>
SSR_BODY void ssr_wave_pass2_body(const SsrWaveParams& p, BLK& blk, int64_t g, double* red) {
  const int NT = SSR_WAVE_NT;
  const SsrWaveTile w = ssr_wave_tile_of(p, g);
  const TT* x = (const TT*)p.tgt + p.tgt_off[w.t];
  const int64_t a = w.a, b = w.a + w.m;
  SSR_REGS(int, regs, blk);
  for (int e = w.e0; e < w.e1; ++e) {
    const TE* y = (const TE*)p.est + p.est_off[e];
    const double mx = p.fin[3 * (int64_t)e], my = p.fin[3 * (int64_t)e + 1], al = p.fin[3 * (int64_t)e + 2];
    SSR_PHASE(blk, regs, {
      double ss = 0.0, rr = 0.0;
      for (int64_t i = a + tid; i < b; i += NT) {
        const double s = al * ((double)x[i] - mx), d = s - ((double)y[i] - my);
        ss += s * s; rr += d * d;
      }
      SSR_WAVE_SUM_STORE(tid, NT, ss, red);
      SSR_WAVE_SUM_STORE(tid, NT, rr, red + 4);
    });
    SSR_PHASE(blk, regs, {
      if (tid == 0) {
        double* o = p.part2 + (p.pair_tile[e] + w.k) * SSR_WAVE_P2;
        o[0] = red[0] + red[1] + red[2] + red[3];
        o[1] = red[4] + red[5] + red[6] + red[7];
      }
    });
  }
}

// ---- finalize 2: pair e, the pass-2 tiles in ascending order
SSR_HD void ssr_wave_finalize2(const SsrWaveParams& p, int e) {
  const int64_t n = p.tgt_len[p.tgt_index[e]];
  double ss = 0.0, rr = 0.0;
  for (int64_t g = p.pair_tile[e]; g < p.pair_tile[e + 1]; ++g) { ss += p.part2[g * SSR_WAVE_P2]; rr += p.part2[g * SSR_WAVE_P2 + 1]; }
  p.out[(int64_t)e * ssr_which_count(p.which) + ssr_which_col(p.which, SSR_WAVE_SI_SDR)] =
      n > 0 ? 10.0 * log10((ss + SSR_WAVE_EPS) / (rr + SSR_WAVE_EPS)) : (double)NAN;
}
