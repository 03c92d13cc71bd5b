// Kernel bodies of the modulation family (the speech-to-reverberation modulation energy ratio, SRMR: Falk, Zheng & Chan 2010, and a
// modulation-spectrum distance), restated in DESIGN §24.  Signals are the n_tgt targets followed by the n_est estimates, float32 or
// float64 read in their own dtype; all arithmetic is float64.
//
//   filterbank  §23's complex gammatone (ssr_auditory.h), unchanged: |z_c| is the Hilbert envelope of band c
//   envelope    hop-blocks of hop_e samples: NB = len / hop_e for len >= 2 hop_e (else 0); env[m][c] = sqrt(B[m][c] / hop_e), B the
//               block sum of |z_c|^2 in sample order (sweep 2 of §23)
//   bank        K = 8 second-order band-passes per band, mod[k] = (b0, b1, b2, a1, a2), run on env at the rate fs / hop_e from the
//               zero state in transposed direct form II: y = b0 x + z0, z0 = b1 x - a1 y + z1, z1 = b2 x - a2 y
//   frames      W = 4 S samples every S, window w [W]: F = 1 + (NB - W) / S for NB >= W (else 0);
//               E_f[c][k] = sum_i (w[i] y[f S + i])^2 in sample order; Ebar[c][k] = (sum_f E_f) / F in frame order
//   srmr        e_c = sum_k Ebar[c][k]; c90: the lowest band whose running sum of e_c exceeds 0.9 of the total; K* = kstar[c90];
//               srmr = sum_c sum_{k < 4} Ebar / sum_c sum_{4 <= k < K*} Ebar
//   pair        f = sum Ebar_target / sum Ebar_estimate; top = max Ebar_target, floor = 10 log10 top - R;
//               D = max(10 log10 Ebar, floor) (the estimate's Ebar times f); mod_dist = sqrt(mean (D_e - D_t)^2) over all cells, over
//               the bands c >= split and over those below; srmr_diff = srmr_e - srmr_t
//   NaN         F = 0, a silent signal, a zero denominator: that signal's srmr; a target without frames or energy, a level factor
//               that is not finite: every value of the pair.  No infinity leaves a kernel
//
//   geometry, sweeps, scan   ssr_auditory.h's bodies as they are, with hop = hop_e
//   bank       one workgroup per signal, lane = (band c, modulation band k), at more than 32 bands two bands per lane.  The block
//              sums are staged through an LDS tile of SSR_MOD_TILE rows [m][C], the square root taken once per cell while staging;
//              the eight k-lanes of a band read one address.  The biquad runs sequentially in m in registers.  W = 4 S: a sample
//              belongs to exactly four frames, whose accumulators rotate every S samples; the window comes from an LDS table
//   signal     one workgroup per signal: e_c per lane, then one lane walks the bands in order
//   pair       one workgroup per estimate: a band's cells per lane in k order, then one lane walks the bands in order
//
// Every sum shape depends on the signal's own length, hop_e, S and the band count only: a signal and a pair give the same bits alone,
// in any batch and at any position.  No atomics.  All bodies compile on the host too (SSR_HOST_EMU, tests/emu/modulation_emu.cpp).
#pragma once
#include "ssr_auditory.h"

#define SSR_MOD_NT 256                     // threads of every workgroup of the family
#define SSR_MOD_K 8                        // modulation bands
#define SSR_MOD_TILE 32                    // envelope rows of the bank's staging tile
#define SSR_MOD_MAX_S 1024                 // frame step in envelope samples: the window table holds 4 S values
#define SSR_MOD_TAB (SSR_MOD_K * 5)        // the biquads; the window follows them in the table of a call
#define SSR_MOD_SIG_COLS 4                 // srmr, K*, c90, sum Ebar
#define SSR_MOD_PAIR_COLS 4                // srmr_diff, mod_dist, mod_dist_hf, mod_dist_lf
static_assert(SSR_MOD_NT == SSR_AUD_NT, "the sweeps are ssr_auditory.h's");
static_assert(SSR_MOD_NT == 32 * SSR_MOD_K, "32 bands of 8 lanes fill a workgroup");

SSR_HD int ssr_mod_frames(int nb, int S) { return nb >= 4 * S ? 1 + (nb - 4 * S) / S : 0; }
// x where it is finite, else NaN
SSR_HD double ssr_mod_finite(double x) { return x - x == 0.0 ? x : (double)NAN; }

// ---- host: the table of a call, float64: mod [8][5], then the Hamming window of W = 4 S samples
inline void ssr_mod_tables_host(const double* mod, int S, std::vector<double>& tab) {
  const int W = 4 * S;
  tab.assign((size_t)SSR_MOD_TAB + W, 0.0);
  for (int j = 0; j < SSR_MOD_TAB; ++j) tab[j] = mod[j];
  for (int i = 0; i < W; ++i) tab[SSR_MOD_TAB + i] = 0.54 - 0.46 * cos(2.0 * M_PI * (double)i / (double)(W - 1));
}

struct SsrModParams {
  const int32_t* tgt_len;       // [n_tgt] (workspace copy)
  const int32_t* tgt_index;     // [n_est] (workspace copy)
  int n_tgt, n_est;
  int hop, C, S;
  double range_db;
  const int32_t* sig_index;     // [n_sig] signal -> the target that gives its length (the geometry's)
  const int64_t* seg_off;       // [n_sig + 1] segment prefix over signals (the geometry's)
  const double* blk;            // [segments][SSR_AUD_SEG][C] block sums B of sweep 2
  const double* tab;            // [SSR_MOD_TAB + 4 S] (workspace copy)
  const int32_t* kstar;         // [C] (workspace copy)
  const int32_t* split;         // [n_est] first band of the pair's upper part in [0, C], -1: no split (workspace copy)
  double* emod;                 // [n_sig][C][8] Ebar
  double* signal_out;           // [n_sig][SSR_MOD_SIG_COLS]
  double* pair_out;             // [n_est][SSR_MOD_PAIR_COLS]
  double* spectrum_out;         // [n_sig][C][8] or null
};

struct SsrModBankLds { double env[SSR_MOD_TILE * SSR_AUD_MAX_BANDS], win[4 * SSR_MOD_MAX_S]; };
// one (band, modulation band) couple of a lane
struct SsrModCouple {
  double z0, z1;                            // the biquad's state
  double a0, a1, a2, a3;                    // the frames under way: a_j has had j S + pos samples
  double sum;                               // finished frames, in frame order
};
struct SsrModBankRegs {
  SsrModCouple q[2];
  int pos, blocks;                          // the sample's place in its block of S, whole blocks of S passed
};

// one envelope sample through a couple's biquad and into its four frames; w_j: the window at j S + pos
SSR_DEV void ssr_mod_step(SsrModCouple& q, double x, const double* b, double w0, double w1, double w2, double w3) {
  const double y = b[0] * x + q.z0;
  q.z0 = (b[1] * x - b[3] * y) + q.z1;
  q.z1 = b[2] * x - b[4] * y;
  const double u0 = w0 * y, u1 = w1 * y, u2 = w2 * y, u3 = w3 * y;
  q.a0 += u0 * u0; q.a1 += u1 * u1; q.a2 += u2 * u2; q.a3 += u3 * u3;
}
// a block of S samples is over: the oldest frame is whole (once three blocks lie behind it), the others move up
SSR_DEV void ssr_mod_rotate(SsrModCouple& q, bool whole) {
  if (whole) q.sum += q.a3;
  q.a3 = q.a2; q.a2 = q.a1; q.a1 = q.a0; q.a0 = 0.0;
}

// ---- bank: workgroup s turns the block sums of signal s into Ebar [C][8].  TWO: more than 32 bands, lane (c, k) also carries (c + 32, k)
template <bool TWO, typename BLK> SSR_BODY void ssr_mod_bank_body(const SsrModParams& p, BLK& blk, int s, SsrModBankLds& L) {
  constexpr int NT = SSR_MOD_NT, K = SSR_MOD_K, TM = SSR_MOD_TILE;
  const int C = p.C, S = p.S, W = 4 * S;
  const int NB = ssr_aud_blocks(p.tgt_len[p.sig_index[s]], p.hop), F = ssr_mod_frames(NB, S);
  const int M = F > 0 ? (F - 1) * S + W : 0;                       // the samples the frames cover: M <= NB
  const double* B = p.blk + p.seg_off[s] * SSR_AUD_SEG * C;
  const double hop = (double)p.hop;
  SSR_REGS(SsrModBankRegs, regs, blk);
  SSR_PHASE(blk, regs, {
    for (int i = tid; i < W; i += NT) L.win[i] = p.tab[SSR_MOD_TAB + i];
    SSR_UNROLL for (int j = 0; j < 2; ++j) {
      R.q[j].z0 = R.q[j].z1 = 0.0;
      R.q[j].a0 = R.q[j].a1 = R.q[j].a2 = R.q[j].a3 = R.q[j].sum = 0.0;
    }
    R.pos = 0; R.blocks = 0;
  });
  for (int m0 = 0; m0 < M; m0 += TM) {
    const int tn = M - m0 < TM ? M - m0 : TM;
    SSR_PHASE(blk, regs, {
      for (int i = tid; i < tn * C; i += NT) L.env[i] = sqrt(B[(int64_t)m0 * C + i] / hop);
    });
    SSR_PHASE(blk, regs, {
      const int k = tid & (K - 1), c = tid / K;
      if (c < C) {
        const bool two = TWO && c + 32 < C;
        double b[5];
        SSR_UNROLL for (int j = 0; j < 5; ++j) b[j] = p.tab[k * 5 + j];
        int pos = R.pos, blocks = R.blocks;
        for (int i = 0; i < tn; ++i) {
          const double w0 = L.win[pos], w1 = L.win[S + pos], w2 = L.win[2 * S + pos], w3 = L.win[3 * S + pos];
          ssr_mod_step(R.q[0], L.env[i * C + c], b, w0, w1, w2, w3);
          if (two) ssr_mod_step(R.q[1], L.env[i * C + c + 32], b, w0, w1, w2, w3);
          if (++pos == S) {
            ssr_mod_rotate(R.q[0], blocks >= 3);
            if (two) ssr_mod_rotate(R.q[1], blocks >= 3);
            pos = 0; ++blocks;
          }
        }
        R.pos = pos; R.blocks = blocks;
      }
    });
  }
  SSR_PHASE(blk, regs, {
    const int k = tid & (K - 1), c = tid / K;
    double* out = p.emod + (int64_t)s * C * K;
    if (c < C) out[c * K + k] = F > 0 ? R.q[0].sum / (double)F : (double)NAN;
    if (TWO && c + 32 < C) out[(c + 32) * K + k] = F > 0 ? R.q[1].sum / (double)F : (double)NAN;
  });
}

struct SsrModSignalLds { double e[SSR_AUD_MAX_BANDS], lo[SSR_AUD_MAX_BANDS], hi[SSR_AUD_MAX_BANDS][4]; };

// ---- signal: workgroup s scores signal s on its own, SSR_MOD_NT threads
template <typename BLK> SSR_BODY void ssr_mod_signal_body(const SsrModParams& p, BLK& blk, int s, SsrModSignalLds& L) {
  constexpr int K = SSR_MOD_K;
  const int C = p.C;
  const double* E = p.emod + (int64_t)s * C * K;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    if (tid < C) {
      double lo = 0.0, all = 0.0;
      SSR_UNROLL for (int k = 0; k < K; ++k) {
        const double v = E[tid * K + k];
        all += v;
        if (k < 4) lo += v; else L.hi[tid][k - 4] = v;
      }
      L.e[tid] = all; L.lo[tid] = lo;
    }
    if (p.spectrum_out)
      for (int i = tid; i < C * K; i += SSR_MOD_NT) p.spectrum_out[(int64_t)s * C * K + i] = ssr_mod_finite(E[i]);
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      double total = 0.0;
      for (int c = 0; c < C; ++c) total += L.e[c];
      double* out = p.signal_out + (int64_t)s * SSR_MOD_SIG_COLS;
      // (F = 0: total is NaN; a sum that overflowed is the signal's NaN rule too)
      if (!(total > 0.0) || total - total != 0.0) {
        out[0] = (double)NAN; out[1] = (double)NAN; out[2] = (double)NAN; out[3] = total == 0.0 ? 0.0 : (double)NAN;
      } else {
        const double bar = 0.9 * total;
        int c90 = C - 1;
        double run = 0.0;
        for (int c = 0; c < C; ++c) {
          run += L.e[c];
          if (run > bar) { c90 = c; break; }
        }
        const int ks = p.kstar[c90];
        double num = 0.0, den = 0.0;
        for (int c = 0; c < C; ++c) {
          num += L.lo[c];
          double d = 0.0;
          for (int k = 4; k < ks; ++k) d += L.hi[c][k - 4];
          den += d;
        }
        out[0] = den > 0.0 ? ssr_mod_finite(num / den) : (double)NAN;
        out[1] = (double)ks; out[2] = (double)c90; out[3] = total;
      }
    }
  });
}

struct SsrModPairLds { double top[SSR_AUD_MAX_BANDS], sq[SSR_AUD_MAX_BANDS], res[2]; };

// ---- pair: workgroup e scores estimate e against its target, SSR_MOD_NT threads
template <typename BLK> SSR_BODY void ssr_mod_pair_body(const SsrModParams& p, BLK& blk, int e, SsrModPairLds& L) {
  constexpr int K = SSR_MOD_K;
  const int C = p.C, sy = p.n_tgt + e, sx = p.tgt_index[e];
  const double* Et = p.emod + (int64_t)sx * C * K;
  const double* Ee = p.emod + (int64_t)sy * C * K;
  const double* st = p.signal_out + (int64_t)sx * SSR_MOD_SIG_COLS;
  const double* se = p.signal_out + (int64_t)sy * SSR_MOD_SIG_COLS;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    if (tid < C) {
      double mx = 0.0;
      SSR_UNROLL for (int k = 0; k < K; ++k) { const double v = Et[tid * K + k]; mx = v > mx ? v : mx; }
      L.top[tid] = mx;
    }
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      double mx = 0.0;
      for (int c = 0; c < C; ++c) mx = L.top[c] > mx ? L.top[c] : mx;
      const double f = st[3] / se[3];                     // (a silent estimate: infinity, the pair's NaN rule)
      L.res[0] = mx; L.res[1] = f;
    }
  });
  SSR_PHASE(blk, regs, {
    const double top = L.res[0], f = L.res[1];
    if (tid < C) {
      const double floor_db = 10.0 * log10(top) - p.range_db;
      double a = 0.0;
      SSR_UNROLL for (int k = 0; k < K; ++k) {
        const double dt = 10.0 * log10(Et[tid * K + k]), de = 10.0 * log10(Ee[tid * K + k] * f);
        const double d = (de > floor_db ? de : floor_db) - (dt > floor_db ? dt : floor_db);      // (Ebar = 0: -inf -> the floor)
        a += d * d;
      }
      L.sq[tid] = a;
    }
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      const double top = L.res[0], f = L.res[1];
      const bool ok = st[3] > 0.0 && top > 0.0 && f > 0.0 && f - f == 0.0;
      const int sp = p.split[e];
      double all = 0.0, lf = 0.0, hf = 0.0;
      for (int c = 0; c < C; ++c) {
        all += L.sq[c];
        if (c < sp) lf += L.sq[c]; else hf += L.sq[c];
      }
      const int n_lf = sp >= 0 ? sp : 0, n_hf = sp >= 0 ? C - sp : 0;
      double* out = p.pair_out + (int64_t)e * SSR_MOD_PAIR_COLS;
      out[0] = ok ? ssr_mod_finite(se[0] - st[0]) : (double)NAN;
      out[1] = ok ? ssr_mod_finite(sqrt(all / (double)(C * K))) : (double)NAN;
      out[2] = ok && n_hf > 0 ? ssr_mod_finite(sqrt(hf / (double)(n_hf * K))) : (double)NAN;
      out[3] = ok && n_lf > 0 ? ssr_mod_finite(sqrt(lf / (double)(n_lf * K))) : (double)NAN;
    }
  });
}
