// Kernel bodies of the bootstrap of the aggregate (not in the reference): replicates of "mean over speakers of each
// speaker's mean over its files" for every column of the per-file table at once, and their per-column summary.
//
//   means    one workgroup per (replicate b, chunk of SSR_BOOT_NT columns).  For each speaker slot t the workgroup draws the slot's
//            files into LDS, SSR_BOOT_TILE draws at a time: thread i of a tile computes ONE Philox4x32-10 block, counter
//            (b, j / 4, t, 0), and stores the four rows it selects - 256 threads, 256 different blocks, 1,024 draws.  Then the lanes
//            sit across the columns: lane c adds table[row][c] for the tile's rows in draw order, so a gathered row is one
//            contiguous read of the workgroup (the row index is wave-uniform: scalar base, lane offset).  The table is a few MB and
//            is served from L2 / MALL; what limits a lane is the latency of its chain of loads, so the loop is unrolled and the
//            loads of a group are issued before its adds.
//   mask     one workgroup per (64 columns, SSR_BOOT_MASK_ROWS rows): a column with a non-finite table entry gets NaN in every
//            replicate (the same value whichever workgroup writes it: no atomics, no order)
//   summary  one workgroup per column: the B <= 16,384 replicates of the column in LDS (128 KiB), mean and two-pass standard error
//            (ddof 1) in a fixed order, a bitonic sort (padded with +inf to a power of two), then NumPy's linear quantiles
//            pos = q (B - 1) and the exact counts of replicates <= 0 and >= 0 by binary search.
//
// ACCUMULATION ORDER of one replicate of one column: slot t = 0 .. S-1 in turn; inside a slot a = 0, a += x[draw j] for
// j = 0 .. n-1 in draw order; m_t = a / n; r = 0, r += m_t in slot order; replicate = r / S.  One lane owns the whole chain, so
// the bits do not depend on the grid, on the tile size, on K or on the columns beside it.
// All bodies compile on the host too (SSR_HOST_EMU, tests/emu/bootstrap_emu.cpp).
#pragma once
#include "ssr_block.h"

#define SSR_BOOT_UTTERANCE 0              // slot t is speaker t
#define SSR_BOOT_SPEAKER 1                // slot t is a speaker drawn with replacement
#define SSR_BOOT_NT 256                   // threads of a means / mask workgroup (4 waves)
#define SSR_BOOT_TILE (4 * SSR_BOOT_NT)   // draws per index tile: one Philox block of four words per thread
#define SSR_BOOT_MAX_SPK 512              // spk_off travels in the kernel arguments
#define SSR_BOOT_MAX_B 16384              // replicates of a column that fit the summary's LDS
#define SSR_BOOT_MAX_Q 8
#define SSR_BOOT_SUM_NT 1024              // threads of a summary workgroup (16 waves)
#define SSR_BOOT_MASK_ROWS 128            // table rows per mask workgroup

#ifdef SSR_HOST_EMU
#define SSR_BOOT_UNIFORM(x) (x)
static inline uint32_t ssr_boot_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
#else
#define SSR_BOOT_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)      // a value every lane of the wave holds -> a scalar register
SSR_DEV uint32_t ssr_boot_mulhi(uint32_t a, uint32_t b) { return __umulhi(a, b); }
#endif

// Philox4x32-10 (Salmon, Moraes, Dror & Shaw, SC 2011): c[0..3] counter in, four random words out
SSR_DEV void ssr_philox4x32_10(uint32_t* c, uint32_t k0, uint32_t k1) {
  SSR_UNROLL
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = ssr_boot_mulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = ssr_boot_mulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
// a 32-bit word -> an index in [0, n): the high half of the 64-bit product (no rejection; P(i) differs from 1/n by < 2^-32)
SSR_DEV int ssr_boot_pick(uint32_t u, uint32_t n) { return (int)(((uint64_t)u * n) >> 32); }

struct SsrBootParams {
  const double* table;          // [n_rows][n_cols]
  int64_t n_rows;
  int n_cols, n_spk, n_boot, scheme;
  uint32_t key0, key1;
  double* reps;                 // [n_boot][n_cols]
  int32_t spk_off[SSR_BOOT_MAX_SPK + 1];     // rows of speaker s: spk_off[s] .. spk_off[s + 1] - 1
};

struct SsrBootRegs { double acc, total; };

// ---- means: replicate b, columns col0 .. col0 + NT - 1.  LDS: idx [SSR_BOOT_TILE] int, slot_spk [SSR_BOOT_MAX_SPK] int.
template <typename BLK> SSR_BODY void ssr_boot_means_body(const SsrBootParams& p, BLK& blk, int b, int col0, int* idx, int* slot_spk) {
  const int NT = SSR_BOOT_NT, S = p.n_spk, K = p.n_cols;
  SSR_REGS(SsrBootRegs, regs, blk);
  SSR_PHASE(blk, regs, {
    R.total = 0.0;
    if (p.scheme == SSR_BOOT_SPEAKER) {
      for (int q = tid; 4 * q < S; q += NT) {
        uint32_t c[4] = {(uint32_t)b, (uint32_t)q, 0u, 1u};
        ssr_philox4x32_10(c, p.key0, p.key1);
        for (int w = 0; w < 4; ++w)
          if (4 * q + w < S) slot_spk[4 * q + w] = ssr_boot_pick(c[w], (uint32_t)S);
      }
    } else {
      for (int t = tid; t < S; t += NT) slot_spk[t] = t;
    }
  });
  for (int t = 0; t < S; ++t) {
    const int s = SSR_BOOT_UNIFORM(slot_spk[t]);
    const int base = p.spk_off[s], n = p.spk_off[s + 1] - base;
    for (int j0 = 0; j0 < n; j0 += SSR_BOOT_TILE) {
      const int m = n - j0 < SSR_BOOT_TILE ? n - j0 : SSR_BOOT_TILE;      // draws of this tile
      SSR_PHASE(blk, regs, {
        if (j0 == 0) R.acc = 0.0;
        if (4 * tid < m) {
          uint32_t c[4] = {(uint32_t)b, (uint32_t)(j0 / 4 + tid), (uint32_t)t, 0u};
          ssr_philox4x32_10(c, p.key0, p.key1);
          for (int w = 0; w < 4; ++w)
            if (4 * tid + w < m) idx[4 * tid + w] = base + ssr_boot_pick(c[w], (uint32_t)n);
        }
      });
      SSR_PHASE(blk, regs, {
        const int col = col0 + tid;
        if (col < K) {
          const double* x = p.table + col;
          double a = R.acc;
          int j = 0;
          for (; j + 8 <= m; j += 8) {          // eight row requests in flight, then their adds in draw order
            double v[8];
            SSR_UNROLL
            for (int u = 0; u < 8; ++u) v[u] = x[(int64_t)SSR_BOOT_UNIFORM(idx[j + u]) * K];
            SSR_UNROLL
            for (int u = 0; u < 8; ++u) a += v[u];
          }
          for (; j < m; ++j) a += x[(int64_t)SSR_BOOT_UNIFORM(idx[j]) * K];
          R.acc = a;
          if (j0 + m == n) R.total += a / (double)n;
        }
      });
    }
  }
  SSR_PHASE(blk, regs, {
    const int col = col0 + tid;
    if (col < K) p.reps[(int64_t)b * K + col] = R.total / (double)S;
  });
}

// ---- mask: columns col0 .. col0 + 63, rows row0 .. row0 + SSR_BOOT_MASK_ROWS - 1.  LDS: bad [NT] int.
template <typename BLK> SSR_BODY void ssr_boot_mask_body(const SsrBootParams& p, BLK& blk, int col0, int64_t row0, int* bad) {
  const int NT = SSR_BOOT_NT, K = p.n_cols;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    const int col = col0 + (tid & 63);
    int f = 0;
    if (col < K)
      for (int64_t r = row0 + (tid >> 6); r < row0 + SSR_BOOT_MASK_ROWS && r < p.n_rows; r += NT / 64) {
        const double v = p.table[r * K + col];
        f |= !(fabs(v) <= 1.7976931348623157e308);
      }
    bad[tid] = f;
  });
  SSR_PHASE(blk, regs, {
    const int lane = tid & 63, col = col0 + lane;
    if (col < K && (bad[lane] | bad[64 + lane] | bad[128 + lane] | bad[192 + lane]))
      for (int b = tid >> 6; b < p.n_boot; b += NT / 64) p.reps[(int64_t)b * K + col] = NAN;
  });
}

struct SsrBootSumParams {
  const double* reps;           // [n_boot][n_cols]
  int n_boot, n_cols, n_q;
  double q[SSR_BOOT_MAX_Q];
  double* out;                  // [n_cols][2 + n_q]: mean, standard error, the quantiles
  int32_t* counts;              // [n_cols][2]: replicates <= 0, replicates >= 0
};

SSR_HD int ssr_boot_pow2(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// NumPy's _lerp: a + (b - a) t, from the other end for t >= 0.5 (separately rounded products: no fused multiply-add)
SSR_DEV double ssr_boot_lerp(double a, double b, double t) {
  const double d = b - a;
  return t >= 0.5 ? ssr_fadd_rn(b, -ssr_fmul_rn(d, 1.0 - t)) : ssr_fadd_rn(a, ssr_fmul_rn(d, t));
}

// ---- summary of column c.  LDS: s [pow2(n_boot)] double, wsum / wsq [NT / 64] double, wflag [NT / 64] int.
template <typename BLK> SSR_BODY void ssr_boot_summary_body(const SsrBootSumParams& p, BLK& blk, int c, double* s, double* wsum,
                                                            double* wsq, int* wflag) {
  const int NT = SSR_BOOT_SUM_NT, B = p.n_boot, K = p.n_cols, P = ssr_boot_pow2(B), NQ = p.n_q;
  SSR_REGS(double, regs, blk);
  SSR_PHASE(blk, regs, {
    double part = 0.0;
    int f = 0;
    for (int i = tid; i < P; i += NT) {
      double v = INFINITY;
      if (i < B) {
        v = p.reps[(int64_t)i * K + c];
        f |= !(fabs(v) <= 1.7976931348623157e308);
        part += v;
      }
      s[i] = v;
    }
    SSR_WAVE_SUM_STORE(tid, NT, part, wsum);
    SSR_WAVE_ANY_STORE(tid, f, wflag);
  });
  int bad = 0;
  double sum = 0.0;
  for (int w = 0; w < NT / 64; ++w) { bad |= wflag[w]; sum += wsum[w]; }
  const double mean = sum / (double)B;
  SSR_PHASE(blk, regs, {
    double part = 0.0;
    for (int i = tid; i < B; i += NT) { const double d = s[i] - mean; part += d * d; }
    SSR_WAVE_SUM_STORE(tid, NT, part, wsq);
  });
  if (!bad) {
    for (int k = 2; k <= P; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        SSR_PHASE(blk, regs, {
          for (int h = tid; h < P / 2; h += NT) {
            const int i = ((h & ~(j - 1)) << 1) | (h & (j - 1)), l = i + j;
            const double a = s[i], d = s[l];
            if ((a > d) == ((i & k) == 0)) { s[i] = d; s[l] = a; }
          }
        });
      }
  }
  SSR_PHASE(blk, regs, {
    double* o = p.out + (int64_t)c * (2 + NQ);
    if (tid == 0) {
      double ss = 0.0;
      for (int w = 0; w < NT / 64; ++w) ss += wsq[w];
      o[0] = bad ? NAN : mean;
      o[1] = bad ? NAN : sqrt(ss / (double)(B - 1));          // B = 1: 0 / 0 = NaN
    } else if (tid >= 64 && tid < 64 + NQ) {
      const double pos = p.q[tid - 64] * (double)(B - 1);
      int lo = (int)floor(pos);
      lo = lo < 0 ? 0 : (lo > B - 1 ? B - 1 : lo);
      const int hi = lo + 1 < B ? lo + 1 : B - 1;
      o[2 + tid - 64] = bad ? NAN : ssr_boot_lerp(s[lo], s[hi], pos - (double)lo);
    } else if (tid == 128 || tid == 192) {
      // first index with s > 0 (tid 128: the count of replicates <= 0) or with s >= 0 (tid 192: B minus it = replicates >= 0)
      int a = 0, e = B;
      while (a < e) {
        const int mid = (a + e) >> 1;
        if (tid == 128 ? s[mid] <= 0.0 : s[mid] < 0.0) a = mid + 1; else e = mid;
      }
      p.counts[2 * (int64_t)c + (tid == 192)] = bad ? -1 : (tid == 128 ? a : B - a);
    }
  });
}
