// Distribution family: does a SET of embeddings look like another set?  The Fréchet distance of the Gaussians fitted to
// two sets and the unbiased kernel distance (MMD^2, Gaussian kernel) - "everything after the embedding" of FAD and KAD.  Kernel bodies
// in ssr_block.h's phase style: hipcc compiles them for gfx950, g++ -DSSR_HOST_EMU for the tests on a machine without a GPU.
//
// Sets      a reference set R[n][D] and K >= 1 estimate sets E_k[m_k][D]; rows float32 or float64, read where they lie with a leading
//           dimension ld >= D.  All arithmetic float64.
// Moments   mu = column mean, Sigma = centred covariance with ddof = 1.  Two passes: the mean first, then sums of products of centred
//           values (never sum x x^T - n mu mu^T).  Every sum has a fixed shape: row chunks of ssr_dstr_chunk_rows(D) rows, the chunk
//           partials added in chunk order.
// Fréchet   fd = |mu_r - mu_e|^2 + tr Sigma_r + tr Sigma_e - 2 tr sqrt(Sigma_r Sigma_e).  With Sigma_r = V L V^T and W = V L^(1/2) the last
//           term is sum_i sqrt(g_i), g_i >= 0 the eigenvalues of the symmetric G = W^T Sigma_e W.  Both eigenproblems: one-sided
//           (Hestenes) Jacobi on the columns of the symmetric PSD matrix; V is accumulated for Sigma_r only, for G only the column norms
//           are needed; eigenvalue i is the 2-norm of final column i.  Pair order: round-robin, D - 1 steps of floor(D / 2) disjoint
//           pairs per sweep, a bye for odd D.  Columns p < q, a = |c_p|^2, b = |c_q|^2, c = c_p . c_q:
//             skip if a or b <= D 2^-104 max_j |c_j|^2 (a null column; the maximum is over the columns of the input matrix)
//             skip if |c| <= D 2^-52 sqrt(a b)
//             else zeta = (b - a) / (2 c), t = sgn(zeta) / (|zeta| + sqrt(1 + zeta^2)) with sgn(0) = 1, cs = 1 / sqrt(1 + t^2), sn = cs t,
//             c_p <- cs c_p - sn c_q, c_q <- sn c_p + cs c_q.
//           A sweep without a rotation ends the iteration.  The sweep loop has the fixed bound max_sweeps: not converged at the bound
//           gives fd = tr_sqrt = NaN and sweeps = -1; it never runs longer.  No clamp on fd.  n < 2, m_k < 2 or a non-finite moment give
//           NaN; no infinity leaves the library.
// Kernel    mmd2 = sum_{i != j} k(r_i, r_j) / (n (n - 1)) + sum_{i != j} k(e_i, e_j) / (m (m - 1)) - 2 sum_{i, j} k(r_i, e_j) / (n m) with
//           k(x, y) = exp(-gamma |x - y|^2), |x - y|^2 the sum of squared differences (not |x|^2 + |y|^2 - 2 x.y); kd = scale mmd2; up
//           to 8 gamma per call; the reference's own sum once per call.  n < 2 or m_k < 2 give NaN.
//
// Hang safety: every loop bound is known at launch; no spin-wait, no flag, no hand-off between workgroups inside a kernel - ordering
// between workgroups happens at kernel boundaries on the caller's stream only.  No atomics, no inline assembly.
#pragma once
#include "ssr_block.h"

#define SSR_DSTR_MAX_DIM 1024
#define SSR_DSTR_MAX_GAMMA 8
#define SSR_DSTR_NT 256            // threads of the tile kernels: 16 x 16 lanes of 4 x 4 outputs
#define SSR_DSTR_TILE 64           // tile edge: columns (moments) or rows (kernel sums)
#define SSR_DSTR_SLAB 16           // rows (moments) or dimensions (kernel sums) staged through LDS at a time
#define SSR_DSTR_JNT 1024          // threads of the Jacobi workgroup: 16 waves
#define SSR_DSTR_JWAVES 16
#define SSR_DSTR_OUT_COLS 8
#define SSR_DSTR_KD_COLS 4

// rows per chunk of the moment sums: a function of D alone, so a set's bits do not depend on its neighbours
SSR_HD int ssr_dstr_chunk_rows(int D) { return 4 * D > 256 ? 4 * D : 256; }
SSR_HD int64_t ssr_dstr_chunks(int64_t rows, int D) { const int cr = ssr_dstr_chunk_rows(D); return (rows + cr - 1) / cr; }
SSR_HD int ssr_dstr_tiles(int64_t n) { return (int)((n + SSR_DSTR_TILE - 1) / SSR_DSTR_TILE); }

// one set: element offset of its first row, rows, its first chunk among all chunks of the call, its chunks
struct SsrDstrSet { int64_t off, rows, chunk0, chunks; };

struct SsrDstrParams {
  const void* data; int64_t ld; int D, K, max_sweeps;
  const SsrDstrSet* sets;       // [1 + K]: the reference, then the estimates
  double *mean_part, *mean;     // [chunks][D], [1 + K][D]
  double *cov_part, *cov;       // [chunks][D][D] (tiles tj >= ti), [1 + K][D][D]
  double* stats;                // [1 + K][2] = tr Sigma, |mu_r - mu|^2
  double *jwork, *V, *jstat;    // the reference's Jacobi: columns, rotations (then W), [2] = sweeps, rank
  double *T, *G, *gwork;        // [K][D][D] each: Sigma_e W, the symmetrised W^T Sigma_e W, the columns of its Jacobi
  double *out, *moments_out;    // [K][8]; [1 + K][D + D D] or null
};

template <typename X> SSR_DEV double ssr_dstr_elem(const void* data, int64_t at) { return (double)((const X*)data)[at]; }

// ---- k_dstr_mean: partial column sums of one row chunk; 4 row lanes x 64 columns ----------------------------------------------
struct SsrDstrMeanLds { double s[4][SSR_DSTR_TILE]; };

template <typename X> SSR_BODY void ssr_dstr_mean_body(const SsrDstrParams& p, SsrBlk& blk, int cb, int64_t chunk, int set, SsrDstrMeanLds& lds) {
  const SsrDstrSet S = p.sets[set];
  if (chunk >= S.chunks) return;
  const int cr = ssr_dstr_chunk_rows(p.D);
  const int64_t r0 = chunk * cr, r1 = r0 + cr < S.rows ? r0 + cr : S.rows;
  SSR_REGS(double, regs, blk);
  SSR_PHASE(blk, regs, {
    const int col = cb * SSR_DSTR_TILE + (tid & 63), rl = tid >> 6;
    double s = 0.0;
    if (col < p.D)
      for (int64_t r = r0 + rl; r < r1; r += 4) s += ssr_dstr_elem<X>(p.data, S.off + r * p.ld + col);
    lds.s[rl][tid & 63] = s;
  });
  SSR_PHASE(blk, regs, {
    const int col = cb * SSR_DSTR_TILE + tid;
    if (tid < SSR_DSTR_TILE && col < p.D)
      p.mean_part[(S.chunk0 + chunk) * p.D + col] = (lds.s[0][tid] + lds.s[1][tid]) + (lds.s[2][tid] + lds.s[3][tid]);
  });
}

// the chunk partials in chunk order -> the mean (no row: NaN)
SSR_DEV void ssr_dstr_mean_finish_lane(const SsrDstrParams& p, int64_t id) {
  if (id >= (int64_t)(1 + p.K) * p.D) return;
  const int set = (int)(id / p.D), col = (int)(id % p.D);
  const SsrDstrSet S = p.sets[set];
  double s = 0.0;
  for (int64_t c = 0; c < S.chunks; ++c) s += p.mean_part[(S.chunk0 + c) * p.D + col];
  const double m = s / (double)S.rows;
  p.mean[(int64_t)set * p.D + col] = m;
  if (p.moments_out) p.moments_out[(int64_t)set * ((int64_t)p.D + (int64_t)p.D * p.D) + col] = m;
}

// ---- the tile product: acc(i, j) += sum_{r0 <= r < r1} A(r, i) B(r, j) over a 64 x 64 tile, 4 x 4 per lane, rows staged through LDS in
// slabs of 16 in row order (la / lb: (row, column within the tile) -> the value, 0 outside the matrix) -----------------------------
struct SsrDstrTileLds { double a[SSR_DSTR_SLAB][SSR_DSTR_TILE], b[SSR_DSTR_SLAB][SSR_DSTR_TILE]; };
struct SsrDstrAcc { double v[16]; };

template <typename REGS, typename LA, typename LB>
SSR_BODY void ssr_dstr_tile_product(SsrBlk& blk, REGS& acc, SsrDstrTileLds& lds, int64_t r0, int64_t r1, LA la, LB lb) {
  SSR_PHASE(blk, acc, { SSR_UNROLL for (int q = 0; q < 16; ++q) R.v[q] = 0.0; });
  for (int64_t s0 = r0; s0 < r1; s0 += SSR_DSTR_SLAB) {
    SSR_PHASE(blk, acc, {
      for (int e = tid; e < SSR_DSTR_SLAB * SSR_DSTR_TILE; e += SSR_DSTR_NT) {
        const int rr = e >> 6, cc = e & 63;
        const int64_t r = s0 + rr;
        lds.a[rr][cc] = r < r1 ? la(r, cc) : 0.0;
        lds.b[rr][cc] = r < r1 ? lb(r, cc) : 0.0;
      }
    });
    SSR_PHASE(blk, acc, {
      const int ty = (tid >> 4) * 4, tx = (tid & 15) * 4;
      for (int rr = 0; rr < SSR_DSTR_SLAB; ++rr) {
        double a[4], b[4];
        SSR_UNROLL for (int i = 0; i < 4; ++i) { a[i] = lds.a[rr][ty + i]; b[i] = lds.b[rr][tx + i]; }
        SSR_UNROLL for (int i = 0; i < 4; ++i) {
          SSR_UNROLL for (int j = 0; j < 4; ++j) R.v[i * 4 + j] = ssr_fma(a[i], b[j], R.v[i * 4 + j]);
        }
      }
    });
  }
}

// the lane's 4 x 4 outputs -> row-major dst[D][D], tile (ti, tj)
template <typename REGS> SSR_BODY void ssr_dstr_tile_store(SsrBlk& blk, REGS& acc, double* dst, int D, int ti, int tj) {
  SSR_PHASE(blk, acc, {
    const int i0 = ti * SSR_DSTR_TILE + (tid >> 4) * 4, j0 = tj * SSR_DSTR_TILE + (tid & 15) * 4;
    SSR_UNROLL for (int i = 0; i < 4; ++i) {
      SSR_UNROLL for (int j = 0; j < 4; ++j)
        if (i0 + i < D && j0 + j < D) dst[(int64_t)(i0 + i) * D + j0 + j] = R.v[i * 4 + j];
    }
  });
}

// ---- k_dstr_cov: the centred Gram matrix of one row chunk, tile (ti, tj >= ti) -------------------------------------------------
template <typename X> SSR_BODY void ssr_dstr_cov_body(const SsrDstrParams& p, SsrBlk& blk, int ti, int tj, int64_t chunk, int set, SsrDstrTileLds& lds) {
  const SsrDstrSet S = p.sets[set];
  if (tj < ti || chunk >= S.chunks) return;
  const int cr = ssr_dstr_chunk_rows(p.D), D = p.D;
  const int64_t r0 = chunk * cr, r1 = r0 + cr < S.rows ? r0 + cr : S.rows;
  const double* mu = p.mean + (int64_t)set * D;
  SSR_REGS(SsrDstrAcc, acc, blk);
  auto la = [&](int64_t r, int cc) { const int col = ti * SSR_DSTR_TILE + cc; return col < D ? ssr_dstr_elem<X>(p.data, S.off + r * p.ld + col) - mu[col] : 0.0; };
  auto lb = [&](int64_t r, int cc) { const int col = tj * SSR_DSTR_TILE + cc; return col < D ? ssr_dstr_elem<X>(p.data, S.off + r * p.ld + col) - mu[col] : 0.0; };
  ssr_dstr_tile_product(blk, acc, lds, r0, r1, la, lb);
  ssr_dstr_tile_store(blk, acc, p.cov_part + (S.chunk0 + chunk) * D * D, D, ti, tj);
}

// the finish pass: chunk partials in chunk order, / (n - 1), mirrored (fewer than two rows: NaN)
SSR_DEV void ssr_dstr_cov_finish_lane(const SsrDstrParams& p, int64_t id) {
  const int64_t DD = (int64_t)p.D * p.D;
  if (id >= (1 + p.K) * DD) return;
  const int set = (int)(id / DD), i = (int)(id % DD / p.D), j = (int)(id % p.D);
  if (j < i) return;
  const SsrDstrSet S = p.sets[set];
  double s = 0.0;
  for (int64_t c = 0; c < S.chunks; ++c) s += p.cov_part[(S.chunk0 + c) * DD + (int64_t)i * p.D + j];
  const double v = S.rows >= 2 ? s / (double)(S.rows - 1) : (double)NAN;
  double* cov = p.cov + set * DD;
  cov[(int64_t)i * p.D + j] = v;
  cov[(int64_t)j * p.D + i] = v;
  if (p.moments_out) {
    double* m = p.moments_out + set * (p.D + DD) + p.D;
    m[(int64_t)i * p.D + j] = v;
    m[(int64_t)j * p.D + i] = v;
  }
}

// the traces and |mu_r - mu|^2, in index order: one lane per set
SSR_DEV void ssr_dstr_stats_lane(const SsrDstrParams& p, int64_t set) {
  if (set > p.K) return;
  const double* cov = p.cov + set * (int64_t)p.D * p.D;
  double tr = 0.0, d2 = 0.0;
  for (int i = 0; i < p.D; ++i) {
    tr += cov[(int64_t)i * p.D + i];
    const double d = p.mean[i] - p.mean[set * (int64_t)p.D + i];
    d2 = ssr_fma(d, d, d2);
  }
  p.stats[2 * set] = tr;
  p.stats[2 * set + 1] = d2;
}

// ---- k_dstr_project: G_k = W^T Sigma_e W.  PASS 0: T = Sigma_e W; PASS 1: W^T T (into gwork); PASS 2: G = (gwork + gwork^T) / 2.  W is
// column-major (the Jacobi's V scaled), T and G row-major ------------------------------------------------------------------------
template <int PASS> SSR_BODY void ssr_dstr_project_body(const SsrDstrParams& p, SsrBlk& blk, int ti, int tj, int k, SsrDstrTileLds& lds) {
  const int D = p.D;
  const int64_t DD = (int64_t)D * D;
  const double* W = p.V;
  if constexpr (PASS == 2) {
    const double* src = p.gwork + k * DD;
    double* dst = p.G + k * DD;
    SSR_REGS(double, regs, blk);
    SSR_PHASE(blk, regs, {
      const int i0 = ti * SSR_DSTR_TILE + (tid >> 4) * 4, j0 = tj * SSR_DSTR_TILE + (tid & 15) * 4;
      for (int i = i0; i < i0 + 4 && i < D; ++i)
        for (int j = j0; j < j0 + 4 && j < D; ++j) dst[(int64_t)i * D + j] = 0.5 * (src[(int64_t)i * D + j] + src[(int64_t)j * D + i]);
    });
  } else {
    SSR_REGS(SsrDstrAcc, acc, blk);
    const double* A = PASS == 0 ? p.cov + (1 + k) * DD : W;
    const double* B = PASS == 0 ? W : p.T + k * DD;
    // PASS 0: A(r, i) = Sigma_e[r][i], B(r, j) = W[r][j];  PASS 1: A(r, i) = W[r][i], B(r, j) = T[r][j]
    auto la = [&](int64_t r, int cc) {
      const int col = ti * SSR_DSTR_TILE + cc;
      return col < D ? (PASS == 0 ? A[r * D + col] : A[(int64_t)col * D + r]) : 0.0;
    };
    auto lb = [&](int64_t r, int cc) {
      const int col = tj * SSR_DSTR_TILE + cc;
      return col < D ? (PASS == 0 ? B[(int64_t)col * D + r] : B[r * D + col]) : 0.0;
    };
    ssr_dstr_tile_product(blk, acc, lds, 0, D, la, lb);
    ssr_dstr_tile_store(blk, acc, (PASS == 0 ? p.T : p.gwork) + k * DD, D, ti, tj);
  }
}

// ---- k_dstr_jacobi: one workgroup per matrix, whole sweeps inside the kernel ------------------------------------------------------
// The columns pass from wave to wave through GLOBAL memory: the step boundary is SSR_PHASE_GLOBAL (ssr_block.h), a workgroup barrier
// that orders global stores and loads too.
struct SsrDstrJacobiLds {
  double a[SSR_DSTR_MAX_DIM], b[SSR_DSTR_MAX_DIM], c[SSR_DSTR_MAX_DIM];
  double maxn, sum;
  int rot[SSR_DSTR_JWAVES];
  int done, sweeps, rank;         // done: 0 iterating, 1 converged, 2 non-finite input
};

// pair pi (0 <= pi < N / 2) of step `step` (0 <= step < N - 1) of the round-robin over N (even) places; place N - 1 stays
SSR_DEV void ssr_dstr_pair(int step, int pi, int N, int& p, int& q) {
  const int M = N - 1;
  int a, b;
  if (pi == 0) { a = M; b = step; }
  else { a = (step + pi) % M; b = (step - pi + M) % M; }
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// sum of squares of every column of w (column-major [D][D]) -> lds.a[column]: a wave per column, lanes over rows
#define SSR_DSTR_COLUMN_NORMS(blk, regs, w, D, lds)                                             \
  SSR_PHASE(blk, regs, {                                                                        \
    const int wave = ssr_wave_of(tid), lane = tid & 63;                                         \
    for (int c0 = 0; c0 < (D); c0 += SSR_DSTR_JWAVES) {                                         \
      if (c0 + wave < (D)) {                                                                    \
        const double* col = (w) + (int64_t)(c0 + wave) * (D);                                   \
        double s = 0.0;                                                                         \
        for (int r = lane; r < (D); r += 64) s = ssr_fma(col[r], col[r], s);                    \
        SSR_WAVE_SUM_STORE(tid, SSR_DSTR_JNT, s, (lds).a + c0);                                 \
      }                                                                                         \
    }                                                                                           \
  })

// REF: the reference's covariance (set 0) -> jwork, V accumulated and scaled to W = V L^(1/2), jstat = sweeps, rank.
// !REF: G_k -> gwork[k], column norms only; writes the row out[k].
template <bool REF> SSR_BODY void ssr_dstr_jacobi_body(const SsrDstrParams& p, SsrBlk& blk, int k, SsrDstrJacobiLds& lds) {
  const int D = p.D, N = (D + 1) & ~1, npairs = N / 2;
  const int64_t DD = (int64_t)D * D;
  const double* in = REF ? p.cov : p.G + k * DD;
  double* w = REF ? p.jwork : p.gwork + k * DD;
  double* V = p.V;
  SSR_REGS(double, regs, blk);
  SSR_PHASE_GLOBAL(blk, regs, {
    for (int64_t e = tid; e < DD; e += SSR_DSTR_JNT) {
      w[e] = in[e];
      if (REF) V[e] = (e / D == e % D) ? 1.0 : 0.0;
    }
    if (tid < SSR_DSTR_JWAVES) lds.rot[tid] = 0;
  });
  SSR_DSTR_COLUMN_NORMS(blk, regs, w, D, lds);
  SSR_PHASE(blk, regs, if (tid == 0) {
    double m = 0.0;
    bool finite = true;
    for (int j = 0; j < D; ++j) {
      finite = finite && fabs(lds.a[j]) <= 1.7e308;
      m = lds.a[j] > m ? lds.a[j] : m;
    }
    lds.maxn = m; lds.done = finite ? 0 : 2; lds.sweeps = 0;
  });
  const double null_sq = (double)D * 0x1p-104 * lds.maxn, tol = (double)D * 0x1p-52;
  for (int sweep = 0; sweep < p.max_sweeps; ++sweep) {
    if (lds.done) break;
    for (int step = 0; step < N - 1; ++step) {
      // a, b, c of the step's pairs: pair pi belongs to wave pi % 16
      SSR_PHASE(blk, regs, {
        const int wave = ssr_wave_of(tid), lane = tid & 63;
        for (int p0 = 0; p0 < npairs; p0 += SSR_DSTR_JWAVES) {
          const int pi = p0 + wave;
          int cp, cq;
          ssr_dstr_pair(step, pi < npairs ? pi : 0, N, cp, cq);
          if (pi < npairs && cq < D) {
            const double *x = w + (int64_t)cp * D, *y = w + (int64_t)cq * D;
            double sa = 0.0, sb = 0.0, sc = 0.0;
            for (int r = lane; r < D; r += 64) {
              const double xv = x[r], yv = y[r];
              sa = ssr_fma(xv, xv, sa); sb = ssr_fma(yv, yv, sb); sc = ssr_fma(xv, yv, sc);
            }
            SSR_WAVE_SUM_STORE(tid, SSR_DSTR_JNT, sa, lds.a + p0);
            SSR_WAVE_SUM_STORE(tid, SSR_DSTR_JNT, sb, lds.b + p0);
            SSR_WAVE_SUM_STORE(tid, SSR_DSTR_JNT, sc, lds.c + p0);
          }
        }
      });
      // the rotations; the same wave owns the pair
      SSR_PHASE_GLOBAL(blk, regs, {
        const int wave = ssr_wave_of(tid), lane = tid & 63;
        for (int p0 = 0; p0 < npairs; p0 += SSR_DSTR_JWAVES) {
          const int pi = p0 + wave;
          int cp, cq;
          ssr_dstr_pair(step, pi < npairs ? pi : 0, N, cp, cq);
          if (pi < npairs && cq < D) {
            const double a = lds.a[pi], b = lds.b[pi], c = lds.c[pi];
            if (!(a <= null_sq) && !(b <= null_sq) && !(fabs(c) <= tol * (sqrt(a) * sqrt(b)))) {
              const double zeta = (b - a) / (2.0 * c);
              const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
              const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
              double *x = w + (int64_t)cp * D, *y = w + (int64_t)cq * D;
              for (int r = lane; r < D; r += 64) {
                const double xv = x[r], yv = y[r];
                x[r] = cs * xv - sn * yv;
                y[r] = sn * xv + cs * yv;
              }
              if (REF) {
                double *vx = V + (int64_t)cp * D, *vy = V + (int64_t)cq * D;
                for (int r = lane; r < D; r += 64) {
                  const double xv = vx[r], yv = vy[r];
                  vx[r] = cs * xv - sn * yv;
                  vy[r] = sn * xv + cs * yv;
                }
              }
              if (lane == 0) lds.rot[wave] = 1;
            }
          }
        }
      });
    }
    SSR_PHASE(blk, regs, if (tid == 0) {
      int any = 0;
      for (int i = 0; i < SSR_DSTR_JWAVES; ++i) { any |= lds.rot[i]; lds.rot[i] = 0; }
      lds.sweeps = sweep + 1;
      if (!any) lds.done = 1;
    });
  }
  SSR_DSTR_COLUMN_NORMS(blk, regs, w, D, lds);
  // eigenvalue i = |c_i| = sqrt(lds.a[i])
  SSR_PHASE(blk, regs, if (tid == 0) {
    int rank = 0;
    double s = 0.0;
    for (int j = 0; j < D; ++j) {
      rank += lds.a[j] > null_sq ? 1 : 0;
      s += sqrt(sqrt(lds.a[j]));
    }
    lds.rank = rank; lds.sum = s;
  });
  if (REF) {
    SSR_PHASE_GLOBAL(blk, regs, {
      for (int64_t e = tid; e < DD; e += SSR_DSTR_JNT) V[e] *= sqrt(sqrt(lds.a[e / D]));
      if (tid == 0) { p.jstat[0] = lds.done == 1 ? (double)lds.sweeps : -1.0; p.jstat[1] = (double)lds.rank; }
    });
  } else {
    SSR_PHASE(blk, regs, if (tid == 0) {
      const double sweeps_ref = p.jstat[0], sweeps_est = lds.done == 1 ? (double)lds.sweeps : -1.0;
      double v[5] = {0.0, p.stats[2 * (1 + k) + 1], p.stats[0], p.stats[2 * (1 + k)], lds.sum};
      v[0] = v[1] + v[2] + v[3] - 2.0 * v[4];
      const bool ok = sweeps_ref > 0.0 && sweeps_est > 0.0 && fabs(v[0]) <= 1.7e308 && fabs(v[4]) <= 1.7e308;
      if (!ok) v[0] = v[4] = (double)NAN;
      double* o = p.out + (int64_t)k * SSR_DSTR_OUT_COLS;
      for (int j = 0; j < 5; ++j) o[j] = fabs(v[j]) <= 1.7e308 ? v[j] : (double)NAN;
      o[5] = sweeps_ref; o[6] = sweeps_est; o[7] = p.jstat[1];
    });
  }
}

// ---- the kernel sums ----------------------------------------------------------------------------------------------------------
// one (set, set) combination: rows a x rows b; same: inside one set (tiles tj >= ti, the diagonal excluded)
struct SsrDstrCombo { int64_t off_a, rows_a, off_b, rows_b, part0, same; };

struct SsrDstrPairParams {
  const void* data; int64_t ld; int D, K, n_gamma;
  double gamma[SSR_DSTR_MAX_GAMMA]; double scale;
  const SsrDstrCombo* combos;     // [1 + 2 K]: (R, R), then (E_k, E_k), (R, E_k) per k
  const int64_t* index;           // the "write d" variant: row i of the combination is row index[i] of the set; else null
  double *part, *sums, *out, *dist_out;   // [tiles][n_gamma], [combos][n_gamma], [K][n_gamma][4]; [n (n - 1) / 2]
};

struct SsrDstrPairsLds {
  double a[SSR_DSTR_SLAB][SSR_DSTR_TILE + 1], b[SSR_DSTR_SLAB][SSR_DSTR_TILE + 1];
  double red[SSR_DSTR_MAX_GAMMA][SSR_DSTR_NT], red16[SSR_DSTR_MAX_GAMMA][16];
};

// fixed-shape block sum of lds.red[g][0 .. 256) -> red16 -> f(g, sum) on lanes g < n_gamma
#define SSR_DSTR_BLOCK_SUMS(blk, regs, lds, n_gamma, ...)                                       \
  SSR_PHASE(blk, regs, if (tid < 16) {                                                          \
    for (int g = 0; g < (n_gamma); ++g) {                                                       \
      double s_ = 0.0;                                                                          \
      for (int i_ = tid; i_ < SSR_DSTR_NT; i_ += 16) s_ += (lds).red[g][i_];                    \
      (lds).red16[g][tid] = s_;                                                                 \
    }                                                                                           \
  });                                                                                           \
  SSR_PHASE(blk, regs, if (tid < (n_gamma)) {                                                   \
    const int g = tid;                                                                          \
    double sum = 0.0;                                                                           \
    for (int i_ = 0; i_ < 16; ++i_) sum += (lds).red16[g][i_];                                  \
    __VA_ARGS__;                                                                                \
  })

template <typename X, bool WRITE_D> SSR_BODY void ssr_dstr_pairs_body(const SsrDstrPairParams& p, SsrBlk& blk, int ti, int tj, int combo, SsrDstrPairsLds& lds) {
  const SsrDstrCombo C = p.combos[combo];
  const int Ta = ssr_dstr_tiles(C.rows_a), Tb = ssr_dstr_tiles(C.rows_b), D = p.D;
  if (ti >= Ta || tj >= Tb || (C.same && tj < ti)) return;
  SSR_REGS(SsrDstrAcc, acc, blk);
  SSR_PHASE(blk, acc, { SSR_UNROLL for (int q = 0; q < 16; ++q) R.v[q] = 0.0; });
  for (int d0 = 0; d0 < D; d0 += SSR_DSTR_SLAB) {
    SSR_PHASE(blk, acc, {
      for (int e = tid; e < SSR_DSTR_SLAB * SSR_DSTR_TILE; e += SSR_DSTR_NT) {
        const int rr = e >> 4, dd = e & 15;
        int64_t ra = (int64_t)ti * SSR_DSTR_TILE + rr, rb = (int64_t)tj * SSR_DSTR_TILE + rr;
        const bool oka = ra < C.rows_a && d0 + dd < D, okb = rb < C.rows_b && d0 + dd < D;
        if (p.index) { ra = oka ? p.index[ra] : 0; rb = okb ? p.index[rb] : 0; }
        lds.a[dd][rr] = oka ? ssr_dstr_elem<X>(p.data, C.off_a + ra * p.ld + d0 + dd) : 0.0;
        lds.b[dd][rr] = okb ? ssr_dstr_elem<X>(p.data, C.off_b + rb * p.ld + d0 + dd) : 0.0;
      }
    });
    SSR_PHASE(blk, acc, {
      const int ty = (tid >> 4) * 4, tx = (tid & 15) * 4;
      for (int dd = 0; dd < SSR_DSTR_SLAB; ++dd) {
        double a[4], b[4];
        SSR_UNROLL for (int i = 0; i < 4; ++i) { a[i] = lds.a[dd][ty + i]; b[i] = lds.b[dd][tx + i]; }
        SSR_UNROLL for (int i = 0; i < 4; ++i) {
          SSR_UNROLL for (int j = 0; j < 4; ++j) { const double d = a[i] - b[j]; R.v[i * 4 + j] = ssr_fma(d, d, R.v[i * 4 + j]); }
        }
      }
    });
  }
  if constexpr (WRITE_D) {
    SSR_PHASE(blk, acc, {
      const int64_t i0 = (int64_t)ti * SSR_DSTR_TILE + (tid >> 4) * 4, j0 = (int64_t)tj * SSR_DSTR_TILE + (tid & 15) * 4, n = C.rows_a;
      SSR_UNROLL for (int i = 0; i < 4; ++i) {
        SSR_UNROLL for (int j = 0; j < 4; ++j) {
          const int64_t gi = i0 + i, gj = j0 + j;
          if (gi < gj && gj < n) p.dist_out[gi * n - gi * (gi + 1) / 2 + (gj - gi - 1)] = sqrt(R.v[i * 4 + j]);
        }
      }
    });
  } else {
    SSR_PHASE(blk, acc, {
      const int64_t i0 = (int64_t)ti * SSR_DSTR_TILE + (tid >> 4) * 4, j0 = (int64_t)tj * SSR_DSTR_TILE + (tid & 15) * 4;
      for (int g = 0; g < p.n_gamma; ++g) {
        double s = 0.0;
        SSR_UNROLL for (int i = 0; i < 4; ++i) {
          SSR_UNROLL for (int j = 0; j < 4; ++j) {
            const int64_t gi = i0 + i, gj = j0 + j;
            if (gi < C.rows_a && gj < C.rows_b && !(C.same && gi == gj)) s += exp(-p.gamma[g] * R.v[i * 4 + j]);
          }
        }
        lds.red[g][tid] = s;
      }
    });
    SSR_DSTR_BLOCK_SUMS(blk, acc, lds, p.n_gamma, p.part[(C.part0 + (int64_t)ti * Tb + tj) * p.n_gamma + g] = sum);
  }
}

// k_dstr_finish, PASS 0: the tile partials of one combination in tile order (lane t takes tiles t, t + 256, ...; a tile above the
// diagonal of a set's own combination counts twice) -> sums[combo][g]
SSR_BODY void ssr_dstr_finish_sums_body(const SsrDstrPairParams& p, SsrBlk& blk, int combo, SsrDstrPairsLds& lds) {
  const SsrDstrCombo C = p.combos[combo];
  const int64_t Ta = ssr_dstr_tiles(C.rows_a), Tb = ssr_dstr_tiles(C.rows_b);
  SSR_REGS(double, regs, blk);
  SSR_PHASE(blk, regs, {
    double s[SSR_DSTR_MAX_GAMMA];
    for (int g = 0; g < p.n_gamma; ++g) s[g] = 0.0;
    for (int64_t t = tid; t < Ta * Tb; t += SSR_DSTR_NT) {
      const int64_t ti = t / Tb, tj = t % Tb;
      if (C.same && tj < ti) continue;
      const double wgt = C.same && tj > ti ? 2.0 : 1.0;
      for (int g = 0; g < p.n_gamma; ++g) s[g] += wgt * p.part[(C.part0 + t) * p.n_gamma + g];
    }
    for (int g = 0; g < p.n_gamma; ++g) lds.red[g][tid] = s[g];
  });
  SSR_DSTR_BLOCK_SUMS(blk, regs, lds, p.n_gamma, p.sums[(int64_t)combo * p.n_gamma + g] = sum);
}

// k_dstr_finish, PASS 1: mmd2 and kd of (k, g)
SSR_DEV void ssr_dstr_finish_lane(const SsrDstrPairParams& p, int64_t id) {
  if (id >= (int64_t)p.K * p.n_gamma) return;
  const int k = (int)(id / p.n_gamma), g = (int)(id % p.n_gamma);
  const double n = (double)p.combos[0].rows_a, m = (double)p.combos[1 + 2 * k].rows_a;
  double* o = p.out + id * SSR_DSTR_KD_COLS;
  if (n < 2.0 || m < 2.0) { o[0] = o[1] = o[2] = o[3] = (double)NAN; return; }
  const double rr = p.sums[g] / (n * (n - 1.0)), ee = p.sums[(int64_t)(1 + 2 * k) * p.n_gamma + g] / (m * (m - 1.0)),
               re = p.sums[(int64_t)(2 + 2 * k) * p.n_gamma + g] / (n * m);
  const double mmd2 = rr + ee - 2.0 * re, v[4] = {p.scale * mmd2, mmd2, rr, ee};
  for (int j = 0; j < 4; ++j) o[j] = fabs(v[j]) <= 1.7e308 ? v[j] : (double)NAN;
}
