// Kernel bodies of the DTW-aligned mel-cepstral distortion on magnitude images that already sit in HBM.
// For every image on its own:  c[t, d] = orthonormal DCT-II over m of ln⁺((S W)[t, m]),  d = 1 .. n_cep  (float64; NOT the DCT of a
// difference: frames of different indices are compared).  For an (estimate E, target G) pair of T frames each and a radius R:
//   δ(i, j)  = (10 / ln 10) sqrt( 2 Σ_d (c_E[i, d] - c_G[j, d])² )           inside the band |i - j| <= R, +inf outside
//   D[0][0]  = 2 δ(0, 0)
//   D[i][j]  = min( D[i-1][j-1] + 2 δ(i, j),  D[i-1][j] + δ(i, j),  D[i][j-1] + δ(i, j) )
//              (formed in that order; a later candidate replaces an earlier one only when strictly smaller)
//   mcd_dtw  = D[T-1][T-1] / (2 T);   len = cells on the chosen path, dev_sum = Σ |i - j| over them:  dtw_len = len,
//   dtw_dev  = dev_sum / len.
//
//   cepstra  one wave per (image, run of SSR_MEL_RUN rows), the K estimate planes and the target plane alike.  Per row: staged in
//            LDS and projected with ssr_mel.h's balanced schedule, ln⁺ of the filters to LDS, then k_mel_metrics' split DCT
//            (Q = 64 / n_cep lanes per index over a part of the m range each, one lane per index adds the Q partials in order).
//            The row's n_cep float64 coefficients go to the workspace: plane k, row c_row(item) + t.
//   dtw      one wave per (item, key).  The wave sweeps the anti-diagonals s = i + j = 0 .. 2 T - 2; lane l owns the band offset
//            o = i - j = l - 32 (63 offsets in 64 lanes: R <= 31; lane 0 is never in the band).  A cell's three predecessors are
//            the lane's own value two steps back (a register) and the values one step back of the lanes below (o - 1: cell
//            (i-1, j)) and above (o + 1: cell (i, j-1)), one whole-wave DPP shift each way.  A cell outside the band, the matrix
//            or the parity of s has δ = +inf, so its D is +inf and every neighbour reads that: no other edge handling (a lane
//            that owns a cell at step s held +inf at step s - 1, so the shifted-in value at lanes 0 and 63 is +inf as well).
//            Only the offsets with the parity of s own a cell in a step: half the lanes carry +inf.  δ of step s + 1 is formed
//            before the min / add chain of step s (it does not depend on D), from the two cepstrum rows read straight from
//            memory (L2 / L1 hits: the rows of a step are 2 (R + 1) consecutive rows, shared with the next steps): no LDS, nothing
//            that grows with T.  len and dev_sum travel with D as int32.
// δ of a cell is the same instruction sequence whatever R, batch or launch: a wider band gives a D that is <= bit for bit, and a
// pair gives the same bits alone and in any batch.  No atomics.  All bodies compile on the host too (SSR_HOST_EMU,
// tests/emu/mel_dtw_emu.cpp): there the lane exchange goes through three arrays of 64.
#pragma once
#include "ssr_mel.h"

#ifndef SSR_DTW_MAX_RADIUS
#define SSR_DTW_MAX_RADIUS 31              // include/ssr_hip.h
#endif
#define SSR_DTW_LANE0 32                   // the lane of band offset 0

struct SsrMelCepParams {
  const float* x;              // estimate images: key k of item i at x + k * x_plane + x_row[i] * pitch
  const float* y;              // target images:   item i at y + y_row[i] * pitch
  const int64_t* x_row;        // [n_items]
  const int64_t* y_row;        // [n_items]
  const int32_t* n_rows;       // [n_items]
  const int64_t* c_row;        // [n_items] first cepstrum row of item i (null: i * c_stride)
  SsrMelFb f;
  int64_t x_plane, c_plane, c_stride;      // c_plane: doubles per cepstrum plane
  int F, pitch, n_items, n_chunks, n_keys;
  double* cep;                 // [n_keys + 1 planes][rows][n_cep]; plane n_keys: the targets
};

SSR_DEV int64_t ssr_dtw_row(const int64_t* c_row, int64_t c_stride, int item) { return c_row ? c_row[item] : (int64_t)item * c_stride; }

// LDS: buf [F rounded up to whole quads] floats, seg [SSR_MEL_SEGS], dl [SSR_MEL_MAX], cp [SSR_MEL_MAX] doubles
template <bool VEC, typename BLK>
SSR_BODY void ssr_mel_cepstra_body(const SsrMelCepParams& p, BLK& blk, int chunk, int v, float* buf, double* seg, double* dl, double* cp) {
  const int k = v / p.n_items, item = v % p.n_items;
  const int T = p.n_rows[item];
  const int t0 = chunk * SSR_MEL_RUN;
  const int t1 = (t0 + SSR_MEL_RUN < T) ? t0 + SSR_MEL_RUN : T;
  const int M = p.f.n_mels, S = (M + SSR_MEL_NT - 1) / SSR_MEL_NT, nc = p.f.n_cep;
  const int Q = ssr_mel_dct_split(nc), mq = (M + Q - 1) / Q;
  const float* src = k < p.n_keys ? p.x + (int64_t)k * p.x_plane + p.x_row[item] * (int64_t)p.pitch : p.y + p.y_row[item] * (int64_t)p.pitch;
  double* out = p.cep + (int64_t)k * p.c_plane + ssr_dtw_row(p.c_row, p.c_stride, item) * nc;
  SSR_REGS(int, regs, blk);
  for (int t = t0; t < t1; ++t) {
    SSR_WPHASE(blk, regs, ssr_mel_stage<VEC>(src + (int64_t)t * p.pitch, buf, p.F, tid));
    SSR_WPHASE(blk, regs, ssr_mel_segments(p.f, buf, seg, tid));
    SSR_WPHASE(blk, regs, {
      SSR_UNROLL
      for (int s = 0; s < SSR_MEL_SLOTS; ++s) {
        const int m = tid + SSR_MEL_NT * s;
        if (s < S && m < M) dl[m] = ssr_mel_ln(ssr_mel_value(p.f, seg, m));
      }
    });
    SSR_WPHASE(blk, regs, {      // lane (q, d): c_d over m in [q mq, (q + 1) mq)
      for (int i = tid; i < Q * nc; i += SSR_MEL_NT) {
        const int q = i / nc, d = i % nc;
        const int m1 = (q + 1) * mq < M ? (q + 1) * mq : M;
        double c = 0.0;
        for (int m = q * mq; m < m1; ++m) c += dl[m] * p.f.dct[(int64_t)m * nc + d];
        cp[i] = c;
      }
    });
    SSR_WPHASE(blk, regs, {
      for (int d = tid; d < nc; d += SSR_MEL_NT) {
        double c = 0.0;
        for (int q = 0; q < Q; ++q) c += cp[q * nc + d];
        out[(int64_t)t * nc + d] = c;
      }
    });
  }
}

struct SsrMelDtwParams {
  const double* cep;           // as SsrMelCepParams::cep
  const int64_t* c_row;
  const int32_t* n_rows;       // [n_items]
  int64_t c_plane, c_stride;
  int n_items, n_keys, n_cep, radius;
  double* out;                 // [n_items][n_keys][3]: mcd_dtw, dtw_dev, dtw_len
};

// the lane exchange of one step: the value the lane below / above held (`fill` past the ends of the wave)
#ifdef SSR_HOST_EMU
#define SSR_DTW_PUBLISH(arr, tid, v) ((arr)[tid] = (v))
template <typename V> static inline V ssr_dtw_below(const V* arr, int tid, V, V fill) { return tid > 0 ? arr[tid - 1] : fill; }
template <typename V> static inline V ssr_dtw_above(const V* arr, int tid, V, V fill) { return tid < SSR_MEL_NT - 1 ? arr[tid + 1] : fill; }
#else
#define SSR_DTW_PUBLISH(arr, tid, v) ((void)0)
// DPP wave_shr:1 (0x138): lane n reads lane n - 1; wave_shl:1 (0x130): lane n reads lane n + 1; the end lane keeps `fill`
SSR_DEV int ssr_dtw_below(const int*, int, int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false); }
SSR_DEV int ssr_dtw_above(const int*, int, int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x130, 0xf, 0xf, false); }
SSR_DEV double ssr_dtw_below(const double*, int, double v, double fill) {
  union { double d; int i[2]; } a, o, b;
  a.d = v; o.d = fill;
  b.i[0] = __builtin_amdgcn_update_dpp(o.i[0], a.i[0], 0x138, 0xf, 0xf, false);
  b.i[1] = __builtin_amdgcn_update_dpp(o.i[1], a.i[1], 0x138, 0xf, 0xf, false);
  return b.d;
}
SSR_DEV double ssr_dtw_above(const double*, int, double v, double fill) {
  union { double d; int i[2]; } a, o, b;
  a.d = v; o.d = fill;
  b.i[0] = __builtin_amdgcn_update_dpp(o.i[0], a.i[0], 0x130, 0xf, 0xf, false);
  b.i[1] = __builtin_amdgcn_update_dpp(o.i[1], a.i[1], 0x130, 0xf, 0xf, false);
  return b.d;
}
#endif

// δ of the cell lane offset `o` owns on anti-diagonal s; +inf where it owns none (outside the band, the matrix or the parity)
SSR_DEV double ssr_dtw_delta(const double* e, const double* g, int nc, int T, int R, int s, int o) {
  const int i2 = s + o, j2 = s - o;
  const bool own = o >= -R && o <= R && !(i2 & 1) && i2 >= 0 && j2 >= 0 && (i2 >> 1) < T && (j2 >> 1) < T;
  if (!own) return (double)INFINITY;
  const double* ce = e + (int64_t)(i2 >> 1) * nc;
  const double* cg = g + (int64_t)(j2 >> 1) * nc;
  double acc = 0.0;
  SSR_UNROLL4
  for (int d = 0; d < nc; ++d) {      // (unrolled: the loads of four coefficients in flight together; the sum keeps its order)
    const double df = ce[d] - cg[d];
    acc += df * df;
  }
  return (10.0 / M_LN10) * sqrt(2.0 * acc);
}

// per-lane state: D, len and dev_sum of the lane's offset one (1) and two (2) steps back, δ of the coming step
struct SsrDtwLane { double d1, d2, dn; int l1, l2, v1, v2; };

// xd / xl / xv [64]: the host emulation's lane exchange (unused on the device)
template <typename BLK> SSR_BODY void ssr_mel_dtw_body(const SsrMelDtwParams& p, BLK& blk, int v, double* xd, int* xl, int* xv) {
  const int key = v / p.n_items, item = v % p.n_items;
  const int T = p.n_rows[item], nc = p.n_cep;
  const int64_t row = ssr_dtw_row(p.c_row, p.c_stride, item) * nc;
  const double* e = p.cep + (int64_t)key * p.c_plane + row;
  const double* g = p.cep + (int64_t)p.n_keys * p.c_plane + row;
  const double inf = (double)INFINITY;
  SSR_REGS(SsrDtwLane, regs, blk);
  SSR_WPHASE(blk, regs, {      // before step 0: the cell (-1, -1) of offset 0 is the path's empty start
    const bool origin = tid == SSR_DTW_LANE0;
    R.d1 = inf; R.d2 = origin ? 0.0 : inf;
    R.l1 = 0; R.l2 = 0; R.v1 = 0; R.v2 = 0;
    R.dn = ssr_dtw_delta(e, g, nc, T, p.radius, 0, tid - SSR_DTW_LANE0);
  });
  for (int s = 0; s <= 2 * T - 2; ++s) {
    SSR_WPHASE(blk, regs, {
      SSR_DTW_PUBLISH(xd, tid, R.d1);
      SSR_DTW_PUBLISH(xl, tid, R.l1);
      SSR_DTW_PUBLISH(xv, tid, R.v1);
    });
    SSR_WPHASE(blk, regs, {
      const int o = tid - SSR_DTW_LANE0;
      const double dl = R.dn;
      R.dn = ssr_dtw_delta(e, g, nc, T, p.radius, s + 1, o);
      const double ud = ssr_dtw_below(xd, tid, R.d1, inf), ad = ssr_dtw_above(xd, tid, R.d1, inf);
      const int ul = ssr_dtw_below(xl, tid, R.l1, 0), al = ssr_dtw_above(xl, tid, R.l1, 0);
      const int uv = ssr_dtw_below(xv, tid, R.v1, 0), av = ssr_dtw_above(xv, tid, R.v1, 0);
      double best = R.d2 + 2.0 * dl;
      int bl = R.l2, bv = R.v2;
      const double cu = ud + dl, ca = ad + dl;
      if (cu < best) { best = cu; bl = ul; bv = uv; }
      if (ca < best) { best = ca; bl = al; bv = av; }
      R.d2 = R.d1; R.l2 = R.l1; R.v2 = R.v1;
      R.d1 = best; R.l1 = bl + 1; R.v1 = bv + (o < 0 ? -o : o);
    });
  }
  SSR_WPHASE(blk, regs, {
    if (tid == SSR_DTW_LANE0) {
      double* o3 = p.out + ((int64_t)item * p.n_keys + key) * 3;
      o3[0] = T > 0 ? R.d1 / (2.0 * (double)T) : NAN;
      o3[1] = T > 0 ? (double)R.v1 / (double)R.l1 : NAN;
      o3[2] = T > 0 ? (double)R.l1 : NAN;
    }
  });
}
