// Kernel bodies of the mel-spectrogram distances on magnitude images that already sit in HBM:
//   M[t, m]  = Σ_f S[t, f] W[f, m]                                    (mel image of a [T, F] magnitude image S)
//   mel_lsd  = mean_t sqrt( mean_m log10( G^2 / (E + 1e-12)^2 + 1e-12 )^2 )
//   mel_l1   = mean_{t,m} | ln⁺(E) - ln⁺(G) |,   ln⁺(x) = ln(max(x, 1e-5))
//   mcd      = mean_t (10 / ln 10) sqrt( 2 Σ_{d=1..n_cep} c_d^2 ),   c = orthonormal DCT-II over m of ln⁺(E) - ln⁺(G)
// with E / G the estimate's / target's mel image.
//
//   schedule  one workgroup, one thread per filter: the support [lo, hi) of column m of the dense filterbank (validated on the
//             host: one contiguous run of non-zero weights), then a balanced projection schedule.  The non-zero weights of all
//             filters, filter after filter, form one sequence of nnz entries; lane l of a wave owns the C = ceil(nnz / 64)
//             consecutive entries [l C, (l + 1) C), stored step-major (entry j of every lane side by side: coalesced loads).  A lane
//             ends a SEGMENT where a filter ends or its own entries end; filter m's value is the sum of its segments
//             seg_first[m] .. seg_first[m + 1] - 1 (one, or two where a lane boundary cuts the filter), in order.  Also the DCT table.
//   metrics   one wave per (key group, item, run of SSR_MEL_RUN rows).  Per row: the target row is staged in LDS and projected -
//             lanes over the schedule, each a float64 segmented sum of its C entries (every lane runs the same C steps whatever
//             the filter widths; a float32 x float32 product is exact in float64), the segments to LDS, then lanes over filters
//             add their segments - and its log-mel terms are kept in registers; then each of the KG estimate rows of the group
//             goes through the same LDS buffer and is projected against them.  mel_lsd's and mel_l1's per-row sums are wave
//             reductions; for mcd the log-mel difference goes to LDS, Q = 64 / n_cep (1 .. 8) lanes per cepstral index sum a
//             quarter (Q = 4 at n_cep = 13) of the m range each, and one lane per index adds the Q partials in order.  Every
//             per-frame term is float64.  The wave's run totals go to one partial record per (image, run).
//   finalize  one thread per (image, metric): the runs in ascending order, divided by T (by T * n_mels for mel_l1).
//   project   (mel_spectrogram) one wave per (image, run of rows): the same projection, the mel rows as float32.
// The schedule depends on the filterbank only, so a mel value has the same bits wherever it is computed.
// Runs are SSR_MEL_RUN rows of one image whatever the batch, sums have a fixed order and there are no atomics: a pair gives the
// same bits alone, in any batch and on every run.  All bodies compile on the host too (SSR_HOST_EMU, tests/emu/mel_emu.cpp).
#pragma once
#include "ssr_block.h"

#ifndef SSR_MEL_MAX
#define SSR_MEL_MAX 256                    // filters: four per lane (include/ssr_hip.h)
#define SSR_MEL_LSD 1                      // `which` bits; out columns are always [mel_lsd, mel_l1, mcd]
#define SSR_MEL_L1 2
#define SSR_MEL_MCD 4
#endif
#define SSR_MEL_SLOTS 4
#define SSR_MEL_RUN 16                     // rows per wave
#define SSR_MEL_NT 64                      // one wave per workgroup
#define SSR_MEL_FLOOR 1e-5
#define SSR_MEL_EPS 1e-12

#define SSR_MEL_SCHED_NT 256               // threads of the schedule kernel (one per filter)
#define SSR_MEL_SEGS (SSR_MEL_MAX + SSR_MEL_NT)    // segments: one per filter plus at most one per lane boundary

struct SsrMelFb {
  const float* fb;              // dense [n_bins][n_mels] (workspace copy of the caller's table)
  int32_t* sched_bin;           // [steps][64]: bin | (segment + 1) << 16 where the entry ends a segment (0 in the high half else)
  float* sched_w;               // [steps][64]: weight (0 for the padding after nnz)
  int32_t* seg_first;           // [n_mels + 1]
  double* dct;                  // [n_mels][n_cep]: sqrt(2 / n_mels) cos(pi d (2 m + 1) / (2 n_mels)), d = 1 .. n_cep
  int n_bins, n_mels, n_cep, steps;
};

// LDS: lo, w, start [SSR_MEL_MAX] int
template <typename BLK> SSR_BODY void ssr_mel_schedule_body(const SsrMelFb& f, BLK& blk, int* lo, int* wd, int* start) {
  const int M = f.n_mels, C = f.steps;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    for (int m = tid; m < M; m += SSR_MEL_SCHED_NT) {
      int a = -1, b = -1;
      for (int k = 0; k < f.n_bins; ++k)
        if (f.fb[(int64_t)k * M + m] != 0.0f) {
          if (a < 0) a = k;
          b = k + 1;
        }
      lo[m] = a < 0 ? 0 : a;
      wd[m] = a < 0 ? 0 : b - a;
      const double sc = sqrt(2.0 / (double)M);
      for (int d = 1; d <= f.n_cep; ++d)
        f.dct[(int64_t)m * f.n_cep + d - 1] = sc * cos(M_PI * (double)d * (double)(2 * m + 1) / (double)(2 * M));
    }
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {           // entry offsets and segment numbers: a lane boundary l C strictly inside a filter adds a segment
      int o = 0, sg = 0;
      for (int m = 0; m < M; ++m) {
        start[m] = o;
        f.seg_first[m] = sg;
        sg += 1 + (o + wd[m] - 1) / C - o / C;
        o += wd[m];
      }
      f.seg_first[M] = sg;
    }
  });
  SSR_PHASE(blk, regs, {
    for (int m = tid; m < M; m += SSR_MEL_SCHED_NT) {
      int sg = f.seg_first[m];
      for (int k = 0; k < wd[m]; ++k) {
        const int i = start[m] + k, l = i / C, j = i % C;
        const bool end = k == wd[m] - 1 || j == C - 1;
        f.sched_bin[j * SSR_MEL_NT + l] = (lo[m] + k) | (end ? (sg + 1) << 16 : 0);
        f.sched_w[j * SSR_MEL_NT + l] = f.fb[(int64_t)(lo[m] + k) * M + m];
        if (end) ++sg;
      }
    }
    const int nnz = start[M - 1] + wd[M - 1];
    for (int i = nnz + tid; i < C * SSR_MEL_NT; i += SSR_MEL_SCHED_NT) {
      f.sched_bin[(i % C) * SSR_MEL_NT + i / C] = 0;
      f.sched_w[(i % C) * SSR_MEL_NT + i / C] = 0.0f;
    }
  });
}

struct SsrMelParams {
  const float* x;              // estimate images: key k of item i at x + k * x_plane + x_row[i] * pitch
  const float* y;              // target images:   item i at y + y_row[i] * pitch (unused by the projection)
  const int64_t* x_row;        // [n_items]
  const int64_t* y_row;        // [n_items]
  const int32_t* n_rows;       // [n_items]
  SsrMelFb f;
  int64_t x_plane;
  int F, pitch, n_items, n_chunks, kg, which;
  double* part;                // [n_keys * n_items][n_chunks][3]: run totals (image v = k * n_items + i)
  float* mel;                  // projection: row r of item i at mel + (x_row[i] + r) * n_mels
};

// Stage row `r` (F floats) in LDS.  VEC: 16-byte aligned rows with a pitch of whole quads (the pair pipeline's images).
template <bool VEC> SSR_DEV void ssr_mel_stage(const float* r, float* buf, int F, int tid) {
  const int nq = (F + 3) / 4;
  for (int q = tid; q < nq; q += SSR_MEL_NT) {
    const int k0 = 4 * q;
    if constexpr (VEC) {
#ifdef SSR_HOST_EMU
      for (int j = 0; j < 4; ++j) buf[k0 + j] = r[k0 + j];
#else
      const float4 v = reinterpret_cast<const float4*>(r)[q];
      buf[k0] = v.x; buf[k0 + 1] = v.y; buf[k0 + 2] = v.z; buf[k0 + 3] = v.w;
#endif
    } else {
      for (int j = 0; j < 4; ++j)
        if (k0 + j < F) buf[k0 + j] = r[k0 + j];
    }
  }
}

// phase 1 of a projection: lane `tid`'s segmented sum over its C schedule entries of the staged row, segments to seg[]
SSR_DEV void ssr_mel_segments(const SsrMelFb& f, const float* buf, double* seg, int tid) {
  double acc = 0.0;
  for (int j = 0; j < f.steps; ++j) {
    const int e = f.sched_bin[j * SSR_MEL_NT + tid];
    acc += (double)buf[e & 0xffff] * (double)f.sched_w[j * SSR_MEL_NT + tid];
    if (e >> 16) {
      seg[(e >> 16) - 1] = acc;
      acc = 0.0;
    }
  }
}

// phase 2: filter m's value, its segments in order
SSR_DEV double ssr_mel_value(const SsrMelFb& f, const double* seg, int m) {
  double v = 0.0;
  for (int k = f.seg_first[m]; k < f.seg_first[m + 1]; ++k) v += seg[k];
  return v;
}

SSR_DEV double ssr_mel_ln(double v) { return log(v > SSR_MEL_FLOOR ? v : SSR_MEL_FLOOR); }

// doubles of LDS the staged row takes (F floats rounded up to whole quads)
SSR_HD int ssr_mel_buf_doubles(int F) { return ((F + 3) & ~3) / 2; }

// per-lane state of the metrics body: the target's terms of the lane's filters m = tid + 64 s
struct SsrMelLane { double g2[SSR_MEL_SLOTS], lg[SSR_MEL_SLOTS]; };

// lanes per cepstral index in the DCT (1 .. 8; a function of n_cep only)
SSR_HD int ssr_mel_dct_split(int n_cep) { const int q = SSR_MEL_NT / n_cep; return q < 1 ? 1 : (q > 8 ? 8 : q); }

// LDS: buf [F rounded up to whole quads] floats, seg [SSR_MEL_SEGS], dl [SSR_MEL_MAX], cp [SSR_MEL_MAX], red [4], tot [3 kg] doubles
template <bool VEC, typename BLK>
SSR_BODY void ssr_mel_metrics_body(const SsrMelParams& p, BLK& blk, int chunk, int group_v, float* buf, double* seg, double* dl,
                                   double* cp, double* red, double* tot) {
  const int key0 = (group_v / p.n_items) * p.kg, item = group_v % p.n_items;
  const int T = p.n_rows[item];
  const int t0 = chunk * SSR_MEL_RUN;
  const int t1 = (t0 + SSR_MEL_RUN < T) ? t0 + SSR_MEL_RUN : T;
  const int M = p.f.n_mels, S = (M + SSR_MEL_NT - 1) / SSR_MEL_NT, nc = p.f.n_cep;
  const int Q = ssr_mel_dct_split(nc), mq = (M + Q - 1) / Q;
  const bool lsd = (p.which & SSR_MEL_LSD) != 0, l1 = (p.which & SSR_MEL_L1) != 0, mcd = (p.which & SSR_MEL_MCD) != 0;
  const float* x = p.x + (int64_t)key0 * p.x_plane + p.x_row[item] * (int64_t)p.pitch;
  const float* y = p.y + p.y_row[item] * (int64_t)p.pitch;
  SSR_REGS(SsrMelLane, regs, blk);
  SSR_WPHASE(blk, regs, { if (tid < 3 * p.kg) tot[tid] = 0.0; });
  for (int t = t0; t < t1; ++t) {
    SSR_WPHASE(blk, regs, ssr_mel_stage<VEC>(y + (int64_t)t * p.pitch, buf, p.F, tid));
    SSR_WPHASE(blk, regs, ssr_mel_segments(p.f, buf, seg, tid));
    SSR_WPHASE(blk, regs, {
      SSR_UNROLL
      for (int s = 0; s < SSR_MEL_SLOTS; ++s) {
        const int m = tid + SSR_MEL_NT * s;
        const double g = (s < S && m < M) ? ssr_mel_value(p.f, seg, m) : 0.0;
        R.g2[s] = g * g;
        R.lg[s] = ssr_mel_ln(g);
      }
    });
    for (int g = 0; g < p.kg; ++g) {
      SSR_WPHASE(blk, regs, ssr_mel_stage<VEC>(x + (int64_t)g * p.x_plane + (int64_t)t * p.pitch, buf, p.F, tid));
      SSR_WPHASE(blk, regs, ssr_mel_segments(p.f, buf, seg, tid));
      SSR_WPHASE(blk, regs, {
        double sl = 0.0, sa = 0.0;
        SSR_UNROLL
        for (int s = 0; s < SSR_MEL_SLOTS; ++s) {
          const int m = tid + SSR_MEL_NT * s;
          if (s < S && m < M) {
            const double e = ssr_mel_value(p.f, seg, m);
            if (lsd) {
              const double ee = e + SSR_MEL_EPS;
              const double d = log10(R.g2[s] / (ee * ee) + SSR_MEL_EPS);
              sl += d * d;
            }
            const double dd = ssr_mel_ln(e) - R.lg[s];
            sa += fabs(dd);
            if (mcd) dl[m] = dd;
          }
        }
        SSR_WAVE_SUM_STORE(tid, SSR_MEL_NT, sl, red);
        SSR_WAVE_SUM_STORE(tid, SSR_MEL_NT, sa, red + 1);
      });
      if (mcd) {
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
          double sc = 0.0;
          for (int d = tid; d < nc; d += SSR_MEL_NT) {
            double c = 0.0;
            for (int q = 0; q < Q; ++q) c += cp[q * nc + d];
            sc += c * c;
          }
          SSR_WAVE_SUM_STORE(tid, SSR_MEL_NT, sc, red + 2);
        });
      }
      SSR_WPHASE(blk, regs, {
        if (tid == 0) {
          if (lsd) tot[3 * g] += sqrt(red[0] / (double)M);
          if (l1) tot[3 * g + 1] += red[1];
          if (mcd) tot[3 * g + 2] += (10.0 / M_LN10) * sqrt(2.0 * red[2]);
        }
      });
    }
  }
  SSR_WPHASE(blk, regs, {
    if (tid < 3 * p.kg) {
      const int g = tid / 3, j = tid % 3;
      p.part[(((int64_t)(key0 + g) * p.n_items + item) * p.n_chunks + chunk) * 3 + j] = tot[tid];
    }
  });
}

struct SsrMelFinalizeParams {
  const double* part;          // as SsrMelParams::part
  const int32_t* n_rows;       // [n_items]
  int n_chunks, n_items, n_keys, n_mels, which;
  double* out;                 // [n_items][n_keys][3]
};

// one thread per (image, metric): the run totals in run order, divided by T; metrics not asked for are NaN
SSR_HD void ssr_mel_finalize(const SsrMelFinalizeParams& p, int64_t idx) {
  const int64_t v = idx / 3;
  const int j = (int)(idx % 3);
  const int key = (int)(v / p.n_items), item = (int)(v % p.n_items);
  double s = 0.0;
  for (int c = 0; c < p.n_chunks; ++c) s += p.part[(v * p.n_chunks + c) * 3 + j];
  const double T = (double)p.n_rows[item];
  p.out[((int64_t)item * p.n_keys + key) * 3 + j] = !(p.which & (1 << j)) ? NAN : (j == 1 ? s / (T * (double)p.n_mels) : s / T);
}

// projection only: the mel rows of image `item`'s run `chunk`, float32
template <bool VEC, typename BLK>
SSR_BODY void ssr_mel_project_body(const SsrMelParams& p, BLK& blk, int chunk, int item, float* buf, double* seg) {
  const int T = p.n_rows[item];
  const int t0 = chunk * SSR_MEL_RUN;
  const int t1 = (t0 + SSR_MEL_RUN < T) ? t0 + SSR_MEL_RUN : T;
  const int M = p.f.n_mels, S = (M + SSR_MEL_NT - 1) / SSR_MEL_NT;
  const float* x = p.x + p.x_row[item] * (int64_t)p.pitch;
  SSR_REGS(int, regs, blk);
  for (int t = t0; t < t1; ++t) {
    SSR_WPHASE(blk, regs, ssr_mel_stage<VEC>(x + (int64_t)t * p.pitch, buf, p.F, tid));
    SSR_WPHASE(blk, regs, ssr_mel_segments(p.f, buf, seg, tid));
    SSR_WPHASE(blk, regs, {
      float* o = p.mel + (p.x_row[item] + t) * (int64_t)M;
      for (int s = 0; s < S; ++s) {
        const int m = tid + SSR_MEL_NT * s;
        if (m < M) o[m] = (float)ssr_mel_value(p.f, seg, m);
      }
    });
  }
}
