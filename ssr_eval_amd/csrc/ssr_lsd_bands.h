// Band-split LSD on magnitude images that already sit in HBM: AudioMetrics.lsd (ssr_eval/metrics.py:109-112) restricted to the
// columns [a, b) of each band,
//   lsd_band(E, T, a, b) = mean_t sqrt( mean_{a <= k < b} log10( T^2 / (E + 1e-12)^2 + 1e-12 )^2 ),
// for up to SSR_MAX_BANDS bands per image.  One wave per (key group, item, run of rows), lanes over bins, modelled on
// k_specred_wave (ssr_specred_wave.h): KG estimate images of an item against their one target image, the target row fetched
// once per group and its t * t formed once per bin.  The per-bin term is term 0 of ssr_spec_est2 / ssr_accumulate_metrics<true>
// (the float32 sequence of the LSD epilogue, same bits); per-band row sums and frame totals are float64.
//
// Band assignment.  Every image has its own edges e_0 < e_1 < ... < e_B <= F (validated on the host).  A lane walks its bins in
// increasing order within a row (4 l + 256 j .. + 3), so it keeps ONE running float64 sum `cur` for the band its current bin lies
// in and a register with the next edge; crossing an edge (rare: at most B + 1 times per lane and row) flushes `cur` into that
// band's lane-private accumulator through a select chain - no runtime-indexed register array (it would live in scratch).  Bins
// before e_0 or from e_B on (the pitch padding included) go into a `cur` that is dropped.  At the end of a row each band is one
// wave reduction, sqrt(sum / width) of band j is added to the frame total that lane j holds.
//
// Registers: KG * NB float64 accumulators + KG running sums + KG frame totals.  NB = 2 (the LF / HF split, 12 VGPRs of
// accumulators at KG = 3) and NB = SSR_MAX_BANDS (48 at KG = 3) are separate instantiations, so the common split does not pay the
// occupancy of eight.  Device code only.
//
// Summation order.  The frame totals of an image are added in quanta of SSR_LSD_BANDS_Q rows that start at multiples of Q - rows in
// row order inside a quantum, the quanta in order at the end - and a wave's run of rows is a whole number of quanta.  How many rows
// a wave takes depends on the batch (its longest image and its size); the quanta do not, so an image has the same bits in any batch.
#pragma once
#include "ssr_stft.h"

#define SSR_LSD_BANDS_Q 8                  // rows of a summation quantum

struct SsrLsdBandsParams {
  const float* x;              // estimate images: key k of item i at x + k * x_plane + x_row[i] * pitch
  const float* y;              // target images:   item i at y + y_row[i] * pitch
  const int64_t* x_row;        // [n_items]
  const int64_t* y_row;        // [n_items]
  const int32_t* n_rows;       // [n_items]
  const int32_t* edges;        // [n_keys * n_items][n_bands + 1], image v = k * n_items + i
  int64_t x_plane;
  int F, pitch, n_bands, n_items, rows_per_chunk, n_chunks;       // rows_per_chunk: a multiple of SSR_LSD_BANDS_Q
  int n_quanta;                // n_chunks * rows_per_chunk / SSR_LSD_BANDS_Q: quantum slots per image
  double* part;                // [n_keys * n_items][n_quanta][n_bands]: sum over the quantum's rows of the band's frame LSD
};

// adds `v` to acc[b] (b in [0, NB): a lane-varying index) through a select chain; any other b drops it
template <int NB>
__device__ __forceinline__ void ssr_band_flush(double (&acc)[NB], int b, double v) {
#pragma unroll
  for (int j = 0; j < NB; ++j) acc[j] += (b == j) ? v : 0.0;
}

// VEC: rows are 16-byte aligned with a pitch that is a multiple of four floats (the pair pipeline's images): one float4 load per
// image, row and quad; otherwise scalar loads of the caller's [T, F] tensors.
template <int KG, int NB, bool VEC>
__device__ __forceinline__ void ssr_lsd_bands_body(const SsrLsdBandsParams& p, int chunk, int group_v) {
  const int lane = (int)threadIdx.x;
  const int key0 = (group_v / p.n_items) * KG, item = group_v % p.n_items;
  const int T = p.n_rows[item];
  const int t0 = chunk * p.rows_per_chunk;
  const int t1 = (t0 + p.rows_per_chunk < T) ? t0 + p.rows_per_chunk : T;
  const int nb = p.n_bands;                           // <= NB, wave-uniform
  const float* x = p.x + (int64_t)key0 * p.x_plane + p.x_row[item] * (int64_t)p.pitch;
  const float* y = p.y + p.y_row[item] * (int64_t)p.pitch;
  const int32_t* eg[KG];
  int e_first[KG];
#pragma unroll
  for (int g = 0; g < KG; ++g) {
    eg[g] = p.edges + ((int64_t)(key0 + g) * p.n_items + item) * (nb + 1);
    e_first[g] = eg[g][0];
  }
  double ft[KG];                                      // lane j: frame total of band j
#pragma unroll
  for (int g = 0; g < KG; ++g) ft[g] = 0.0;
  const f2 EPS2 = f2_splat(1e-12f);
  const int nq = (p.F + 3) / 4;
  for (int t = t0; t < t1; ++t) {
    double acc[KG][NB], cur[KG];
    int b[KG], nxt[KG];
#pragma unroll
    for (int g = 0; g < KG; ++g) {
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[g][j] = 0.0;
      cur[g] = 0.0; b[g] = -1; nxt[g] = e_first[g];
    }
    const float* yr = y + (int64_t)t * p.pitch;
    for (int q = lane; q < nq; q += 64) {
      const int k0 = 4 * q;
      float4 yv;
      if constexpr (VEC) {
        yv = reinterpret_cast<const float4*>(yr)[q];
      } else {
        yv.x = yr[k0];
        yv.y = k0 + 1 < p.F ? yr[k0 + 1] : 0.0f;
        yv.z = k0 + 2 < p.F ? yr[k0 + 2] : 0.0f;
        yv.w = k0 + 3 < p.F ? yr[k0 + 3] : 0.0f;
      }
      const f2 y01 = f2_make(yv.x, yv.y), y23 = f2_make(yv.z, yv.w);
      const f2 tt01 = y01 * y01, tt23 = y23 * y23;
#pragma unroll
      for (int g = 0; g < KG; ++g) {
        const float* xr = x + (int64_t)g * p.x_plane + (int64_t)t * p.pitch;
        float4 xv;
        if constexpr (VEC) {
          xv = reinterpret_cast<const float4*>(xr)[q];
        } else {
          xv.x = xr[k0];
          xv.y = k0 + 1 < p.F ? xr[k0 + 1] : 0.0f;
          xv.z = k0 + 2 < p.F ? xr[k0 + 2] : 0.0f;
          xv.w = k0 + 3 < p.F ? xr[k0 + 3] : 0.0f;
        }
        // term 0 of ssr_spec_est2: d = log10(t^2 / (e + EPS)^2 + EPS), d * d
        const f2 e01 = f2_make(xv.x, xv.y) + EPS2, e23 = f2_make(xv.z, xv.w) + EPS2;
        const f2 d01 = ssr_log10f_fast2(ssr_divf_fast2(tt01, e01 * e01) + EPS2);
        const f2 d23 = ssr_log10f_fast2(ssr_divf_fast2(tt23, e23 * e23) + EPS2);
        const f2 s01 = d01 * d01, s23 = d23 * d23;
        const double v[4] = {(double)s01.x, (double)s01.y, (double)s23.x, (double)s23.y};
        if (k0 + 3 < nxt[g]) {                          // the whole quad inside the current band (the common case)
          cur[g] += v[0]; cur[g] += v[1]; cur[g] += v[2]; cur[g] += v[3];
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            while (k0 + i >= nxt[g]) {                  // crossing an edge: flush, move to the next band
              ssr_band_flush<NB>(acc[g], b[g], cur[g]);
              cur[g] = 0.0;
              ++b[g];
              nxt[g] = b[g] < nb ? eg[g][b[g] + 1] : 0x7fffffff;
            }
            cur[g] += v[i];
          }
        }
      }
    }
#pragma unroll
    for (int g = 0; g < KG; ++g) {
      ssr_band_flush<NB>(acc[g], b[g], cur[g]);
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        if (j < nb) {                                   // wave-uniform
          const double s = ssr_wave_sum<64>(acc[g][j]);
          const double w = (double)(eg[g][j + 1] - eg[g][j]);
          if (lane == j) ft[g] += sqrt(s / w);
        }
      }
    }
    if ((t + 1) % SSR_LSD_BANDS_Q == 0 || t + 1 == t1) {   // the quantum ends (t0 is a multiple of Q; wave-uniform)
      const int q = t / SSR_LSD_BANDS_Q;                   // < n_quanta: t < n_chunks * rows_per_chunk
#pragma unroll
      for (int g = 0; g < KG; ++g) {
        if (lane < nb) p.part[(((int64_t)(key0 + g) * p.n_items + item) * p.n_quanta + q) * nb + lane] = ft[g];
        ft[g] = 0.0;
      }
    }
  }
}

struct SsrLsdBandsFinalizeParams {
  const double* part;          // as SsrLsdBandsParams::part
  const int32_t* n_rows;       // [n_items]
  int n_quanta, n_bands, n_items, n_keys;
  double* out;                 // [n_items][n_keys][n_bands]
};

// one thread per (image, band): the totals of the image's own quanta in order, divided by T
__device__ __forceinline__ void ssr_lsd_bands_finalize(const SsrLsdBandsFinalizeParams& p, int64_t idx) {
  const int nb = p.n_bands;
  const int64_t v = idx / nb;
  const int band = (int)(idx % nb);
  const int key = (int)(v / p.n_items), item = (int)(v % p.n_items);
  const int T = p.n_rows[item];
  int nq = (T + SSR_LSD_BANDS_Q - 1) / SSR_LSD_BANDS_Q;     // the slots the image's rows wrote
  if (nq > p.n_quanta) nq = p.n_quanta;
  double s = 0.0;
  for (int q = 0; q < nq; ++q) s += p.part[(v * p.n_quanta + q) * nb + band];
  p.out[((int64_t)item * p.n_keys + key) * nb + band] = s / (double)T;
}
