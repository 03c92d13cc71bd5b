// libssrhip.so translation unit: SSIM / spectrogram reductions / finalisation kernels (K3-K5) and the metric entry
// points (ssr_pair_metrics*, ssr_spectrogram_metrics).
#include "ssr_host.h"
#include "ssr_metrics.h"
#include "ssr_pair_transform.h"

// (the eight-column CONTIG variant is compiled for two waves per SIMD - 256 VGPRs; every other variant as before)
template <int CPT, bool CONTIG>
__global__ __launch_bounds__(SSR_SSIM_NT, (CPT == 8 ? 2 : 1)) void k_ssim(SsrSsimParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  SsrBlk blk{(int)threadIdx.x};
  const int tiles = p.n_row_tiles * p.n_strips;
  ssr_ssim_body<CPT, CONTIG>(p, blk, blockIdx.x % tiles, blockIdx.x / tiles, smem);
}


__global__ __launch_bounds__(256) void k_specred(SsrSpecRedParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  SsrBlk blk{(int)threadIdx.x};
  ssr_specred_body(p, blk, blockIdx.x % p.n_chunks, blockIdx.x / p.n_chunks, smem);
}

__global__ __launch_bounds__(64) void k_finalize(SsrFinalizeParams p) {
  const int item = blockIdx.x * 64 + threadIdx.x;
  if (item < p.n_items) ssr_finalize_item(p, item);
}

struct SsimGeom { int rows_per_tile, n_row_tiles, n_strips, cpt; };
// aligned_rows: the pair pipeline's images (rows padded to 16 bytes on 256-byte-aligned bases) - eligible for the CONTIG kernel
static SsimGeom ssim_geom(int max_rows, int n_bins, int n_items, bool aligned_rows) {
  SsimGeom g;
  const int out_rows = max_rows - 6 > 1 ? max_rows - 6 : 1;
  int64_t r = ((int64_t)out_rows * n_items + ssr_target_wgs() - 1) / ssr_target_wgs();
  if (r < 8) r = 8;
  if (r > 128) r = 128;
  if (r > out_rows) r = out_rows;
  g.rows_per_tile = (int)r;
  g.n_row_tiles = ssr_ceil_div(out_rows, g.rows_per_tile);
  g.cpt = ssr_ssim_pick_cpt(n_bins);
  if (aligned_rows && g.cpt != 4) {
    // The CONTIG kernel (four consecutive columns per lane, both seven-row rings, no branches) costs ~0.68 of the strided one per
    // column slot (measured on 401 x 1115 images: five CONTIG strips 0.83 ms against three six-column strips 1.03 ms per 1024
    // pairs), so it is taken whenever its strips x 5 slots x 0.68 undercut the strided choice's strips x (cpt + 1).
    const int outs = n_bins - (SSR_SSIM_WIN - 1);
    if (outs > 0) {
      const int strips4 = ssr_ceil_div(outs, ssr_ssim_strip_out(4)), strips_c = ssr_ceil_div(outs, ssr_ssim_strip_out(g.cpt));
      if (strips4 * 5 * 68 < strips_c * (g.cpt + 1) * 100) g.cpt = 4;
    }
  }
  if (aligned_rows && g.cpt == 4) {
    // Eight consecutive columns per lane (k_ssim<8, true>: strips of 512 outputs, two waves per SIMD instead of three).  The kernel
    // is issue-bound, so a strip row is priced by the instructions of the steady fourteen-step trip of the compiled loops:
    // SSR_SSIM_TRIP4 for 256 outputs against SSR_SSIM_TRIP8 for 512 (disassembly of the shipped code objects,
    // profiles/ssim_wide_notes.md).  F = 1025: 2 x 6371 < 4 x 3731 and F = 513: 1 x 6371 < 2 x 3731 take eight columns;
    // F = 1115: 3 x 6371 > 5 x 3731 stays on four.
    constexpr int SSR_SSIM_TRIP4 = 3731, SSR_SSIM_TRIP8 = 6371;
    const int outs = n_bins - (SSR_SSIM_WIN - 1);
    if (outs > 0 && ssr_ceil_div(outs, ssr_ssim_strip_out(8)) * SSR_SSIM_TRIP8 < ssr_ceil_div(outs, ssr_ssim_strip_out(4)) * SSR_SSIM_TRIP4)
      g.cpt = 8;
  }
  g.n_strips = n_bins > 6 ? ssr_ceil_div(n_bins - 6, ssr_ssim_strip_out(g.cpt)) : 1;
  return g;
}


struct PairWs {
  SsrPairGeom g;
  SsimGeom sg;
  SsrPairImages im;
  size_t off_part, off_ssim, total;
};
// want_mag: the two magnitude images are only materialised when SSIM is asked for (8 bytes per bin of the batch - 38 GB for
// 12,500 utterances of 4 s - against a few hundred bytes per item for the partial records)
static PairWs pair_ws(const ssr_plan* pl, int n_items, int max_len, int64_t total_rows, bool in64, bool want_mag) {
  PairWs w;
  w.g = ssr_pair_geom(pl, n_items, max_len, in64);
  w.sg = ssim_geom((int)ssr_num_frames(pl, max_len), pl->n_bins, n_items, true);
  w.im = ssr_pair_images_layout(pl, 1, total_rows, in64, want_mag);
  size_t o = w.im.end;
  w.off_part = o; o += ssr_align256((size_t)n_items * w.g.n_chunks * SSR_NPART * sizeof(double));
  w.off_ssim = o; o += ssr_align256((size_t)n_items * w.sg.n_row_tiles * w.sg.n_strips * sizeof(double));
  w.total = o;
  return w;
}

// ----------------------------------------------------------------------------------------------------
extern "C" size_t ssr_pair_metrics_workspace_bytes_for(const ssr_plan* pl, int n_items, int max_len, int64_t total_rows,
                                                        unsigned metric_mask) {
  if (!pl || n_items <= 0) return 0;
  const bool mag = metric_mask & SSR_METRIC_SSIM;
  // the float32 and float64-signal entry points may chunk differently (different engines): cover both
  const size_t a = pair_ws(pl, n_items, max_len, total_rows, false, mag).total, b = pair_ws(pl, n_items, max_len, total_rows, true, mag).total;
  return (a > b ? a : b) + ssr_align256((size_t)n_items * sizeof(int32_t));
}

extern "C" size_t ssr_pair_metrics_workspace_bytes(const ssr_plan* pl, int n_items, int max_len, int64_t total_rows) {
  return ssr_pair_metrics_workspace_bytes_for(pl, n_items, max_len, total_rows, SSR_METRIC_ALL);
}

template <int CPT, bool CONTIG = false> static int launch_ssim_inst(const SsrSsimParams& p, int grid, hipStream_t s) {
  const size_t lds = SsrSsimLds<CPT, CONTIG>::bytes();
  static thread_local SsrLdsSlot slot;
  if (int rc = ssr_allow_lds((const void*)k_ssim<CPT, CONTIG>, lds, &slot)) return rc;
  hipLaunchKernelGGL((k_ssim<CPT, CONTIG>), dim3(grid), dim3(SSR_SSIM_NT), lds, s, p);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}

// pitch: floats between image rows (0: F, the caller's own [T, F] tensors).  vi_n / x_plane: n_items virtual items, item k * vi_n + i
// reading estimate plane k against the one target image of item i (SsrSsimParams; 0: plain items)
static int launch_ssim(const float* x, const float* y, const int64_t* frame_off, const int32_t* n_rows, int n_items,
                       int F, int pitch, const SsimGeom& g, double* part, hipStream_t s, int vi_n = 0, int64_t x_plane = 0) {
  SsrSsimParams p{x, y, frame_off, n_rows, F, g.rows_per_tile, g.n_row_tiles, g.n_strips, part, pitch, vi_n, x_plane};
  const int grid = n_items * g.n_row_tiles * g.n_strips;
  // four or eight consecutive columns per thread through aligned 16-byte loads: rows and both bases 16-byte aligned
  const bool contig = pitch > 0 && pitch % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
  if (g.cpt == 8) {                // chosen for aligned rows only (ssim_geom), and it has no strided form
    if (!contig) return ssr_fail(SSR_ERR_UNSUPPORTED, "eight-column SSIM geometry on unaligned rows");
    return launch_ssim_inst<8, true>(p, grid, s);
  }
  if (g.cpt == 4 && contig) return launch_ssim_inst<4, true>(p, grid, s);
  switch (g.cpt) {
    case 1: return launch_ssim_inst<1>(p, grid, s);
    case 2: return launch_ssim_inst<2>(p, grid, s);
    case 3: return launch_ssim_inst<3>(p, grid, s);
    case 4: return launch_ssim_inst<4>(p, grid, s);
    case 5: return launch_ssim_inst<5>(p, grid, s);
    case 6: return launch_ssim_inst<6>(p, grid, s);
  }
  return ssr_fail(SSR_ERR_UNSUPPORTED, "bad SSIM geometry");
}

static int launch_finalize(const double* part, int n_chunks, const double* ssim_part, int n_tiles, const int32_t* n_rows,
                           int F, unsigned mask, int n_items, double* out, hipStream_t s) {
  SsrFinalizeParams p{part, n_chunks, ssim_part, n_tiles, n_rows, F, (int)mask, n_items, out};
  hipLaunchKernelGGL(k_finalize, dim3(ssr_ceil_div(n_items, 64)), dim3(64), 0, s, p);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}

// n_rows (T_i) for the finalisation is derived on device from len: a tiny kernel fills it.
__global__ void k_rows_from_len(const int32_t* len, int n_items, int n_fft, int hop, int32_t* rows) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_items) rows[i] = ssr_num_frames_dev(len[i], n_fft, hop);
}
int ssr_launch_rows_from_len(const ssr_plan* pl, const int32_t* len, int n_items, int32_t* rows, hipStream_t s) {
  hipLaunchKernelGGL(k_rows_from_len, dim3(ssr_ceil_div(n_items, 256)), dim3(256), 0, s, len, n_items, pl->n_fft, pl->hop, rows);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}

// stages: 1 = STFT + LSD/SISpec epilogue, 2 = SSIM, 4 = finalise (bench.py times stages separately)
static int pair_metrics_impl(const ssr_plan* pl, const float* est, const double* est64, const int64_t* est_off,
                             const float* tgt, const double* tgt64, const int64_t* tgt_off, const int32_t* len, const int64_t* frame_off,
                             int n_items, int max_len, int64_t total_rows, unsigned mask, double* out,
                             void* workspace, size_t workspace_bytes, void* stream, int stages) {
  int max_T;
  if (int rc = ssr_check_pair_batch(pl, (est || est64) && (tgt || tgt64) && est_off && tgt_off && len && frame_off && out, n_items, 1, max_len,
                                    mask & SSR_METRIC_SSIM, &max_T))
    return rc;
  if (!max_T) return SSR_OK;
  if ((mask & ~SSR_METRIC_ALL) || mask == 0) return ssr_fail(SSR_ERR_INVALID_ARG, "bad metric mask");
  const bool want_ssim = mask & SSR_METRIC_SSIM;
  if (want_ssim && (max_T < 7 || pl->n_bins < 7)) return ssr_fail(SSR_ERR_INVALID_ARG, "win_size exceeds image extent");
  const PairWs w = pair_ws(pl, n_items, max_len, total_rows, est64 != nullptr, want_ssim);
  // rows array lives at the tail of the ssim partial area's alignment slack: allocate it explicitly
  const size_t rows_bytes = ssr_align256((size_t)n_items * sizeof(int32_t));
  if (!workspace || workspace_bytes < w.total + rows_bytes) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  int32_t* rows = (int32_t*)(ws + w.total);
  float *est_plane = (float*)(ws + w.im.off_est), *tgt_plane = (float*)(ws + w.im.off_tgt);
  hipStream_t s = (hipStream_t)stream;
  int rc = SSR_OK;
  if (stages & 1) {
    if ((rc = ssr_launch_rows_from_len(pl, len, n_items, rows, s))) return rc;
    // (the workspace pointers go in either way: without SSIM the planes are empty and nothing is written)
    rc = ssr_pair_transform(pl, {len, frame_off, n_items, w.g},
                            {est, est64, est_off, tgt, tgt64, tgt_off, mask, want_ssim ? SSR_OUT_MAG : SSR_OUT_NONE, est_plane, tgt_plane,
                             (double*)(ws + w.off_part)}, s);
    if (rc) return rc;
  }
  if ((stages & 2) && want_ssim) {
    rc = launch_ssim(est_plane, tgt_plane, frame_off, rows, n_items, pl->n_bins, ssr_mag_pitch(pl->n_bins), w.sg, (double*)(ws + w.off_ssim), s);
    if (rc) return rc;
  }
  if (stages & 4) {
    rc = launch_finalize((const double*)(ws + w.off_part), w.g.n_chunks, want_ssim ? (const double*)(ws + w.off_ssim) : nullptr,
                         w.sg.n_row_tiles * w.sg.n_strips, rows, pl->n_bins, mask, n_items, out, s);
  }
  return rc;
}

extern "C" int ssr_pair_metrics_stages(const ssr_plan* pl, const float* est, const int64_t* est_off, const float* tgt,
                                       const int64_t* tgt_off, const int32_t* len, const int64_t* frame_off,
                                       int n_items, int max_len, int64_t total_rows, unsigned mask, double* out,
                                       void* workspace, size_t workspace_bytes, void* stream, int stages) {
  return pair_metrics_impl(pl, est, nullptr, est_off, tgt, nullptr, tgt_off, len, frame_off, n_items, max_len, total_rows,
                           mask, out, workspace, workspace_bytes, stream, stages);
}

extern "C" int ssr_pair_metrics(const ssr_plan* pl, const float* est, const int64_t* est_off, const float* tgt,
                                const int64_t* tgt_off, const int32_t* len, const int64_t* frame_off, int n_items,
                                int max_len, int64_t total_rows, unsigned mask, double* out, void* workspace,
                                size_t workspace_bytes, void* stream) {
  return pair_metrics_impl(pl, est, nullptr, est_off, tgt, nullptr, tgt_off, len, frame_off, n_items, max_len, total_rows,
                           mask, out, workspace, workspace_bytes, stream, 7);
}

extern "C" int ssr_pair_metrics_est64(const ssr_plan* pl, const double* est, const int64_t* est_off, const float* tgt,
                                      const int64_t* tgt_off, const int32_t* len, const int64_t* frame_off, int n_items,
                                      int max_len, int64_t total_rows, unsigned mask, double* out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  return pair_metrics_impl(pl, nullptr, est, est_off, tgt, nullptr, tgt_off, len, frame_off, n_items, max_len, total_rows,
                           mask, out, workspace, workspace_bytes, stream, 7);
}

extern "C" int ssr_pair_metrics_f64(const ssr_plan* pl, const double* est, const int64_t* est_off, const double* tgt,
                                    const int64_t* tgt_off, const int32_t* len, const int64_t* frame_off, int n_items,
                                    int max_len, int64_t total_rows, unsigned mask, double* out, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return pair_metrics_impl(pl, nullptr, est, est_off, nullptr, tgt, tgt_off, len, frame_off, n_items, max_len, total_rows,
                           mask, out, workspace, workspace_bytes, stream, 7);
}

// ----------------------------------------------------------------------------------------------------
// ssr_pair_metrics_multi: ONE target, K estimates per item (SSR_Eval_Helper.evaluate_single, ssr_eval/eval.py:136-154: every
// degradation key of a file is scored against the same target).  The target is transformed ONCE - with estimate 0, by the pair
// kernel exactly as ssr_pair_metrics runs it (key 0 is bit-identical) - and its magnitude image written once; the other estimates
// go through the same kernel TWO PER COMPLEX TRANSFORM (no target, no metric epilogue: magnitude rows only), their LSD / SISpec
// terms come from k_specred_wave against the stored target image, and k_ssim reads that one image for every key:
// K + 1 real transforms and K + 1 images instead of 2 K and 2 K.
#include "ssr_specred_wave.h"
template <int KG> __global__ __launch_bounds__(64) void k_specred_wave(SsrSpecWaveParams p) {
  ssr_specred_wave_body<KG>(p, blockIdx.x % p.n_chunks, blockIdx.x / p.n_chunks);
}

struct MultiWs {
  SsrPairGeom g;                  // chunking of the transform passes
  SsimGeom sg;                    // for n_items * n_keys virtual items on the fast path
  SsrPairImages im;
  size_t off_part_a, off_part_s, off_ssim, off_rows, total;
  int spec_rows_per_chunk, spec_chunks, spec_kg, n_tiles;
  bool fast;
};
static MultiWs multi_ws(const ssr_plan* pl, int n_items, int n_keys, int max_len, int64_t total_rows, unsigned mask, bool est64 = false) {
  MultiWs m;
  const bool want_ssim = mask & SSR_METRIC_SSIM;
  m.fast = ssr_multi_fast_path(pl, est64) && n_keys > 1;
  m.g = ssr_pair_geom(pl, n_items, max_len, est64);
  const int max_T = (int)ssr_num_frames(pl, max_len);
  m.sg = ssim_geom(max_T, pl->n_bins, m.fast ? n_items * n_keys : n_items, true);    // (the plain passes keep ssr_pair_metrics' tiles)
  m.n_tiles = m.sg.n_row_tiles * m.sg.n_strips;
  m.im = ssr_pair_images_layout(pl, n_keys, total_rows, est64, want_ssim || m.fast, false);
  const int n_spec = ((n_keys - 1) / 2) * 2;                                  // keys whose reductions come from the images (in pairs)
  // keys of an item per wave (they share the target's rows).  Measured on cfg-3 (6 such keys, 1024 items): 1 key per wave 4.37 ms
  // (20 GB of images at 4.6 TB/s: HBM-bound), 2 per wave 3.2-3.4 ms (90 VGPRs, five waves per SIMD), 3 per wave the same,
  // 6 per wave 5.11 ms (173 VGPRs: latency-bound at two waves per SIMD)
  // after the round-4 packing of the float32 sequences (VALU-bound before, close to HBM-bound now): 2 per wave 2.92 ms, 3 per wave
  // 2.77 ms - three where the keys divide by three (cfg-3: 6)
  m.spec_kg = ssr_keys_per_wave(n_spec);                                      // (n_spec is even)
  m.spec_rows_per_chunk = ssr_wave_rows_per_wg(max_T, (int64_t)n_items * (n_spec > 0 ? n_spec / m.spec_kg : 1));
  m.spec_chunks = ssr_ceil_div(max_T, m.spec_rows_per_chunk);
  size_t o = m.im.end;
  m.off_part_a = o; o += 2 * ssr_align256((size_t)n_items * m.g.n_chunks * SSR_NPART * sizeof(double));      // key 0 and an odd last key
  m.off_part_s = o; o += ssr_align256((size_t)n_items * n_keys * m.spec_chunks * SSR_NPART * sizeof(double));
  m.off_ssim = o; o += ssr_align256((size_t)n_items * n_keys * m.n_tiles * sizeof(double));
  m.off_rows = o; o += ssr_align256((size_t)n_items * sizeof(int32_t));
  m.total = o;
  return m;
}

extern "C" size_t ssr_pair_metrics_multi_workspace_bytes(const ssr_plan* pl, int n_items, int n_keys, int max_len, int64_t total_rows,
                                                         unsigned metric_mask) {
  if (!pl || n_items <= 0 || n_keys <= 0) return 0;
  return multi_ws(pl, n_items, n_keys, max_len, total_rows, metric_mask).total;
}

// est / est64: the K estimates as float32 or as float64 signals (the other pointer null)
static int pair_metrics_multi_impl(const ssr_plan* pl, const float* est, const double* est64, const int64_t* est_off, const float* tgt,
                                   const int64_t* tgt_off, const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len,
                                   int64_t total_rows, unsigned mask, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  int max_T;
  if (int rc = ssr_check_pair_batch(pl, (est || est64) && est_off && tgt && tgt_off && len && frame_off && out, n_items, n_keys, max_len, true,
                                    &max_T))
    return rc;
  if (!max_T) return SSR_OK;
  if ((mask & ~SSR_METRIC_ALL) || mask == 0) return ssr_fail(SSR_ERR_INVALID_ARG, "bad metric mask");
  const bool want_ssim = mask & SSR_METRIC_SSIM;
  if (want_ssim && (max_T < 7 || pl->n_bins < 7)) return ssr_fail(SSR_ERR_INVALID_ARG, "win_size exceeds image extent");
  const MultiWs m = multi_ws(pl, n_items, n_keys, max_len, total_rows, mask, est64 != nullptr);
  if (!workspace || workspace_bytes < m.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* rows = (int32_t*)(ws + m.off_rows);
  int rc;
  if ((rc = ssr_launch_rows_from_len(pl, len, n_items, rows, s))) return rc;
  const SsrPairBatch bt{len, frame_off, n_items, m.g};
  const bool mag = m.im.plane != 0;
  const int pitch = ssr_mag_pitch(pl->n_bins);
  const int64_t plane_floats = (int64_t)(m.im.plane / sizeof(float));
  const unsigned red_mask = mask & (SSR_METRIC_LSD | SSR_METRIC_LOG_SISPEC | SSR_METRIC_SISPEC);
  auto plane_of = [&](int k) { return mag ? (float*)(ws + m.im.off_est + (size_t)k * m.im.plane) : nullptr; };
  float* tgt_plane = mag ? (float*)(ws + m.im.off_tgt) : nullptr;
  double* part0 = (double*)(ws + m.off_part_a);
  double* ssim_part = (double*)(ws + m.off_ssim);
  auto finalize = [&](const double* part, int n_chunks, const double* sp, int n_virtual, int key0) {
    SsrFinalizeParams p{part, n_chunks, want_ssim ? sp : nullptr, m.n_tiles, rows, pl->n_bins, (int)mask, n_virtual, out, n_items, n_keys, key0};
    hipLaunchKernelGGL(k_finalize, dim3(ssr_ceil_div(n_virtual, 64)), dim3(64), 0, s, p);
    return hipGetLastError();
  };
  auto ssim = [&](int key0, int n_k) {      // keys key0 .. key0 + n_k - 1 against the one target image
    return launch_ssim(plane_of(key0), tgt_plane, frame_off, rows, n_items * n_k, pl->n_bins, pitch, m.sg,
                       ssim_part + (size_t)key0 * n_items * m.n_tiles, s, n_items, plane_floats);
  };
  if (!m.fast) {
    // every key through the pair kernel against the target, as K calls of ssr_pair_metrics would (bit-identical to them): block
    // engines (float64-signal plans have their own entry points), or a single key.  One partial-sum area serves every key in turn.
    for (int k = 0; k < n_keys; ++k) {
      rc = ssr_pair_transform(pl, bt, {est, est64, est_off + (size_t)k * n_items, tgt, nullptr, tgt_off, mask, mag ? SSR_OUT_MAG : SSR_OUT_NONE,
                                       plane_of(k), tgt_plane, part0}, s);
      if (rc) return rc;
      if (want_ssim && (rc = ssim(k, 1))) return rc;
      HIP_TRY(finalize(part0, m.g.n_chunks, ssim_part + (size_t)k * n_items * m.n_tiles, n_items, k));
    }
    return SSR_OK;
  }
  // key 0 with the target (metrics in the epilogue, both images written), keys 1 .. two per complex transform (images only), an odd
  // last key with the target again, whose rows are not rewritten
  const int n_spec = ((n_keys - 1) / 2) * 2;        // keys 1 .. n_spec get their reductions from the images
  const int k_last = n_spec + 1;
  const bool odd_last = k_last < n_keys;
  double* part_last = (double*)(ws + m.off_part_a + ssr_align256((size_t)n_items * m.g.n_chunks * SSR_NPART * sizeof(double)));
  if ((rc = ssr_pair_images(pl, bt, est, est64, est_off, tgt, tgt_off, n_keys, m.im, ws, s, mask, part0, part_last))) return rc;
  if (n_spec > 0 && red_mask) {
    SsrSpecWaveParams q{plane_of(1), tgt_plane, frame_off, rows, pl->n_bins, pitch, (int)red_mask, m.spec_rows_per_chunk, m.spec_chunks, n_items,
                        plane_floats, (double*)(ws + m.off_part_s)};
    // KG keys of an item per wave share the target's rows (n_spec is even: the keys came in pairs)
    const int kg = m.spec_kg;
    const dim3 grid((unsigned)((int64_t)(n_spec / kg) * n_items * m.spec_chunks));
    if (kg == 3) hipLaunchKernelGGL(k_specred_wave<3>, grid, dim3(64), 0, s, q);
    else if (kg == 2) hipLaunchKernelGGL(k_specred_wave<2>, grid, dim3(64), 0, s, q);
    else hipLaunchKernelGGL(k_specred_wave<1>, grid, dim3(64), 0, s, q);
    HIP_TRY(hipGetLastError());
  }
  if (want_ssim && (rc = ssim(0, n_keys))) return rc;
  HIP_TRY(finalize(part0, m.g.n_chunks, ssim_part, n_items, 0));
  if (n_spec > 0)
    HIP_TRY(finalize(red_mask ? (const double*)(ws + m.off_part_s) : nullptr, m.spec_chunks, ssim_part + (size_t)n_items * m.n_tiles, n_spec * n_items, 1));
  if (odd_last) HIP_TRY(finalize(part_last, m.g.n_chunks, ssim_part + (size_t)k_last * n_items * m.n_tiles, n_items, k_last));
  return SSR_OK;
}

extern "C" int ssr_pair_metrics_multi(const ssr_plan* pl, const float* est, const int64_t* est_off, const float* tgt, const int64_t* tgt_off,
                                      const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len, int64_t total_rows,
                                      unsigned mask, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!est) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  return pair_metrics_multi_impl(pl, est, nullptr, est_off, tgt, tgt_off, len, frame_off, n_items, n_keys, max_len, total_rows, mask, out,
                                 workspace, workspace_bytes, stream);
}

// K float64 estimates per float32 target (ssr_hip.h): key 0 through the float64-estimate pair kernel with the target, the others two per
// complex transform into float32 magnitude rows (|.| of the unrounded float64 spectrum, rounded once), their terms from k_specred_wave
extern "C" size_t ssr_pair_metrics_multi_est64_workspace_bytes(const ssr_plan* pl, int n_items, int n_keys, int max_len, int64_t total_rows,
                                                               unsigned metric_mask) {
  if (!pl || n_items <= 0 || n_keys <= 0) return 0;
  return multi_ws(pl, n_items, n_keys, max_len, total_rows, metric_mask, true).total;
}
extern "C" int ssr_pair_metrics_multi_est64(const ssr_plan* pl, const double* est, const int64_t* est_off, const float* tgt, const int64_t* tgt_off,
                                            const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len,
                                            int64_t total_rows, unsigned mask, double* out, void* workspace, size_t workspace_bytes,
                                            void* stream) {
  if (!est) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  return pair_metrics_multi_impl(pl, nullptr, est, est_off, tgt, tgt_off, len, frame_off, n_items, n_keys, max_len, total_rows, mask, out,
                                 workspace, workspace_bytes, stream);
}

// ----------------------------------------------------------------------------------------------------
struct SpecWs { size_t off_part, off_ssim, total; int rows_per_chunk, n_chunks; SsimGeom sg; };
static SpecWs spec_ws(int n_items, int max_rows, int n_bins) {
  SpecWs w;
  w.rows_per_chunk = ssr_units_per_chunk_for(max_rows, n_items);
  w.n_chunks = ssr_ceil_div(max_rows, w.rows_per_chunk);
  w.sg = ssim_geom(max_rows, n_bins, n_items, false);
  size_t o = 0;
  w.off_part = o; o += ssr_align256((size_t)n_items * w.n_chunks * SSR_NPART * sizeof(double));
  w.off_ssim = o; o += ssr_align256((size_t)n_items * w.sg.n_row_tiles * w.sg.n_strips * sizeof(double));
  w.total = o;
  return w;
}

extern "C" size_t ssr_spectrogram_metrics_workspace_bytes(int n_items, int max_rows, int n_bins) {
  if (n_items <= 0) return 0;
  return spec_ws(n_items, max_rows, n_bins).total;
}

extern "C" int ssr_spectrogram_metrics(const float* est_sp, const float* tgt_sp, const int64_t* frame_off,
                                       const int32_t* n_rows, int n_items, int max_rows, int n_bins, unsigned mask,
                                       double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!est_sp || !tgt_sp || !frame_off || !n_rows || !out) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  if (n_items <= 0) return SSR_OK;
  if ((mask & ~SSR_METRIC_ALL) || mask == 0) return ssr_fail(SSR_ERR_INVALID_ARG, "bad metric mask");
  if (max_rows < 1 || n_bins < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "empty spectrogram");
  if ((int64_t)max_rows * n_bins >= ((int64_t)1 << 30))
    return ssr_fail(SSR_ERR_UNSUPPORTED, "spectrogram of 2^30 elements or more (4 GiB buffer views)");
  const bool want_ssim = mask & SSR_METRIC_SSIM;
  if (want_ssim && (max_rows < 7 || n_bins < 7)) return ssr_fail(SSR_ERR_INVALID_ARG, "win_size exceeds image extent");
  const SpecWs w = spec_ws(n_items, max_rows, n_bins);
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const bool want_red = mask & (SSR_METRIC_LSD | SSR_METRIC_SISPEC | SSR_METRIC_LOG_SISPEC);
  if (want_red) {
    SsrSpecRedParams p{est_sp, tgt_sp, frame_off, n_rows, n_bins, (int)mask, w.rows_per_chunk, w.n_chunks,
                       (double*)(ws + w.off_part)};
    hipLaunchKernelGGL(k_specred, dim3(n_items * w.n_chunks), dim3(256), SsrSpecRedLds::bytes(), s, p);
    HIP_TRY(hipGetLastError());
  }
  if (want_ssim) {
    int rc = launch_ssim(est_sp, tgt_sp, frame_off, n_rows, n_items, n_bins, 0, w.sg, (double*)(ws + w.off_ssim), s);
    if (rc) return rc;
  }
  return launch_finalize(want_red ? (const double*)(ws + w.off_part) : nullptr, w.n_chunks,
                         want_ssim ? (const double*)(ws + w.off_ssim) : nullptr, w.sg.n_row_tiles * w.sg.n_strips, n_rows,
                         n_bins, mask, n_items, out, s);
}
