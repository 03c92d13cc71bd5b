// libssrhip.so translation unit: band-split LSD (ssr_lsd_bands.h) and its entry points (ssr_spectrogram_lsd_bands,
// ssr_pair_lsd_bands, ssr_pair_lsd_bands_est64).
#include "ssr_host.h"
#include "ssr_lsd_bands.h"
#include "ssr_pair_transform.h"

template <int KG, int NB, bool VEC> __global__ __launch_bounds__(64) void k_lsd_bands(SsrLsdBandsParams p) {
  ssr_lsd_bands_body<KG, NB, VEC>(p, blockIdx.x % p.n_chunks, blockIdx.x / p.n_chunks);
}

__global__ __launch_bounds__(256) void k_lsd_bands_finalize(SsrLsdBandsFinalizeParams p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) ssr_lsd_bands_finalize(p, i);
}

// host-side validation of the caller's edges: nothing reaches the device unless every band lies inside [0, n_bins)
static int check_edges(const int32_t* edges, int64_t n_images, int n_bands, int n_bins) {
  if (n_bands < 1 || n_bands > SSR_MAX_BANDS) return ssr_fail(SSR_ERR_INVALID_ARG, "n_bands must be in 1..SSR_MAX_BANDS");
  if (!edges) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int64_t v = 0; v < n_images; ++v) {
    const int32_t* e = edges + v * (n_bands + 1);
    if (e[0] < 0) return ssr_fail(SSR_ERR_INVALID_ARG, "band edges must be >= 0");
    for (int j = 0; j < n_bands; ++j)
      if (e[j + 1] <= e[j]) return ssr_fail(SSR_ERR_INVALID_ARG, "band edges must be strictly ascending");
    if (e[n_bands] > n_bins) return ssr_fail(SSR_ERR_INVALID_ARG, "last band edge exceeds n_bins");
  }
  return SSR_OK;
}

template <int KG, int NB>
static void launch_bands_kg(const SsrLsdBandsParams& p, bool vec, dim3 grid, hipStream_t s) {
  if (vec) hipLaunchKernelGGL((k_lsd_bands<KG, NB, true>), grid, dim3(64), 0, s, p);
  else hipLaunchKernelGGL((k_lsd_bands<KG, NB, false>), grid, dim3(64), 0, s, p);
}

// the reduction + the finalisation; `edges_dev` already on the device, n_keys * n_items images
// rows of a wave: ssr_wave_rows_per_wg's, rounded up to whole summation quanta
static int band_rows_per_chunk(int max_rows, int64_t groups) {
  return ssr_ceil_div(ssr_wave_rows_per_wg(max_rows, groups), SSR_LSD_BANDS_Q) * SSR_LSD_BANDS_Q;
}

static int launch_bands(SsrLsdBandsParams p, int n_keys, int kg, int max_rows, const int32_t* n_rows, double* out, hipStream_t s) {
  p.rows_per_chunk = band_rows_per_chunk(max_rows, (int64_t)p.n_items * (n_keys / kg));
  p.n_chunks = ssr_ceil_div(max_rows, p.rows_per_chunk);
  p.n_quanta = p.n_chunks * (p.rows_per_chunk / SSR_LSD_BANDS_Q);
  const bool vec = ssr_images_vec16(p.x, p.y, p.pitch, p.x_plane);
  const dim3 grid((unsigned)((int64_t)(n_keys / kg) * p.n_items * p.n_chunks));
  const bool two = p.n_bands <= 2;        // the LF / HF split: 2 accumulators per key instead of SSR_MAX_BANDS
  switch (kg * 2 + (two ? 1 : 0)) {
    case 7: launch_bands_kg<3, 2>(p, vec, grid, s); break;
    case 6: launch_bands_kg<3, SSR_MAX_BANDS>(p, vec, grid, s); break;
    case 5: launch_bands_kg<2, 2>(p, vec, grid, s); break;
    case 4: launch_bands_kg<2, SSR_MAX_BANDS>(p, vec, grid, s); break;
    case 3: launch_bands_kg<1, 2>(p, vec, grid, s); break;
    default: launch_bands_kg<1, SSR_MAX_BANDS>(p, vec, grid, s); break;
  }
  HIP_TRY(hipGetLastError());
  SsrLsdBandsFinalizeParams f{p.part, n_rows, p.n_quanta, p.n_bands, p.n_items, n_keys, out};
  const int64_t n = (int64_t)n_keys * p.n_items * p.n_bands;
  hipLaunchKernelGGL(k_lsd_bands_finalize, dim3((unsigned)ssr_ceil_div(n, 256)), dim3(256), 0, s, f, n);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}

static size_t part_bytes(int64_t n_images, int max_rows, int n_bands, int64_t groups) {
  const int rows = band_rows_per_chunk(max_rows, groups);
  const int n_quanta = ssr_ceil_div(max_rows, rows) * (rows / SSR_LSD_BANDS_Q);
  return ssr_align256((size_t)n_images * n_quanta * n_bands * sizeof(double));
}
static size_t edges_bytes(int64_t n_images, int n_bands) { return ssr_align256((size_t)n_images * (n_bands + 1) * sizeof(int32_t)); }

// ----------------------------------------------------------------------------------------------------
// image level: one image per (est, target) view, one key (KG = 1), the caller's [*, n_bins] pitch
extern "C" size_t ssr_spectrogram_lsd_bands_workspace_bytes(int n_images, int max_rows, int n_bands) {
  if (n_images <= 0 || max_rows < 1 || n_bands < 1 || n_bands > SSR_MAX_BANDS) return 0;
  return part_bytes(n_images, max_rows, n_bands, n_images) + edges_bytes(n_images, n_bands);
}

extern "C" int ssr_spectrogram_lsd_bands(const float* est_sp, const int64_t* est_frame_off, const float* tgt_sp, const int64_t* tgt_frame_off,
                                         const int32_t* n_rows, int n_images, int max_rows, int n_bins, const int32_t* edges, int n_bands,
                                         double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!est_sp || !est_frame_off || !tgt_sp || !tgt_frame_off || !n_rows || !edges || !out) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  if (n_images <= 0) return SSR_OK;
  if (max_rows < 1 || n_bins < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "empty spectrogram");
  if ((int64_t)max_rows * n_bins >= ((int64_t)1 << 30))
    return ssr_fail(SSR_ERR_UNSUPPORTED, "spectrogram of 2^30 elements or more (4 GiB buffer views)");
  if (int rc = check_edges(edges, n_images, n_bands, n_bins)) return rc;
  const size_t pb = part_bytes(n_images, max_rows, n_bands, n_images);
  if (!workspace || workspace_bytes < pb + edges_bytes(n_images, n_bands)) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* e_dev = (int32_t*)(ws + pb);
  HIP_TRY(hipMemcpyAsync(e_dev, edges, (size_t)n_images * (n_bands + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
  SsrLsdBandsParams p{est_sp, tgt_sp, est_frame_off, tgt_frame_off, n_rows, e_dev, 0, n_bins, n_bins, n_bands, n_images, 0, 0, 0,
                      (double*)ws};
  return launch_bands(p, 1, 1, max_rows, n_rows, out, s);
}

// ----------------------------------------------------------------------------------------------------
// waveform level: K + 1 magnitude images per item (the pair transform of ssr_pair_metrics_multi), then the reduction
struct BandWs { SsrPairGeom g; SsrPairImages im; size_t off_part, off_edges, off_rows, total; int kg; };
static BandWs band_ws(const ssr_plan* pl, int n_items, int n_keys, int max_len, int64_t total_rows, int n_bands, bool in64) {
  BandWs w;
  w.g = ssr_pair_geom(pl, n_items, max_len, in64);
  w.im = ssr_pair_images_layout(pl, n_keys, total_rows, in64);
  const int max_T = (int)ssr_num_frames(pl, max_len);
  w.kg = ssr_keys_per_wave(n_keys);
  size_t o = w.im.end;
  w.off_part = o; o += part_bytes((int64_t)n_keys * n_items, max_T, n_bands, (int64_t)n_items * (n_keys / w.kg));
  w.off_edges = o; o += edges_bytes((int64_t)n_keys * n_items, n_bands);
  w.off_rows = o; o += ssr_align256((size_t)n_items * sizeof(int32_t));
  w.total = o;
  return w;
}

extern "C" size_t ssr_pair_lsd_bands_workspace_bytes(const ssr_plan* pl, int n_items, int n_keys, int max_len, int64_t total_rows, int n_bands) {
  if (!pl || n_items <= 0 || n_keys <= 0 || max_len < 1 || n_bands < 1 || n_bands > SSR_MAX_BANDS) return 0;
  const size_t a = band_ws(pl, n_items, n_keys, max_len, total_rows, n_bands, false).total;
  const size_t b = band_ws(pl, n_items, n_keys, max_len, total_rows, n_bands, true).total;
  return a > b ? a : b;
}

static int pair_lsd_bands_impl(const ssr_plan* pl, const float* est, const double* est64, const int64_t* est_off, const float* tgt,
                               const int64_t* tgt_off, const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len,
                               int64_t total_rows, const int32_t* edges, int n_bands, double* out, void* workspace, size_t workspace_bytes,
                               void* stream) {
  int max_T;
  if (int rc = ssr_check_pair_batch(pl, (est || est64) && est_off && tgt && tgt_off && len && frame_off && edges && out, n_items, n_keys, max_len,
                                    true, &max_T, [&] {
        return n_bands < 1 || n_bands > SSR_MAX_BANDS ? ssr_fail(SSR_ERR_INVALID_ARG, "n_bands must be in 1..SSR_MAX_BANDS") : SSR_OK;
      }))
    return rc;
  if (!max_T) return SSR_OK;
  if (int rc = check_edges(edges, (int64_t)n_items * n_keys, n_bands, pl->n_bins)) return rc;
  const BandWs w = band_ws(pl, n_items, n_keys, max_len, total_rows, n_bands, est64 != nullptr);
  // the contract is the size the query reports - one size for both entry points - not this layout's own (smaller or equal) need
  if (!workspace || workspace_bytes < ssr_pair_lsd_bands_workspace_bytes(pl, n_items, n_keys, max_len, total_rows, n_bands))
    return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* rows = (int32_t*)(ws + w.off_rows);
  int32_t* e_dev = (int32_t*)(ws + w.off_edges);
  HIP_TRY(hipMemcpyAsync(e_dev, edges, (size_t)n_items * n_keys * (n_bands + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (int rc = ssr_launch_rows_from_len(pl, len, n_items, rows, s)) return rc;
  if (int rc = ssr_pair_images(pl, {len, frame_off, n_items, w.g}, est, est64, est_off, tgt, tgt_off, n_keys, w.im, ws, s)) return rc;
  SsrLsdBandsParams p{(float*)(ws + w.im.off_est), (float*)(ws + w.im.off_tgt), frame_off, frame_off, rows, e_dev,
                      (int64_t)(w.im.plane / sizeof(float)), pl->n_bins,
                      ssr_mag_pitch(pl->n_bins), n_bands, n_items, 0, 0, 0, (double*)(ws + w.off_part)};
  return launch_bands(p, n_keys, w.kg, max_T, rows, out, s);
}

extern "C" int ssr_pair_lsd_bands(const ssr_plan* pl, const float* est, const int64_t* est_off, const float* tgt, const int64_t* tgt_off,
                                  const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len, int64_t total_rows,
                                  const int32_t* edges, int n_bands, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!est) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  return pair_lsd_bands_impl(pl, est, nullptr, est_off, tgt, tgt_off, len, frame_off, n_items, n_keys, max_len, total_rows, edges, n_bands,
                             out, workspace, workspace_bytes, stream);
}

extern "C" int ssr_pair_lsd_bands_est64(const ssr_plan* pl, const double* est, const int64_t* est_off, const float* tgt, const int64_t* tgt_off,
                                        const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len, int64_t total_rows,
                                        const int32_t* edges, int n_bands, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!est) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  return pair_lsd_bands_impl(pl, nullptr, est, est_off, tgt, tgt_off, len, frame_off, n_items, n_keys, max_len, total_rows, edges, n_bands,
                             out, workspace, workspace_bytes, stream);
}
