// libssrhip.so translation unit: DTW-aligned mel-cepstral distortion (ssr_mel_dtw.h) and its entry points
// (ssr_spectrogram_mel_dtw, ssr_pair_mel_dtw, ssr_pair_mel_dtw_est64).  The filterbank area of the workspace is tu_mel.hip's.
#include <cmath>

#include "ssr_host.h"
#include "ssr_mel_dtw.h"
#include "ssr_pair_transform.h"

// dynamic LDS: the row buffer (F rounded up to whole quads), then seg [SSR_MEL_SEGS], dl and cp [SSR_MEL_MAX] doubles
static size_t cep_lds_bytes(int F) { return (ssr_mel_buf_doubles(F) + SSR_MEL_SEGS + 2 * SSR_MEL_MAX) * 8; }

template <bool VEC> __global__ __launch_bounds__(SSR_MEL_NT) void k_mel_cepstra(SsrMelCepParams p) {
  extern __shared__ double lds[];
  double* seg = lds + ssr_mel_buf_doubles(p.F);
  SsrBlk blk{(int)threadIdx.x};
  ssr_mel_cepstra_body<VEC>(p, blk, blockIdx.x % p.n_chunks, blockIdx.x / p.n_chunks, (float*)lds, seg, seg + SSR_MEL_SEGS,
                            seg + SSR_MEL_SEGS + SSR_MEL_MAX);
}

__global__ __launch_bounds__(SSR_MEL_NT) void k_mel_dtw(SsrMelDtwParams p) {
  SsrBlk blk{(int)threadIdx.x};
  ssr_mel_dtw_body(p, blk, blockIdx.x, nullptr, nullptr, nullptr);
}

static size_t cep_bytes(int n_keys, int64_t rows, int n_cep) { return ssr_align256((size_t)(n_keys + 1) * rows * n_cep * sizeof(double)); }

static int check_dtw(int n_cep, int radius) {
  if (radius < 0 || radius > SSR_DTW_MAX_RADIUS) return ssr_fail(SSR_ERR_INVALID_ARG, "radius must be in 0..SSR_DTW_MAX_RADIUS");
  if (n_cep < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "n_cep must be in 1..n_mels - 1");
  return SSR_OK;
}

static SsrLdsSlot g_lds_cepstra[2];

// the cepstra of the n_keys + 1 planes, then one wave per (item, key); c.f packed on the device, c.cep sized by cep_bytes
static int launch_dtw(SsrMelCepParams c, int max_rows, int radius, double* out, hipStream_t s) {
  c.n_chunks = ssr_ceil_div(max_rows, SSR_MEL_RUN);
  const bool vec = ssr_images_vec16(c.x, c.y, c.pitch, c.x_plane);
  const size_t lds = cep_lds_bytes(c.F);
  const int64_t grid = (int64_t)(c.n_keys + 1) * c.n_items * c.n_chunks;
  if (grid > 0x7fffffff) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  const void* fn = vec ? (const void*)k_mel_cepstra<true> : (const void*)k_mel_cepstra<false>;
  if (int rc = ssr_allow_lds(fn, lds, &g_lds_cepstra[vec ? 1 : 0])) return rc;
  if (vec) hipLaunchKernelGGL(k_mel_cepstra<true>, dim3((unsigned)grid), dim3(SSR_MEL_NT), lds, s, c);
  else hipLaunchKernelGGL(k_mel_cepstra<false>, dim3((unsigned)grid), dim3(SSR_MEL_NT), lds, s, c);
  HIP_TRY(hipGetLastError());
  SsrMelDtwParams d{c.cep, c.c_row, c.n_rows, c.c_plane, c.c_stride, c.n_items, c.n_keys, c.f.n_cep, radius, out};
  hipLaunchKernelGGL(k_mel_dtw, dim3((unsigned)(c.n_keys * c.n_items)), dim3(SSR_MEL_NT), 0, s, d);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}

// ----------------------------------------------------------------------------------------------------
// image level: one (est, target) view per image, one key, the caller's [*, n_bins] pitch; cepstrum rows of image v from v * max_rows
extern "C" size_t ssr_spectrogram_mel_dtw_workspace_bytes(int n_images, int max_rows, int n_bins, int n_mels, int n_cep, int radius) {
  if (n_images <= 0 || max_rows < 1 || n_bins < 1 || n_mels < 2 || n_mels > SSR_MEL_MAX || n_cep < 1 || n_cep >= n_mels || radius < 0 ||
      radius > SSR_DTW_MAX_RADIUS)
    return 0;
  return ssr_mel_fb_bytes(n_bins, n_mels, n_cep) + cep_bytes(1, (int64_t)n_images * max_rows, n_cep);
}

extern "C" int ssr_spectrogram_mel_dtw(const float* est_sp, const int64_t* est_frame_off, const float* tgt_sp, const int64_t* tgt_frame_off,
                                       const int32_t* n_rows, int n_images, int max_rows, int n_bins, const float* fb, int n_mels, int n_cep,
                                       int radius, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!est_sp || !est_frame_off || !tgt_sp || !tgt_frame_off || !n_rows || !fb || !out) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  if (int rc = check_dtw(n_cep, radius)) return rc;
  int nnz = 0;
  if (int rc = ssr_mel_check_fb(fb, n_bins, n_mels, n_cep, &nnz)) return rc;
  if (n_images <= 0) return SSR_OK;
  if (max_rows < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "empty spectrogram");
  if ((int64_t)max_rows * n_bins >= ((int64_t)1 << 30))
    return ssr_fail(SSR_ERR_UNSUPPORTED, "spectrogram of 2^30 elements or more (4 GiB buffer views)");
  const size_t fbb = ssr_mel_fb_bytes(n_bins, n_mels, n_cep);
  if (!workspace || workspace_bytes < fbb + cep_bytes(1, (int64_t)n_images * max_rows, n_cep)) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  SsrMelCepParams c{};
  if (int rc = ssr_mel_upload_fb(fb, n_bins, n_mels, n_cep, nnz, ws, s, &c.f)) return rc;
  c.x = est_sp; c.y = tgt_sp; c.x_row = est_frame_off; c.y_row = tgt_frame_off; c.n_rows = n_rows; c.c_row = nullptr;
  c.c_stride = max_rows; c.c_plane = (int64_t)n_images * max_rows * n_cep;
  c.F = n_bins; c.pitch = n_bins; c.n_items = n_images; c.n_keys = 1; c.cep = (double*)(ws + fbb);
  return launch_dtw(c, max_rows, radius, out, s);
}

// ----------------------------------------------------------------------------------------------------
// waveform level: K + 1 magnitude images per item (ssr_pair_images), their cepstra (item i from row frame_off[i]), then the warp
struct DtwWs { SsrPairGeom g; SsrPairImages im; size_t off_fb, off_cep, off_rows, total; };
static DtwWs dtw_ws(const ssr_plan* pl, int n_items, int n_keys, int max_len, int64_t total_rows, int n_mels, int n_cep, bool in64) {
  DtwWs w;
  w.g = ssr_pair_geom(pl, n_items, max_len, in64);
  w.im = ssr_pair_images_layout(pl, n_keys, total_rows, in64);
  size_t o = w.im.end;
  w.off_fb = o; o += ssr_mel_fb_bytes(pl->n_bins, n_mels, n_cep);
  w.off_cep = o; o += cep_bytes(n_keys, total_rows, n_cep);
  w.off_rows = o; o += ssr_align256((size_t)n_items * sizeof(int32_t));
  w.total = o;
  return w;
}

extern "C" size_t ssr_pair_mel_dtw_workspace_bytes(const ssr_plan* pl, int n_items, int n_keys, int max_len, int64_t total_rows, int n_mels,
                                                   int n_cep, int radius) {
  if (!pl || n_items <= 0 || n_keys <= 0 || max_len < 1 || total_rows < 1 || n_mels < 2 || n_mels > SSR_MEL_MAX || n_cep < 1 ||
      n_cep >= n_mels || radius < 0 || radius > SSR_DTW_MAX_RADIUS)
    return 0;
  const size_t a = dtw_ws(pl, n_items, n_keys, max_len, total_rows, n_mels, n_cep, false).total;
  const size_t b = dtw_ws(pl, n_items, n_keys, max_len, total_rows, n_mels, n_cep, true).total;
  return a > b ? a : b;
}

static int pair_dtw_impl(const ssr_plan* pl, const float* est, const double* est64, const int64_t* est_off, const float* tgt,
                         const int64_t* tgt_off, const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len,
                         int64_t total_rows, const float* fb, int n_mels, int n_cep, int radius, double* out, void* workspace,
                         size_t workspace_bytes, void* stream) {
  int max_T, nnz = 0;
  if (int rc = ssr_check_pair_batch(pl, (est || est64) && est_off && tgt && tgt_off && len && frame_off && fb && out, n_items, n_keys, max_len,
                                    true, &max_T, [&] {
        if (int rc = check_dtw(n_cep, radius)) return rc;
        return ssr_mel_check_fb(fb, pl->n_bins, n_mels, n_cep, &nnz);
      }))
    return rc;
  if (!max_T) return SSR_OK;
  if (total_rows < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "total_rows must be the batch's frames");
  const DtwWs w = dtw_ws(pl, n_items, n_keys, max_len, total_rows, n_mels, n_cep, est64 != nullptr);
  // the contract is the size the query reports - one size for both entry points - not this layout's own (smaller or equal) need
  if (!workspace || workspace_bytes < ssr_pair_mel_dtw_workspace_bytes(pl, n_items, n_keys, max_len, total_rows, n_mels, n_cep, radius))
    return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  SsrMelCepParams c{};
  if (int rc = ssr_mel_upload_fb(fb, pl->n_bins, n_mels, n_cep, nnz, ws + w.off_fb, s, &c.f)) return rc;
  int32_t* rows = (int32_t*)(ws + w.off_rows);
  if (int rc = ssr_launch_rows_from_len(pl, len, n_items, rows, s)) return rc;
  if (int rc = ssr_pair_images(pl, {len, frame_off, n_items, w.g}, est, est64, est_off, tgt, tgt_off, n_keys, w.im, ws, s)) return rc;
  c.x = (float*)(ws + w.im.off_est); c.y = (float*)(ws + w.im.off_tgt); c.x_row = frame_off; c.y_row = frame_off; c.n_rows = rows;
  c.c_row = frame_off; c.c_stride = 0; c.c_plane = total_rows * n_cep;
  c.x_plane = (int64_t)(w.im.plane / sizeof(float));
  c.F = pl->n_bins; c.pitch = ssr_mag_pitch(pl->n_bins); c.n_items = n_items; c.n_keys = n_keys; c.cep = (double*)(ws + w.off_cep);
  return launch_dtw(c, max_T, radius, out, s);
}

extern "C" int ssr_pair_mel_dtw(const ssr_plan* pl, const float* est, const int64_t* est_off, const float* tgt, const int64_t* tgt_off,
                                const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len, int64_t total_rows,
                                const float* fb, int n_mels, int n_cep, int radius, double* out, void* workspace, size_t workspace_bytes,
                                void* stream) {
  if (!est) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  return pair_dtw_impl(pl, est, nullptr, est_off, tgt, tgt_off, len, frame_off, n_items, n_keys, max_len, total_rows, fb, n_mels, n_cep,
                       radius, out, workspace, workspace_bytes, stream);
}

extern "C" int ssr_pair_mel_dtw_est64(const ssr_plan* pl, const double* est, const int64_t* est_off, const float* tgt, const int64_t* tgt_off,
                                      const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len, int64_t total_rows,
                                      const float* fb, int n_mels, int n_cep, int radius, double* out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  if (!est) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  return pair_dtw_impl(pl, nullptr, est, est_off, tgt, tgt_off, len, frame_off, n_items, n_keys, max_len, total_rows, fb, n_mels, n_cep,
                       radius, out, workspace, workspace_bytes, stream);
}
