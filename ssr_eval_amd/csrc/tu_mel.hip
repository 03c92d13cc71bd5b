// libssrhip.so translation unit: mel-spectrogram distances and projection (ssr_mel.h) and their entry points
// (ssr_spectrogram_mel, ssr_spectrogram_mel_metrics, ssr_pair_mel_metrics, ssr_pair_mel_metrics_est64).
#include <cmath>

#include "ssr_host.h"
#include "ssr_mel.h"
#include "ssr_pair_transform.h"

__global__ __launch_bounds__(SSR_MEL_SCHED_NT) void k_mel_schedule(SsrMelFb f) {
  __shared__ int lo[SSR_MEL_MAX], wd[SSR_MEL_MAX], start[SSR_MEL_MAX];
  SsrBlk blk{(int)threadIdx.x};
  ssr_mel_schedule_body(f, blk, lo, wd, start);
}

// dynamic LDS: the row buffer (F rounded up to whole quads), then seg [SSR_MEL_SEGS], dl and cp [SSR_MEL_MAX], red [4], tot [3 kg]
// doubles (the projection: the row buffer and seg only)
static size_t mel_lds_bytes(int F, int kg) { return (ssr_mel_buf_doubles(F) + SSR_MEL_SEGS + 2 * SSR_MEL_MAX + 4 + 3 * kg) * 8; }

template <bool VEC> __global__ __launch_bounds__(SSR_MEL_NT) void k_mel_metrics(SsrMelParams p) {
  extern __shared__ double lds[];
  float* buf = (float*)lds;
  double* seg = lds + ssr_mel_buf_doubles(p.F);
  double* dl = seg + SSR_MEL_SEGS;
  SsrBlk blk{(int)threadIdx.x};
  ssr_mel_metrics_body<VEC>(p, blk, blockIdx.x % p.n_chunks, blockIdx.x / p.n_chunks, buf, seg, dl, dl + SSR_MEL_MAX,
                            dl + 2 * SSR_MEL_MAX, dl + 2 * SSR_MEL_MAX + 4);
}

template <bool VEC> __global__ __launch_bounds__(SSR_MEL_NT) void k_mel_project(SsrMelParams p) {
  extern __shared__ double lds[];
  SsrBlk blk{(int)threadIdx.x};
  ssr_mel_project_body<VEC>(p, blk, blockIdx.x % p.n_chunks, blockIdx.x / p.n_chunks, (float*)lds, lds + ssr_mel_buf_doubles(p.F));
}

__global__ __launch_bounds__(256) void k_mel_finalize(SsrMelFinalizeParams p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) ssr_mel_finalize(p, i);
}

// Host-side validation of the caller's dense filterbank [n_bins][n_mels]: finite, >= 0, every filter one contiguous run of
// non-zero weights; nothing reaches the device otherwise.  n_cep = 0: projection only.  -> *nnz: the non-zero weights.
static int check_fb(const float* fb, int n_bins, int n_mels, int n_cep, int* nnz) {
  if (!fb) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  if (n_mels < 1 || n_mels > SSR_MEL_MAX) return ssr_fail(SSR_ERR_INVALID_ARG, "n_mels must be in 1..SSR_MEL_MAX");
  if (n_cep < 0 || (n_cep > 0 && n_cep >= n_mels)) return ssr_fail(SSR_ERR_INVALID_ARG, "n_cep must be in 1..n_mels - 1");
  if (n_bins < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "empty spectrogram");
  if (n_bins > 0xffff) return ssr_fail(SSR_ERR_UNSUPPORTED, "mel filterbanks of more than 65535 bins");
  *nnz = 0;
  for (int m = 0; m < n_mels; ++m) {
    int lo = -1, hi = -1;
    for (int b = 0; b < n_bins; ++b) {
      const float v = fb[(int64_t)b * n_mels + m];
      if (!std::isfinite(v) || v < 0.0f) return ssr_fail(SSR_ERR_INVALID_ARG, "filterbank weights must be finite and >= 0");
      if (v != 0.0f) {
        if (hi >= 0 && hi != b) return ssr_fail(SSR_ERR_INVALID_ARG, "mel filter " + std::to_string(m) + " has a gap: the support must be contiguous");
        if (lo < 0) lo = b;
        hi = b + 1;
      }
    }
    if (lo < 0)
      return ssr_fail(SSR_ERR_INVALID_ARG, "mel filter " + std::to_string(m) + " is all zero: use fewer mels or a lower f_min");
    *nnz += hi - lo;
  }
  return SSR_OK;
}

// the filterbank area of a workspace: dense copy, schedule (nnz <= n_bins * n_mels entries, padded to whole steps), segment
// starts, DCT table
static size_t sched_bytes(int n_bins, int n_mels) { return ssr_align256(((size_t)n_bins * n_mels + SSR_MEL_NT) * 4); }
static size_t fb_bytes(int n_bins, int n_mels, int n_cep) {
  return 3 * sched_bytes(n_bins, n_mels) + ssr_align256((size_t)(n_mels + 1) * sizeof(int32_t)) +
         ssr_align256((size_t)n_mels * (n_cep > 0 ? n_cep : 1) * sizeof(double));
}

// copy the table into the workspace at `ws` and pack it there (on `s`)
static int upload_fb(const float* fb, int n_bins, int n_mels, int n_cep, int nnz, char* ws, hipStream_t s, SsrMelFb* f) {
  const size_t sb = sched_bytes(n_bins, n_mels);
  float* fb_dev = (float*)ws;
  f->fb = fb_dev;
  f->sched_bin = (int32_t*)(ws + sb);
  f->sched_w = (float*)(ws + 2 * sb);
  f->seg_first = (int32_t*)(ws + 3 * sb);
  f->dct = (double*)(ws + 3 * sb + ssr_align256((size_t)(n_mels + 1) * sizeof(int32_t)));
  f->n_bins = n_bins; f->n_mels = n_mels; f->n_cep = n_cep; f->steps = ssr_ceil_div(nnz, SSR_MEL_NT);
  // (host table: from page-locked memory this copy is asynchronous - the caller keeps it unchanged until the stream has passed)
  HIP_TRY(hipMemcpyAsync(fb_dev, fb, (size_t)n_bins * n_mels * sizeof(float), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_mel_schedule, dim3(1), dim3(SSR_MEL_SCHED_NT), 0, s, *f);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}

// the same for the other mel translation units (ssr_host.h)
int ssr_mel_check_fb(const float* fb, int n_bins, int n_mels, int n_cep, int* nnz) { return check_fb(fb, n_bins, n_mels, n_cep, nnz); }
size_t ssr_mel_fb_bytes(int n_bins, int n_mels, int n_cep) { return fb_bytes(n_bins, n_mels, n_cep); }
int ssr_mel_upload_fb(const float* fb, int n_bins, int n_mels, int n_cep, int nnz, char* ws, hipStream_t s, SsrMelFb* f) {
  return upload_fb(fb, n_bins, n_mels, n_cep, nnz, ws, s, f);
}

static int mel_chunks(int max_rows) { return ssr_ceil_div(max_rows, SSR_MEL_RUN); }
static size_t mel_part_bytes(int64_t n_images, int max_rows) { return ssr_align256((size_t)n_images * mel_chunks(max_rows) * 3 * sizeof(double)); }

static SsrLdsSlot g_lds_metrics[2], g_lds_project[2];

// the reduction + the finalisation on n_keys * n_items images; p.f packed on the device
static int launch_mel(SsrMelParams p, int n_keys, int max_rows, double* out, hipStream_t s) {
  p.n_chunks = mel_chunks(max_rows);
  const bool vec = ssr_images_vec16(p.x, p.y, p.pitch, p.x_plane);
  const size_t lds = mel_lds_bytes(p.F, p.kg);
  const int64_t grid = (int64_t)(n_keys / p.kg) * p.n_items * p.n_chunks;
  if (grid > 0x7fffffff) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  const void* fn = vec ? (const void*)k_mel_metrics<true> : (const void*)k_mel_metrics<false>;
  if (int rc = ssr_allow_lds(fn, lds, &g_lds_metrics[vec ? 1 : 0])) return rc;
  if (vec) hipLaunchKernelGGL(k_mel_metrics<true>, dim3((unsigned)grid), dim3(SSR_MEL_NT), lds, s, p);
  else hipLaunchKernelGGL(k_mel_metrics<false>, dim3((unsigned)grid), dim3(SSR_MEL_NT), lds, s, p);
  HIP_TRY(hipGetLastError());
  SsrMelFinalizeParams fp{p.part, p.n_rows, p.n_chunks, p.n_items, n_keys, p.f.n_mels, p.which, out};
  const int64_t n = (int64_t)n_keys * p.n_items * 3;
  hipLaunchKernelGGL(k_mel_finalize, dim3((unsigned)ssr_ceil_div(n, 256)), dim3(256), 0, s, fp, n);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}

static int check_which(int which) {
  if (which < 1 || which > 7) return ssr_fail(SSR_ERR_INVALID_ARG, "which must be a non-empty combination of SSR_MEL_LSD, SSR_MEL_L1, SSR_MEL_MCD");
  return SSR_OK;
}

// ----------------------------------------------------------------------------------------------------
// projection only
extern "C" size_t ssr_spectrogram_mel_workspace_bytes(int n_bins, int n_mels) {
  if (n_bins < 1 || n_mels < 1 || n_mels > SSR_MEL_MAX) return 0;
  return fb_bytes(n_bins, n_mels, 0);
}

extern "C" int ssr_spectrogram_mel(const float* sp, const int64_t* frame_off, const int32_t* n_rows, int n_images, int max_rows, int n_bins,
                                   const float* fb, int n_mels, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!sp || !frame_off || !n_rows || !fb || !out) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  int nnz = 0;
  if (int rc = check_fb(fb, n_bins, n_mels, 0, &nnz)) return rc;
  if (n_images <= 0) return SSR_OK;
  if (max_rows < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "empty spectrogram");
  if ((int64_t)max_rows * n_bins >= ((int64_t)1 << 30))
    return ssr_fail(SSR_ERR_UNSUPPORTED, "spectrogram of 2^30 elements or more (4 GiB buffer views)");
  if (!workspace || workspace_bytes < fb_bytes(n_bins, n_mels, 0)) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  SsrMelParams p{};
  if (int rc = upload_fb(fb, n_bins, n_mels, 0, nnz, (char*)workspace, s, &p.f)) return rc;
  p.x = sp; p.y = sp; p.x_row = frame_off; p.y_row = frame_off; p.n_rows = n_rows;
  p.F = n_bins; p.pitch = n_bins; p.n_items = n_images; p.n_chunks = mel_chunks(max_rows); p.kg = 1; p.which = 0; p.mel = out;
  const int64_t grid = (int64_t)n_images * p.n_chunks;
  if (grid > 0x7fffffff) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  const bool vec = ssr_images_vec16(p.x, p.y, p.pitch, p.x_plane);
  const size_t lds = (ssr_mel_buf_doubles(n_bins) + SSR_MEL_SEGS) * 8;
  const void* fn = vec ? (const void*)k_mel_project<true> : (const void*)k_mel_project<false>;
  if (int rc = ssr_allow_lds(fn, lds, &g_lds_project[vec ? 1 : 0])) return rc;
  if (vec) hipLaunchKernelGGL(k_mel_project<true>, dim3((unsigned)grid), dim3(SSR_MEL_NT), lds, s, p);
  else hipLaunchKernelGGL(k_mel_project<false>, dim3((unsigned)grid), dim3(SSR_MEL_NT), lds, s, p);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}

// ----------------------------------------------------------------------------------------------------
// image level: one (est, target) view per image, one key (KG = 1), the caller's [*, n_bins] pitch
extern "C" size_t ssr_spectrogram_mel_metrics_workspace_bytes(int n_images, int max_rows, int n_bins, int n_mels, int n_cep) {
  if (n_images <= 0 || max_rows < 1 || n_bins < 1 || n_mels < 2 || n_mels > SSR_MEL_MAX || n_cep < 1 || n_cep >= n_mels) return 0;
  return fb_bytes(n_bins, n_mels, n_cep) + mel_part_bytes(n_images, max_rows);
}

extern "C" int ssr_spectrogram_mel_metrics(const float* est_sp, const int64_t* est_frame_off, const float* tgt_sp, const int64_t* tgt_frame_off,
                                           const int32_t* n_rows, int n_images, int max_rows, int n_bins, const float* fb, int n_mels,
                                           int n_cep, int which, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!est_sp || !est_frame_off || !tgt_sp || !tgt_frame_off || !n_rows || !fb || !out) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  if (int rc = check_which(which)) return rc;
  if (n_cep < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "n_cep must be in 1..n_mels - 1");
  int nnz = 0;
  if (int rc = check_fb(fb, n_bins, n_mels, n_cep, &nnz)) return rc;
  if (n_images <= 0) return SSR_OK;
  if (max_rows < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "empty spectrogram");
  if ((int64_t)max_rows * n_bins >= ((int64_t)1 << 30))
    return ssr_fail(SSR_ERR_UNSUPPORTED, "spectrogram of 2^30 elements or more (4 GiB buffer views)");
  const size_t fbb = fb_bytes(n_bins, n_mels, n_cep);
  if (!workspace || workspace_bytes < fbb + mel_part_bytes(n_images, max_rows)) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  SsrMelParams p{};
  if (int rc = upload_fb(fb, n_bins, n_mels, n_cep, nnz, ws, s, &p.f)) return rc;
  p.x = est_sp; p.y = tgt_sp; p.x_row = est_frame_off; p.y_row = tgt_frame_off; p.n_rows = n_rows;
  p.F = n_bins; p.pitch = n_bins; p.n_items = n_images; p.kg = 1; p.which = which; p.part = (double*)(ws + fbb);
  return launch_mel(p, 1, max_rows, out, s);
}

// ----------------------------------------------------------------------------------------------------
// waveform level: K + 1 magnitude images per item (ssr_pair_images), then the reduction
struct MelWs { SsrPairGeom g; SsrPairImages im; size_t off_fb, off_part, off_rows, total; };
static MelWs mel_ws(const ssr_plan* pl, int n_items, int n_keys, int max_len, int64_t total_rows, int n_mels, int n_cep, bool in64) {
  MelWs w;
  w.g = ssr_pair_geom(pl, n_items, max_len, in64);
  w.im = ssr_pair_images_layout(pl, n_keys, total_rows, in64);
  size_t o = w.im.end;
  w.off_fb = o; o += fb_bytes(pl->n_bins, n_mels, n_cep);
  w.off_part = o; o += mel_part_bytes((int64_t)n_keys * n_items, (int)ssr_num_frames(pl, max_len));
  w.off_rows = o; o += ssr_align256((size_t)n_items * sizeof(int32_t));
  w.total = o;
  return w;
}

extern "C" size_t ssr_pair_mel_metrics_workspace_bytes(const ssr_plan* pl, int n_items, int n_keys, int max_len, int64_t total_rows,
                                                      int n_mels, int n_cep) {
  if (!pl || n_items <= 0 || n_keys <= 0 || max_len < 1 || n_mels < 2 || n_mels > SSR_MEL_MAX || n_cep < 1 || n_cep >= n_mels) return 0;
  const size_t a = mel_ws(pl, n_items, n_keys, max_len, total_rows, n_mels, n_cep, false).total;
  const size_t b = mel_ws(pl, n_items, n_keys, max_len, total_rows, n_mels, n_cep, true).total;
  return a > b ? a : b;
}

static int pair_mel_impl(const ssr_plan* pl, const float* est, const double* est64, const int64_t* est_off, const float* tgt,
                         const int64_t* tgt_off, const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len,
                         int64_t total_rows, const float* fb, int n_mels, int n_cep, int which, double* out, void* workspace,
                         size_t workspace_bytes, void* stream) {
  int max_T, nnz = 0;
  if (int rc = ssr_check_pair_batch(pl, (est || est64) && est_off && tgt && tgt_off && len && frame_off && fb && out, n_items, n_keys, max_len,
                                    true, &max_T, [&] {
        if (int rc = check_which(which)) return rc;
        if (n_cep < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "n_cep must be in 1..n_mels - 1");
        return check_fb(fb, pl->n_bins, n_mels, n_cep, &nnz);
      }))
    return rc;
  if (!max_T) return SSR_OK;
  const MelWs w = mel_ws(pl, n_items, n_keys, max_len, total_rows, n_mels, n_cep, est64 != nullptr);
  // the contract is the size the query reports - one size for both entry points - not this layout's own (smaller or equal) need
  if (!workspace || workspace_bytes < ssr_pair_mel_metrics_workspace_bytes(pl, n_items, n_keys, max_len, total_rows, n_mels, n_cep))
    return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  SsrMelParams p{};
  if (int rc = upload_fb(fb, pl->n_bins, n_mels, n_cep, nnz, ws + w.off_fb, s, &p.f)) return rc;
  int32_t* rows = (int32_t*)(ws + w.off_rows);
  if (int rc = ssr_launch_rows_from_len(pl, len, n_items, rows, s)) return rc;
  if (int rc = ssr_pair_images(pl, {len, frame_off, n_items, w.g}, est, est64, est_off, tgt, tgt_off, n_keys, w.im, ws, s)) return rc;
  p.x = (float*)(ws + w.im.off_est); p.y = (float*)(ws + w.im.off_tgt); p.x_row = frame_off; p.y_row = frame_off; p.n_rows = rows;
  p.x_plane = (int64_t)(w.im.plane / sizeof(float));
  p.F = pl->n_bins; p.pitch = ssr_mag_pitch(pl->n_bins); p.n_items = n_items; p.kg = ssr_keys_per_wave(n_keys); p.which = which;
  p.part = (double*)(ws + w.off_part);
  return launch_mel(p, n_keys, max_T, out, s);
}

extern "C" int ssr_pair_mel_metrics(const ssr_plan* pl, const float* est, const int64_t* est_off, const float* tgt, const int64_t* tgt_off,
                                    const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len, int64_t total_rows,
                                    const float* fb, int n_mels, int n_cep, int which, double* out, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (!est) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  return pair_mel_impl(pl, est, nullptr, est_off, tgt, tgt_off, len, frame_off, n_items, n_keys, max_len, total_rows, fb, n_mels, n_cep,
                       which, out, workspace, workspace_bytes, stream);
}

extern "C" int ssr_pair_mel_metrics_est64(const ssr_plan* pl, const double* est, const int64_t* est_off, const float* tgt,
                                          const int64_t* tgt_off, const int32_t* len, const int64_t* frame_off, int n_items, int n_keys,
                                          int max_len, int64_t total_rows, const float* fb, int n_mels, int n_cep, int which, double* out,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  if (!est) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  return pair_mel_impl(pl, nullptr, est, est_off, tgt, tgt_off, len, frame_off, n_items, n_keys, max_len, total_rows, fb, n_mels, n_cep,
                       which, out, workspace, workspace_bytes, stream);
}
