// libssrhip.so translation unit: STOI / ESTOI on 10 kHz float64 signals (ssr_stoi.h) and its entry points (ssr_stoi,
// ssr_stoi_workspace_bytes, ssr_stoi_band_edges).
#include "ssr_host.h"
#include "ssr_stoi.h"

__global__ __launch_bounds__(SSR_STOI_NT) void k_stoi_geometry(SsrStoiParams p) {
  __shared__ int64_t sums[2 * SSR_STOI_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_stoi_geometry_body(p, blk, sums);
}

__global__ __launch_bounds__(256) void k_stoi_energy(SsrStoiParams p, int64_t n) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g < n) ssr_stoi_energy(p, g);
}

__global__ __launch_bounds__(SSR_STOI_NT) void k_stoi_vad(SsrStoiParams p) {
  __shared__ double red[SSR_STOI_NT];
  __shared__ int cnt[SSR_STOI_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_stoi_vad_body(p, blk, (int)blockIdx.x, red, cnt);
}

__global__ __launch_bounds__(SSR_STOI_NT) void k_stoi_bands(SsrStoiParams p) {
  __shared__ double re[SSR_STOI_NFFT], im[SSR_STOI_NFFT], twr[256], twi[256], pw[257];
  SsrBlk blk{(int)threadIdx.x};
  ssr_stoi_bands_body(p, blk, (int64_t)blockIdx.x, re, im, twr, twi, pw);
}

__global__ __launch_bounds__(SSR_STOI_SEG) void k_stoi_segments(SsrStoiParams p) {
  __shared__ double X[SSR_STOI_SEG_ROWS * SSR_STOI_BANDS], Y[SSR_STOI_SEG_ROWS * SSR_STOI_BANDS];
  __shared__ double rs[4 * SSR_STOI_BANDS * SSR_STOI_SEG], red[2 * SSR_STOI_SEG];
  SsrBlk blk{(int)threadIdx.x};
  ssr_stoi_segments_body(p, blk, (int64_t)blockIdx.x, X, Y, rs, red);
}

__global__ __launch_bounds__(256) void k_stoi_finalize(SsrStoiParams p) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < p.n_est) ssr_stoi_finalize(p, e);
}

extern "C" int ssr_stoi_band_edges(int32_t* lo, int32_t* hi) {
  if (!lo || !hi) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  int l[SSR_STOI_BANDS], h[SSR_STOI_BANDS];
  ssr_stoi_band_edges_host(l, h);
  for (int k = 0; k < SSR_STOI_BANDS; ++k) { lo[k] = l[k]; hi[k] = h[k]; }
  return SSR_OK;
}

// workspace layout: a deterministic function of the target lengths and the pair -> target map
struct StoiWs { size_t off_len, off_idx, off_fr, off_st, off_win, off_energy, off_kept, off_nkept, off_tob, off_part, total;
                int64_t tgt_frames, all_frames, tiles; };
static StoiWs stoi_ws(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est) {
  StoiWs w{};
  for (int t = 0; t < n_tgt; ++t) w.tgt_frames += ssr_stoi_frames(tgt_len[t]);
  w.all_frames = w.tgt_frames;
  for (int e = 0; e < n_est; ++e) {
    const int f = ssr_stoi_frames(tgt_len[tgt_index[e]]);
    w.all_frames += f;
    w.tiles += ssr_stoi_seg_tiles(f);
  }
  const int S = n_tgt + n_est;
  SsrWsLayout l;
  w.off_len = l.take((size_t)S * sizeof(int32_t));
  w.off_idx = l.take((size_t)n_est * sizeof(int32_t));
  w.off_fr = l.take((size_t)(S + 1) * sizeof(int64_t));
  w.off_st = l.take((size_t)(n_est + 1) * sizeof(int64_t));
  w.off_win = l.take(SSR_STOI_FRAME * sizeof(double));
  w.off_energy = l.take((size_t)w.tgt_frames * sizeof(double));
  w.off_kept = l.take((size_t)w.tgt_frames * sizeof(int32_t));
  w.off_nkept = l.take((size_t)n_tgt * sizeof(int32_t));
  w.off_tob = l.take((size_t)w.all_frames * SSR_STOI_BANDS * sizeof(double));
  w.off_part = l.take((size_t)w.tiles * 2 * sizeof(double));
  w.total = l.o;
  return w;
}

// host-side validation: nothing is queued unless every length and index is usable
static int check_stoi_args(const int32_t* tgt_len, int n_tgt, const int32_t* est_len, const int32_t* tgt_index, int n_est) {
  if (int rc = ssr_check_pair_index(tgt_len, n_tgt, tgt_index, n_est, 1 << 29, "target lengths must be in [0, 2^29)")) return rc;
  for (int e = 0; est_len && e < n_est; ++e)
    if (est_len[e] != tgt_len[tgt_index[e]]) return ssr_fail(SSR_ERR_INVALID_ARG, "an estimate's length differs from its target's");
  return SSR_OK;
}

extern "C" size_t ssr_stoi_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est) {
  if (check_stoi_args(tgt_len, n_tgt, nullptr, tgt_index, n_est)) return 0;
  return stoi_ws(tgt_len, n_tgt, tgt_index, n_est).total;
}

extern "C" int ssr_stoi(const double* tgt, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const double* est,
                        const int64_t* est_off, const int32_t* est_len, const int32_t* tgt_index, int n_est, int which, double* out,
                        void* workspace, size_t workspace_bytes, void* stream) {
  if (which < SSR_STOI || which > SSR_STOI_BOTH) return ssr_fail(SSR_ERR_INVALID_ARG, "which must be SSR_STOI, SSR_ESTOI or SSR_STOI_BOTH");
  if (n_est > 0 && (!tgt || !tgt_off || !tgt_len || !est || !est_off || !est_len || !tgt_index || !out))
    return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  if (int rc = check_stoi_args(tgt_len, n_tgt, est_len, tgt_index, n_est)) return rc;
  if (n_est == 0) return SSR_OK;
  const StoiWs w = stoi_ws(tgt_len, n_tgt, tgt_index, n_est);
  if (w.all_frames > 0x7fffffff || w.tiles > 0x7fffffff) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* len_dev = (int32_t*)(ws + w.off_len);
  int32_t* idx_dev = (int32_t*)(ws + w.off_idx);
  if (int rc = ssr_upload_pair_index(tgt_len, n_tgt, tgt_index, n_est, len_dev, idx_dev, s)) return rc;
  HIP_TRY(hipMemcpyAsync(len_dev + n_tgt, est_len, (size_t)n_est * sizeof(int32_t), hipMemcpyHostToDevice, s));   // (as those two)
  SsrStoiParams p{};
  p.tgt = tgt; p.tgt_off = tgt_off; p.est = est; p.est_off = est_off; p.len = len_dev; p.tgt_index = idx_dev;
  p.n_tgt = n_tgt; p.n_est = n_est; p.which = which;
  p.fr_off = (int64_t*)(ws + w.off_fr); p.st_off = (int64_t*)(ws + w.off_st); p.win = (double*)(ws + w.off_win);
  p.energy = (double*)(ws + w.off_energy); p.kept = (int32_t*)(ws + w.off_kept); p.n_kept = (int32_t*)(ws + w.off_nkept);
  p.tob = (double*)(ws + w.off_tob); p.part = (double*)(ws + w.off_part); p.out = out;
  ssr_stoi_band_edges_host(p.band_lo, p.band_hi);
  SSR_LAUNCH(k_stoi_geometry, dim3(1), dim3(SSR_STOI_NT), s, p);
  if (w.tgt_frames > 0) SSR_LAUNCH(k_stoi_energy, dim3((unsigned)ssr_ceil_div(w.tgt_frames, 256)), dim3(256), s, p, w.tgt_frames);
  if (n_tgt > 0) SSR_LAUNCH(k_stoi_vad, dim3((unsigned)n_tgt), dim3(SSR_STOI_NT), s, p);
  if (w.all_frames > 0) SSR_LAUNCH(k_stoi_bands, dim3((unsigned)w.all_frames), dim3(SSR_STOI_NT), s, p);
  if (w.tiles > 0) SSR_LAUNCH(k_stoi_segments, dim3((unsigned)w.tiles), dim3(SSR_STOI_SEG), s, p);
  SSR_LAUNCH(k_stoi_finalize, dim3((unsigned)ssr_ceil_div(n_est, 256)), dim3(256), s, p);
  return SSR_OK;
}
