// libssrhip.so translation unit: YIN F0 tracking and the pitch pair metrics on 16 kHz float64 signals (ssr_pitch.h) and their
// entry points (ssr_f0_track, ssr_f0_metrics and their workspace queries).
#include "ssr_host.h"
#include "ssr_pitch.h"

__global__ __launch_bounds__(SSR_PITCH_NT) void k_pitch_geometry(SsrPitchParams p) {
  __shared__ int64_t sums[2 * SSR_PITCH_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_pitch_geometry_body(p, blk, sums);
}

__global__ __launch_bounds__(SSR_PITCH_NT) void k_pitch_track(SsrPitchParams p) {
  __shared__ double xs[SSR_PITCH_XS], d[SSR_PITCH_F * SSR_PITCH_TAU_MAX];
  __shared__ double wsum[SSR_PITCH_NT], wpart[SSR_PITCH_NT], wmin[SSR_PITCH_NT];
  __shared__ int wtau[SSR_PITCH_NT], wcand[SSR_PITCH_NT], wfirst[SSR_PITCH_NT / 64];
  SsrBlk blk{(int)threadIdx.x};
  ssr_pitch_track_body(p, blk, (int64_t)blockIdx.x, xs, d, wsum, wpart, wmin, wtau, wcand, wfirst);
}

__global__ __launch_bounds__(SSR_PITCH_NT) void k_pitch_voicing(SsrPitchParams p) {
  __shared__ double red[SSR_PITCH_NT + 1];
  SsrBlk blk{(int)threadIdx.x};
  ssr_pitch_voicing_body(p, blk, (int)blockIdx.x, red);
}

__global__ __launch_bounds__(SSR_PITCH_NT) void k_pitch_pairs(SsrPitchParams p) {
  __shared__ double red[5 * SSR_PITCH_NT], mm[4 * SSR_PITCH_NT], tot[12];
  __shared__ int64_t cnt[3 * SSR_PITCH_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_pitch_pair_body(p, blk, (int)blockIdx.x, red, cnt, mm, tot);
}

// host-side validation: nothing is queued unless every argument is usable
static int check_pitch_range(double fmin, double fmax) {
  if (!(fmin >= 40.0 && fmin < fmax && fmax <= 1000.0)) return ssr_fail(SSR_ERR_INVALID_ARG, "fmin / fmax must satisfy 40 <= fmin < fmax <= 1000");
  if (ssr_pitch_tau_hi(fmin) - ssr_pitch_tau_lo(fmax) < 2) return ssr_fail(SSR_ERR_INVALID_ARG, "fmin / fmax leave fewer than three lags");
  return SSR_OK;
}

static int check_pitch_lens(const int32_t* len, int n) {
  if (n < 0) return ssr_fail(SSR_ERR_INVALID_ARG, "signal counts must be >= 0");
  if (n > 0 && !len) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int i = 0; i < n; ++i)
    if (len[i] < 0 || len[i] >= (1 << 29)) return ssr_fail(SSR_ERR_INVALID_ARG, "lengths must be in [0, 2^29)");
  return SSR_OK;
}

static int check_metrics_args(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, double fmin, double fmax,
                              int which) {
  if (which < 1 || which > 31) return ssr_fail(SSR_ERR_INVALID_ARG, "which must be a non-empty combination of the SSR_PITCH_* bits");
  if (int rc = check_pitch_range(fmin, fmax)) return rc;
  return ssr_check_pair_index(tgt_len, n_tgt, tgt_index, n_est, 1 << 29, "lengths must be in [0, 2^29)", "signal counts must be >= 0");
}

// workspace layout: a deterministic function of the lengths (and the pair -> target map)
struct PitchWs { size_t off_len, off_idx, off_tp, off_fp, off_f0, off_ap, off_en, off_vo, total; int64_t tiles, frames; };
static PitchWs pitch_ws(const int32_t* len, int n_a, const int32_t* idx, int n_b, bool tracks) {
  PitchWs w{};
  for (int i = 0; i < n_a + n_b; ++i) {
    const int64_t m = i < n_a ? len[i] : len[idx[i - n_a]];
    w.tiles += ssr_pitch_tiles(m);
    w.frames += ssr_pitch_frames(m);
  }
  const size_t nf = tracks ? (size_t)w.frames : 0;
  SsrWsLayout l;
  w.off_len = l.take((size_t)n_a * sizeof(int32_t));
  w.off_idx = l.take((size_t)n_b * sizeof(int32_t));
  w.off_tp = l.take((size_t)(n_a + n_b + 1) * sizeof(int64_t));
  w.off_fp = l.take((size_t)(n_a + n_b + 1) * sizeof(int64_t));
  w.off_f0 = l.take(nf * sizeof(double));
  w.off_ap = l.take(nf * sizeof(double));
  w.off_en = l.take(nf * sizeof(double));
  w.off_vo = l.take(nf);
  w.total = l.o;
  return w;
}

static void pitch_options(SsrPitchParams& p, double fmin, double fmax) {
  p.tau_lo = ssr_pitch_tau_lo(fmax); p.tau_hi = ssr_pitch_tau_hi(fmin); p.nb = ssr_pitch_runs(p.tau_hi);
}

// geometry, tracker and voicing for the n_a + n_b signals of p
static int launch_tracks(SsrPitchParams& p, int64_t tiles, hipStream_t s) {
  SSR_LAUNCH(k_pitch_geometry, dim3(1), dim3(SSR_PITCH_NT), s, p);
  if (tiles > 0) SSR_LAUNCH(k_pitch_track, dim3((unsigned)tiles), dim3(SSR_PITCH_NT), s, p);
  SSR_LAUNCH(k_pitch_voicing, dim3((unsigned)(p.n_a + p.n_b)), dim3(SSR_PITCH_NT), s, p);
  return SSR_OK;
}

extern "C" size_t ssr_f0_track_workspace_bytes(const int32_t* len, int n, double fmin, double fmax) {
  if (check_pitch_range(fmin, fmax) || check_pitch_lens(len, n)) return 0;
  return pitch_ws(len, n, nullptr, 0, false).total;
}

extern "C" int ssr_f0_track(const double* sig, const int64_t* off, const int32_t* len, int n, double fmin, double fmax, double* f0,
                            double* aperiodicity, double* energy, uint8_t* voiced, const int64_t* frame_off, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (int rc = check_pitch_range(fmin, fmax)) return rc;
  if (int rc = check_pitch_lens(len, n)) return rc;
  if (n == 0) return SSR_OK;
  const PitchWs w = pitch_ws(len, n, nullptr, 0, false);
  if (!off || !frame_off || (w.frames > 0 && (!sig || !f0 || !aperiodicity || !energy || !voiced)))
    return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  if (w.tiles > 0x7fffffff) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* len_dev = (int32_t*)(ws + w.off_len);
  // (host array: from page-locked memory this copy is asynchronous - the caller keeps it until the stream has passed)
  HIP_TRY(hipMemcpyAsync(len_dev, len, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  SsrPitchParams p{};
  p.sig_a = sig; p.off_a = off; p.len_a = len_dev; p.n_a = n; p.n_b = 0;
  pitch_options(p, fmin, fmax);
  p.tile_pre = (int64_t*)(ws + w.off_tp); p.frame_pre = (int64_t*)(ws + w.off_fp); p.frame_off = frame_off;
  p.f0 = f0; p.ap = aperiodicity; p.en = energy; p.voiced = voiced;
  return launch_tracks(p, w.tiles, s);
}

extern "C" size_t ssr_f0_metrics_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, double fmin,
                                                 double fmax, int which) {
  if (check_metrics_args(tgt_len, n_tgt, tgt_index, n_est, fmin, fmax, which)) return 0;
  return pitch_ws(tgt_len, n_tgt, tgt_index, n_est, true).total;
}

extern "C" int ssr_f0_metrics(const double* tgt, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const double* est,
                              const int64_t* est_off, const int32_t* tgt_index, int n_est, double fmin, double fmax, int which,
                              double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_metrics_args(tgt_len, n_tgt, tgt_index, n_est, fmin, fmax, which)) return rc;
  if (n_est == 0) return SSR_OK;
  const PitchWs w = pitch_ws(tgt_len, n_tgt, tgt_index, n_est, true);
  if (!tgt_off || !est_off || !out || (w.frames > 0 && (!tgt || !est))) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  if (w.tiles > 0x7fffffff) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* len_dev = (int32_t*)(ws + w.off_len);
  int32_t* idx_dev = (int32_t*)(ws + w.off_idx);
  if (int rc = ssr_upload_pair_index(tgt_len, n_tgt, tgt_index, n_est, len_dev, idx_dev, s)) return rc;
  SsrPitchParams p{};
  p.sig_a = tgt; p.off_a = tgt_off; p.sig_b = est; p.off_b = est_off; p.len_a = len_dev; p.idx_b = idx_dev;
  p.n_a = n_tgt; p.n_b = n_est;
  pitch_options(p, fmin, fmax);
  p.tile_pre = (int64_t*)(ws + w.off_tp); p.frame_pre = (int64_t*)(ws + w.off_fp); p.frame_off = p.frame_pre;
  p.f0 = (double*)(ws + w.off_f0); p.ap = (double*)(ws + w.off_ap); p.en = (double*)(ws + w.off_en);
  p.voiced = (uint8_t*)(ws + w.off_vo);
  p.which = which; p.out = out;
  if (int rc = launch_tracks(p, w.tiles, s)) return rc;
  SSR_LAUNCH(k_pitch_pairs, dim3((unsigned)n_est), dim3(SSR_PITCH_NT), s, p);
  return SSR_OK;
}
