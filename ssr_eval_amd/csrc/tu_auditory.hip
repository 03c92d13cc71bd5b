// libssrhip.so translation unit: the auditory family on float32 / float64 signals (ssr_auditory.h) and its entry points
// (ssr_auditory, ssr_auditory_workspace_bytes).
#include "ssr_host.h"
#include "ssr_auditory.h"

static_assert(SSR_AUD_MIN_BANDS == SSR_AUDITORY_MIN_BANDS && SSR_AUD_MAX_BANDS == SSR_AUDITORY_MAX_BANDS, "the band limits are the C ABI's");
static_assert(SSR_AUD_MAX_BLOCKS == SSR_AUDITORY_MAX_BLOCKS && SSR_AUD_PAIR_COLS == SSR_AUDITORY_PAIR_COLS, "the block limit and the row width are the C ABI's");

__global__ __launch_bounds__(SSR_AUD_NT) void k_aud_geometry(SsrAudParams p) {
  __shared__ int64_t sums[3 * SSR_AUD_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_aud_geometry_body(p, blk, sums);
}

// g0: the first workgroup of the side (targets: 0, estimates: the targets' workgroups) whose element type is X
template <typename X, bool SECOND> __global__ __launch_bounds__(SSR_AUD_NT) void k_aud_sweep(SsrAudParams p, int64_t g0) {
  __shared__ SsrAudSweepLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_aud_sweep_body<X, SECOND>(p, blk, g0 + (int64_t)blockIdx.x, lds);
}

__global__ __launch_bounds__(64) void k_aud_scan(SsrAudParams p) { ssr_aud_scan_lane(p, (int64_t)blockIdx.x * 64 + threadIdx.x); }

// s0: the first signal of the launch (the targets' launch comes before the estimates')
__global__ __launch_bounds__(SSR_AUD_NT) void k_aud_image(SsrAudParams p, int s0) {
  __shared__ SsrAudImageLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_aud_image_body(p, blk, s0 + (int)blockIdx.x, lds);
}

__global__ __launch_bounds__(SSR_AUD_NT) void k_aud_score(SsrAudParams p) {
  __shared__ SsrAudScoreLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_aud_score_body(p, blk, (int)blockIdx.x, lds);
}

// workspace layout: a deterministic function of the target lengths, the pair -> target map, hop and the band count
struct AudWs {
  size_t off_len, off_idx, off_split, off_tab, off_si, off_so, off_wo, off_ro, off_state, off_blk, off_stat, off_gimg, total;
  int64_t segs, tgt_wgs, est_wgs, rows;
};
static AudWs aud_ws(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int hop, int n_bands) {
  AudWs w{};
  const int cp = ssr_aud_lanes(n_bands);
  for (int t = 0; t < n_tgt; ++t) {
    w.segs += ssr_aud_segments(tgt_len[t], hop); w.tgt_wgs += ssr_aud_wgs(tgt_len[t], hop, cp); w.rows += ssr_aud_rows(tgt_len[t], hop);
  }
  for (int e = 0; e < n_est; ++e) {
    const int n = tgt_len[tgt_index[e]];
    w.segs += ssr_aud_segments(n, hop); w.est_wgs += ssr_aud_wgs(n, hop, cp); w.rows += ssr_aud_rows(n, hop);
  }
  const size_t n_sig = (size_t)n_tgt + (size_t)n_est, C = (size_t)n_bands;
  SsrWsLayout l;
  w.off_len = l.take((size_t)n_tgt * sizeof(int32_t));
  w.off_idx = l.take((size_t)n_est * sizeof(int32_t));
  w.off_split = l.take((size_t)n_est * sizeof(int32_t));
  w.off_tab = l.take(C * SSR_AUD_TAB * sizeof(double));
  w.off_si = l.take(n_sig * sizeof(int32_t));
  w.off_so = l.take((n_sig + 1) * sizeof(int64_t));
  w.off_wo = l.take((n_sig + 1) * sizeof(int64_t));
  w.off_ro = l.take((n_sig + 1) * sizeof(int64_t));
  w.off_state = l.take((size_t)w.segs * C * 8 * sizeof(double));
  w.off_blk = l.take((size_t)w.segs * SSR_AUD_SEG * C * sizeof(double));
  w.off_stat = l.take(n_sig * 2 * sizeof(double));
  w.off_gimg = l.take((size_t)w.rows * C * sizeof(double));
  w.total = l.o;
  return w;
}

// host-side validation: nothing is queued unless every argument is usable
static int check_aud_args(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int hop, int n_bands) {
  if (hop < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "hop must be >= 1");
  if (n_bands < SSR_AUDITORY_MIN_BANDS || n_bands > SSR_AUDITORY_MAX_BANDS) return ssr_fail(SSR_ERR_INVALID_ARG, "n_bands must be in [3, 64]");
  if (int rc = ssr_check_pair_index(tgt_len, n_tgt, tgt_index, n_est, (int64_t)1 << 29, "target lengths must be in [0, 2^29)")) return rc;
  if ((int64_t)n_tgt + n_est > (1 << 24)) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  for (int t = 0; t < n_tgt; ++t)
    if (ssr_aud_blocks(tgt_len[t], hop) > SSR_AUDITORY_MAX_BLOCKS)
      return ssr_fail(SSR_ERR_UNSUPPORTED, "a signal may hold at most 65536 hop-blocks");
  return SSR_OK;
}

extern "C" size_t ssr_auditory_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int hop, int n_bands) {
  if (check_aud_args(tgt_len, n_tgt, tgt_index, n_est, hop, n_bands)) return 0;
  return aud_ws(tgt_len, n_tgt, tgt_index, n_est, hop, n_bands).total;
}

extern "C" int ssr_auditory(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                            int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int hop, int n_bands,
                            const double* coef, double range_db, int match_level, const int32_t* split_band, double* pair_out,
                            double* band_out, double* image_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_aud_args(tgt_len, n_tgt, tgt_index, n_est, hop, n_bands)) return rc;
  if (!(range_db > 0.0 && range_db <= 150.0)) return ssr_fail(SSR_ERR_INVALID_ARG, "range_db must be in (0, 150]");
  if (!coef) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int c = 0; c < n_bands; ++c) {
    const double ar = coef[3 * c], ai = coef[3 * c + 1], g = coef[3 * c + 2];
    if (!(ar * ar + ai * ai < 1.0) || !(fabs(g) <= 1.7e308))
      return ssr_fail(SSR_ERR_INVALID_ARG, "coef must hold finite (Re a, Im a, g) with |a| < 1");
  }
  if (n_est > 0 && !split_band) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int e = 0; e < n_est; ++e)
    if (split_band[e] < -1 || split_band[e] == 0 || split_band[e] > n_bands - 1)
      return ssr_fail(SSR_ERR_INVALID_ARG, "split_band must be -1 or in [1, n_bands - 1]");
  if (n_tgt + n_est == 0) return SSR_OK;
  int64_t tgt_samples = 0, est_samples = 0;
  for (int t = 0; t < n_tgt; ++t) tgt_samples += tgt_len[t];
  for (int e = 0; e < n_est; ++e) est_samples += tgt_len[tgt_index[e]];
  if ((n_tgt > 0 && !tgt_off) || (n_est > 0 && (!est_off || !pair_out)) || (tgt_samples > 0 && !tgt) || (est_samples > 0 && !est))
    return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  const AudWs w = aud_ws(tgt_len, n_tgt, tgt_index, n_est, hop, n_bands);
  const int n_sig = n_tgt + n_est;
  // (the launches stay below 2^32 threads, which every HIP runtime takes)
  if ((w.tgt_wgs + w.est_wgs) * SSR_AUD_NT > 0xffffffffLL || (int64_t)n_sig * SSR_AUD_NT > 0xffffffffLL)
    return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  // the table of the call: kept for the life of the process (the asynchronous copy reads it after the call returned)
  static SsrHostTables<std::vector<double>, std::vector<double>> tables;
  std::vector<double> key(coef, coef + 3 * (size_t)n_bands);
  key.push_back((double)hop);
  const std::vector<double>& tab = tables.get(key, [&](std::vector<double>& t) { ssr_aud_tables_host(coef, n_bands, hop, t); });
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* len_dev = (int32_t*)(ws + w.off_len);
  int32_t* idx_dev = (int32_t*)(ws + w.off_idx);
  if (n_tgt) HIP_TRY(hipMemcpyAsync(len_dev, tgt_len, (size_t)n_tgt * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (n_est) HIP_TRY(hipMemcpyAsync(idx_dev, tgt_index, (size_t)n_est * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (n_est) HIP_TRY(hipMemcpyAsync(ws + w.off_split, split_band, (size_t)n_est * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ws + w.off_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
  SsrAudParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, len_dev, idx_dev, n_tgt, n_est);
  p.hop = hop; p.C = n_bands; p.CP = ssr_aud_lanes(n_bands); p.range_db = range_db; p.match = match_level != 0;
  p.tab = (const double*)(ws + w.off_tab); p.split = (const int32_t*)(ws + w.off_split);
  p.sig_index = (int32_t*)(ws + w.off_si);
  p.seg_off = (int64_t*)(ws + w.off_so); p.wg_off = (int64_t*)(ws + w.off_wo); p.row_off = (int64_t*)(ws + w.off_ro);
  p.state = (double*)(ws + w.off_state); p.blk = (double*)(ws + w.off_blk); p.stat = (double*)(ws + w.off_stat);
  p.gimg = (double*)(ws + w.off_gimg);
  p.pair_out = pair_out; p.band_out = band_out; p.image_out = image_out;
  SSR_LAUNCH(k_aud_geometry, dim3(1), dim3(SSR_AUD_NT), s, p);
  const int64_t first[2] = {0, w.tgt_wgs}, count[2] = {w.tgt_wgs, w.est_wgs};
  const int f64[2] = {tgt_f64, est_f64};
  for (int second = 0; second < 2; ++second) {
    for (int side = 0; side < 2; ++side) {
      if (count[side] == 0) continue;
      const dim3 grid((unsigned)count[side]), block(SSR_AUD_NT);
      if (f64[side] && !second) SSR_LAUNCH((k_aud_sweep<double, false>), grid, block, s, p, first[side]);
      else if (f64[side]) SSR_LAUNCH((k_aud_sweep<double, true>), grid, block, s, p, first[side]);
      else if (!second) SSR_LAUNCH((k_aud_sweep<float, false>), grid, block, s, p, first[side]);
      else SSR_LAUNCH((k_aud_sweep<float, true>), grid, block, s, p, first[side]);
    }
    if (!second && w.segs > 0) SSR_LAUNCH(k_aud_scan, dim3((unsigned)(((int64_t)n_sig * n_bands + 63) / 64)), dim3(64), s, p);
  }
  if (n_tgt) SSR_LAUNCH(k_aud_image, dim3((unsigned)n_tgt), dim3(SSR_AUD_NT), s, p, 0);
  if (n_est) SSR_LAUNCH(k_aud_image, dim3((unsigned)n_est), dim3(SSR_AUD_NT), s, p, n_tgt);
  if (n_est) SSR_LAUNCH(k_aud_score, dim3((unsigned)n_est), dim3(SSR_AUD_NT), s, p);
  return SSR_OK;
}
