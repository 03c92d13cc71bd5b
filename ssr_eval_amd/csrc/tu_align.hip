// libssrhip.so translation unit: delay estimation and compensation on float32 / float64 signals (ssr_align.h) and its entry points
// (ssr_align, ssr_align_workspace_bytes).
#include "ssr_host.h"
#include "ssr_align.h"

static_assert(SSR_ALIGN_LAG_LIMIT == SSR_ALIGN_MAX_LAG && SSR_ALIGN_COLS == SSR_ALIGN_COLUMNS, "ssr_hip_align.h");

__global__ __launch_bounds__(SSR_ALIGN_NT) void k_align_geometry(SsrAlignParams p) {
  __shared__ int64_t sums[2 * SSR_ALIGN_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_align_geometry_body(p, blk, sums);
}

template <typename TT, typename TE> __global__ __launch_bounds__(SSR_ALIGN_NT) void k_align_corr(SsrAlignParams p) {
  __shared__ double xs[SSR_ALIGN_X_LDS], ys[SSR_ALIGN_Y_LDS], red[12];
  SsrBlk blk{(int)threadIdx.x};
  ssr_align_corr_body<TT, TE>(p, blk, (int64_t)blockIdx.x, xs, ys, red);
}

__global__ __launch_bounds__(64) void k_align_pick(SsrAlignParams p) {
  __shared__ double mx[128], hs[SSR_ALIGN_TAPS], st[8];
  SsrBlk blk{(int)threadIdx.x};
  ssr_align_pick_body(p, blk, (int)blockIdx.x, mx, hs, st);
}

template <typename TE> __global__ __launch_bounds__(SSR_ALIGN_NT) void k_align_shift(SsrAlignParams p) {
  __shared__ double ysh[SSR_ALIGN_S_LDS], hs[SSR_ALIGN_TAPS];
  SsrBlk blk{(int)threadIdx.x};
  ssr_align_shift_body<TE>(p, blk, (int64_t)blockIdx.x, ysh, hs);
}

// workspace layout: a deterministic function of the lengths, the pair -> target map and the largest lag
struct AlignWs { size_t off_len, off_elen, off_idx, off_pt, off_po, off_cp, off_ep, off_taps, total; int64_t pair_tiles, out_tiles; };
static AlignWs align_ws(const int32_t* tgt_len, int n_tgt, const int32_t* est_len, const int32_t* tgt_index, int n_est, int L) {
  AlignWs w{};
  for (int e = 0; e < n_est; ++e) {
    w.pair_tiles += ssr_align_tiles(tgt_len[tgt_index[e]]);
    w.out_tiles += ssr_align_out_tiles(est_len[e]);
  }
  SsrWsLayout l;
  w.off_len = l.take((size_t)n_tgt * sizeof(int32_t));
  w.off_elen = l.take((size_t)n_est * sizeof(int32_t));
  w.off_idx = l.take((size_t)n_est * sizeof(int32_t));
  w.off_pt = l.take((size_t)(n_est + 1) * sizeof(int64_t));
  w.off_po = l.take((size_t)(n_est + 1) * sizeof(int64_t));
  w.off_cp = l.take((size_t)w.pair_tiles * (2 * L + 1) * sizeof(double));
  w.off_ep = l.take((size_t)w.pair_tiles * 2 * sizeof(double));
  w.off_taps = l.take((size_t)n_est * SSR_ALIGN_TAPS * sizeof(double));
  w.total = l.o;
  return w;
}

// host-side validation: nothing is queued unless every argument is usable
static int check_align_args(const int32_t* tgt_len, int n_tgt, const int32_t* est_len, const int32_t* tgt_index, int n_est, int max_lag) {
  if (max_lag < 1 || max_lag > SSR_ALIGN_MAX_LAG) return ssr_fail(SSR_ERR_INVALID_ARG, "max_lag must be in [1, SSR_ALIGN_MAX_LAG]");
  if (int rc = ssr_check_pair_index(tgt_len, n_tgt, tgt_index, n_est, (int64_t)1 << 29, "signal lengths must be in [0, 2^29)")) return rc;
  if (n_est > 0 && !est_len) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int e = 0; e < n_est; ++e)
    if (est_len[e] < 0 || est_len[e] >= (1 << 29)) return ssr_fail(SSR_ERR_INVALID_ARG, "signal lengths must be in [0, 2^29)");
  return SSR_OK;
}

extern "C" size_t ssr_align_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* est_len, const int32_t* tgt_index,
                                            int n_est, int max_lag) {
  if (check_align_args(tgt_len, n_tgt, est_len, tgt_index, n_est, max_lag)) return 0;
  return align_ws(tgt_len, n_tgt, est_len, tgt_index, n_est, max_lag).total;
}

extern "C" int ssr_align(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                         int est_f64, const int64_t* est_off, const int32_t* est_len, const int32_t* tgt_index, int n_est, int max_lag,
                         int subsample, double* rows, void* shifted, const int64_t* shifted_off, double* c, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (int rc = check_align_args(tgt_len, n_tgt, est_len, tgt_index, n_est, max_lag)) return rc;
  if (n_est == 0) return SSR_OK;
  int64_t tgt_samples = 0, est_samples = 0;
  for (int e = 0; e < n_est; ++e) { tgt_samples += tgt_len[tgt_index[e]]; est_samples += est_len[e]; }
  if (!tgt_off || !est_off || !rows || (tgt_samples > 0 && !tgt) || (est_samples > 0 && !est) || (shifted && !shifted_off))
    return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  const AlignWs w = align_ws(tgt_len, n_tgt, est_len, tgt_index, n_est, max_lag);
  // (the launches stay below 2^32 threads, which every HIP runtime takes)
  if (w.pair_tiles * ssr_align_lag_blocks(max_lag) * SSR_ALIGN_NT > 0xffffffffLL || w.out_tiles * SSR_ALIGN_NT > 0xffffffffLL)
    return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* len_dev = (int32_t*)(ws + w.off_len);
  int32_t* idx_dev = (int32_t*)(ws + w.off_idx);
  if (int rc = ssr_upload_pair_index(tgt_len, n_tgt, tgt_index, n_est, len_dev, idx_dev, s)) return rc;
  HIP_TRY(hipMemcpyAsync(ws + w.off_elen, est_len, (size_t)n_est * sizeof(int32_t), hipMemcpyHostToDevice, s));
  SsrAlignParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, len_dev, idx_dev, n_tgt, n_est);
  p.est_len = (const int32_t*)(ws + w.off_elen); p.L = max_lag; p.subsample = subsample ? 1 : 0;
  p.pair_tile = (int64_t*)(ws + w.off_pt); p.pair_out = (int64_t*)(ws + w.off_po);
  p.cpart = (double*)(ws + w.off_cp); p.epart = (double*)(ws + w.off_ep); p.taps = (double*)(ws + w.off_taps);
  p.rows = rows; p.c = c; p.out = shifted; p.out_off = shifted_off;
  SSR_LAUNCH(k_align_geometry, dim3(1), dim3(SSR_ALIGN_NT), s, p);
  const dim3 nt(SSR_ALIGN_NT);
  const unsigned corr_grid = (unsigned)(w.pair_tiles * ssr_align_lag_blocks(max_lag));
  return ssr_dispatch_pair_dtypes(tgt_f64, est_f64, [&](auto tt, auto te) -> int {
    using TT = decltype(tt);
    using TE = decltype(te);
    if (corr_grid > 0) SSR_LAUNCH((k_align_corr<TT, TE>), dim3(corr_grid), nt, s, p);
    SSR_LAUNCH(k_align_pick, dim3((unsigned)n_est), dim3(64), s, p);
    if (shifted && w.out_tiles > 0) SSR_LAUNCH(k_align_shift<TE>, dim3((unsigned)w.out_tiles), nt, s, p);
    return SSR_OK;
  });
}
