// libssrhip.so translation unit: the filter-invariant SDR of BSS Eval on float32 / float64 signals (ssr_bss.h) and its entry
// points (ssr_bss_sdr, ssr_bss_sdr_workspace_bytes).
#include "ssr_host.h"
#include "ssr_bss.h"

__global__ __launch_bounds__(SSR_BSS_NT) void k_bss_geometry(SsrBssParams p) {
  __shared__ int64_t sums[3 * SSR_BSS_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_bss_geometry_body(p, blk, sums);
}

template <typename TT, typename TE> __global__ __launch_bounds__(SSR_BSS_NT) void k_bss_corr(SsrBssParams p) {
  __shared__ double xs[SSR_BSS_CORR_LDS], ys[SSR_BSS_CORR_LDS], part[SSR_BSS_PART_LDS];
  SsrBlk blk{(int)threadIdx.x};
  ssr_bss_corr_body<TT, TE>(p, blk, (int64_t)blockIdx.x, xs, ys, part);
}

__global__ __launch_bounds__(64) void k_bss_solve(SsrBssParams p) {
  __shared__ double rr[SSR_BSS_MAX_TAPS], bb[SSR_BSS_MAX_TAPS], av[SSR_BSS_MAX_TAPS], cv[SSR_BSS_MAX_TAPS], red[2], st[4], mx[128];
  SsrBlk blk{(int)threadIdx.x};
  ssr_bss_solve_body(p, blk, (int)blockIdx.x, rr, bb, av, cv, red, st, mx);
}

template <typename TT, typename TE> __global__ __launch_bounds__(SSR_BSS_NT) void k_bss_resid(SsrBssParams p) {
  __shared__ double xs[SSR_BSS_RESID_LDS], cs[SSR_BSS_MAX_TAPS], red[8];
  SsrBlk blk{(int)threadIdx.x};
  ssr_bss_resid_body<TT, TE>(p, blk, (int64_t)blockIdx.x, xs, cs, red);
}

__global__ __launch_bounds__(256) void k_bss_finalize(SsrBssParams p) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < p.n_est) ssr_bss_finalize(p, e);
}

// workspace layout: a deterministic function of the target lengths, the pair -> target map and the tap count
struct BssWs { size_t off_len, off_idx, off_rs, off_rt, off_pt, off_pr, off_rp, off_bp, off_c, off_fin, off_p2, total;
               int n_runs; int64_t run_tiles, pair_tiles; };
static BssWs bss_ws(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int taps) {
  BssWs w{};
  for (int e = 0; e < n_est; ++e) {
    const int64_t nt = ssr_bss_tiles(tgt_len[tgt_index[e]]);
    if (e == 0 || tgt_index[e] != tgt_index[e - 1]) { ++w.n_runs; w.run_tiles += nt; }
    w.pair_tiles += nt;
  }
  SsrWsLayout l;
  w.off_len = l.take((size_t)n_tgt * sizeof(int32_t));
  w.off_idx = l.take((size_t)n_est * sizeof(int32_t));
  w.off_rs = l.take((size_t)(w.n_runs + 1) * sizeof(int32_t));
  w.off_rt = l.take((size_t)(w.n_runs + 1) * sizeof(int64_t));
  w.off_pt = l.take((size_t)(n_est + 1) * sizeof(int64_t));
  w.off_pr = l.take((size_t)n_est * sizeof(int32_t));
  w.off_rp = l.take((size_t)w.run_tiles * taps * sizeof(double));
  w.off_bp = l.take((size_t)w.pair_tiles * taps * sizeof(double));
  w.off_c = l.take((size_t)n_est * taps * sizeof(double));
  w.off_fin = l.take((size_t)n_est * sizeof(double));
  w.off_p2 = l.take((size_t)w.pair_tiles * 2 * sizeof(double));
  w.total = l.o;
  return w;
}

// host-side validation: nothing is queued unless every argument is usable
static int check_bss_args(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int taps) {
  if (taps < 1 || taps > SSR_BSS_MAX_TAPS) return ssr_fail(SSR_ERR_INVALID_ARG, "taps must be in [1, SSR_BSS_MAX_TAPS]");
  return ssr_check_pair_index(tgt_len, n_tgt, tgt_index, n_est, (int64_t)1 << 29, "target lengths must be in [0, 2^29)");
}

extern "C" size_t ssr_bss_sdr_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int taps) {
  if (check_bss_args(tgt_len, n_tgt, tgt_index, n_est, taps)) return 0;
  return bss_ws(tgt_len, n_tgt, tgt_index, n_est, taps).total;
}

extern "C" int ssr_bss_sdr(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                           int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int taps, double* out,
                           double* filt, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_bss_args(tgt_len, n_tgt, tgt_index, n_est, taps)) return rc;
  if (n_est == 0) return SSR_OK;
  if (int rc = ssr_check_pair_buffers(tgt, tgt_off, est, est_off, out, tgt_len, n_tgt)) return rc;
  const BssWs w = bss_ws(tgt_len, n_tgt, tgt_index, n_est, taps);
  if (w.pair_tiles > 0x7fffffff) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* len_dev = (int32_t*)(ws + w.off_len);
  int32_t* idx_dev = (int32_t*)(ws + w.off_idx);
  if (int rc = ssr_upload_pair_index(tgt_len, n_tgt, tgt_index, n_est, len_dev, idx_dev, s)) return rc;
  SsrBssParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, len_dev, idx_dev, n_tgt, n_est);
  p.n_runs = w.n_runs; p.L = taps;
  p.run_start = (int32_t*)(ws + w.off_rs); p.run_tile = (int64_t*)(ws + w.off_rt); p.pair_tile = (int64_t*)(ws + w.off_pt);
  p.pair_run = (int32_t*)(ws + w.off_pr); p.rpart = (double*)(ws + w.off_rp); p.bpart = (double*)(ws + w.off_bp);
  p.c = (double*)(ws + w.off_c); p.fin = (double*)(ws + w.off_fin); p.part2 = (double*)(ws + w.off_p2);
  p.out = out; p.filt = filt;
  SSR_LAUNCH(k_bss_geometry, dim3(1), dim3(SSR_BSS_NT), s, p);
  const dim3 nt(SSR_BSS_NT);
  return ssr_dispatch_pair_dtypes(tgt_f64, est_f64, [&](auto tt, auto te) -> int {
    using TT = decltype(tt);
    using TE = decltype(te);
    if (w.run_tiles > 0) SSR_LAUNCH((k_bss_corr<TT, TE>), dim3((unsigned)w.run_tiles), nt, s, p);
    SSR_LAUNCH(k_bss_solve, dim3((unsigned)n_est), dim3(64), s, p);
    if (w.pair_tiles > 0) SSR_LAUNCH((k_bss_resid<TT, TE>), dim3((unsigned)w.pair_tiles), nt, s, p);
    SSR_LAUNCH(k_bss_finalize, dim3((unsigned)ssr_ceil_div(n_est, 256)), dim3(256), s, p);
    return SSR_OK;
  });
}
