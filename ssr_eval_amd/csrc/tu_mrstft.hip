// libssrhip.so translation unit: the multi-resolution STFT distance (spectral convergence and log-magnitude distance per
// resolution and their means) on float32 / float64 signals (ssr_mrstft.h) and its entry points (ssr_mrstft_metrics,
// ssr_mrstft_workspace_bytes).
#include <utility>

#include "ssr_host.h"
#include "ssr_mrstft.h"

__global__ __launch_bounds__(SSR_PHASE_NT) void k_mrstft_geometry(SsrMrstftSig p, SsrMrstftRes q) {
  __shared__ int64_t sums[SSR_PHASE_NT];
  SsrBlk blk{(int)threadIdx.x};
  const SsrPhaseParams g = ssr_mrstft_geometry_params(p, q);
  ssr_phase_geometry_body(g, blk, sums);
}

template <typename TT, typename TE, int LOGN>
__global__ __launch_bounds__((1 << LOGN) / 8) void k_mrstft_dist(SsrMrstftSig p, SsrMrstftRes q, double eps) {
  __shared__ SsrMrstftLds<LOGN> lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_mrstft_dist_body<TT, TE, LOGN>(p, q, eps, blk, (int64_t)blockIdx.x, lds);
}

__global__ __launch_bounds__(SSR_PHASE_FIN_NT) void k_mrstft_finalize(SsrMrstftSig p, SsrMrstftAll a) {
  SsrBlk blk{(int)threadIdx.x};
  ssr_mrstft_finalize_body(p, a, blk, (int)blockIdx.x);
}

// the window per (transform size, window length): built once on the host, never written again (the workspace copies read it)
static const std::vector<double>& mrstft_window(int n_fft, int win) {
  static SsrHostTables<std::pair<int, int>, std::vector<double>> tables;
  return tables.get({n_fft, win}, [&](std::vector<double>& w) { ssr_mrstft_window_host(n_fft, win, w); });
}

// workspace layout: a deterministic function of the target lengths, the pair -> target map and the resolutions' n_fft and hop
struct MrstftWs {
  size_t off_len, off_idx, total;
  size_t off_co[SSR_MRSTFT_MAX_RES], off_tw[SSR_MRSTFT_MAX_RES], off_win[SSR_MRSTFT_MAX_RES], off_part[SSR_MRSTFT_MAX_RES];
  int64_t chunks[SSR_MRSTFT_MAX_RES];
};
static MrstftWs mrstft_ws(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_res, const int32_t* n_fft,
                          const int32_t* hop) {
  MrstftWs w{};
  SsrWsLayout l;
  w.off_len = l.take((size_t)n_tgt * sizeof(int32_t));
  w.off_idx = l.take((size_t)n_est * sizeof(int32_t));
  for (int r = 0; r < n_res; ++r) {
    for (int e = 0; e < n_est; ++e) w.chunks[r] += ssr_phase_chunks(tgt_len[tgt_index[e]], n_fft[r], hop[r]);
    w.off_co[r] = l.take((size_t)(n_est + 1) * sizeof(int64_t));
    w.off_tw[r] = l.take((size_t)n_fft[r] * sizeof(cx<double>));
    w.off_win[r] = l.take((size_t)n_fft[r] * sizeof(double));
    w.off_part[r] = l.take((size_t)w.chunks[r] * 3 * sizeof(double));
  }
  w.total = l.o;
  return w;
}

// host-side validation: nothing is queued unless every argument is usable
static int check_mrstft_args(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_res, const int32_t* n_fft,
                             const int32_t* hop, const int32_t* win) {
  if (n_res < 1 || n_res > SSR_MRSTFT_MAX_RES) return ssr_fail(SSR_ERR_INVALID_ARG, "n_res must be in [1, 8]");
  if (!n_fft || !hop || !win) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int r = 0; r < n_res; ++r) {
    if (ssr_phase_log2_nfft(n_fft[r]) < 0) return ssr_fail(SSR_ERR_INVALID_ARG, "n_fft must be 256, 512, 1024 or 2048");
    if (hop[r] < 1 || hop[r] > n_fft[r]) return ssr_fail(SSR_ERR_INVALID_ARG, "hop must be in [1, n_fft]");
    if (win[r] < 2 || win[r] > n_fft[r]) return ssr_fail(SSR_ERR_INVALID_ARG, "win must be in [2, n_fft]");
  }
  return ssr_check_pair_index(tgt_len, n_tgt, tgt_index, n_est, (int64_t)1 << 29, "target lengths must be in [0, 2^29)");
}

extern "C" size_t ssr_mrstft_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_res,
                                             const int32_t* n_fft, const int32_t* hop, const int32_t* win) {
  if (check_mrstft_args(tgt_len, n_tgt, tgt_index, n_est, n_res, n_fft, hop, win)) return 0;
  return mrstft_ws(tgt_len, n_tgt, tgt_index, n_est, n_res, n_fft, hop).total;
}

extern "C" int ssr_mrstft_metrics(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt,
                                  const void* est, int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_res,
                                  const int32_t* n_fft, const int32_t* hop, const int32_t* win, const int32_t* bin_lo,
                                  const int32_t* bin_hi, double eps, double* out, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  if (int rc = check_mrstft_args(tgt_len, n_tgt, tgt_index, n_est, n_res, n_fft, hop, win)) return rc;
  if (!bin_lo || !bin_hi) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int r = 0; r < n_res; ++r)
    if (bin_lo[r] < 0 || bin_lo[r] > bin_hi[r] || bin_hi[r] > n_fft[r] / 2)
      return ssr_fail(SSR_ERR_INVALID_ARG, "bins must satisfy 0 <= bin_lo <= bin_hi <= n_fft / 2");
  if (!(eps > 0.0) || !(eps <= 1.7976931348623157e308)) return ssr_fail(SSR_ERR_INVALID_ARG, "eps must be finite and > 0");
  if (n_est == 0) return SSR_OK;
  if (int rc = ssr_check_pair_buffers(tgt, tgt_off, est, est_off, out, tgt_len, n_tgt)) return rc;
  const MrstftWs w = mrstft_ws(tgt_len, n_tgt, tgt_index, n_est, n_res, n_fft, hop);
  // (one workgroup per chunk: every launch stays below 2^32 threads, which every HIP runtime takes)
  for (int r = 0; r < n_res; ++r)
    if (w.chunks[r] * (n_fft[r] / 8) > 0xffffffffLL) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* len_dev = (int32_t*)(ws + w.off_len);
  int32_t* idx_dev = (int32_t*)(ws + w.off_idx);
  if (int rc = ssr_upload_pair_index(tgt_len, n_tgt, tgt_index, n_est, len_dev, idx_dev, s)) return rc;
  SsrMrstftSig p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, len_dev, idx_dev, n_tgt, n_est);
  SsrMrstftAll a{};
  a.n_res = n_res; a.out = out;
  for (int r = 0; r < n_res; ++r) {
    // (the tables are cached for the life of the process: the caller need not keep them)
    const std::vector<cx<double>>& tw = ssr_twiddles_cached(n_fft[r]);
    const std::vector<double>& wn = mrstft_window(n_fft[r], win[r]);
    HIP_TRY(hipMemcpyAsync(ws + w.off_tw[r], tw.data(), tw.size() * sizeof(cx<double>), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ws + w.off_win[r], wn.data(), wn.size() * sizeof(double), hipMemcpyHostToDevice, s));
    SsrMrstftRes& q = a.res[r];
    q.N = n_fft[r]; q.H = hop[r]; q.k_lo = bin_lo[r]; q.k_hi = bin_hi[r];
    q.tw = (const cx<double>*)(ws + w.off_tw[r]); q.win = (const double*)(ws + w.off_win[r]);
    q.chunk_off = (int64_t*)(ws + w.off_co[r]); q.part = (double*)(ws + w.off_part[r]);
  }
  for (int r = 0; r < n_res; ++r) {
    const SsrMrstftRes& q = a.res[r];
    SSR_LAUNCH(k_mrstft_geometry, dim3(1), dim3(SSR_PHASE_NT), s, p, q);
    if (w.chunks[r] > 0) {
      const int rc = ssr_dispatch_pair_dtypes(tgt_f64, est_f64, [&](auto tt, auto te) {
        return ssr_dispatch_logn<SSR_PHASE_LOGN_MIN, SSR_PHASE_LOGN_MAX>(ssr_phase_log2_nfft(q.N), [&](auto logn) -> int {
          constexpr int LOGN = decltype(logn)::value;
          SSR_LAUNCH((k_mrstft_dist<decltype(tt), decltype(te), LOGN>), dim3((unsigned)w.chunks[r]), dim3((1u << LOGN) / 8), s, p, q, eps);
          return SSR_OK;
        });
      });
      if (rc) return rc;
    }
  }
  SSR_LAUNCH(k_mrstft_finalize, dim3((unsigned)ssr_ceil_div(n_est, SSR_PHASE_FIN_NT)), dim3(SSR_PHASE_FIN_NT), s, p, a);
  return SSR_OK;
}
