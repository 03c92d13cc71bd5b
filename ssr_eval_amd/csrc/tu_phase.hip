// libssrhip.so translation unit: the anti-wrapping phase distances IP, GD and IAF on float32 / float64 signals (ssr_phase.h) and
// its entry points (ssr_phase_metrics, ssr_phase_metrics_workspace_bytes).
#include "ssr_host.h"
#include "ssr_phase.h"

__global__ __launch_bounds__(SSR_PHASE_NT) void k_phase_geometry(SsrPhaseParams p) {
  __shared__ int64_t sums[SSR_PHASE_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_phase_geometry_body(p, blk, sums);
}

template <typename TT, typename TE, int LOGN> __global__ __launch_bounds__((1 << LOGN) / 8) void k_phase_dist(SsrPhaseParams p) {
  __shared__ SsrPhaseLds<LOGN> lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_phase_dist_body<TT, TE, LOGN>(p, blk, (int64_t)blockIdx.x, lds);
}

__global__ __launch_bounds__(SSR_PHASE_FIN_NT) void k_phase_finalize(SsrPhaseParams p) {
  SsrBlk blk{(int)threadIdx.x};
  ssr_phase_finalize_body(p, blk, (int)blockIdx.x);
}

// workspace layout: a deterministic function of the target lengths, the pair -> target map, n_fft and hop
struct PhaseWs { size_t off_len, off_idx, off_co, off_tw, off_part, total; int64_t chunks; };
static PhaseWs phase_ws(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft, int hop) {
  PhaseWs w{};
  for (int e = 0; e < n_est; ++e) w.chunks += ssr_phase_chunks(tgt_len[tgt_index[e]], n_fft, hop);
  SsrWsLayout l;
  w.off_len = l.take((size_t)n_tgt * sizeof(int32_t));
  w.off_idx = l.take((size_t)n_est * sizeof(int32_t));
  w.off_co = l.take((size_t)(n_est + 1) * sizeof(int64_t));
  w.off_tw = l.take((size_t)n_fft * sizeof(cx<double>));
  w.off_part = l.take((size_t)w.chunks * 3 * sizeof(double));
  w.total = l.o;
  return w;
}

// host-side validation: nothing is queued unless every argument is usable
static int check_phase_args(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft, int hop, int which) {
  if (which < 1 || which > 7)
    return ssr_fail(SSR_ERR_INVALID_ARG, "which must be a non-empty combination of SSR_PHASE_IP, SSR_PHASE_GD, SSR_PHASE_IAF");
  if (ssr_phase_log2_nfft(n_fft) < 0) return ssr_fail(SSR_ERR_INVALID_ARG, "n_fft must be 256, 512, 1024 or 2048");
  if (hop < 1 || hop > n_fft) return ssr_fail(SSR_ERR_INVALID_ARG, "hop must be in [1, n_fft]");
  return ssr_check_pair_index(tgt_len, n_tgt, tgt_index, n_est, (int64_t)1 << 29, "target lengths must be in [0, 2^29)");
}

extern "C" size_t ssr_phase_metrics_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft,
                                                    int hop, int which) {
  if (check_phase_args(tgt_len, n_tgt, tgt_index, n_est, n_fft, hop, which)) return 0;
  return phase_ws(tgt_len, n_tgt, tgt_index, n_est, n_fft, hop).total;
}

extern "C" int ssr_phase_metrics(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt,
                                 const void* est, int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_fft,
                                 int hop, int bin_lo, int bin_hi, int which, double* out, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  if (int rc = check_phase_args(tgt_len, n_tgt, tgt_index, n_est, n_fft, hop, which)) return rc;
  if (bin_lo < 0 || bin_lo > bin_hi || bin_hi > n_fft / 2) return ssr_fail(SSR_ERR_INVALID_ARG, "bins must satisfy 0 <= bin_lo <= bin_hi <= n_fft / 2");
  if (n_est == 0) return SSR_OK;
  if (int rc = ssr_check_pair_buffers(tgt, tgt_off, est, est_off, out, tgt_len, n_tgt)) return rc;
  const PhaseWs w = phase_ws(tgt_len, n_tgt, tgt_index, n_est, n_fft, hop);
  // (one workgroup per chunk: the launch stays below 2^32 threads, which every HIP runtime takes)
  if (w.chunks * (n_fft / 8) > 0xffffffffLL) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  const std::vector<cx<double>>& tw = ssr_twiddles_cached(n_fft);
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* len_dev = (int32_t*)(ws + w.off_len);
  int32_t* idx_dev = (int32_t*)(ws + w.off_idx);
  if (int rc = ssr_upload_pair_index(tgt_len, n_tgt, tgt_index, n_est, len_dev, idx_dev, s)) return rc;
  // (the table is cached for the life of the process: the caller need not keep it)
  HIP_TRY(hipMemcpyAsync(ws + w.off_tw, tw.data(), tw.size() * sizeof(cx<double>), hipMemcpyHostToDevice, s));
  SsrPhaseParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, len_dev, idx_dev, n_tgt, n_est);
  p.which = which; p.N = n_fft; p.H = hop; p.k_lo = bin_lo; p.k_hi = bin_hi;
  p.tw = (const cx<double>*)(ws + w.off_tw); p.chunk_off = (int64_t*)(ws + w.off_co); p.part = (double*)(ws + w.off_part);
  p.out = out;
  SSR_LAUNCH(k_phase_geometry, dim3(1), dim3(SSR_PHASE_NT), s, p);
  if (w.chunks > 0) {
    const int rc = ssr_dispatch_pair_dtypes(tgt_f64, est_f64, [&](auto tt, auto te) {
      return ssr_dispatch_logn<SSR_PHASE_LOGN_MIN, SSR_PHASE_LOGN_MAX>(ssr_phase_log2_nfft(n_fft), [&](auto logn) -> int {
        constexpr int LOGN = decltype(logn)::value;
        SSR_LAUNCH((k_phase_dist<decltype(tt), decltype(te), LOGN>), dim3((unsigned)w.chunks), dim3((1u << LOGN) / 8), s, p);
        return SSR_OK;
      });
    });
    if (rc) return rc;
  }
  SSR_LAUNCH(k_phase_finalize, dim3((unsigned)ssr_ceil_div(n_est, SSR_PHASE_FIN_NT)), dim3(SSR_PHASE_FIN_NT), s, p);
  return SSR_OK;
}
