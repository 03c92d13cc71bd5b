// libssrhip.so translation unit: the coherence speech intelligibility index on float32 / float64 signals (ssr_csii.h) and its
// entry points (ssr_csii, ssr_csii_workspace_bytes).
#include "ssr_host.h"
#include "ssr_csii.h"

static_assert(SSR_CSII_MAX_BANDS == SSR_CSII_BANDS && SSR_CSII_COLS == SSR_CSII_COLUMNS, "the limits are the C ABI's");

__global__ __launch_bounds__(SSR_CSII_NT) void k_csii_geometry(SsrCsiiParams p) {
  __shared__ int64_t sums[3 * SSR_CSII_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_csii_geometry_body(p, blk, sums);
}

template <typename TT> __global__ __launch_bounds__(SSR_CSII_NT) void k_csii_levels(SsrCsiiParams p) {
  __shared__ SsrCsiiLevelsLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_csii_levels_body<TT>(p, blk, (int)blockIdx.x, lds);
}

template <typename TT, typename TE, int LOGN> __global__ __launch_bounds__((1 << LOGN) / 8) void k_csii_spectra(SsrCsiiParams p) {
  __shared__ SsrCohLds<LOGN> lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_csii_spectra_body<TT, TE, LOGN>(p, blk, (int64_t)blockIdx.x, lds);
}

__global__ __launch_bounds__(SSR_CSII_NT) void k_csii_bands(SsrCsiiParams p) {
  __shared__ SsrCsiiBandsLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_csii_bands_body(p, blk, (int)blockIdx.x, lds);
}

// workspace layout: a deterministic function of the target lengths, the pair -> target map, n_fft, hop and the band count
struct CsiiWs {
  size_t off_len, off_idx, off_split, off_imp, off_so, off_rs, off_rc, off_co, off_tw, off_cls, off_part, total;
  int64_t chunks, segments;
};
static CsiiWs csii_ws(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft, int hop, int n_bands) {
  CsiiWs w{};
  for (int e = 0; e < n_est; ++e) w.chunks += ssr_coh_chunks(tgt_len[tgt_index[e]], n_fft, hop);
  for (int t = 0; t < n_tgt; ++t) w.segments += ssr_coh_segments(tgt_len[t], n_fft, hop);
  SsrWsLayout l;
  w.off_len = l.take((size_t)n_tgt * sizeof(int32_t));
  w.off_idx = l.take((size_t)n_est * sizeof(int32_t));
  w.off_split = l.take((size_t)n_est * sizeof(int32_t));
  w.off_imp = l.take((size_t)n_bands * sizeof(double));
  w.off_so = l.take((size_t)(n_tgt + 1) * sizeof(int64_t));
  w.off_rs = l.take((size_t)(n_est + 1) * sizeof(int32_t));
  w.off_rc = l.take((size_t)(n_est + 1) * sizeof(int64_t));
  w.off_co = l.take((size_t)(n_est + 1) * sizeof(int64_t));
  w.off_tw = l.take((size_t)n_fft * sizeof(cx<double>));
  w.off_cls = l.take((size_t)w.segments);
  w.off_part = l.take((size_t)w.chunks * SSR_CSII_SETS * (n_fft / 2 + 1) * 4 * sizeof(double));
  w.total = l.o;
  return w;
}

// host-side validation: nothing is queued unless every argument is usable
static int check_csii_args(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft, int hop, int n_bands) {
  if (ssr_phase_log2_nfft(n_fft) < 0) return ssr_fail(SSR_ERR_INVALID_ARG, "n_fft must be 256, 512, 1024 or 2048");
  if (hop < 1 || hop > n_fft) return ssr_fail(SSR_ERR_INVALID_ARG, "hop must be in [1, n_fft]");
  if (n_bands < 1 || n_bands > SSR_CSII_BANDS) return ssr_fail(SSR_ERR_INVALID_ARG, "n_bands must be in [1, SSR_CSII_BANDS]");
  return ssr_check_pair_index(tgt_len, n_tgt, tgt_index, n_est, (int64_t)1 << 29, "target lengths must be in [0, 2^29)");
}

extern "C" size_t ssr_csii_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft, int hop,
                                           int n_bands) {
  if (check_csii_args(tgt_len, n_tgt, tgt_index, n_est, n_fft, hop, n_bands)) return 0;
  return csii_ws(tgt_len, n_tgt, tgt_index, n_est, n_fft, hop, n_bands).total;
}

extern "C" int ssr_csii(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                        int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_fft, int hop, int n_bands,
                        const double* weights, const double* importance, const int32_t* split, double* out, double* bands_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_csii_args(tgt_len, n_tgt, tgt_index, n_est, n_fft, hop, n_bands)) return rc;
  if (n_est == 0) return SSR_OK;
  if (!weights || !importance || !split) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int j = 0; j < n_bands; ++j)
    if (!(importance[j] > 0.0 && importance[j] <= 1.0)) return ssr_fail(SSR_ERR_INVALID_ARG, "importance must lie in (0, 1]");
  for (int e = 0; e < n_est; ++e)
    if (split[e] < -1 || split[e] > n_bands) return ssr_fail(SSR_ERR_INVALID_ARG, "split must be -1 or a band in [0, n_bands]");
  if (int rc = ssr_check_pair_buffers(tgt, tgt_off, est, est_off, out, tgt_len, n_tgt)) return rc;
  const CsiiWs w = csii_ws(tgt_len, n_tgt, tgt_index, n_est, n_fft, hop, n_bands);
  // (one workgroup per chunk: the launch stays below 2^32 threads, which every HIP runtime takes)
  if (w.chunks * (n_fft / 8) > 0xffffffffLL) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  const std::vector<cx<double>>& tw = ssr_twiddles_cached(n_fft);
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* len_dev = (int32_t*)(ws + w.off_len);
  int32_t* idx_dev = (int32_t*)(ws + w.off_idx);
  if (int rc = ssr_upload_pair_index(tgt_len, n_tgt, tgt_index, n_est, len_dev, idx_dev, s)) return rc;
  HIP_TRY(hipMemcpyAsync(ws + w.off_split, split, (size_t)n_est * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ws + w.off_imp, importance, (size_t)n_bands * sizeof(double), hipMemcpyHostToDevice, s));
  // (the table is cached for the life of the process: the caller need not keep it)
  HIP_TRY(hipMemcpyAsync(ws + w.off_tw, tw.data(), tw.size() * sizeof(cx<double>), hipMemcpyHostToDevice, s));
  SsrCsiiParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, len_dev, idx_dev, n_tgt, n_est);
  p.N = n_fft; p.H = hop; p.n_bands = n_bands;
  p.split = (const int32_t*)(ws + w.off_split); p.weights = weights; p.importance = (const double*)(ws + w.off_imp);
  p.tw = (const cx<double>*)(ws + w.off_tw); p.seg_off = (int64_t*)(ws + w.off_so); p.cls = (int8_t*)(ws + w.off_cls);
  p.run_start = (int32_t*)(ws + w.off_rs); p.run_chunk = (int64_t*)(ws + w.off_rc); p.chunk_off = (int64_t*)(ws + w.off_co);
  p.part = (double*)(ws + w.off_part);
  p.out = out; p.bands_out = bands_out;
  SSR_LAUNCH(k_csii_geometry, dim3(1), dim3(SSR_CSII_NT), s, p);
  if (tgt_f64) SSR_LAUNCH(k_csii_levels<double>, dim3((unsigned)n_tgt), dim3(SSR_CSII_NT), s, p);
  else SSR_LAUNCH(k_csii_levels<float>, dim3((unsigned)n_tgt), dim3(SSR_CSII_NT), s, p);
  if (w.chunks > 0) {
    const int rc = ssr_dispatch_pair_dtypes(tgt_f64, est_f64, [&](auto tt, auto te) {
      return ssr_dispatch_logn<SSR_PHASE_LOGN_MIN, SSR_PHASE_LOGN_MAX>(ssr_phase_log2_nfft(n_fft), [&](auto logn) -> int {
        constexpr int LOGN = decltype(logn)::value;
        SSR_LAUNCH((k_csii_spectra<decltype(tt), decltype(te), LOGN>), dim3((unsigned)w.chunks), dim3((1u << LOGN) / 8), s, p);
        return SSR_OK;
      });
    });
    if (rc) return rc;
  }
  SSR_LAUNCH(k_csii_bands, dim3((unsigned)n_est), dim3(SSR_CSII_NT), s, p);
  return SSR_OK;
}
