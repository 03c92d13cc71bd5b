// libssrhip.so translation unit: LLR, LPC cepstral distance, WSS and fwSNRseg on float32 / float64 signals (ssr_quality.h) and
// its entry points (ssr_quality_metrics, ssr_quality_metrics_workspace_bytes, ssr_quality_bands).
#include "ssr_host.h"
#include "ssr_quality.h"

__global__ __launch_bounds__(SSR_QUAL_NT) void k_qual_geometry(SsrQualParams p) {
  __shared__ int64_t sums[3 * SSR_QUAL_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_qual_geometry_body(p, blk, sums);
}

template <typename TT, typename TE> __global__ __launch_bounds__(64) void k_qual_lpc(SsrQualParams p) {
  __shared__ SsrQualLpcLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_qual_lpc_body<TT, TE>(p, blk, (int64_t)blockIdx.x, lds);
}

template <typename TT, typename TE, int LOGN> __global__ __launch_bounds__((1 << LOGN) / 8) void k_qual_bands(SsrQualParams p) {
  __shared__ SsrQualBandLds<LOGN> lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_qual_bands_body<TT, TE, LOGN>(p, blk, (int64_t)blockIdx.x, lds);
}

__global__ __launch_bounds__(SSR_QUAL_NT) void k_qual_finalize(SsrQualParams p) {
  __shared__ SsrQualFinLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_qual_finalize_body(p, blk, (int)blockIdx.x, lds);
}

// band filters and twiddles per sample rate: built once on the host, never written again (the workspace copies read them)
static const SsrQualTables& qual_tables(int fs) {
  static SsrHostTables<int, SsrQualTables> tables;
  return tables.get(fs, [&](SsrQualTables& t) { ssr_qual_tables_host(fs, t); });
}

// workspace layout: a deterministic function of the target lengths, the pair -> target map, fs and which
struct QualWs { size_t off_len, off_idx, off_rs, off_rf, off_pf, off_win, off_tw, off_fw, off_val, total;
                int n_runs; int64_t run_frames, pair_frames; };
static QualWs qual_ws(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int fs, int which) {
  QualWs w{};
  for (int e = 0; e < n_est; ++e) {
    const int64_t M = ssr_qual_frames(tgt_len[tgt_index[e]], fs);
    if (e == 0 || tgt_index[e] != tgt_index[e - 1]) { ++w.n_runs; w.run_frames += M; }
    w.pair_frames += M;
  }
  const bool bands = (which & (SSR_QUAL_WSS | SSR_QUAL_FWSEG)) != 0;
  const SsrQualTables& t = qual_tables(fs);
  SsrWsLayout l;
  w.off_len = l.take((size_t)n_tgt * sizeof(int32_t));
  w.off_idx = l.take((size_t)n_est * sizeof(int32_t));
  w.off_rs = l.take((size_t)(w.n_runs + 1) * sizeof(int32_t));
  w.off_rf = l.take((size_t)(w.n_runs + 1) * sizeof(int64_t));
  w.off_pf = l.take((size_t)(n_est + 1) * sizeof(int64_t));
  w.off_win = l.take((size_t)ssr_qual_frame_len(fs) * sizeof(double));
  w.off_tw = l.take(bands ? (size_t)t.N * sizeof(cx<double>) : 0);
  w.off_fw = l.take(bands ? (t.packed.size() + 1) * sizeof(double) : 0);
  w.off_val = l.take((size_t)w.pair_frames * 4 * sizeof(double));
  w.total = l.o;
  return w;
}

// host-side validation: nothing is queued unless every argument is usable
static int check_qual_args(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int fs, int lpc_order, int which) {
  if (which < 1 || which > 15)
    return ssr_fail(SSR_ERR_INVALID_ARG, "which must be a non-empty combination of SSR_QUAL_LLR, SSR_QUAL_CEP, SSR_QUAL_WSS, SSR_QUAL_FWSEG");
  if (fs < SSR_QUAL_FS_MIN || fs > SSR_QUAL_FS_MAX) return ssr_fail(SSR_ERR_INVALID_ARG, "fs must be in [8000, 48000]");
  if (lpc_order < 0 || lpc_order > SSR_QUAL_PMAX) return ssr_fail(SSR_ERR_INVALID_ARG, "lpc_order must be 0 (default) or in [1, 32]");
  return ssr_check_pair_index(tgt_len, n_tgt, tgt_index, n_est, (int64_t)1 << 31, "target lengths must be in [0, 2^31)");
}

extern "C" size_t ssr_quality_metrics_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int fs,
                                                      int lpc_order, int which) {
  if (check_qual_args(tgt_len, n_tgt, tgt_index, n_est, fs, lpc_order, which)) return 0;
  return qual_ws(tgt_len, n_tgt, tgt_index, n_est, fs, which).total;
}

extern "C" int ssr_quality_bands(int fs, int32_t* n_fft, double* cent, double* bw, double* filters, size_t filters_len) {
  if (fs < SSR_QUAL_FS_MIN || fs > SSR_QUAL_FS_MAX) return ssr_fail(SSR_ERR_INVALID_ARG, "fs must be in [8000, 48000]");
  const SsrQualTables& t = qual_tables(fs);
  if (n_fft) *n_fft = t.N;
  for (int b = 0; b < SSR_QUAL_BANDS; ++b) {
    if (cent) cent[b] = SSR_QUAL_CENT[b];
    if (bw) bw[b] = SSR_QUAL_BW[b];
  }
  if (filters) {
    if (filters_len < t.dense.size()) return ssr_fail(SSR_ERR_INVALID_ARG, "filters must hold 25 * n_fft / 2 doubles");
    for (size_t i = 0; i < t.dense.size(); ++i) filters[i] = t.dense[i];
  }
  return SSR_OK;
}

extern "C" int ssr_quality_metrics(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt,
                                   const void* est, int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int fs,
                                   int lpc_order, int which, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_qual_args(tgt_len, n_tgt, tgt_index, n_est, fs, lpc_order, which)) return rc;
  if (n_est == 0) return SSR_OK;
  if (int rc = ssr_check_pair_buffers(tgt, tgt_off, est, est_off, out, tgt_len, n_tgt)) return rc;
  const QualWs w = qual_ws(tgt_len, n_tgt, tgt_index, n_est, fs, which);
  if (w.run_frames > 0x7fffffff) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  const SsrQualTables& t = qual_tables(fs);
  const bool lpc = (which & (SSR_QUAL_LLR | SSR_QUAL_CEP)) != 0, bands = (which & (SSR_QUAL_WSS | SSR_QUAL_FWSEG)) != 0;
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* len_dev = (int32_t*)(ws + w.off_len);
  int32_t* idx_dev = (int32_t*)(ws + w.off_idx);
  if (int rc = ssr_upload_pair_index(tgt_len, n_tgt, tgt_index, n_est, len_dev, idx_dev, s)) return rc;
  if (bands) {      // (the tables are cached for the life of the process: the caller need not keep them)
    HIP_TRY(hipMemcpyAsync(ws + w.off_tw, t.tw.data(), t.tw.size() * sizeof(cx<double>), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ws + w.off_fw, t.packed.data(), t.packed.size() * sizeof(double), hipMemcpyHostToDevice, s));
  }
  SsrQualParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, len_dev, idx_dev, n_tgt, n_est);
  p.n_runs = w.n_runs; p.which = which; p.fs = fs;
  p.L = ssr_qual_frame_len(fs); p.R = ssr_qual_hop(fs); p.P = lpc_order ? lpc_order : ssr_qual_default_order(fs); p.N = t.N;
  p.run_start = (int32_t*)(ws + w.off_rs); p.run_frame = (int64_t*)(ws + w.off_rf);
  p.pair_frame = (int64_t*)(ws + w.off_pf); p.win = (double*)(ws + w.off_win);
  p.tw = bands ? (const cx<double>*)(ws + w.off_tw) : nullptr;
  p.fw = bands ? (const double*)(ws + w.off_fw) : nullptr;
  for (int b = 0; b < SSR_QUAL_BANDS; ++b) { p.band_lo[b] = t.lo[b]; p.band_hi[b] = t.hi[b]; p.band_off[b] = t.off[b]; }
  p.val = (double*)(ws + w.off_val); p.n_val = w.pair_frames; p.out = out;
  SSR_LAUNCH(k_qual_geometry, dim3(1), dim3(SSR_QUAL_NT), s, p);
  const dim3 frames((unsigned)w.run_frames);
  const int rc = ssr_dispatch_pair_dtypes(tgt_f64, est_f64, [&](auto tt, auto te) -> int {
    using TT = decltype(tt);
    using TE = decltype(te);
    if (lpc && w.run_frames > 0) SSR_LAUNCH((k_qual_lpc<TT, TE>), frames, dim3(64), s, p);
    if (bands && w.run_frames > 0)
      return ssr_dispatch_logn<9, 12>(ssr_qual_log2_nfft(fs), [&](auto logn) -> int {
        constexpr int LOGN = decltype(logn)::value;
        SSR_LAUNCH((k_qual_bands<TT, TE, LOGN>), frames, dim3((1u << LOGN) / 8), s, p);
        return SSR_OK;
      });
    return SSR_OK;
  });
  if (rc) return rc;
  SSR_LAUNCH(k_qual_finalize, dim3((unsigned)n_est), dim3(SSR_QUAL_NT), s, p);
  return SSR_OK;
}
