// libssrhip.so translation unit: the noise-to-mask family on float32 / float64 signals (ssr_nmr.h) and its entry points (ssr_nmr,
// ssr_nmr_workspace_bytes).
#include "ssr_host.h"
#include "ssr_nmr.h"

static_assert(SSR_NMR_MAX_BANDS == SSR_NMR_BANDS && SSR_NMR_COLS == SSR_NMR_COLUMNS && SSR_NMR_TAB == SSR_NMR_TABLE, "the limits are the C ABI's");

__global__ __launch_bounds__(SSR_NMR_NT) void k_nmr_geometry(SsrNmrParams p) {
  __shared__ int64_t sums[3 * SSR_NMR_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_nmr_geometry_body(p, blk, sums);
}

template <typename TT, int LOGN> __global__ __launch_bounds__((1 << LOGN) / 8) void k_nmr_excite(SsrNmrParams p) {
  __shared__ SsrNmrLds<LOGN> lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_nmr_excite_body<TT, LOGN>(p, blk, (int64_t)blockIdx.x, lds);
}

__global__ __launch_bounds__(SSR_NMR_BT) void k_nmr_mask(SsrNmrParams p) {
  SsrBlk blk{(int)threadIdx.x};
  ssr_nmr_mask_body(p, blk, (int)blockIdx.x);
}

template <typename TT, typename TE, int LOGN> __global__ __launch_bounds__((1 << LOGN) / 8) void k_nmr_noise(SsrNmrParams p) {
  __shared__ SsrNmrLds<LOGN> lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_nmr_noise_body<TT, TE, LOGN>(p, blk, (int64_t)blockIdx.x, lds);
}

__global__ __launch_bounds__(SSR_NMR_BT) void k_nmr_score(SsrNmrParams p) {
  __shared__ SsrNmrScoreLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_nmr_score_body(p, blk, (int)blockIdx.x, lds);
}

// workspace layout: a deterministic function of the target lengths, the pair -> target map, n_fft and the band count
struct NmrWs {
  size_t off_len, off_idx, off_split, off_bins, off_tab, off_so, off_to, off_rs, off_rc, off_co, off_tw, off_mask, off_part, total;
  int64_t chunks, tchunks, frames;
};
static NmrWs nmr_ws(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft, int n_bands) {
  NmrWs w{};
  const int hop = n_fft / 2;
  for (int e = 0; e < n_est; ++e) w.chunks += ssr_coh_chunks(tgt_len[tgt_index[e]], n_fft, hop);
  for (int t = 0; t < n_tgt; ++t) {
    w.frames += ssr_coh_segments(tgt_len[t], n_fft, hop);
    w.tchunks += ssr_coh_chunks(tgt_len[t], n_fft, hop);
  }
  SsrWsLayout l;
  w.off_len = l.take((size_t)n_tgt * sizeof(int32_t));
  w.off_idx = l.take((size_t)n_est * sizeof(int32_t));
  w.off_split = l.take((size_t)n_est * sizeof(int32_t));
  w.off_bins = l.take((size_t)n_bands * 2 * sizeof(int32_t));
  w.off_tab = l.take((size_t)n_bands * SSR_NMR_TAB * sizeof(double));
  w.off_so = l.take((size_t)(n_tgt + 1) * sizeof(int64_t));
  w.off_to = l.take((size_t)(n_tgt + 1) * sizeof(int64_t));
  w.off_rs = l.take((size_t)(n_est + 1) * sizeof(int32_t));
  w.off_rc = l.take((size_t)(n_est + 1) * sizeof(int64_t));
  w.off_co = l.take((size_t)(n_est + 1) * sizeof(int64_t));
  w.off_tw = l.take((size_t)n_fft * sizeof(cx<double>));
  w.off_mask = l.take((size_t)w.frames * n_bands * sizeof(double));
  w.off_part = l.take((size_t)w.chunks * (n_bands + 2) * sizeof(double));
  w.total = l.o;
  return w;
}

// host-side validation: nothing is queued unless every argument is usable
static int check_nmr_args(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft, int n_bands) {
  if (ssr_phase_log2_nfft(n_fft) < 0) return ssr_fail(SSR_ERR_INVALID_ARG, "n_fft must be 256, 512, 1024 or 2048");
  if (n_bands < 1 || n_bands > SSR_NMR_BANDS) return ssr_fail(SSR_ERR_INVALID_ARG, "n_bands must be in [1, SSR_NMR_BANDS]");
  return ssr_check_pair_index(tgt_len, n_tgt, tgt_index, n_est, (int64_t)1 << 29, "target lengths must be in [0, 2^29)");
}

extern "C" size_t ssr_nmr_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft, int n_bands) {
  if (check_nmr_args(tgt_len, n_tgt, tgt_index, n_est, n_fft, n_bands)) return 0;
  return nmr_ws(tgt_len, n_tgt, tgt_index, n_est, n_fft, n_bands).total;
}

extern "C" int ssr_nmr(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est, int est_f64,
                       const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_fft, int n_bands, const double* weights,
                       const int32_t* bins, const double* table, const int32_t* split, double* out, double* bands_out, double* mask_out,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_nmr_args(tgt_len, n_tgt, tgt_index, n_est, n_fft, n_bands)) return rc;
  if (n_est == 0) return SSR_OK;
  if (!weights || !bins || !table || !split) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  auto finite = [](double v) { return v - v == 0.0; };
  for (int i = 0; i < n_bands; ++i) {
    const double* r = table + (size_t)i * SSR_NMR_TAB;
    if (bins[2 * i] < 0 || bins[2 * i] > bins[2 * i + 1] || bins[2 * i + 1] > n_fft / 2)
      return ssr_fail(SSR_ERR_INVALID_ARG, "bins must hold 0 <= k_lo <= k_hi <= n_fft / 2 per band");
    const bool ok = r[0] >= 0.0 && r[0] <= 1.0 && r[1] >= 0.0 && r[1] <= 1.0 && finite(r[2]) && r[2] > 0.0 && finite(r[3]) && finite(r[4]) &&
                    r[4] >= 0.0 && finite(r[5]) && r[5] > 0.0 && r[6] >= 0.0 && r[6] < 1.0 && finite(r[7]) && r[7] > 0.0;
    if (!ok) return ssr_fail(SSR_ERR_INVALID_ARG, "table must hold u_lo, u_hi in [0, 1], Ein, 1 / Bs, mgain > 0, finite c_up, ad >= 0 and a in [0, 1)");
  }
  for (int e = 0; e < n_est; ++e)
    if (split[e] < -1 || split[e] > n_bands) return ssr_fail(SSR_ERR_INVALID_ARG, "split must be -1 or a band in [0, n_bands]");
  if (int rc = ssr_check_pair_buffers(tgt, tgt_off, est, est_off, out, tgt_len, n_tgt)) return rc;
  const NmrWs w = nmr_ws(tgt_len, n_tgt, tgt_index, n_est, n_fft, n_bands);
  // (one workgroup per chunk, per target and per estimate: every launch stays below 2^32 threads, which every HIP runtime takes)
  if ((w.chunks > w.tchunks ? w.chunks : w.tchunks) * (n_fft / 8) > 0xffffffffLL ||
      (int64_t)(n_tgt > n_est ? n_tgt : n_est) * SSR_NMR_BT > 0xffffffffLL)
    return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  const std::vector<cx<double>>& tw = ssr_twiddles_cached(n_fft);
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* len_dev = (int32_t*)(ws + w.off_len);
  int32_t* idx_dev = (int32_t*)(ws + w.off_idx);
  if (int rc = ssr_upload_pair_index(tgt_len, n_tgt, tgt_index, n_est, len_dev, idx_dev, s)) return rc;
  HIP_TRY(hipMemcpyAsync(ws + w.off_split, split, (size_t)n_est * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ws + w.off_bins, bins, (size_t)n_bands * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ws + w.off_tab, table, (size_t)n_bands * SSR_NMR_TAB * sizeof(double), hipMemcpyHostToDevice, s));
  // (the table is cached for the life of the process: the caller need not keep it)
  HIP_TRY(hipMemcpyAsync(ws + w.off_tw, tw.data(), tw.size() * sizeof(cx<double>), hipMemcpyHostToDevice, s));
  SsrNmrParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, len_dev, idx_dev, n_tgt, n_est);
  p.N = n_fft; p.H = n_fft / 2; p.n_bands = n_bands;
  p.split = (const int32_t*)(ws + w.off_split); p.bins = (const int32_t*)(ws + w.off_bins); p.tab = (const double*)(ws + w.off_tab);
  p.w2 = weights; p.tw = (const cx<double>*)(ws + w.off_tw);
  p.seg_off = (int64_t*)(ws + w.off_so); p.tchunk_off = (int64_t*)(ws + w.off_to);
  p.run_start = (int32_t*)(ws + w.off_rs); p.run_chunk = (int64_t*)(ws + w.off_rc); p.chunk_off = (int64_t*)(ws + w.off_co);
  p.mask = (double*)(ws + w.off_mask); p.part = (double*)(ws + w.off_part);
  p.out = out; p.bands_out = bands_out; p.mask_out = mask_out;
  SSR_LAUNCH(k_nmr_geometry, dim3(1), dim3(SSR_NMR_NT), s, p);
  if (w.tchunks > 0) {
    const int rc = ssr_dispatch_logn<SSR_PHASE_LOGN_MIN, SSR_PHASE_LOGN_MAX>(ssr_phase_log2_nfft(n_fft), [&](auto logn) -> int {
      constexpr int LOGN = decltype(logn)::value;
      if (tgt_f64) SSR_LAUNCH((k_nmr_excite<double, LOGN>), dim3((unsigned)w.tchunks), dim3((1u << LOGN) / 8), s, p);
      else SSR_LAUNCH((k_nmr_excite<float, LOGN>), dim3((unsigned)w.tchunks), dim3((1u << LOGN) / 8), s, p);
      return SSR_OK;
    });
    if (rc) return rc;
    SSR_LAUNCH(k_nmr_mask, dim3((unsigned)n_tgt), dim3(SSR_NMR_BT), s, p);
  }
  if (w.chunks > 0) {
    const int rc = ssr_dispatch_pair_dtypes(tgt_f64, est_f64, [&](auto tt, auto te) {
      return ssr_dispatch_logn<SSR_PHASE_LOGN_MIN, SSR_PHASE_LOGN_MAX>(ssr_phase_log2_nfft(n_fft), [&](auto logn) -> int {
        constexpr int LOGN = decltype(logn)::value;
        SSR_LAUNCH((k_nmr_noise<decltype(tt), decltype(te), LOGN>), dim3((unsigned)w.chunks), dim3((1u << LOGN) / 8), s, p);
        return SSR_OK;
      });
    });
    if (rc) return rc;
  }
  SSR_LAUNCH(k_nmr_score, dim3((unsigned)n_est), dim3(SSR_NMR_BT), s, p);
  return SSR_OK;
}
