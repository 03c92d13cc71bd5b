// libssrhip.so translation unit: the spectrum family on float32 / float64 signals (ssr_spectrum.h) and its entry points
// (ssr_spectrum, ssr_spectrum_workspace_bytes).
#include "ssr_host.h"
#include "ssr_spectrum.h"

static_assert(SSR_SPEC_MAX_BANDS == SSR_SPECTRUM_MAX_BANDS, "the band limit is the C ABI's");
static_assert(SSR_SPEC_SIG_COLS == SSR_SPECTRUM_SIG_COLS && SSR_SPEC_PAIR_COLS == SSR_SPECTRUM_PAIR_COLS, "the row widths are the C ABI's");

__global__ __launch_bounds__(SSR_SPEC_NT) void k_spec_geometry(SsrSpecParams p) {
  __shared__ int64_t sums[3 * SSR_SPEC_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_spec_geometry_body(p, blk, sums);
}

// g0: the first chunk of the side (targets: 0, estimates: the targets' chunks) whose element type is T
template <typename T, int LOGN> __global__ __launch_bounds__((1 << LOGN) / 8) void k_spec_ltas(SsrSpecParams p, int64_t g0) {
  __shared__ SsrSpecLds<LOGN> lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_spec_ltas_body<T, LOGN>(p, blk, g0 + (int64_t)blockIdx.x, lds);
}

__global__ __launch_bounds__(SSR_SPEC_NT) void k_spec_signal(SsrSpecParams p) {
  __shared__ SsrSpecSignalLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_spec_signal_body(p, blk, (int)blockIdx.x, lds);
}

__global__ __launch_bounds__(SSR_SPEC_NT) void k_spec_pair(SsrSpecParams p) {
  __shared__ SsrSpecPairLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_spec_pair_body(p, blk, (int)blockIdx.x, lds);
}

// workspace layout: a deterministic function of the target lengths, the pair -> target map, n_fft, hop and the band count
struct SpecWs {
  size_t off_len, off_idx, off_bands, off_split, off_si, off_rs, off_rc, off_co, off_tw, off_part, off_cp, off_sig, off_lev, total;
  int64_t tgt_chunks, est_chunks;
};
static SpecWs spec_ws(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft, int hop, int n_bands) {
  SpecWs w{};
  for (int t = 0; t < n_tgt; ++t) w.tgt_chunks += ssr_spec_chunks(tgt_len[t], n_fft, hop);
  for (int e = 0; e < n_est; ++e) w.est_chunks += ssr_spec_chunks(tgt_len[tgt_index[e]], n_fft, hop);
  const size_t n_sig = (size_t)n_tgt + (size_t)n_est, nb = (size_t)n_fft / 2 + 1;
  SsrWsLayout l;
  w.off_len = l.take((size_t)n_tgt * sizeof(int32_t));
  w.off_idx = l.take((size_t)n_est * sizeof(int32_t));
  w.off_bands = l.take((size_t)n_bands * 2 * sizeof(int32_t));
  w.off_split = l.take((size_t)n_est * sizeof(int32_t));
  w.off_si = l.take(n_sig * sizeof(int32_t));
  w.off_rs = l.take((n_sig + 1) * sizeof(int32_t));
  w.off_rc = l.take((n_sig + 1) * sizeof(int64_t));
  w.off_co = l.take((n_sig + 1) * sizeof(int64_t));
  w.off_tw = l.take((size_t)n_fft * sizeof(cx<double>));
  w.off_part = l.take((size_t)(w.tgt_chunks + w.est_chunks) * nb * 2 * sizeof(double));
  w.off_cp = l.take(n_sig * nb * sizeof(double));
  w.off_sig = l.take(n_sig * 4 * sizeof(double));
  w.off_lev = l.take(n_sig * (size_t)n_bands * sizeof(double));
  w.total = l.o;
  return w;
}

// host-side validation: nothing is queued unless every argument is usable
static int check_spec_args(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft, int hop, int n_bands) {
  if (ssr_phase_log2_nfft(n_fft) < 0) return ssr_fail(SSR_ERR_INVALID_ARG, "n_fft must be 256, 512, 1024 or 2048");
  if (hop < 1 || hop > n_fft) return ssr_fail(SSR_ERR_INVALID_ARG, "hop must be in [1, n_fft]");
  if (n_bands < 1 || n_bands > SSR_SPECTRUM_MAX_BANDS) return ssr_fail(SSR_ERR_INVALID_ARG, "n_bands must be in [1, SSR_SPECTRUM_MAX_BANDS]");
  if (int rc = ssr_check_pair_index(tgt_len, n_tgt, tgt_index, n_est, (int64_t)1 << 29, "target lengths must be in [0, 2^29)")) return rc;
  if ((int64_t)n_tgt + n_est > (1 << 24)) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  return SSR_OK;
}

extern "C" size_t ssr_spectrum_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft,
                                               int hop, int n_bands) {
  if (check_spec_args(tgt_len, n_tgt, tgt_index, n_est, n_fft, hop, n_bands)) return 0;
  return spec_ws(tgt_len, n_tgt, tgt_index, n_est, n_fft, hop, n_bands).total;
}

extern "C" int ssr_spectrum(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                            int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_fft, int hop, int lo, int hi,
                            double rho, double drop_db, int n_bands, const int32_t* bands, const int32_t* split, double* sig_out,
                            double* pair_out, double* ltas_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_spec_args(tgt_len, n_tgt, tgt_index, n_est, n_fft, hop, n_bands)) return rc;
  if (!(rho > 0.0 && rho < 1.0)) return ssr_fail(SSR_ERR_INVALID_ARG, "rho must be in (0, 1)");
  if (!(drop_db > 0.0 && drop_db <= 150.0)) return ssr_fail(SSR_ERR_INVALID_ARG, "drop_db must be in (0, 150]");
  if (lo <= hi && (lo < 0 || hi > n_fft / 2))
    return ssr_fail(SSR_ERR_INVALID_ARG, "the band must be empty (lo > hi) or satisfy 0 <= lo <= hi <= n_fft / 2");
  if (!bands) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int b = 0; b < n_bands; ++b) {
    const int b0 = bands[2 * b], b1 = bands[2 * b + 1];
    if (b0 < 0 || b0 > b1 || b1 > n_fft / 2 || (b > 0 && b0 <= bands[2 * b - 1]))
      return ssr_fail(SSR_ERR_INVALID_ARG, "bands must be disjoint ascending ranges with 0 <= lo <= hi <= n_fft / 2");
  }
  if (n_est > 0 && !split) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int e = 0; e < n_est; ++e)
    if (split[e] < -1) return ssr_fail(SSR_ERR_INVALID_ARG, "split must be a bin >= 0, or -1 for none");
  if (n_tgt + n_est == 0) return SSR_OK;
  int64_t tgt_samples = 0, est_samples = 0;
  for (int t = 0; t < n_tgt; ++t) tgt_samples += tgt_len[t];
  for (int e = 0; e < n_est; ++e) est_samples += tgt_len[tgt_index[e]];
  if (!sig_out || (n_tgt > 0 && !tgt_off) || (n_est > 0 && (!est_off || !pair_out)) || (tgt_samples > 0 && !tgt) || (est_samples > 0 && !est))
    return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  const SpecWs w = spec_ws(tgt_len, n_tgt, tgt_index, n_est, n_fft, hop, n_bands);
  // (one workgroup per chunk: the launches stay below 2^32 threads, which every HIP runtime takes)
  if ((w.tgt_chunks + w.est_chunks) * (n_fft / 8) > 0xffffffffLL) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  const std::vector<cx<double>>& tw = ssr_twiddles_cached(n_fft);
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const int n_sig = n_tgt + n_est;
  int32_t* len_dev = (int32_t*)(ws + w.off_len);
  int32_t* idx_dev = (int32_t*)(ws + w.off_idx);
  if (n_tgt) HIP_TRY(hipMemcpyAsync(len_dev, tgt_len, (size_t)n_tgt * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (n_est) HIP_TRY(hipMemcpyAsync(idx_dev, tgt_index, (size_t)n_est * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (n_est) HIP_TRY(hipMemcpyAsync(ws + w.off_split, split, (size_t)n_est * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ws + w.off_bands, bands, (size_t)n_bands * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
  // (the table is cached for the life of the process: the caller need not keep it)
  HIP_TRY(hipMemcpyAsync(ws + w.off_tw, tw.data(), tw.size() * sizeof(cx<double>), hipMemcpyHostToDevice, s));
  SsrSpecParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, len_dev, idx_dev, n_tgt, n_est);
  p.N = n_fft; p.H = hop; p.lo = lo; p.hi = hi; p.n_bands = n_bands; p.rho = rho; p.thr_lin = pow(10.0, -drop_db / 10.0);
  p.bands = (const int32_t*)(ws + w.off_bands); p.split = (const int32_t*)(ws + w.off_split); p.tw = (const cx<double>*)(ws + w.off_tw);
  p.sig_index = (int32_t*)(ws + w.off_si);
  p.run_start = (int32_t*)(ws + w.off_rs); p.run_chunk = (int64_t*)(ws + w.off_rc); p.chunk_off = (int64_t*)(ws + w.off_co);
  p.part = (double*)(ws + w.off_part); p.cp = (double*)(ws + w.off_cp); p.sig = (double*)(ws + w.off_sig); p.lev = (double*)(ws + w.off_lev);
  p.sig_out = sig_out; p.pair_out = pair_out; p.ltas_out = ltas_out;
  SSR_LAUNCH(k_spec_geometry, dim3(1), dim3(SSR_SPEC_NT), s, p);
  const int64_t first[2] = {0, w.tgt_chunks}, count[2] = {w.tgt_chunks, w.est_chunks};
  const int f64[2] = {tgt_f64, est_f64};
  for (int side = 0; side < 2; ++side) {
    if (count[side] == 0) continue;
    const int rc = ssr_dispatch_logn<SSR_PHASE_LOGN_MIN, SSR_PHASE_LOGN_MAX>(ssr_phase_log2_nfft(n_fft), [&](auto logn) -> int {
      constexpr int LOGN = decltype(logn)::value;
      if (f64[side]) SSR_LAUNCH((k_spec_ltas<double, LOGN>), dim3((unsigned)count[side]), dim3((1u << LOGN) / 8), s, p, first[side]);
      else SSR_LAUNCH((k_spec_ltas<float, LOGN>), dim3((unsigned)count[side]), dim3((1u << LOGN) / 8), s, p, first[side]);
      return SSR_OK;
    });
    if (rc) return rc;
  }
  SSR_LAUNCH(k_spec_signal, dim3((unsigned)n_sig), dim3(SSR_SPEC_NT), s, p);
  if (n_est) SSR_LAUNCH(k_spec_pair, dim3((unsigned)n_est), dim3(SSR_SPEC_NT), s, p);
  return SSR_OK;
}
