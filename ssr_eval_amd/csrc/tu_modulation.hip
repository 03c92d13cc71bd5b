// libssrhip.so translation unit: the modulation family on float32 / float64 signals (ssr_modulation.h, on the sweeps of
// ssr_auditory.h) and its entry points (ssr_modulation, ssr_modulation_workspace_bytes).
#include "ssr_host.h"
#include "ssr_modulation.h"

static_assert(SSR_MOD_K == SSR_MODULATION_BANDS && SSR_AUD_MAX_BLOCKS == SSR_MODULATION_MAX_BLOCKS, "the band count and the block limit are the C ABI's");
static_assert(SSR_MOD_MAX_S == SSR_MODULATION_MAX_STEP, "the frame step limit is the C ABI's");
static_assert(SSR_MOD_SIG_COLS == SSR_MODULATION_SIGNAL_COLS && SSR_MOD_PAIR_COLS == SSR_MODULATION_PAIR_COLS, "the row widths are the C ABI's");

__global__ __launch_bounds__(SSR_AUD_NT) void k_mod_geometry(SsrAudParams p) {
  __shared__ int64_t sums[3 * SSR_AUD_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_aud_geometry_body(p, blk, sums);
}

// g0: the first workgroup of the side (targets: 0, estimates: the targets' workgroups) whose element type is X
template <typename X, bool SECOND> __global__ __launch_bounds__(SSR_AUD_NT) void k_mod_sweep(SsrAudParams p, int64_t g0) {
  __shared__ SsrAudSweepLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_aud_sweep_body<X, SECOND>(p, blk, g0 + (int64_t)blockIdx.x, lds);
}

__global__ __launch_bounds__(64) void k_mod_scan(SsrAudParams p) { ssr_aud_scan_lane(p, (int64_t)blockIdx.x * 64 + threadIdx.x); }

template <bool TWO> __global__ __launch_bounds__(SSR_MOD_NT) void k_mod_bank(SsrModParams p) {
  __shared__ SsrModBankLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_mod_bank_body<TWO>(p, blk, (int)blockIdx.x, lds);
}

__global__ __launch_bounds__(SSR_MOD_NT) void k_mod_signal(SsrModParams p) {
  __shared__ SsrModSignalLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_mod_signal_body(p, blk, (int)blockIdx.x, lds);
}

__global__ __launch_bounds__(SSR_MOD_NT) void k_mod_pair(SsrModParams p) {
  __shared__ SsrModPairLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_mod_pair_body(p, blk, (int)blockIdx.x, lds);
}

// workspace layout: a deterministic function of the target lengths, the pair -> target map, hop_e and the band count
struct ModWs {
  size_t off_len, off_idx, off_split, off_kstar, off_tab, off_mtab, off_si, off_so, off_wo, off_ro, off_state, off_blk, off_emod, total;
  int64_t segs, tgt_wgs, est_wgs;
};
static ModWs mod_ws(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int hop, int n_bands) {
  ModWs w{};
  const int cp = ssr_aud_lanes(n_bands);
  for (int t = 0; t < n_tgt; ++t) { w.segs += ssr_aud_segments(tgt_len[t], hop); w.tgt_wgs += ssr_aud_wgs(tgt_len[t], hop, cp); }
  for (int e = 0; e < n_est; ++e) {
    const int n = tgt_len[tgt_index[e]];
    w.segs += ssr_aud_segments(n, hop); w.est_wgs += ssr_aud_wgs(n, hop, cp);
  }
  const size_t n_sig = (size_t)n_tgt + (size_t)n_est, C = (size_t)n_bands;
  SsrWsLayout l;
  w.off_len = l.take((size_t)n_tgt * sizeof(int32_t));
  w.off_idx = l.take((size_t)n_est * sizeof(int32_t));
  w.off_split = l.take((size_t)n_est * sizeof(int32_t));
  w.off_kstar = l.take(C * sizeof(int32_t));
  w.off_tab = l.take(C * SSR_AUD_TAB * sizeof(double));
  w.off_mtab = l.take((size_t)(SSR_MOD_TAB + 4 * SSR_MOD_MAX_S) * sizeof(double));
  w.off_si = l.take(n_sig * sizeof(int32_t));
  w.off_so = l.take((n_sig + 1) * sizeof(int64_t));
  w.off_wo = l.take((n_sig + 1) * sizeof(int64_t));
  w.off_ro = l.take((n_sig + 1) * sizeof(int64_t));
  w.off_state = l.take((size_t)w.segs * C * 8 * sizeof(double));
  w.off_blk = l.take((size_t)w.segs * SSR_AUD_SEG * C * sizeof(double));
  w.off_emod = l.take(n_sig * C * SSR_MOD_K * sizeof(double));
  w.total = l.o;
  return w;
}

// host-side validation: nothing is queued unless every argument is usable
static int check_mod_args(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int hop, int n_bands) {
  if (hop < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "hop_e must be >= 1");
  if (n_bands < SSR_AUDITORY_MIN_BANDS || n_bands > SSR_AUDITORY_MAX_BANDS) return ssr_fail(SSR_ERR_INVALID_ARG, "n_bands must be in [3, 64]");
  if (int rc = ssr_check_pair_index(tgt_len, n_tgt, tgt_index, n_est, (int64_t)1 << 29, "target lengths must be in [0, 2^29)")) return rc;
  if ((int64_t)n_tgt + n_est > (1 << 24)) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  for (int t = 0; t < n_tgt; ++t)
    if (ssr_aud_blocks(tgt_len[t], hop) > SSR_MODULATION_MAX_BLOCKS)
      return ssr_fail(SSR_ERR_UNSUPPORTED, "a signal may hold at most 65536 blocks of hop_e samples");
  return SSR_OK;
}

extern "C" size_t ssr_modulation_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int hop_e, int n_bands) {
  if (check_mod_args(tgt_len, n_tgt, tgt_index, n_est, hop_e, n_bands)) return 0;
  return mod_ws(tgt_len, n_tgt, tgt_index, n_est, hop_e, n_bands).total;
}

extern "C" int ssr_modulation(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                              int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int hop_e, int n_bands,
                              const double* coef, const double* mod, int S, const int32_t* kstar, double range_db, const int32_t* split_band,
                              double* signal_out, double* pair_out, double* spectrum_out, void* workspace, size_t workspace_bytes,
                              void* stream) {
  if (int rc = check_mod_args(tgt_len, n_tgt, tgt_index, n_est, hop_e, n_bands)) return rc;
  if (S < 1 || S > SSR_MODULATION_MAX_STEP) return ssr_fail(SSR_ERR_INVALID_ARG, "S must be in [1, 1024]");
  if (!(range_db > 0.0 && range_db <= 150.0)) return ssr_fail(SSR_ERR_INVALID_ARG, "range_db must be in (0, 150]");
  if (!coef || !mod || !kstar) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int c = 0; c < n_bands; ++c) {
    const double ar = coef[3 * c], ai = coef[3 * c + 1], g = coef[3 * c + 2];
    if (!(ar * ar + ai * ai < 1.0) || !(fabs(g) <= 1.7e308))
      return ssr_fail(SSR_ERR_INVALID_ARG, "coef must hold finite (Re a, Im a, g) with |a| < 1");
  }
  for (int k = 0; k < SSR_MOD_K; ++k) {
    const double* b = mod + 5 * k;
    bool ok = true;
    for (int j = 0; j < 5; ++j) ok = ok && fabs(b[j]) <= 1.7e308;
    // (the stability triangle of 1 + a1 / z + a2 / z^2)
    if (!ok || !(fabs(b[4]) < 1.0) || !(fabs(b[3]) < 1.0 + b[4]))
      return ssr_fail(SSR_ERR_INVALID_ARG, "mod must hold finite (b0, b1, b2, a1, a2) of stable biquads");
  }
  for (int c = 0; c < n_bands; ++c)
    if (kstar[c] < 5 || kstar[c] > SSR_MOD_K) return ssr_fail(SSR_ERR_INVALID_ARG, "kstar must be in [5, 8]");
  if (n_est > 0 && !split_band) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int e = 0; e < n_est; ++e)
    if (split_band[e] < -1 || split_band[e] > n_bands) return ssr_fail(SSR_ERR_INVALID_ARG, "split_band must be in [-1, n_bands]");
  if (n_tgt + n_est == 0) return SSR_OK;
  int64_t tgt_samples = 0, est_samples = 0;
  for (int t = 0; t < n_tgt; ++t) tgt_samples += tgt_len[t];
  for (int e = 0; e < n_est; ++e) est_samples += tgt_len[tgt_index[e]];
  if ((n_tgt > 0 && !tgt_off) || !signal_out || (n_est > 0 && (!est_off || !pair_out)) || (tgt_samples > 0 && !tgt) || (est_samples > 0 && !est))
    return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  const ModWs w = mod_ws(tgt_len, n_tgt, tgt_index, n_est, hop_e, n_bands);
  const int n_sig = n_tgt + n_est;
  // (the launches stay below 2^32 threads, which every HIP runtime takes)
  if ((w.tgt_wgs + w.est_wgs) * SSR_AUD_NT > 0xffffffffLL || (int64_t)n_sig * SSR_MOD_NT > 0xffffffffLL)
    return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  // the tables of the call: kept for the life of the process (the asynchronous copies read them after the call returned)
  static SsrHostTables<std::vector<double>, std::vector<double>> tables, mod_tables;
  std::vector<double> key(coef, coef + 3 * (size_t)n_bands);
  key.push_back((double)hop_e);
  const std::vector<double>& tab = tables.get(key, [&](std::vector<double>& t) { ssr_aud_tables_host(coef, n_bands, hop_e, t); });
  std::vector<double> mkey(mod, mod + SSR_MOD_TAB);
  mkey.push_back((double)S);
  const std::vector<double>& mtab = mod_tables.get(mkey, [&](std::vector<double>& t) { ssr_mod_tables_host(mod, S, t); });
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* len_dev = (int32_t*)(ws + w.off_len);
  int32_t* idx_dev = (int32_t*)(ws + w.off_idx);
  if (n_tgt) HIP_TRY(hipMemcpyAsync(len_dev, tgt_len, (size_t)n_tgt * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (n_est) HIP_TRY(hipMemcpyAsync(idx_dev, tgt_index, (size_t)n_est * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (n_est) HIP_TRY(hipMemcpyAsync(ws + w.off_split, split_band, (size_t)n_est * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ws + w.off_kstar, kstar, (size_t)n_bands * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ws + w.off_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ws + w.off_mtab, mtab.data(), mtab.size() * sizeof(double), hipMemcpyHostToDevice, s));
  SsrAudParams a{};
  ssr_set_pair_sig(a, tgt, tgt_off, est, est_off, len_dev, idx_dev, n_tgt, n_est);
  a.hop = hop_e; a.C = n_bands; a.CP = ssr_aud_lanes(n_bands);
  a.tab = (const double*)(ws + w.off_tab);
  a.sig_index = (int32_t*)(ws + w.off_si);
  a.seg_off = (int64_t*)(ws + w.off_so); a.wg_off = (int64_t*)(ws + w.off_wo); a.row_off = (int64_t*)(ws + w.off_ro);
  a.state = (double*)(ws + w.off_state); a.blk = (double*)(ws + w.off_blk);
  SsrModParams p{};
  p.tgt_len = len_dev; p.tgt_index = idx_dev; p.n_tgt = n_tgt; p.n_est = n_est;
  p.hop = hop_e; p.C = n_bands; p.S = S; p.range_db = range_db;
  p.sig_index = a.sig_index; p.seg_off = a.seg_off; p.blk = a.blk;
  p.tab = (const double*)(ws + w.off_mtab); p.kstar = (const int32_t*)(ws + w.off_kstar); p.split = (const int32_t*)(ws + w.off_split);
  p.emod = (double*)(ws + w.off_emod);
  p.signal_out = signal_out; p.pair_out = pair_out; p.spectrum_out = spectrum_out;
  SSR_LAUNCH(k_mod_geometry, dim3(1), dim3(SSR_AUD_NT), s, a);
  const int64_t first[2] = {0, w.tgt_wgs}, count[2] = {w.tgt_wgs, w.est_wgs};
  const int f64[2] = {tgt_f64, est_f64};
  for (int second = 0; second < 2; ++second) {
    for (int side = 0; side < 2; ++side) {
      if (count[side] == 0) continue;
      const dim3 grid((unsigned)count[side]), block(SSR_AUD_NT);
      if (f64[side] && !second) SSR_LAUNCH((k_mod_sweep<double, false>), grid, block, s, a, first[side]);
      else if (f64[side]) SSR_LAUNCH((k_mod_sweep<double, true>), grid, block, s, a, first[side]);
      else if (!second) SSR_LAUNCH((k_mod_sweep<float, false>), grid, block, s, a, first[side]);
      else SSR_LAUNCH((k_mod_sweep<float, true>), grid, block, s, a, first[side]);
    }
    if (!second && w.segs > 0) SSR_LAUNCH(k_mod_scan, dim3((unsigned)(((int64_t)n_sig * n_bands + 63) / 64)), dim3(64), s, a);
  }
  if (n_bands > 32) SSR_LAUNCH((k_mod_bank<true>), dim3((unsigned)n_sig), dim3(SSR_MOD_NT), s, p);
  else SSR_LAUNCH((k_mod_bank<false>), dim3((unsigned)n_sig), dim3(SSR_MOD_NT), s, p);
  SSR_LAUNCH(k_mod_signal, dim3((unsigned)n_sig), dim3(SSR_MOD_NT), s, p);
  if (n_est) SSR_LAUNCH(k_mod_pair, dim3((unsigned)n_est), dim3(SSR_MOD_NT), s, p);
  return SSR_OK;
}
