// libssrhip.so translation unit: SNR, SI-SDR and segmental SNR on float32 / float64 signals (ssr_wave_metrics.h) and its entry
// points (ssr_wave_metrics, ssr_wave_metrics_workspace_bytes).
#include "ssr_host.h"
#include "ssr_wave_metrics.h"

__global__ __launch_bounds__(SSR_WAVE_NT) void k_wave_geometry(SsrWaveParams p) {
  __shared__ int64_t sums[3 * SSR_WAVE_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_wave_geometry_body(p, blk, sums);
}

template <typename TT, typename TE> __global__ __launch_bounds__(SSR_WAVE_NT) void k_wave_pass1(SsrWaveParams p) {
  __shared__ double red[16], tst[3], seg[8];
  SsrBlk blk{(int)threadIdx.x};
  ssr_wave_pass1_body<TT, TE>(p, blk, (int64_t)blockIdx.x, red, tst, seg);
}

__global__ __launch_bounds__(256) void k_wave_finalize1(SsrWaveParams p) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < p.n_est) ssr_wave_finalize1(p, e);
}

template <typename TT, typename TE> __global__ __launch_bounds__(SSR_WAVE_NT) void k_wave_pass2(SsrWaveParams p) {
  __shared__ double red[8];
  SsrBlk blk{(int)threadIdx.x};
  ssr_wave_pass2_body<TT, TE>(p, blk, (int64_t)blockIdx.x, red);
}

__global__ __launch_bounds__(256) void k_wave_finalize2(SsrWaveParams p) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < p.n_est) ssr_wave_finalize2(p, e);
}

// workspace layout: a deterministic function of the target lengths, the pair -> target map, fs and which
struct WaveWs { size_t off_len, off_idx, off_rs, off_rt, off_pt, off_win, off_p1, off_p2, off_fin, total;
                int n_runs; int64_t run_tiles, pair_tiles; };
static WaveWs wave_ws(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int fs, int which) {
  WaveWs w{};
  for (int e = 0; e < n_est; ++e) {
    const int64_t nt = ssr_wave_tiles(tgt_len[tgt_index[e]], fs);
    if (e == 0 || tgt_index[e] != tgt_index[e - 1]) { ++w.n_runs; w.run_tiles += nt; }
    w.pair_tiles += nt;
  }
  const bool si = (which & SSR_WAVE_SI_SDR) != 0;
  SsrWsLayout l;
  w.off_len = l.take((size_t)n_tgt * sizeof(int32_t));
  w.off_idx = l.take((size_t)n_est * sizeof(int32_t));
  w.off_rs = l.take((size_t)(w.n_runs + 1) * sizeof(int32_t));
  w.off_rt = l.take((size_t)(w.n_runs + 1) * sizeof(int64_t));
  w.off_pt = l.take((size_t)(n_est + 1) * sizeof(int64_t));
  w.off_win = l.take((size_t)ssr_wave_frame_len(fs) * sizeof(double));
  w.off_p1 = l.take((size_t)w.pair_tiles * SSR_WAVE_P1 * sizeof(double));
  w.off_p2 = l.take(si ? (size_t)w.pair_tiles * SSR_WAVE_P2 * sizeof(double) : 0);
  w.off_fin = l.take(si ? (size_t)n_est * 3 * sizeof(double) : 0);
  w.total = l.o;
  return w;
}

// host-side validation: nothing is queued unless every argument is usable
static int check_wave_args(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int fs, int which) {
  if (which < 1 || which > 7) return ssr_fail(SSR_ERR_INVALID_ARG, "which must be a non-empty combination of SSR_WAVE_SNR, SSR_WAVE_SI_SDR, SSR_WAVE_SEG_SNR");
  if (fs <= 0) return ssr_fail(SSR_ERR_INVALID_ARG, "fs must be > 0");
  return ssr_check_pair_index(tgt_len, n_tgt, tgt_index, n_est, (int64_t)1 << 31, "target lengths must be in [0, 2^31)");
}

extern "C" size_t ssr_wave_metrics_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int fs,
                                                   int which) {
  if (check_wave_args(tgt_len, n_tgt, tgt_index, n_est, fs, which)) return 0;
  return wave_ws(tgt_len, n_tgt, tgt_index, n_est, fs, which).total;
}

extern "C" int ssr_wave_metrics(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt,
                                const void* est, int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int fs,
                                int which, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_wave_args(tgt_len, n_tgt, tgt_index, n_est, fs, which)) return rc;
  if (n_est == 0) return SSR_OK;
  if (int rc = ssr_check_pair_buffers(tgt, tgt_off, est, est_off, out, tgt_len, n_tgt)) return rc;
  const WaveWs w = wave_ws(tgt_len, n_tgt, tgt_index, n_est, fs, which);
  if (w.run_tiles > 0x7fffffff) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int32_t* len_dev = (int32_t*)(ws + w.off_len);
  int32_t* idx_dev = (int32_t*)(ws + w.off_idx);
  if (int rc = ssr_upload_pair_index(tgt_len, n_tgt, tgt_index, n_est, len_dev, idx_dev, s)) return rc;
  SsrWaveParams p{};
  ssr_set_pair_sig(p, tgt, tgt_off, est, est_off, len_dev, idx_dev, n_tgt, n_est);
  p.n_runs = w.n_runs; p.which = which; p.fs = fs;
  p.L = ssr_wave_frame_len(fs); p.R = ssr_wave_hop(fs); p.fpt = ssr_wave_frames_per_tile(fs); p.tile = ssr_wave_tile_len(fs);
  p.run_start = (int32_t*)(ws + w.off_rs); p.run_tile = (int64_t*)(ws + w.off_rt); p.pair_tile = (int64_t*)(ws + w.off_pt);
  p.win = (double*)(ws + w.off_win); p.part1 = (double*)(ws + w.off_p1);
  p.part2 = (which & SSR_WAVE_SI_SDR) ? (double*)(ws + w.off_p2) : nullptr;
  p.fin = (which & SSR_WAVE_SI_SDR) ? (double*)(ws + w.off_fin) : nullptr;
  p.out = out;
  SSR_LAUNCH(k_wave_geometry, dim3(1), dim3(SSR_WAVE_NT), s, p);
  const dim3 tiles((unsigned)w.run_tiles), nt(SSR_WAVE_NT), pairs((unsigned)ssr_ceil_div(n_est, 256));
  return ssr_dispatch_pair_dtypes(tgt_f64, est_f64, [&](auto tt, auto te) -> int {
    using TT = decltype(tt);
    using TE = decltype(te);
    if (w.run_tiles > 0) SSR_LAUNCH((k_wave_pass1<TT, TE>), tiles, nt, s, p);
    SSR_LAUNCH(k_wave_finalize1, pairs, dim3(256), s, p);
    if (which & SSR_WAVE_SI_SDR) {
      if (w.run_tiles > 0) SSR_LAUNCH((k_wave_pass2<TT, TE>), tiles, nt, s, p);
      SSR_LAUNCH(k_wave_finalize2, pairs, dim3(256), s, p);
    }
    return SSR_OK;
  });
}
