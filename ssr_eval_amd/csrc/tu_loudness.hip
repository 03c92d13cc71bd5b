// libssrhip.so translation unit: the loudness family on float32 / float64 signals (ssr_loudness.h) and its entry points
// (ssr_loudness, ssr_loudness_workspace_bytes).
#include "ssr_host.h"
#include "ssr_loudness.h"

__global__ __launch_bounds__(SSR_LOUD_NT) void k_loud_geometry(SsrLoudParams p) {
  __shared__ int64_t sums[2 * SSR_LOUD_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_loud_geometry_body(p, blk, sums);
}

// one wave per workgroup: 64 consecutive (signal, segment) lanes
template <typename X, bool SECOND> __global__ __launch_bounds__(64) void k_loud_filter(SsrLoudParams p, int64_t n_seg) {
  __shared__ __attribute__((aligned(16))) char tile[SSR_PIT_TILEB];
  SsrPitTile t{tile, (int)threadIdx.x};
  ssr_loud_filter_lane<X, SECOND>(p, (int64_t)blockIdx.x * 64 + threadIdx.x, n_seg, t);
}

__global__ __launch_bounds__(64) void k_loud_scan(SsrLoudParams p) { ssr_loud_scan_signal(p, (int)(blockIdx.x * 64 + threadIdx.x)); }

template <typename X> __global__ __launch_bounds__(SSR_LOUD_NT) void k_loud_peak(SsrLoudParams p) {
  __shared__ SsrLoudPeakLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_loud_peak_body<X>(p, blk, (int64_t)blockIdx.x, lds);
}

__global__ __launch_bounds__(SSR_LOUD_NT) void k_loud_gate(SsrLoudParams p) {
  __shared__ SsrLoudGateLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_loud_gate_body(p, blk, (int)blockIdx.x, lds);
}

// workspace layout: a deterministic function of the lengths and the rate
struct LoudWs { size_t off_len, off_boff, off_tab, off_sp, off_tp, off_zend, off_zin, off_part, off_peak, total; int64_t segs, tiles; };
static LoudWs loud_ws(const int32_t* len, int n_sig, int rate) {
  LoudWs w{};
  for (int i = 0; i < n_sig; ++i) { w.segs += ssr_loud_segments(len[i], rate); w.tiles += ssr_loud_tiles(len[i]); }
  SsrWsLayout l;
  w.off_len = l.take((size_t)n_sig * sizeof(int32_t));
  w.off_boff = l.take((size_t)n_sig * sizeof(int64_t));
  w.off_tab = l.take((size_t)SSR_LOUD_TAB_LEN * sizeof(double));
  w.off_sp = l.take((size_t)(n_sig + 1) * sizeof(int64_t));
  w.off_tp = l.take((size_t)(n_sig + 1) * sizeof(int64_t));
  w.off_zend = l.take((size_t)w.segs * 4 * sizeof(double));
  w.off_zin = l.take((size_t)w.segs * 4 * sizeof(double));
  w.off_part = l.take((size_t)w.segs * sizeof(double));
  w.off_peak = l.take((size_t)w.tiles * 2 * sizeof(double));
  w.total = l.o;
  return w;
}

// host-side validation: nothing is queued unless every argument is usable
static int check_loud_args(const int32_t* len, int n_sig, int rate) {
  if (rate < SSR_LOUD_MIN_RATE || rate > SSR_LOUD_MAX_RATE) return ssr_fail(SSR_ERR_INVALID_ARG, "rate must be in [8000, 192000] Hz");
  if (n_sig < 0) return ssr_fail(SSR_ERR_INVALID_ARG, "n_sig must be >= 0");
  if (n_sig > 0 && !len) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int i = 0; i < n_sig; ++i)
    if (len[i] < 0 || len[i] >= (1 << 29)) return ssr_fail(SSR_ERR_INVALID_ARG, "signal lengths must be in [0, 2^29)");
  for (int i = 0; i < n_sig; ++i)
    if (ssr_loud_sub_blocks(len[i], rate) > SSR_LOUD_MAX_SUB)
      return ssr_fail(SSR_ERR_UNSUPPORTED, "a signal may hold at most 6144 sub-blocks of 100 ms");
  return SSR_OK;
}

// the table of a rate: built on first use, kept for the life of the process (the asynchronous copy reads it after the call returned)
static const std::vector<double>& loud_table_cached(int rate) {
  static SsrHostTables<int, std::vector<double>> tables;
  return tables.get(rate, [&](std::vector<double>& t) { ssr_loud_tables_host(rate, t); });
}

extern "C" size_t ssr_loudness_workspace_bytes(const int32_t* len, int n_sig, int rate) {
  if (check_loud_args(len, n_sig, rate)) return 0;
  return loud_ws(len, n_sig, rate).total;
}

extern "C" int ssr_loudness(const void* sig, int sig_f64, const int64_t* off, const int32_t* len, int n_sig, int rate, double* out,
                            const int64_t* blocks_off, double* blocks_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_loud_args(len, n_sig, rate)) return rc;
  if (n_sig == 0) return SSR_OK;
  int64_t samples = 0;
  for (int i = 0; i < n_sig; ++i) samples += len[i];
  if (!off || !out || (samples > 0 && !sig) || (blocks_out && !blocks_off)) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  if (blocks_out)
    for (int i = 0; i < n_sig; ++i)
      if (blocks_off[i] < 0) return ssr_fail(SSR_ERR_INVALID_ARG, "blocks_off must be >= 0");
  const LoudWs w = loud_ws(len, n_sig, rate);
  // (the launches stay below 2^32 threads, which every HIP runtime takes)
  if (w.segs + 64 > 0xffffffffLL || w.tiles * SSR_LOUD_NT > 0xffffffffLL || (int64_t)n_sig * SSR_LOUD_NT > 0xffffffffLL)
    return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  const std::vector<double>& tab = loud_table_cached(rate);
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(ws + w.off_len, len, (size_t)n_sig * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (blocks_out) HIP_TRY(hipMemcpyAsync(ws + w.off_boff, blocks_off, (size_t)n_sig * sizeof(int64_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ws + w.off_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
  SsrLoudParams p{};
  p.sig = sig; p.off = off; p.len = (const int32_t*)(ws + w.off_len); p.n_sig = n_sig; p.rate = rate; p.h = ssr_loud_sub_len(rate);
  p.tab = (const double*)(ws + w.off_tab);
  p.seg_pre = (int64_t*)(ws + w.off_sp); p.tile_pre = (int64_t*)(ws + w.off_tp);
  p.zend = (double*)(ws + w.off_zend); p.zin = (double*)(ws + w.off_zin); p.part = (double*)(ws + w.off_part);
  p.peak = (double*)(ws + w.off_peak);
  p.out = out; p.blocks_off = blocks_out ? (const int64_t*)(ws + w.off_boff) : nullptr; p.blocks_out = blocks_out;
  SSR_LAUNCH(k_loud_geometry, dim3(1), dim3(SSR_LOUD_NT), s, p);
  const unsigned fg = (unsigned)((w.segs + 63) / 64);
  if (sig_f64) {
    if (w.segs > 0) {
      SSR_LAUNCH((k_loud_filter<double, false>), dim3(fg), dim3(64), s, p, w.segs);
      SSR_LAUNCH(k_loud_scan, dim3((unsigned)((n_sig + 63) / 64)), dim3(64), s, p);
      SSR_LAUNCH((k_loud_filter<double, true>), dim3(fg), dim3(64), s, p, w.segs);
    }
    if (w.tiles > 0) SSR_LAUNCH(k_loud_peak<double>, dim3((unsigned)w.tiles), dim3(SSR_LOUD_NT), s, p);
  } else {
    if (w.segs > 0) {
      SSR_LAUNCH((k_loud_filter<float, false>), dim3(fg), dim3(64), s, p, w.segs);
      SSR_LAUNCH(k_loud_scan, dim3((unsigned)((n_sig + 63) / 64)), dim3(64), s, p);
      SSR_LAUNCH((k_loud_filter<float, true>), dim3(fg), dim3(64), s, p, w.segs);
    }
    if (w.tiles > 0) SSR_LAUNCH(k_loud_peak<float>, dim3((unsigned)w.tiles), dim3(SSR_LOUD_NT), s, p);
  }
  SSR_LAUNCH(k_loud_gate, dim3((unsigned)n_sig), dim3(SSR_LOUD_NT), s, p);
  return SSR_OK;
}
