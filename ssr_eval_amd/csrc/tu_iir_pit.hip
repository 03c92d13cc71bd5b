// libssrhip.so translation unit: the segment-parallel (parallel-in-time) zero-phase IIR filter (ssr_iir_pit.h) and its entry
// points (ssr_sosfiltfilt_fast, ssr_sosfiltfilt_fast_f64, ssr_sosfiltfilt_fast_workspace_bytes).
#include "ssr_host.h"
#include "ssr_iir_pit.h"

template <typename X>
__global__ __launch_bounds__(256) void k_pit_map(SsrPitParamsT<X> p) {
  ssr_pit_map_slot(p, (int)(blockIdx.x * 256 + threadIdx.x));
}

// one wave per design
template <typename X>
__global__ __launch_bounds__(64) void k_pit_tables(SsrPitParamsT<X> p) {
  const int d = blockIdx.x;
  SSR_PIT_DISPATCH(p.n_sections[d], (ssr_pit_tables<S, X>(p, d, (int)threadIdx.x)));
}

// workgroup -> (one of the launch's designs of S sections, 64 consecutive slots)
// PASS 0: forward local, 1: backward sweep 1 (end states), 2: backward sweep 2 (y)
template <typename X, int PASS, int S>
__global__ __launch_bounds__(64) void k_pit_local(SsrPitParamsT<X> p, int blocks_per_design) {
  const int d = p.dsel[(int)blockIdx.x / blocks_per_design];
  const int slot = ((int)blockIdx.x % blocks_per_design) * 64 + (int)threadIdx.x;
  __shared__ __attribute__((aligned(16))) char tile[SSR_PIT_TILEB];
  SsrPitTile t{tile, (int)threadIdx.x};
  if constexpr (PASS == 0) ssr_pit_fwd_local<S, X>(p, d, slot, t);
  else ssr_pit_bwd_local<S, PASS == 2, X>(p, d, slot, t);
}
template <typename X, int PASS, int S>
static void pit_launch_one(const SsrPitParamsT<X>& p, unsigned grid, int blocks_per_design, hipStream_t s) {
  hipLaunchKernelGGL((k_pit_local<X, PASS, S>), dim3(grid), dim3(64), 0, s, p, blocks_per_design);
}
// one launch per section count that occurs among the designs
template <typename X, int PASS>
static void pit_launch_local(SsrPitParamsT<X>& p, int64_t blocks_per_design, hipStream_t s) {
  for (int sc = 1; sc <= SSR_PIT_MAXS; ++sc) {
    int n = 0;
    for (int d = 0; d < p.n_designs; ++d)
      if (p.n_sections[d] == sc) p.dsel[n++] = d;
    if (!n) continue;
    SSR_PIT_DISPATCH(sc, (pit_launch_one<X, PASS, S>(p, (unsigned)(blocks_per_design * n), (int)blocks_per_design, s)));
  }
}

// workgroup (one wave) -> (design, 4 utterances), 16 lanes each
template <typename X, bool BACKWARD>
__global__ __launch_bounds__(64) void k_pit_scan(SsrPitParamsT<X> p, int blocks_per_design) {
  const int d = (int)blockIdx.x / blocks_per_design;
  const int item = ((int)blockIdx.x % blocks_per_design) * 4 + (int)threadIdx.x / 16;
  if (item >= p.n_items) return;                       // (whole 16-lane groups leave)
  SSR_PIT_DISPATCH(p.n_sections[d], (ssr_pit_scan_item<S, BACKWARD, X>(p, d, item, (int)threadIdx.x % 16)));
}

// ----------------------------------------------------------------------------------------------------
// workspace = [slot map] [H] [M] [z_in forward] [z_end] [z_in backward] [zero-state forward output of design 0] [of design 1] ...
struct PitWs { size_t map, H, M, zin_f, zend, zin_b, fwd, total; int64_t n_slots; int emax; };
static size_t pit_region_bytes(int64_t total_len, int n_items, int edge) {
  return ssr_align256(((size_t)total_len + (size_t)2 * edge * n_items) * sizeof(double));
}
static PitWs pit_ws(int64_t total_len, int n_items, const int32_t* edge, int n_designs) {
  PitWs w{};
  for (int d = 0; d < n_designs; ++d) w.emax = edge[d] > w.emax ? edge[d] : w.emax;
  w.n_slots = (total_len + (int64_t)2 * w.emax * n_items) / SSR_PIT_L + n_items + 1;
  size_t b = 0;
  w.map = b; b += ssr_align256((size_t)w.n_slots * sizeof(int32_t));
  w.H = b; b += ssr_align256((size_t)n_designs * SSR_PIT_L * SSR_PIT_ZS * sizeof(double));
  w.M = b; b += ssr_align256((size_t)n_designs * SSR_PIT_ZS * SSR_PIT_ZS * sizeof(double));
  const size_t st = ssr_align256((size_t)n_designs * (size_t)w.n_slots * SSR_PIT_ZS * sizeof(double));
  w.zin_f = b; b += st;
  w.zend = b; b += st;
  w.zin_b = b; b += st;
  w.fwd = b;
  for (int d = 0; d < n_designs; ++d) b += pit_region_bytes(total_len, n_items, edge[d] < 0 ? 0 : edge[d]);
  w.total = b;
  return w;
}

extern "C" size_t ssr_sosfiltfilt_fast_workspace_bytes(int64_t total_len, int n_items, const int32_t* edge, int n_designs) {
  if (total_len <= 0 || n_items <= 0 || !edge || n_designs <= 0) return 0;
  return pit_ws(total_len, n_items, edge, n_designs).total;
}

template <typename X>
static int sosfiltfilt_fast_t(const X* x, const int64_t* off, const int32_t* len, int n_items, int64_t total_len, const double* sos,
                              const double* zi, const int32_t* n_sections, const int32_t* edge, int n_designs, double* y,
                              int64_t y_stride, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !off || !len || !sos || !zi || !n_sections || !edge || !y) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  if (n_designs < 1 || n_designs > SSR_PIT_MAXD) return ssr_fail(SSR_ERR_UNSUPPORTED, "1 to 48 designs per call");
  if (y_stride < total_len) return ssr_fail(SSR_ERR_INVALID_ARG, "y_stride smaller than the batch");
  for (int d = 0; d < n_designs; ++d) {
    if (n_sections[d] < 1 || n_sections[d] > SSR_PIT_MAXS) return ssr_fail(SSR_ERR_UNSUPPORTED, "n_sections must be in [1, 8] (ssr_sosfiltfilt takes up to 16)");
    if (edge[d] < 0) return ssr_fail(SSR_ERR_INVALID_ARG, "negative edge");
  }
  if (n_items <= 0) return SSR_OK;
  if (total_len <= 0) return ssr_fail(SSR_ERR_INVALID_ARG, "total_len must be positive for a batch with items");
  if (!workspace || workspace_bytes < ssr_sosfiltfilt_fast_workspace_bytes(total_len, n_items, edge, n_designs))
    return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  const PitWs w = pit_ws(total_len, n_items, edge, n_designs);
  const int64_t local_blocks = (w.n_slots + 63) / 64, scan_blocks = ((int64_t)n_items + 3) / 4;
  if (w.n_slots > 0x7fffffff || local_blocks * n_designs > 0x7fffffff || scan_blocks * n_designs > 0x7fffffff)
    return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  char* ws = (char*)workspace;
  SsrPitParamsT<X> p{};
  p.x = x; p.off = off; p.len = len; p.n_items = n_items; p.n_designs = n_designs;
  p.sos = sos; p.zi = zi; p.y = y; p.y_stride = y_stride;
  p.emax = w.emax; p.n_slots = (int)w.n_slots;
  p.map = (int32_t*)(ws + w.map);
  p.H = (double*)(ws + w.H); p.M = (double*)(ws + w.M);
  p.zin_f = (double*)(ws + w.zin_f); p.zend = (double*)(ws + w.zend); p.zin_b = (double*)(ws + w.zin_b);
  p.fwd = (double*)(ws + w.fwd);
  int64_t fo = 0;
  for (int d = 0; d < n_designs; ++d) {
    p.n_sections[d] = n_sections[d]; p.edge[d] = edge[d]; p.fwd_off[d] = fo;
    fo += (int64_t)(pit_region_bytes(total_len, n_items, edge[d]) / sizeof(double));
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 one(64), sg((unsigned)(scan_blocks * n_designs));
  hipLaunchKernelGGL((k_pit_map<X>), dim3((unsigned)((w.n_slots + 255) / 256)), dim3(256), 0, s, p);
  hipLaunchKernelGGL((k_pit_tables<X>), dim3(n_designs), one, 0, s, p);
  pit_launch_local<X, 0>(p, local_blocks, s);
  hipLaunchKernelGGL((k_pit_scan<X, false>), sg, one, 0, s, p, (int)scan_blocks);
  pit_launch_local<X, 1>(p, local_blocks, s);
  hipLaunchKernelGGL((k_pit_scan<X, true>), sg, one, 0, s, p, (int)scan_blocks);
  pit_launch_local<X, 2>(p, local_blocks, s);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}

extern "C" int ssr_sosfiltfilt_fast(const float* x, const int64_t* off, const int32_t* len, int n_items, int64_t total_len,
                                    const double* sos, const double* zi, const int32_t* n_sections, const int32_t* edge,
                                    int n_designs, double* y, int64_t y_stride, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  return sosfiltfilt_fast_t<float>(x, off, len, n_items, total_len, sos, zi, n_sections, edge, n_designs, y, y_stride, workspace,
                                   workspace_bytes, stream);
}

extern "C" int ssr_sosfiltfilt_fast_f64(const double* x, const int64_t* off, const int32_t* len, int n_items, int64_t total_len,
                                        const double* sos, const double* zi, const int32_t* n_sections, const int32_t* edge,
                                        int n_designs, double* y, int64_t y_stride, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  return sosfiltfilt_fast_t<double>(x, off, len, n_items, total_len, sos, zi, n_sections, edge, n_designs, y, y_stride, workspace,
                                    workspace_bytes, stream);
}
