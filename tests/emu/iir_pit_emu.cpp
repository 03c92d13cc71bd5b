// Host emulation of the segment-parallel sosfiltfilt bodies (ssr_eval_amd/csrc/ssr_iir_pit.h) for tests/test_iir_fast_host.py:
// every kernel of ssr_sosfiltfilt_fast run in launch order, one lane after another.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libiir_pit_emu.so iir_pit_emu.cpp
#define SSR_HOST_EMU 1
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_iir_pit.h"

extern "C" int iir_pit_segment_len() { return SSR_PIT_L; }

template <typename X>
static int run(const X* x, const int64_t* off, const int32_t* len, int n_items, int64_t total_len, const double* sos, const double* zi,
               const int32_t* n_sections, const int32_t* edge, int n_designs, double* y, int64_t y_stride) {
  if (n_designs < 1 || n_designs > SSR_PIT_MAXD || n_items < 1) return -1;
  SsrPitParamsT<X> p{};
  p.x = x; p.off = off; p.len = len; p.n_items = n_items; p.n_designs = n_designs;
  p.sos = sos; p.zi = zi; p.y = y; p.y_stride = y_stride;
  for (int d = 0; d < n_designs; ++d) p.emax = edge[d] > p.emax ? edge[d] : p.emax;
  p.n_slots = (int)((total_len + (int64_t)2 * p.emax * n_items) / SSR_PIT_L + n_items + 1);
  std::vector<int32_t> map(p.n_slots, -7);
  std::vector<double> H((size_t)n_designs * SSR_PIT_L * SSR_PIT_ZS), M((size_t)n_designs * SSR_PIT_ZS * SSR_PIT_ZS);
  const size_t st = (size_t)n_designs * p.n_slots * SSR_PIT_ZS;
  const double nan = std::nan("");
  std::vector<double> zin_f(st, nan), zend(st, nan), zin_b(st, nan);     // (whatever is read was written first)
  int64_t fo = 0;
  for (int d = 0; d < n_designs; ++d) {
    p.n_sections[d] = n_sections[d]; p.edge[d] = edge[d]; p.fwd_off[d] = fo;
    fo += total_len + (int64_t)2 * edge[d] * n_items;
  }
  std::vector<double> fwd((size_t)fo, nan);
  p.map = map.data(); p.H = H.data(); p.M = M.data(); p.zin_f = zin_f.data(); p.zend = zend.data(); p.zin_b = zin_b.data();
  p.fwd = fwd.data();
  for (int s = 0; s < p.n_slots; ++s) ssr_pit_map_slot(p, s);
  for (int d = 0; d < n_designs; ++d)
    for (int j = 0; j < 64; ++j) SSR_PIT_DISPATCH(p.n_sections[d], (ssr_pit_tables<S, X>(p, d, j)));
  SsrPitTile tile;
  const int slots64 = (p.n_slots + 63) / 64 * 64;             // whole workgroups: the lanes past n_slots leave by themselves
  for (int d = 0; d < n_designs; ++d)
    for (int s = 0; s < slots64; ++s) SSR_PIT_DISPATCH(p.n_sections[d], (ssr_pit_fwd_local<S, X>(p, d, s, tile)));
  for (int d = 0; d < n_designs; ++d)
    for (int i = 0; i < n_items; ++i) SSR_PIT_DISPATCH(p.n_sections[d], (ssr_pit_scan_item<S, false, X>(p, d, i, 0)));
  for (int d = 0; d < n_designs; ++d)
    for (int s = slots64 - 1; s >= 0; --s) SSR_PIT_DISPATCH(p.n_sections[d], (ssr_pit_bwd_local<S, false, X>(p, d, s, tile)));
  for (int d = 0; d < n_designs; ++d)
    for (int i = 0; i < n_items; ++i) SSR_PIT_DISPATCH(p.n_sections[d], (ssr_pit_scan_item<S, true, X>(p, d, i, 0)));
  for (int d = 0; d < n_designs; ++d)
    for (int s = 0; s < slots64; ++s) SSR_PIT_DISPATCH(p.n_sections[d], (ssr_pit_bwd_local<S, true, X>(p, d, s, tile)));
  return 0;
}

// sos [D][8][6], zi [D][8][2]; y [D][y_stride] in x's ragged layout
extern "C" int iir_pit_emu(const float* x, const int64_t* off, const int32_t* len, int n_items, int64_t total_len, const double* sos,
                           const double* zi, const int32_t* n_sections, const int32_t* edge, int n_designs, double* y,
                           int64_t y_stride) {
  return run<float>(x, off, len, n_items, total_len, sos, zi, n_sections, edge, n_designs, y, y_stride);
}
extern "C" int iir_pit_emu_f64(const double* x, const int64_t* off, const int32_t* len, int n_items, int64_t total_len,
                               const double* sos, const double* zi, const int32_t* n_sections, const int32_t* edge, int n_designs,
                               double* y, int64_t y_stride) {
  return run<double>(x, off, len, n_items, total_len, sos, zi, n_sections, edge, n_designs, y, y_stride);
}
