// Host emulation of the bootstrap kernel bodies (ssr_eval_amd/csrc/ssr_bootstrap.h) for tests/test_bootstrap_host.py: the kernels of
// ssr_bootstrap_means / ssr_bootstrap_summary run in launch order, one workgroup after another.  Test infrastructure; not part of
// the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libbootstrap_emu.so bootstrap_emu.cpp
#define SSR_HOST_EMU 1
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_bootstrap.h"

extern "C" void boot_philox_emu(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  for (int i = 0; i < 4; ++i) out[i] = counter[i];
  ssr_philox4x32_10(out, key[0], key[1]);
}

extern "C" void boot_geometry_emu(int* tile, int* max_boot) { *tile = SSR_BOOT_TILE; *max_boot = SSR_BOOT_MAX_B; }

extern "C" int boot_means_emu(const double* table, int64_t n_rows, int n_cols, const int32_t* spk_off, int n_spk, int n_boot,
                              uint64_t seed, int scheme, double* reps) {
  if (n_spk < 1 || n_spk > SSR_BOOT_MAX_SPK) return -1;
  SsrBootParams p{};
  p.table = table; p.n_rows = n_rows; p.n_cols = n_cols; p.n_spk = n_spk; p.n_boot = n_boot; p.scheme = scheme;
  p.key0 = (uint32_t)(seed & 0xffffffffu); p.key1 = (uint32_t)(seed >> 32);
  p.reps = reps;
  for (int s = 0; s <= n_spk; ++s) p.spk_off[s] = spk_off[s];
  SsrBlk blk{SSR_BOOT_NT};
  std::vector<int> idx(SSR_BOOT_TILE), slot(SSR_BOOT_MAX_SPK), bad(SSR_BOOT_NT);
  for (int b = 0; b < n_boot; ++b)
    for (int c0 = 0; c0 < n_cols; c0 += SSR_BOOT_NT) ssr_boot_means_body(p, blk, b, c0, idx.data(), slot.data());
  for (int c0 = 0; c0 < n_cols; c0 += 64)
    for (int64_t r0 = 0; r0 < n_rows; r0 += SSR_BOOT_MASK_ROWS) ssr_boot_mask_body(p, blk, c0, r0, bad.data());
  return 0;
}

extern "C" int boot_summary_emu(const double* reps, int n_boot, int n_cols, const double* q, int n_q, double* out, int32_t* counts) {
  if (n_boot < 1 || n_boot > SSR_BOOT_MAX_B || n_q < 0 || n_q > SSR_BOOT_MAX_Q) return -1;
  SsrBootSumParams p{};
  p.reps = reps; p.n_boot = n_boot; p.n_cols = n_cols; p.n_q = n_q; p.out = out; p.counts = counts;
  for (int i = 0; i < n_q; ++i) p.q[i] = q[i];
  SsrBlk blk{SSR_BOOT_SUM_NT};
  std::vector<double> s(SSR_BOOT_MAX_B), wsum(SSR_BOOT_SUM_NT / 64), wsq(SSR_BOOT_SUM_NT / 64);
  std::vector<int> wflag(SSR_BOOT_SUM_NT / 64);
  for (int c = 0; c < n_cols; ++c) ssr_boot_summary_body(p, blk, c, s.data(), wsum.data(), wsq.data(), wflag.data());
  return 0;
}
