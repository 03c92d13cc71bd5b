// Host emulation of what the per-pair families share (ssr_eval_amd/csrc/ssr_pairs.h) for tests/test_pairs_host.py: the run
// geometry on per-target counts given as they are, and the prefix search.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libpairs_emu.so pairs_emu.cpp
#define SSR_HOST_EMU 1
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_pairs.h"

extern "C" int pairs_nt() { return SSR_PAIRS_NT; }

// tgt_count[t]: the items of target t (the body's count function is the identity); run_start, run_pre: [n_runs + 1];
// pair_pre: [n_est + 1]; win: [L]
extern "C" void pairs_run_geometry(const int32_t* tgt_count, const int32_t* tgt_index, int n_est, int L,
                                   int32_t* run_start, int64_t* run_pre, int64_t* pair_pre, double* win) {
  std::vector<int64_t> sums(3 * SSR_PAIRS_NT);
  SsrBlk blk{SSR_PAIRS_NT};
  ssr_run_geometry_body(tgt_count, tgt_index, n_est, [](int32_t n) { return (int64_t)n; }, run_start, run_pre, pair_pre, win,
                        L, blk, sums.data());
}

extern "C" int pairs_prefix_find(const int64_t* off, int n, int64_t g) { return ssr_prefix_find(off, n, g); }
