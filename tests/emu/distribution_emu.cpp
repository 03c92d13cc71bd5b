// Host emulation of the distribution kernel bodies (ssr_eval_amd/csrc/ssr_distribution.h) for tests/test_distribution_host.py: every
// kernel of ssr_frechet, ssr_kernel_distance and ssr_pairwise_distances run in launch order, one workgroup after another, on a
// workspace poisoned with NaN.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libdistribution_emu.so distribution_emu.cpp
#define SSR_HOST_EMU 1
#include <memory>
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_distribution.h"

template <typename X> static void moments(SsrDstrParams& p, int64_t max_chunks) {
  const int nt = ssr_dstr_tiles(p.D);
  SsrBlk blk{SSR_DSTR_NT};
  auto ml = std::make_unique<SsrDstrMeanLds>();
  for (int s = 0; s <= p.K; ++s)
    for (int cb = 0; cb < nt; ++cb)
      for (int64_t c = 0; c < max_chunks; ++c) ssr_dstr_mean_body<X>(p, blk, cb, c, s, *ml);
  for (int64_t id = 0; id < ((int64_t)(1 + p.K) * p.D + 255) / 256 * 256; ++id) ssr_dstr_mean_finish_lane(p, id);
  auto tl = std::make_unique<SsrDstrTileLds>();
  for (int s = 0; s <= p.K; ++s)
    for (int t = 0; t < nt * nt; ++t)
      for (int64_t c = 0; c < max_chunks; ++c) ssr_dstr_cov_body<X>(p, blk, t / nt, t % nt, c, s, *tl);
  for (int64_t id = 0; id < ((int64_t)(1 + p.K) * p.D * p.D + 255) / 256 * 256; ++id) ssr_dstr_cov_finish_lane(p, id);
  for (int64_t id = 0; id < (p.K + 1 + 63) / 64 * 64; ++id) ssr_dstr_stats_lane(p, id);
}

// the arguments of ssr_frechet up to moments_out
extern "C" int frechet_emu(const void* data, int f64, const int64_t* offset, const int64_t* rows, int K, int D, int64_t ld, int max_sweeps,
                           double* out, double* moments_out) {
  if (D < 1 || D > SSR_DSTR_MAX_DIM || K < 1 || ld < D || max_sweeps < 1) return -2;
  std::vector<SsrDstrSet> sets(K + 1);
  int64_t chunks = 0, max_chunks = 0;
  for (int s = 0; s <= K; ++s) {
    sets[s] = SsrDstrSet{offset[s], rows[s], chunks, ssr_dstr_chunks(rows[s], D)};
    chunks += sets[s].chunks;
    max_chunks = sets[s].chunks > max_chunks ? sets[s].chunks : max_chunks;
  }
  const size_t DD = (size_t)D * D, S = (size_t)K + 1;
  const double poison = (double)NAN;
  std::vector<double> mean_part(chunks * D + 1, poison), mean(S * D, poison), cov_part(chunks * DD + 1, poison), cov(S * DD, poison),
      stats(S * 2, poison), jwork(DD, poison), V(DD, poison), jstat(2, poison), T(K * DD, poison), G(K * DD, poison), gwork(K * DD + 1, poison);
  mean_part.back() = cov_part.back() = gwork.back() = -777.0;
  SsrDstrParams p{};
  p.data = data; p.ld = ld; p.D = D; p.K = K; p.max_sweeps = max_sweeps; p.sets = sets.data();
  p.mean_part = mean_part.data(); p.mean = mean.data(); p.cov_part = cov_part.data(); p.cov = cov.data(); p.stats = stats.data();
  p.jwork = jwork.data(); p.V = V.data(); p.jstat = jstat.data(); p.T = T.data(); p.G = G.data(); p.gwork = gwork.data();
  p.out = out; p.moments_out = moments_out;
  if (f64) moments<double>(p, max_chunks); else moments<float>(p, max_chunks);
  SsrBlk jb{SSR_DSTR_JNT}, blk{SSR_DSTR_NT};
  auto jl = std::make_unique<SsrDstrJacobiLds>();
  ssr_dstr_jacobi_body<true>(p, jb, 0, *jl);
  const int nt = ssr_dstr_tiles(D);
  auto tl = std::make_unique<SsrDstrTileLds>();
  for (int k = 0; k < K; ++k) for (int t = 0; t < nt * nt; ++t) ssr_dstr_project_body<0>(p, blk, t / nt, t % nt, k, *tl);
  for (int k = 0; k < K; ++k) for (int t = 0; t < nt * nt; ++t) ssr_dstr_project_body<1>(p, blk, t / nt, t % nt, k, *tl);
  for (int k = 0; k < K; ++k) for (int t = 0; t < nt * nt; ++t) ssr_dstr_project_body<2>(p, blk, t / nt, t % nt, k, *tl);
  for (int k = 0; k < K; ++k) ssr_dstr_jacobi_body<false>(p, jb, k, *jl);
  if (mean_part.back() != -777.0 || cov_part.back() != -777.0 || gwork.back() != -777.0) return -3;
  return 0;
}

template <typename X, bool WRITE_D> static void pairs(SsrDstrPairParams& p, const std::vector<SsrDstrCombo>& combos) {
  SsrBlk blk{SSR_DSTR_NT};
  auto lds = std::make_unique<SsrDstrPairsLds>();
  int ta = 0, tb = 0;
  for (const auto& c : combos) { ta = std::max(ta, ssr_dstr_tiles(c.rows_a)); tb = std::max(tb, ssr_dstr_tiles(c.rows_b)); }
  for (int c = 0; c < (int)combos.size(); ++c)
    for (int ti = 0; ti < ta; ++ti)
      for (int tj = 0; tj < tb; ++tj) ssr_dstr_pairs_body<X, WRITE_D>(p, blk, ti, tj, c, *lds);
}

// the arguments of ssr_kernel_distance up to out
extern "C" int kernel_distance_emu(const void* data, int f64, const int64_t* offset, const int64_t* rows, int K, int D, int64_t ld,
                                   const double* gamma, int n_gamma, double scale, double* out) {
  if (D < 1 || K < 1 || ld < D || n_gamma < 1 || n_gamma > SSR_DSTR_MAX_GAMMA) return -2;
  std::vector<SsrDstrCombo> combos;
  int64_t tiles = 0;
  auto add = [&](int a, int b) {
    combos.push_back(SsrDstrCombo{offset[a], rows[a], offset[b], rows[b], tiles, a == b});
    tiles += (int64_t)ssr_dstr_tiles(rows[a]) * ssr_dstr_tiles(rows[b]);
  };
  add(0, 0);
  for (int k = 1; k <= K; ++k) { add(k, k); add(0, k); }
  std::vector<double> part(tiles * n_gamma + 1, (double)NAN), sums(combos.size() * n_gamma + 1, (double)NAN);
  part.back() = sums.back() = -777.0;
  SsrDstrPairParams p{};
  p.data = data; p.ld = ld; p.D = D; p.K = K; p.n_gamma = n_gamma;
  for (int g = 0; g < n_gamma; ++g) p.gamma[g] = gamma[g];
  p.scale = scale; p.combos = combos.data(); p.part = part.data(); p.sums = sums.data(); p.out = out;
  if (f64) pairs<double, false>(p, combos); else pairs<float, false>(p, combos);
  SsrBlk blk{SSR_DSTR_NT};
  auto lds = std::make_unique<SsrDstrPairsLds>();
  for (int c = 0; c < (int)combos.size(); ++c) ssr_dstr_finish_sums_body(p, blk, c, *lds);
  for (int64_t id = 0; id < ((int64_t)K * n_gamma + 255) / 256 * 256; ++id) ssr_dstr_finish_lane(p, id);
  if (part.back() != -777.0 || sums.back() != -777.0) return -3;
  return 0;
}

// the arguments of ssr_pairwise_distances up to out
extern "C" int pairwise_emu(const void* data, int f64, int64_t offset, int64_t rows, int D, int64_t ld, const int64_t* index, int n, double* out) {
  if (D < 1 || ld < D || n < 0 || n > 2048) return -2;
  for (int i = 0; i < n; ++i) if (index[i] < 0 || index[i] >= rows) return -2;
  if (n < 2) return 0;
  std::vector<SsrDstrCombo> combos{SsrDstrCombo{offset, n, offset, n, 0, 1}};
  SsrDstrPairParams p{};
  p.data = data; p.ld = ld; p.D = D; p.combos = combos.data(); p.index = index; p.dist_out = out;
  if (f64) pairs<double, true>(p, combos); else pairs<float, true>(p, combos);
  return 0;
}

// rows per chunk of the moment sums, the tile edge, the Jacobi's threads, the largest D
extern "C" void distribution_geometry(int D, int64_t* res) {
  res[0] = ssr_dstr_chunk_rows(D); res[1] = SSR_DSTR_TILE; res[2] = SSR_DSTR_JNT; res[3] = SSR_DSTR_MAX_DIM;
}
