// libssrhip.so translation unit: the distribution family on float32 / float64 embedding sets (ssr_distribution.h) and its entry
// points (ssr_frechet, ssr_kernel_distance, ssr_pairwise_distances and the two workspace queries).
#include "ssr_host.h"
#include "ssr_distribution.h"

static_assert(SSR_DSTR_MAX_DIM == SSR_DISTRIBUTION_MAX_DIM && SSR_DSTR_MAX_GAMMA == SSR_DISTRIBUTION_MAX_GAMMA, "the limits are the C ABI's");
static_assert(SSR_DSTR_OUT_COLS == SSR_FRECHET_COLS && SSR_DSTR_KD_COLS == SSR_KERNEL_DISTANCE_COLS, "the row widths are the C ABI's");
static_assert(SSR_DISTRIBUTION_PAIRWISE_WORKSPACE == SSR_DISTRIBUTION_MAX_PAIR_ROWS * 8 + 256 && sizeof(SsrDstrCombo) <= 256, "the pairwise workspace");

// grid: x = row chunk, y = block of 64 columns, z = set
template <typename X> __global__ __launch_bounds__(SSR_DSTR_NT) void k_dstr_mean(SsrDstrParams p) {
  __shared__ SsrDstrMeanLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_dstr_mean_body<X>(p, blk, (int)blockIdx.y, (int64_t)blockIdx.x, (int)blockIdx.z, lds);
}
__global__ __launch_bounds__(256) void k_dstr_mean_finish(SsrDstrParams p) { ssr_dstr_mean_finish_lane(p, (int64_t)blockIdx.x * 256 + threadIdx.x); }

// grid: x = row chunk, y = tile pair ti * nt + tj, z = set
template <typename X> __global__ __launch_bounds__(SSR_DSTR_NT) void k_dstr_cov(SsrDstrParams p, int nt) {
  __shared__ SsrDstrTileLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_dstr_cov_body<X>(p, blk, (int)blockIdx.y / nt, (int)blockIdx.y % nt, (int64_t)blockIdx.x, (int)blockIdx.z, lds);
}
__global__ __launch_bounds__(256) void k_dstr_cov_finish(SsrDstrParams p) { ssr_dstr_cov_finish_lane(p, (int64_t)blockIdx.x * 256 + threadIdx.x); }
__global__ __launch_bounds__(64) void k_dstr_cov_stats(SsrDstrParams p) { ssr_dstr_stats_lane(p, (int64_t)blockIdx.x * 64 + threadIdx.x); }

// grid: x = tile pair, y = estimate set
template <int PASS> __global__ __launch_bounds__(SSR_DSTR_NT) void k_dstr_project(SsrDstrParams p, int nt) {
  __shared__ SsrDstrTileLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_dstr_project_body<PASS>(p, blk, (int)blockIdx.x / nt, (int)blockIdx.x % nt, (int)blockIdx.y, lds);
}

// ONE workgroup per matrix: grid [1] for the reference, [K] for the G_k
template <bool REF> __global__ __launch_bounds__(SSR_DSTR_JNT) void k_dstr_jacobi(SsrDstrParams p) {
  __shared__ SsrDstrJacobiLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_dstr_jacobi_body<REF>(p, blk, (int)blockIdx.x, lds);
}

// grid: x = tile of b's rows, y = tile of a's rows, z = combination
template <typename X, bool WRITE_D> __global__ __launch_bounds__(SSR_DSTR_NT) void k_dstr_pairs(SsrDstrPairParams p) {
  __shared__ SsrDstrPairsLds lds;
  SsrBlk blk{(int)threadIdx.x};
  ssr_dstr_pairs_body<X, WRITE_D>(p, blk, (int)blockIdx.y, (int)blockIdx.x, (int)blockIdx.z, lds);
}
// PASS 0: a workgroup per combination adds its tile partials; PASS 1: a lane per (set, gamma) forms mmd2 and kd
template <int PASS> __global__ __launch_bounds__(SSR_DSTR_NT) void k_dstr_finish(SsrDstrPairParams p) {
  if constexpr (PASS == 0) {
    __shared__ SsrDstrPairsLds lds;
    SsrBlk blk{(int)threadIdx.x};
    ssr_dstr_finish_sums_body(p, blk, (int)blockIdx.x, lds);
  } else {
    ssr_dstr_finish_lane(p, (int64_t)blockIdx.x * SSR_DSTR_NT + threadIdx.x);
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static int check_sets(const int64_t* rows, int K, int D) {
  if (D < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "D must be >= 1");
  if (D > SSR_DISTRIBUTION_MAX_DIM) return ssr_fail(SSR_ERR_UNSUPPORTED, "D must be <= 1024");
  if (K < 0) return ssr_fail(SSR_ERR_INVALID_ARG, "K must be >= 0");
  if (K > SSR_DISTRIBUTION_MAX_SETS) return ssr_fail(SSR_ERR_UNSUPPORTED, "at most 16383 estimate sets per call");
  if (!rows) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int s = 0; s <= K; ++s) {
    if (rows[s] < 0) return ssr_fail(SSR_ERR_INVALID_ARG, "row counts must be >= 0");
    if (rows[s] > 0x7fffffffLL) return ssr_fail(SSR_ERR_UNSUPPORTED, "a set may hold at most 2^31 - 1 rows");
  }
  return SSR_OK;
}
static int check_layout(const int64_t* offset, int K, int D, int64_t ld) {
  if (ld < D) return ssr_fail(SSR_ERR_INVALID_ARG, "ld must be >= D");
  if (!offset) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int s = 0; s <= K; ++s)
    if (offset[s] < 0) return ssr_fail(SSR_ERR_INVALID_ARG, "offsets must be >= 0");
  return SSR_OK;
}
static int check_threads(int64_t gx, int64_t gy, int64_t gz, int nt) {
  if (gx < 1 || gy < 1 || gz < 1) return SSR_OK;
  if (gx > 0x7fffffffLL || gy > 65535 || gz > 65535 || (double)gx * (double)gy * (double)gz * nt >= 4294967296.0)
    return ssr_fail(SSR_ERR_UNSUPPORTED, "sets too large for one launch");
  return SSR_OK;
}

// workspace layouts: deterministic functions of the row counts, K and D
struct FdWs {
  size_t off_sets, off_mean_part, off_mean, off_cov_part, off_cov, off_stats, off_jwork, off_V, off_jstat, off_T, off_G, off_gwork, total;
  int64_t chunks, max_chunks;
};
static FdWs fd_ws(const int64_t* rows, int K, int D) {
  FdWs w{};
  for (int s = 0; s <= K; ++s) {
    const int64_t c = ssr_dstr_chunks(rows[s], D);
    w.chunks += c;
    w.max_chunks = c > w.max_chunks ? c : w.max_chunks;
  }
  const size_t DD = (size_t)D * D * sizeof(double), S = (size_t)K + 1;
  SsrWsLayout l;
  w.off_sets = l.take(S * sizeof(SsrDstrSet));
  w.off_mean_part = l.take((size_t)w.chunks * D * sizeof(double));
  w.off_mean = l.take(S * D * sizeof(double));
  w.off_cov_part = l.take((size_t)w.chunks * DD);
  w.off_cov = l.take(S * DD);
  w.off_stats = l.take(S * 2 * sizeof(double));
  w.off_jwork = l.take(DD);
  w.off_V = l.take(DD);
  w.off_jstat = l.take(2 * sizeof(double));
  w.off_T = l.take((size_t)K * DD);
  w.off_G = l.take((size_t)K * DD);
  w.off_gwork = l.take((size_t)K * DD);
  w.total = l.o;
  return w;
}
static int fd_launch_check(const FdWs& w, int K, int D) {
  const int nt = ssr_dstr_tiles(D);
  if (int rc = check_threads(w.max_chunks, (int64_t)nt * nt, K + 1, SSR_DSTR_NT)) return rc;
  if ((double)(K + 1) * D * D >= 4294967296.0) return ssr_fail(SSR_ERR_UNSUPPORTED, "sets too large for one launch");
  return SSR_OK;
}

extern "C" size_t ssr_frechet_workspace_bytes(const int64_t* rows, int K, int D) {
  if (check_sets(rows, K, D)) return 0;
  const FdWs w = fd_ws(rows, K, D);
  if (fd_launch_check(w, K, D)) return 0;
  return w.total;
}

extern "C" int ssr_frechet(const void* data, int f64, const int64_t* offset, const int64_t* rows, int K, int D, int64_t ld, int max_sweeps,
                           double* out, double* moments_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_sets(rows, K, D)) return rc;
  if (int rc = check_layout(offset, K, D, ld)) return rc;
  if (max_sweeps < 1 || max_sweeps > SSR_DISTRIBUTION_MAX_SWEEPS) return ssr_fail(SSR_ERR_INVALID_ARG, "max_sweeps must be in [1, 200]");
  if (K == 0) return SSR_OK;
  int64_t total_rows = 0;
  for (int s = 0; s <= K; ++s) total_rows += rows[s];
  if (!out || (total_rows > 0 && !data)) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  const FdWs w = fd_ws(rows, K, D);
  if (int rc = fd_launch_check(w, K, D)) return rc;
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  std::vector<SsrDstrSet> sets((size_t)K + 1);
  int64_t c0 = 0;
  for (int i = 0; i <= K; ++i) {
    sets[i] = SsrDstrSet{offset[i], rows[i], c0, ssr_dstr_chunks(rows[i], D)};
    c0 += sets[i].chunks;
  }
  // (pageable host memory: the copy has left `sets` when the call returns)
  HIP_TRY(hipMemcpyAsync(ws + w.off_sets, sets.data(), sets.size() * sizeof(SsrDstrSet), hipMemcpyHostToDevice, s));
  SsrDstrParams p{};
  p.data = data; p.ld = ld; p.D = D; p.K = K; p.max_sweeps = max_sweeps;
  p.sets = (const SsrDstrSet*)(ws + w.off_sets);
  p.mean_part = (double*)(ws + w.off_mean_part); p.mean = (double*)(ws + w.off_mean);
  p.cov_part = (double*)(ws + w.off_cov_part); p.cov = (double*)(ws + w.off_cov);
  p.stats = (double*)(ws + w.off_stats);
  p.jwork = (double*)(ws + w.off_jwork); p.V = (double*)(ws + w.off_V); p.jstat = (double*)(ws + w.off_jstat);
  p.T = (double*)(ws + w.off_T); p.G = (double*)(ws + w.off_G); p.gwork = (double*)(ws + w.off_gwork);
  p.out = out; p.moments_out = moments_out;
  const int nt = ssr_dstr_tiles(D);
  const unsigned S = (unsigned)K + 1;
  const int64_t DD = (int64_t)D * D;
  if (w.max_chunks > 0) {
    const dim3 grid((unsigned)w.max_chunks, (unsigned)nt, S);
    if (f64) SSR_LAUNCH(k_dstr_mean<double>, grid, dim3(SSR_DSTR_NT), s, p);
    else SSR_LAUNCH(k_dstr_mean<float>, grid, dim3(SSR_DSTR_NT), s, p);
  }
  SSR_LAUNCH(k_dstr_mean_finish, dim3((unsigned)(((int64_t)S * D + 255) / 256)), dim3(256), s, p);
  if (w.max_chunks > 0) {
    const dim3 grid((unsigned)w.max_chunks, (unsigned)(nt * nt), S);
    if (f64) SSR_LAUNCH(k_dstr_cov<double>, grid, dim3(SSR_DSTR_NT), s, p, nt);
    else SSR_LAUNCH(k_dstr_cov<float>, grid, dim3(SSR_DSTR_NT), s, p, nt);
  }
  SSR_LAUNCH(k_dstr_cov_finish, dim3((unsigned)((S * DD + 255) / 256)), dim3(256), s, p);
  SSR_LAUNCH(k_dstr_cov_stats, dim3((S + 63) / 64), dim3(64), s, p);
  SSR_LAUNCH(k_dstr_jacobi<true>, dim3(1), dim3(SSR_DSTR_JNT), s, p);
  const dim3 pgrid((unsigned)(nt * nt), (unsigned)K);
  SSR_LAUNCH(k_dstr_project<0>, pgrid, dim3(SSR_DSTR_NT), s, p, nt);
  SSR_LAUNCH(k_dstr_project<1>, pgrid, dim3(SSR_DSTR_NT), s, p, nt);
  SSR_LAUNCH(k_dstr_project<2>, pgrid, dim3(SSR_DSTR_NT), s, p, nt);
  SSR_LAUNCH(k_dstr_jacobi<false>, dim3((unsigned)K), dim3(SSR_DSTR_JNT), s, p);
  return SSR_OK;
}

struct KdWs { size_t off_combos, off_part, off_sums, total; int64_t tiles; int max_ta, max_tb; };
static KdWs kd_ws(const int64_t* rows, int K, int n_gamma, std::vector<SsrDstrCombo>* combos) {
  KdWs w{};
  auto add = [&](int64_t ra, int64_t rb, int same, int sa, int sb) {
    const int64_t Ta = ssr_dstr_tiles(ra), Tb = ssr_dstr_tiles(rb);
    if (combos) combos->push_back(SsrDstrCombo{(int64_t)sa, ra, (int64_t)sb, rb, w.tiles, same});      // (offsets: filled in by the caller from the set numbers)
    w.tiles += Ta * Tb;
    w.max_ta = Ta > w.max_ta ? (int)Ta : w.max_ta;
    w.max_tb = Tb > w.max_tb ? (int)Tb : w.max_tb;
  };
  add(rows[0], rows[0], 1, 0, 0);
  for (int k = 1; k <= K; ++k) {
    add(rows[k], rows[k], 1, k, k);
    add(rows[0], rows[k], 0, 0, k);
  }
  SsrWsLayout l;
  w.off_combos = l.take((size_t)(1 + 2 * K) * sizeof(SsrDstrCombo));
  w.off_part = l.take((size_t)w.tiles * n_gamma * sizeof(double));
  w.off_sums = l.take((size_t)(1 + 2 * K) * n_gamma * sizeof(double));
  w.total = l.o;
  return w;
}
static int check_gamma_count(int n_gamma) {
  if (n_gamma < 1 || n_gamma > SSR_DISTRIBUTION_MAX_GAMMA) return ssr_fail(SSR_ERR_INVALID_ARG, "n_gamma must be in [1, 8]");
  return SSR_OK;
}

extern "C" size_t ssr_kernel_distance_workspace_bytes(const int64_t* rows, int K, int D, int n_gamma) {
  if (check_sets(rows, K, D) || check_gamma_count(n_gamma)) return 0;
  const KdWs w = kd_ws(rows, K, n_gamma, nullptr);
  if (check_threads(w.max_tb, w.max_ta, 1 + 2 * K, SSR_DSTR_NT)) return 0;
  return w.total;
}

extern "C" int ssr_kernel_distance(const void* data, int f64, const int64_t* offset, const int64_t* rows, int K, int D, int64_t ld,
                                   const double* gamma, int n_gamma, double scale, double* out, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  if (int rc = check_sets(rows, K, D)) return rc;
  if (int rc = check_layout(offset, K, D, ld)) return rc;
  if (int rc = check_gamma_count(n_gamma)) return rc;
  if (!gamma) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int g = 0; g < n_gamma; ++g)
    if (!(gamma[g] > 0.0 && gamma[g] <= 1.7e308)) return ssr_fail(SSR_ERR_INVALID_ARG, "gamma must be finite and > 0");
  if (!(fabs(scale) <= 1.7e308)) return ssr_fail(SSR_ERR_INVALID_ARG, "scale must be finite");
  if (K == 0) return SSR_OK;
  int64_t total_rows = 0;
  for (int s = 0; s <= K; ++s) total_rows += rows[s];
  if (!out || (total_rows > 0 && !data)) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  std::vector<SsrDstrCombo> combos;
  const KdWs w = kd_ws(rows, K, n_gamma, &combos);
  if (int rc = check_threads(w.max_tb, w.max_ta, 1 + 2 * K, SSR_DSTR_NT)) return rc;
  if (!workspace || workspace_bytes < w.total) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  for (auto& c : combos) { c.off_a = offset[c.off_a]; c.off_b = offset[c.off_b]; }
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(ws + w.off_combos, combos.data(), combos.size() * sizeof(SsrDstrCombo), hipMemcpyHostToDevice, s));
  SsrDstrPairParams p{};
  p.data = data; p.ld = ld; p.D = D; p.K = K; p.n_gamma = n_gamma;
  for (int g = 0; g < n_gamma; ++g) p.gamma[g] = gamma[g];
  p.scale = scale;
  p.combos = (const SsrDstrCombo*)(ws + w.off_combos);
  p.part = (double*)(ws + w.off_part); p.sums = (double*)(ws + w.off_sums); p.out = out;
  if (w.max_ta > 0 && w.max_tb > 0) {
    const dim3 grid((unsigned)w.max_tb, (unsigned)w.max_ta, (unsigned)(1 + 2 * K));
    if (f64) SSR_LAUNCH((k_dstr_pairs<double, false>), grid, dim3(SSR_DSTR_NT), s, p);
    else SSR_LAUNCH((k_dstr_pairs<float, false>), grid, dim3(SSR_DSTR_NT), s, p);
  }
  SSR_LAUNCH(k_dstr_finish<0>, dim3((unsigned)(1 + 2 * K)), dim3(SSR_DSTR_NT), s, p);
  SSR_LAUNCH(k_dstr_finish<1>, dim3((unsigned)(((int64_t)K * n_gamma + SSR_DSTR_NT - 1) / SSR_DSTR_NT)), dim3(SSR_DSTR_NT), s, p);
  return SSR_OK;
}

extern "C" int ssr_pairwise_distances(const void* data, int f64, int64_t offset, int64_t rows, int D, int64_t ld, const int64_t* index, int n,
                                      double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_sets(&rows, 0, D)) return rc;
  if (int rc = check_layout(&offset, 0, D, ld)) return rc;
  if (n < 0 || n > SSR_DISTRIBUTION_MAX_PAIR_ROWS) return ssr_fail(SSR_ERR_INVALID_ARG, "n must be in [0, 2048]");
  if (n > 0 && !index) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int i = 0; i < n; ++i)
    if (index[i] < 0 || index[i] >= rows) return ssr_fail(SSR_ERR_INVALID_ARG, "index out of range");
  if (n < 2) return SSR_OK;
  if (!data || !out) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  if (!workspace || workspace_bytes < SSR_DISTRIBUTION_PAIRWISE_WORKSPACE) return ssr_fail(SSR_ERR_WORKSPACE, "workspace too small");
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  // workspace: the index list, then the one combination (pageable host memory: both copies have left it when the call returns)
  const size_t off_combo = SSR_DISTRIBUTION_MAX_PAIR_ROWS * sizeof(int64_t);
  const SsrDstrCombo combo{offset, (int64_t)n, offset, (int64_t)n, 0, 1};
  HIP_TRY(hipMemcpyAsync(ws, index, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ws + off_combo, &combo, sizeof(combo), hipMemcpyHostToDevice, s));
  SsrDstrPairParams p{};
  p.data = data; p.ld = ld; p.D = D; p.K = 0; p.n_gamma = 0;
  p.combos = (const SsrDstrCombo*)(ws + off_combo);
  p.index = (const int64_t*)ws; p.dist_out = out;
  const int T = ssr_dstr_tiles(n);
  const dim3 grid((unsigned)T, (unsigned)T, 1);
  if (f64) SSR_LAUNCH((k_dstr_pairs<double, true>), grid, dim3(SSR_DSTR_NT), s, p);
  else SSR_LAUNCH((k_dstr_pairs<float, true>), grid, dim3(SSR_DSTR_NT), s, p);
  return SSR_OK;
}
