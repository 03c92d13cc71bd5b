// libssrhip.so translation unit: bootstrap replicates of the mean-of-speaker-means aggregate and their per-column summary
// (ssr_bootstrap.h) and their entry points (ssr_bootstrap_means, ssr_bootstrap_summary, ssr_bootstrap_geometry).
#include "ssr_host.h"
#include "ssr_bootstrap.h"

static_assert(SSR_BOOT_UTTERANCE == SSR_BOOTSTRAP_UTTERANCE && SSR_BOOT_SPEAKER == SSR_BOOTSTRAP_SPEAKER, "scheme codes");
static_assert(SSR_BOOT_MAX_Q == SSR_BOOTSTRAP_MAX_Q && SSR_BOOT_MAX_SPK == SSR_BOOTSTRAP_MAX_SPEAKERS, "limits");

__global__ __launch_bounds__(SSR_BOOT_NT) void k_boot_means(SsrBootParams p) {
  __shared__ int idx[SSR_BOOT_TILE], slot_spk[SSR_BOOT_MAX_SPK];
  SsrBlk blk{(int)threadIdx.x};
  ssr_boot_means_body(p, blk, (int)blockIdx.x, (int)blockIdx.y * SSR_BOOT_NT, idx, slot_spk);
}

__global__ __launch_bounds__(SSR_BOOT_NT) void k_boot_mask(SsrBootParams p) {
  __shared__ int bad[SSR_BOOT_NT];
  SsrBlk blk{(int)threadIdx.x};
  ssr_boot_mask_body(p, blk, (int)blockIdx.x * 64, (int64_t)blockIdx.y * SSR_BOOT_MASK_ROWS, bad);
}

__global__ __launch_bounds__(SSR_BOOT_SUM_NT) void k_boot_summary(SsrBootSumParams p) {
  __shared__ double s[SSR_BOOT_MAX_B], wsum[SSR_BOOT_SUM_NT / 64], wsq[SSR_BOOT_SUM_NT / 64];
  __shared__ int wflag[SSR_BOOT_SUM_NT / 64];
  SsrBlk blk{(int)threadIdx.x};
  ssr_boot_summary_body(p, blk, (int)blockIdx.x, s, wsum, wsq, wflag);
}

// host-side validation: nothing is queued unless every argument is usable
static int check_boot_count(int n_boot) {
  if (n_boot < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "n_boot must be >= 1");
  if (n_boot > SSR_BOOT_MAX_B) return ssr_fail(SSR_ERR_UNSUPPORTED, "n_boot above the cap of 16384 replicates (ssr_bootstrap_geometry)");
  return SSR_OK;
}

extern "C" int ssr_bootstrap_geometry(int* index_tile, int* max_boot) {
  if (!index_tile || !max_boot) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  *index_tile = SSR_BOOT_TILE;
  *max_boot = SSR_BOOT_MAX_B;
  return SSR_OK;
}

extern "C" int ssr_bootstrap_means(const double* table, int64_t n_rows, int n_cols, const int32_t* spk_off, int n_spk, int n_boot,
                                   uint64_t seed, int scheme, double* reps, void* stream) {
  if (!table || !spk_off || !reps) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  if (n_rows < 1 || n_rows > 0x7fffffff || n_cols < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "n_rows must be in [1, 2^31) and n_cols >= 1");
  if (n_spk < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "n_spk must be >= 1");
  if (scheme != SSR_BOOT_UTTERANCE && scheme != SSR_BOOT_SPEAKER)
    return ssr_fail(SSR_ERR_INVALID_ARG, "scheme must be SSR_BOOTSTRAP_UTTERANCE or SSR_BOOTSTRAP_SPEAKER");
  if (int rc = check_boot_count(n_boot)) return rc;
  if (n_spk > SSR_BOOT_MAX_SPK) return ssr_fail(SSR_ERR_UNSUPPORTED, "more than 512 speakers");
  if (spk_off[0] != 0 || spk_off[n_spk] != n_rows) return ssr_fail(SSR_ERR_INVALID_ARG, "spk_off must run from 0 to n_rows");
  for (int s = 0; s < n_spk; ++s) {
    if (spk_off[s + 1] < spk_off[s]) return ssr_fail(SSR_ERR_INVALID_ARG, "spk_off must ascend");
    if (spk_off[s + 1] == spk_off[s]) return ssr_fail(SSR_ERR_INVALID_ARG, "empty speaker in spk_off");
  }
  const int col_chunks = ssr_ceil_div(n_cols, SSR_BOOT_NT), row_chunks = ssr_ceil_div(n_rows, SSR_BOOT_MASK_ROWS);
  if (col_chunks > 65535 || row_chunks > 65535) return ssr_fail(SSR_ERR_UNSUPPORTED, "table too large for one launch");
  SsrBootParams p{};
  p.table = table; p.n_rows = n_rows; p.n_cols = n_cols; p.n_spk = n_spk; p.n_boot = n_boot; p.scheme = scheme;
  p.key0 = (uint32_t)(seed & 0xffffffffu); p.key1 = (uint32_t)(seed >> 32);
  p.reps = reps;
  memcpy(p.spk_off, spk_off, (size_t)(n_spk + 1) * sizeof(int32_t));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_boot_means, dim3((unsigned)n_boot, (unsigned)col_chunks), dim3(SSR_BOOT_NT), 0, s, p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_boot_mask, dim3((unsigned)ssr_ceil_div(n_cols, 64), (unsigned)row_chunks), dim3(SSR_BOOT_NT), 0, s, p);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}

extern "C" int ssr_bootstrap_summary(const double* reps, int n_boot, int n_cols, const double* q, int n_q, double* out,
                                     int32_t* counts, void* stream) {
  if (!reps || !out || !counts || (n_q > 0 && !q)) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  if (n_cols < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "n_cols must be >= 1");
  if (n_q < 0 || n_q > SSR_BOOT_MAX_Q) return ssr_fail(SSR_ERR_INVALID_ARG, "n_q must be in [0, 8]");
  for (int i = 0; i < n_q; ++i)
    if (!(q[i] >= 0.0 && q[i] <= 1.0)) return ssr_fail(SSR_ERR_INVALID_ARG, "q must lie in [0, 1]");
  if (int rc = check_boot_count(n_boot)) return rc;
  SsrBootSumParams p{};
  p.reps = reps; p.n_boot = n_boot; p.n_cols = n_cols; p.n_q = n_q; p.out = out; p.counts = counts;
  for (int i = 0; i < n_q; ++i) p.q[i] = q[i];
  hipLaunchKernelGGL(k_boot_summary, dim3((unsigned)n_cols), dim3(SSR_BOOT_SUM_NT), 0, (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return SSR_OK;
}
