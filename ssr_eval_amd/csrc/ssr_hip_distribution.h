/* Part of the C ABI of libssrhip.so: the distribution family - the Fréchet distance and the kernel distance (unbiased MMD^2) of sets
 * of embedding vectors, "everything after the embedding" of FAD and KAD.  Included by include/ssr_hip.h (which supplies the error
 * codes and the integer types) after ssr_hip_modulation.h; valid C99. */
#ifndef SSR_HIP_DISTRIBUTION_H_
#define SSR_HIP_DISTRIBUTION_H_

#define SSR_DISTRIBUTION_MAX_DIM 1024         /* D, the length of an embedding vector */
#define SSR_DISTRIBUTION_MAX_GAMMA 8          /* kernel bandwidths per call */
#define SSR_DISTRIBUTION_MAX_SETS 16383       /* K, estimate sets per call */
#define SSR_DISTRIBUTION_MAX_SWEEPS 200       /* the largest max_sweeps */
#define SSR_DISTRIBUTION_MAX_PAIR_ROWS 2048   /* rows of ssr_pairwise_distances */
#define SSR_DISTRIBUTION_PAIRWISE_WORKSPACE 16640 /* its workspace in bytes */
#define SSR_FRECHET_COLS 8                    /* columns of ssr_frechet's out */
#define SSR_KERNEL_DISTANCE_COLS 4            /* columns of ssr_kernel_distance's out */

/* Does a SET of outputs look like the set of targets?    One reference set R[n][D] and K >= 1 estimate sets E_k[m_k][D]
 * are scored in one call.  `data` is one DEVICE buffer of float32 rows, or float64 where f64; set s (0: the reference, 1 + k: estimate
 * k) has rows[s] rows of D values, row i at element offset[s] + i ld, ld >= D; what lies between rows and sets is never read.  rows,
 * offset and gamma are HOST arrays: validated before anything is enqueued and copied into the workspace on `stream` (from page-locked
 * memory the copy is asynchronous: keep the values until the stream has reached it).  All arithmetic is float64.
 *   moments   mu = column mean, Sigma = centred covariance with ddof = 1.  Two passes: the mean first, then sums of products of centred
 *             values (never sum x x^T - n mu mu^T).  Every sum has a fixed shape: chunks of max(256, 4 D) rows, the chunk partials added
 *             in chunk order.
 *   Fréchet   fd = |mu_r - mu_e|^2 + tr Sigma_r + tr Sigma_e - 2 tr sqrt(Sigma_r Sigma_e).  With Sigma_r = V L V^T and W = V L^(1/2) the
 *             last term is sum_i sqrt(g_i), g_i >= 0 the eigenvalues of the symmetric G = W^T Sigma_e W.  Both eigenproblems use a
 *             one-sided (Hestenes) Jacobi on the columns of the symmetric PSD matrix (V accumulated for Sigma_r only; eigenvalue i is the
 *             2-norm of final column i), pairs in round-robin order (D - 1 steps of floor(D / 2) disjoint pairs per sweep, a bye for odd
 *             D).  Columns p < q with a = |c_p|^2, b = |c_q|^2, c = c_p . c_q: skipped if a or b <= D 2^-104 max_j |c_j|^2 (a null column;
 *             the maximum over the input's columns) or |c| <= D 2^-52 sqrt(a b); else zeta = (b - a) / (2 c), t = sgn(zeta) / (|zeta| +
 *             sqrt(1 + zeta^2)) with sgn(0) = 1, cs = 1 / sqrt(1 + t^2), sn = cs t, c_p <- cs c_p - sn c_q, c_q <- sn c_p + cs c_q.  A sweep
 *             without a rotation ends the iteration; the sweep loop has the fixed bound max_sweeps (1 .. 200): not converged at the
 *             bound gives fd = tr_sqrt = NaN and sweeps = -1, it never runs longer.  No clamp: identical sets give a value of rounding
 *             size of either sign.  n < 2, m_k < 2 and a non-finite moment give NaN; no infinity leaves the library.
 *   kernel    mmd2 = sum_{i != j} k(r_i, r_j) / (n (n - 1)) + sum_{i != j} k(e_i, e_j) / (m (m - 1)) - 2 sum_{i, j} k(r_i, e_j) / (n m) with
 *             k(x, y) = exp(-gamma |x - y|^2), |x - y|^2 the sum of squared differences; kd = scale mmd2.  The reference's own sum is
 *             computed once per call.  n < 2 or m_k < 2 give NaN.
 * ssr_frechet: out DEVICE double [K][8] = fd, |mu_r - mu_e|^2, tr Sigma_r, tr Sigma_e, tr sqrt(Sigma_r Sigma_e), sweeps_ref, sweeps_est,
 * rank_ref (the sweep counts and the number of non-null columns of the reference's Jacobi, as whole numbers).  moments_out: DEVICE
 * double [1 + K][D + D D], mean and row-major covariance of every set, or NULL; passing it changes no other bit.
 * ssr_kernel_distance: out DEVICE double [K][n_gamma][4] = kd, mmd2, mean k(r, r), mean k(e, e); a row of gamma does not depend on
 * the other gamma.  ssr_pairwise_distances: the distances |x_i - x_j|, i < j, of the n <= 2048 rows index[0 .. n) (HOST, each in [0,
 * rows)) of one set at element `offset`: out DEVICE double [n (n - 1) / 2], pair (i, j) at i n - i (i + 1) / 2 + j - i - 1; workspace: at
 * least SSR_DISTRIBUTION_PAIRWISE_WORKSPACE bytes.
 * Checked before anything is enqueued (SSR_ERR_INVALID_ARG): 1 <= D, ld >= D, K >= 0, rows >= 0, offsets >= 0, 1 <= max_sweeps <= 200,
 * 1 <= n_gamma <= 8, every gamma finite and > 0, scale finite, non-null buffers.  SSR_ERR_UNSUPPORTED: D > SSR_DISTRIBUTION_MAX_DIM, K >
 * SSR_DISTRIBUTION_MAX_SETS, a set of more than 2^31 - 1 rows, a launch of 2^32 threads or more.  A too-small workspace is
 * SSR_ERR_WORKSPACE; the queries return 0 for invalid arguments.  K = 0 enqueues nothing.  Deterministic: fixed-order sums, no atomics;
 * a set gives the same bits alone, as any of the K and at any position.  The Jacobi runs on ONE workgroup per matrix (grid [1] for
 * Sigma_r, [K] for the G_k), O(D^3) per sweep: it runs once per corpus. */
size_t ssr_frechet_workspace_bytes(const int64_t* rows /* [1 + K] */, int K, int D);
int ssr_frechet(const void* data, int f64, const int64_t* offset /* [1 + K] */, const int64_t* rows /* [1 + K] */, int K, int D, int64_t ld,
                int max_sweeps, double* out /* [K][8] */, double* moments_out /* [1 + K][D + D D] or NULL */, void* workspace,
                size_t workspace_bytes, void* stream);
size_t ssr_kernel_distance_workspace_bytes(const int64_t* rows /* [1 + K] */, int K, int D, int n_gamma);
int ssr_kernel_distance(const void* data, int f64, const int64_t* offset /* [1 + K] */, const int64_t* rows /* [1 + K] */, int K, int D,
                        int64_t ld, const double* gamma /* [n_gamma] */, int n_gamma, double scale, double* out /* [K][n_gamma][4] */,
                        void* workspace, size_t workspace_bytes, void* stream);
int ssr_pairwise_distances(const void* data, int f64, int64_t offset, int64_t rows, int D, int64_t ld, const int64_t* index /* [n] */, int n,
                           double* out /* [n (n - 1) / 2] */, void* workspace, size_t workspace_bytes, void* stream);

#endif /* SSR_HIP_DISTRIBUTION_H_ */
