/* Part of the C ABI of libssrhip.so: delay estimation and compensation, a stage in front of the metrics.  Included by
 * include/ssr_hip.h (which supplies the error codes and the integer types); valid C99. */
#ifndef SSR_HIP_ALIGN_H_
#define SSR_HIP_ALIGN_H_

#define SSR_ALIGN_MAX_LAG 4096 /* the largest max_lag */
#define SSR_ALIGN_COLUMNS 4    /* columns of rows */

/* The delay of an estimate against its target by a bounded two-sided cross-correlation in float64, and the estimate with that delay
 * taken out (not in the reference).  Estimate e (est_len[e] = n_y samples, y) is searched against target tgt_index[e]
 * (tgt_len = n_x samples, x); the lengths may differ.  With L = max_lag, 1 <= L <= SSR_ALIGN_MAX_LAG:
 *   c[d] = sum_t x[t] y[t + d] over the t with 0 <= t < n_x and 0 <= t + d < n_y, d = -L .. L (no such t: 0); Ex = sum x^2, Ey = sum y^2
 *   d* = the d of the largest c[d]; among equal values the smallest |d|, among those the non-negative one
 *   frac = 0.5 (c[d*-1] - c[d*+1]) / (c[d*-1] - 2 c[d*] + c[d*+1]) clamped to [-0.5, 0.5]; 0 where |d*| = L (then edge = 1, else 0)
 *          or where the denominator is 0 or not finite
 *   corr = c[d*] / sqrt(Ex Ey)
 *   Ex = 0, Ey = 0, n_x = 0, n_y = 0 or not c[d*] > 0: d* = 0, frac = 0, edge = 0, corr = NaN.
 * A positive d* says the estimate is late.  shifted, where not NULL, receives z of n_y samples in the estimates' dtype at
 * shifted + shifted_off[e]: z[t] = y[t + d*], 0 where t + d* is outside [0, n_y) - a copy, bit for bit; with subsample != 0 and
 * frac != 0, z[t] = sum_{m=-16..16} h[m] y[t + d* + m] (y zero outside its range), h[m] = s(u) w(u) / sum_m s(u) w(u), u = m - frac,
 * s(u) = (-1)^(m+1) sin(pi frac) / (pi u), w(u) = 0.5 (1 + cos(pi u / 17)), in float64 with one rounding to the estimates' dtype.
 * frac is reported whatever subsample says.  Signals hold finite samples.
 * tgt / est: float32, or float64 where tgt_f64 / est_f64, read where they lie; tgt_off / est_off / shifted_off: DEVICE int64 sample
 * offsets; shifted must not overlap est.  tgt_len, est_len and tgt_index are HOST arrays: validated before anything is enqueued
 * (lengths in [0, 2^29), indices in [0, n_tgt)) and copied into the workspace on `stream` (from page-locked memory the copy is
 * asynchronous: keep the values until the stream has reached it).  n_est = 0: nothing is enqueued.
 * rows: DEVICE double [n_est][SSR_ALIGN_COLUMNS] = d*, frac, corr, edge.  c: DEVICE double [n_est][2 L + 1] (lag -L first) or NULL;
 * passing it changes no bit of rows or shifted.  d* and the taps reach the shift through device memory: nothing waits on the host.
 * Deterministic: fixed-order sums, no atomics; a pair gives the same bits alone, in any batch and at any position.  workspace:
 * ssr_align_workspace_bytes (0 for invalid arguments): 8 (2 L + 1) bytes per tile of 16384 target samples of every pair.  One launch
 * holds a workgroup of 256 threads per such tile and block of 2048 of the 2 L lags below +L: SSR_ERR_UNSUPPORTED when that is 2^32 threads or more
 * (checked before anything is enqueued). */
size_t ssr_align_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* est_len, const int32_t* tgt_index, int n_est,
                                 int max_lag);
int ssr_align(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est, int est_f64,
              const int64_t* est_off, const int32_t* est_len, const int32_t* tgt_index, int n_est, int max_lag, int subsample,
              double* rows /* [n_est][SSR_ALIGN_COLUMNS] */, void* shifted /* or NULL */, const int64_t* shifted_off /* [n_est] */,
              double* c /* [n_est][2 max_lag + 1] or NULL */, void* workspace, size_t workspace_bytes, void* stream);

#endif /* SSR_HIP_ALIGN_H_ */
