/* libssrhip - C ABI, part of ssr_hip.h (included by it beside the waveform metrics; include ssr_hip.h, not this file).
 *
 * Filter-invariant SDR (not in the reference): the SDR of BSS Eval (Vincent, Gribonval & Fevotte, "Performance
 * measurement in blind audio source separation", IEEE TASLP 14(4), 2006; mir_eval.separation.bss_eval_sources) for one source,
 * with a causal `taps`-tap FIR filter of the target as the allowed distortion.  float64 throughout, EPS = DBL_EPSILON,
 * x = target, y = estimate, both of n samples, L = taps:
 *   r[k] = sum_{t=0}^{n-1-k} x[t] x[t+k],  b[k] = sum_{t=0}^{n-1-k} x[t] y[t+k],  k = 0 .. L-1   (the correlations over the
 *          zero-padded support of n + L - 1 samples: terms with t + k >= n do not exist)
 *   c      solves Toeplitz(r) c = b (Levinson's recursion, no diagonal loading)
 *   p[t] = sum_k c[k] x[t-k],  e[t] = y[t] - p[t],  t = 0 .. n+L-2 with y zero beyond n, every residual formed sample by sample
 *   sdr     = 10 log10((sum p^2 + EPS) / (sum e^2 + EPS))
 *   sdr_lag = the smallest k with |c[k]| maximal: the estimate's latency in samples
 * n = 0, or r[0] = 0 (a digitally silent target): both NaN, and a filter of zeros.  If the prediction error of the recursion is
 * <= 0 or not finite at order m, the recursion stops there and the taps from m on are 0.
 * Pair e scores estimate e (est + est_off[e], as long as its target) against target tgt_index[e]; pairs next to each other that
 * name one target compute its r once.  tgt / est: float32, or float64 where tgt_f64 / est_f64; tgt_off / est_off: DEVICE int64
 * sample offsets.  tgt_len and tgt_index are HOST int32 arrays: validated before anything is enqueued (taps in [1,
 * SSR_BSS_MAX_TAPS], lengths in [0, 2^29), indices in [0, n_tgt)) and copied into the workspace on `stream` (from page-locked
 * memory the copy is asynchronous: keep the values until the stream has reached it).  n_est = 0: nothing is enqueued.
 * SSR_ERR_UNSUPPORTED, before anything is enqueued, where a grid would not fit one launch.
 * out: double [n_est][2] = sdr, sdr_lag.  filt: double [n_est][taps], the filters c, or NULL.  Deterministic: fixed-order sums, no
 * atomics; a pair gives the same bits alone, in any batch and at any position.  workspace: the size query below (0 for invalid
 * arguments). */
#ifndef SSR_HIP_BSS_H_
#define SSR_HIP_BSS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSR_BSS_MAX_TAPS 512
size_t ssr_bss_sdr_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int taps);
int ssr_bss_sdr(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt,
                const void* est, int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est,
                int taps, double* out /* [n_est][2]: sdr, sdr_lag */, double* filt /* [n_est][taps] or NULL */,
                void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SSR_HIP_BSS_H_ */
