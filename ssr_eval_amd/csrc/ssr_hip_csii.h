/* Part of the C ABI of libssrhip.so: the coherence speech intelligibility index.  Included by include/ssr_hip.h (which supplies the
 * error codes and the integer types); valid C99. */
#ifndef SSR_HIP_CSII_H_
#define SSR_HIP_CSII_H_

#define SSR_CSII_BANDS 21   /* the most bands a call takes: the critical bands of ANSI S3.5-1997 */
#define SSR_CSII_COLUMNS 13 /* columns of out */

/* The coherence speech intelligibility index of an estimate against its target and the fitted three-level index I3 (not in the
 * reference; Kates & Arehart 2005).  Estimate e is scored against target tgt_index[e] and is as long as it.  Framing,
 * spectra and g2 are ssr_coherence's: segments of N = n_fft samples (256, 512, 1024 or 2048) every hop samples (1 <= hop <=
 * n_fft), periodic Hann window, no padding, K = 1 + (len - N) / hop segments for len >= N, else 0; g2[k] = min(1, |Sxy|^2 / (Sxx
 * Syy)), 0 where Sxx Syy == 0.  A target segment's level is its mean square ms_t (N unwindowed samples) against the mean square
 * ms_all of the whole target: class high where ms_t >= ms_all, mid where ms_t >= 0.1 ms_all, low where ms_t >= 0.001 ms_all,
 * dropped below that and where ms_t == 0.  The spectra are summed over four sets of segments - all K, low, mid, high - and per set
 * and band j
 *   num = sum_k W[j][k] g2[k] Syy[k], den = sum_k W[j][k] (1 - g2[k]) Syy[k],
 *   T_j = 0 where num + den == 0 or num == 0, 1 where den == 0, else (clip(10 log10(num / den), -15, 15) + 15) / 30,
 *   CSII = sum_j importance[j] T_j, and above a split band s: sum_{j >= s} importance[j] T_j / sum_{j >= s} importance[j];
 *   i3 = 1 / (1 + exp(-(-3.47 + 1.84 CSII_low + 9.99 CSII_mid))).
 * A set of fewer than 2 segments and a digitally silent target (ms_all == 0) give NaN; i3 is NaN where either input is.  All
 * arithmetic is float64.
 * tgt / est: float32, or float64 where tgt_f64 / est_f64, read where they lie; tgt_off / est_off: DEVICE int64 sample offsets.
 * weights: DEVICE double [n_bands][n_fft / 2 + 1], the band weights W (the caller's table: finite, >= 0), only read.
 * tgt_len, tgt_index, importance and split are HOST arrays: validated before anything is enqueued (lengths in [0, 2^29), indices
 * in [0, n_tgt), 1 <= n_bands <= SSR_CSII_BANDS, importance [n_bands] in (0, 1], split [n_est] = -1 (no split: the four _hf columns
 * NaN) or the first band of the upper part in [0, n_bands] (n_bands: no such band, NaN)) and copied into the workspace on `stream`
 * (from page-locked memory the copy is asynchronous: keep the values until the stream has reached it).  n_est = 0: nothing is
 * enqueued.
 * out: DEVICE double [n_est][SSR_CSII_COLUMNS] = csii (the set of all segments), csii_low, csii_mid, csii_high, i3, the _hf value of
 * the four sets in that order, then the segments in the four sets.  bands_out: DEVICE double [n_est][4][n_bands], T_j of every set
 * (NaN where the set's value is), or NULL; passing it changes no bit of out.  Deterministic: fixed-order sums, no atomics; a target's
 * classes depend on the target alone and a pair gives the same bits alone, in any batch and at any position.  workspace:
 * ssr_csii_workspace_bytes (0 for invalid arguments).  One launch holds a workgroup of n_fft / 8 threads per chunk of 32 segments:
 * SSR_ERR_UNSUPPORTED when that is 2^32 threads or more (checked before anything is enqueued). */
size_t ssr_csii_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft, int hop, int n_bands);
int ssr_csii(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est, int est_f64,
             const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_fft, int hop, int n_bands,
             const double* weights /* [n_bands][n_fft / 2 + 1] */, const double* importance /* [n_bands] */,
             const int32_t* split /* [n_est] */, double* out /* [n_est][SSR_CSII_COLUMNS] */,
             double* bands_out /* [n_est][4][n_bands] or NULL */, void* workspace, size_t workspace_bytes, void* stream);

#endif /* SSR_HIP_CSII_H_ */
