/* Part of the C ABI of libssrhip.so: the magnitude-squared coherence family.  Included by include/ssr_hip.h (which supplies the
 * error codes, SSR_MAX_BANDS and the integer types); valid C99. */
#ifndef SSR_HIP_COHERENCE_H_
#define SSR_HIP_COHERENCE_H_

/* Welch-averaged magnitude-squared coherence of an estimate against its target, and the signal-to-distortion ratio derived
 * from it (not in the reference; Kates 1992, Kates & Arehart 2005).  Estimate e is scored against target
 * tgt_index[e] and is as long as it.  Segments of N = n_fft samples (256, 512, 1024 or 2048) every hop samples (1 <= hop <=
 * n_fft), periodic Hann window, no padding, no centring, no detrending: K = 1 + (len - N) / hop segments for len >= N, else 0.
 * With X[t][k], Y[t][k] the DFTs of segment t of the target and of the estimate, 0 <= k <= N / 2:
 *   Sxx[k] = sum_t |X|^2, Syy[k] = sum_t |Y|^2, Sxy[k] = sum_t Y conj(X)   (every bin once, no density scaling)
 *   g2[k] = min(1, |Sxy|^2 / (Sxx Syy)), and 0 where Sxx Syy == 0: digital silence is incoherent, not NaN
 * and per band of bins lo <= k <= hi
 *   msc = mean of g2, coh_sdr = 10 log10((sum g2 Syy + EPS) / (sum (1 - g2) Syy + EPS)) with EPS = DBL_EPSILON, coh_bins =
 *   the number of bins with g2 >= thr.
 * K < 2 (one segment gives g2 = 1 identically) and an empty band give NaN in all three.  All arithmetic is float64.
 * tgt / est: float32, or float64 where tgt_f64 / est_f64, read where they lie; tgt_off / est_off: DEVICE int64 sample offsets.
 * tgt_len, tgt_index and bands are HOST int32 arrays: validated before anything is enqueued (lengths in [0, 2^29), indices in
 * [0, n_tgt), 1 <= n_bands <= SSR_MAX_BANDS, 0 < thr <= 1) and copied into the workspace on `stream` (from page-locked memory
 * the copy is asynchronous: keep the values until the stream has reached it).  bands: [n_est][n_bands][2], the inclusive (lo, hi)
 * of each band of each estimate; lo > hi is the empty band, otherwise 0 <= lo <= hi <= n_fft / 2.  n_est = 0: nothing is enqueued.
 * out: DEVICE double [n_est][n_bands][3] = msc, coh_sdr, coh_bins.  msc_out: DEVICE double [n_est][n_fft / 2 + 1], g2 of every
 * bin (NaN where K < 2), or NULL; passing it changes no bit of out.  Deterministic: fixed-order sums, no atomics; a pair gives
 * the same bits alone, in any batch and at any position, and a band's row does not depend on the other bands.  workspace:
 * ssr_coherence_workspace_bytes (0 for invalid arguments).  One launch holds a workgroup of n_fft / 8 threads per chunk of 32
 * segments: SSR_ERR_UNSUPPORTED when that is 2^32 threads or more (checked before anything is enqueued). */
size_t ssr_coherence_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft, int hop,
                                     int n_bands);
int ssr_coherence(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                  int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_fft, int hop, int n_bands,
                  const int32_t* bands /* [n_est][n_bands][2] */, double thr, double* out /* [n_est][n_bands][3] */,
                  double* msc_out /* [n_est][n_fft / 2 + 1] or NULL */, void* workspace, size_t workspace_bytes, void* stream);

#endif /* SSR_HIP_COHERENCE_H_ */
