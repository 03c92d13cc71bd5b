/* Part of the C ABI of libssrhip.so: the spectrum family - bandwidth, spectral edge, centroid, HF level and LTAS distance.
 * Included by include/ssr_hip.h (which supplies the error codes and the integer types); valid C99. */
#ifndef SSR_HIP_SPECTRUM_H_
#define SSR_HIP_SPECTRUM_H_

#define SSR_SPECTRUM_MAX_BANDS 40 /* analysis bands of the LTAS distance */
#define SSR_SPECTRUM_SIG_COLS 3   /* columns of sig_out */
#define SSR_SPECTRUM_PAIR_COLS 8  /* columns of pair_out */

/* What bandwidth did a signal come out with, and how much energy lies above a split compared with its target?  (The rolloff is the
 * reference's BasicTestee._find_cutoff, a host-side helper there, as a metric)  Every value comes from the long-term
 * average spectrum of a signal and is invariant to gain.  The signals are the n_tgt targets followed by the n_est estimates;
 * estimate e belongs to target tgt_index[e] and is as long as it.  Segments of N = n_fft samples (256, 512, 1024 or 2048) every hop
 * samples (1 <= hop <= n_fft), periodic Hann window, no padding, no centring, no detrending: K = 1 + (len - N) / hop segments for
 * len >= N, else 0.  With X[t][k] the unscaled DFT of windowed segment t, 0 <= k <= N / 2, and c[k] = 1 at k = 0 and k = N / 2, else 2:
 *   P[k] = sum_t |X|^2, A[k] = sum_t |X|   (A: the reference's magnitude-sum convention);  E_tot = sum c P over the bins lo .. hi
 *   rolloff  = the smallest bin r in lo .. hi with sum_{lo..r} A >= rho sum_{lo..hi} A
 *   edge     = the highest bin e in lo .. hi with P[e] >= max_{lo..hi}(P) 10^(-drop_db / 10)
 *   centroid = sum k c P / sum c P over lo .. hi, in bins
 *   L_b      = 10 log10(max(E_b / E_tot, DBL_EPSILON)), E_b = sum c P over analysis band b
 * and per estimate y with its target x and first upper bin split[e]:
 *   hf_db = 10 log10(max(E_hi / E_tot, DBL_EPSILON)) of each, E_hi = sum c P over the bins max(split[e], lo) .. hi; NaN where
 *   split[e] = -1 or no such bin exists;  d_b = L_b(y) - L_b(x), ltas_dist = sqrt(mean_b d_b^2), ltas_max = max_b |d_b|.
 * K = 0, an empty band (lo > hi) and E_tot = 0 (digital silence) give NaN in every value of the signal and in every pair value
 * that uses it; no infinity leaves the library.  All arithmetic is float64.
 * tgt / est: float32, or float64 where tgt_f64 / est_f64, read where they lie; tgt_off / est_off: DEVICE int64 sample offsets.
 * tgt_len, tgt_index, bands and split are HOST int32 arrays: validated before anything is enqueued (lengths in [0, 2^29), indices in
 * [0, n_tgt), 0 < rho < 1, 0 < drop_db <= 150, lo > hi or 0 <= lo <= hi <= n_fft / 2, 1 <= n_bands <= SSR_SPECTRUM_MAX_BANDS,
 * bands [n_bands][2] inclusive, disjoint and ascending inside 0 .. n_fft / 2, split[e] >= -1) and copied into the workspace on
 * `stream` (from page-locked memory the copy is asynchronous: keep the values until the stream has reached it).  n_est = 0 with
 * n_tgt > 0 measures the targets alone (est, est_off, tgt_index, split and pair_out may be NULL); n_tgt = n_est = 0: nothing is
 * enqueued.
 * sig_out: DEVICE double [n_tgt + n_est][3] = rolloff bin, edge bin, centroid in bins (times rate / n_fft: Hz).  pair_out: DEVICE
 * double [n_est][8] = hf_db of the estimate, hf_db of the target, rolloff / edge / centroid of the estimate minus the target's (in
 * bins), hf_db of the estimate minus the target's, ltas_dist, ltas_max.  ltas_out: DEVICE double [n_tgt + n_est][n_fft / 2 + 1],
 * c P / K of every bin (NaN where K = 0), or NULL; passing it changes no bit of the other outputs.  Deterministic: fixed-order
 * sums, no atomics; a signal and a pair give the same bits alone, in any batch and at any position.  workspace:
 * ssr_spectrum_workspace_bytes (0 for invalid arguments).  One launch holds a workgroup of n_fft / 8 threads per chunk of 32
 * segments of a signal: SSR_ERR_UNSUPPORTED when that is 2^32 threads or more, or with more than 2^24 signals (checked before
 * anything is enqueued). */
size_t ssr_spectrum_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft, int hop,
                                    int n_bands);
int ssr_spectrum(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                 int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_fft, int hop, int lo, int hi,
                 double rho, double drop_db, int n_bands, const int32_t* bands /* [n_bands][2] */, const int32_t* split /* [n_est] */,
                 double* sig_out /* [n_tgt + n_est][3] */, double* pair_out /* [n_est][8] */,
                 double* ltas_out /* [n_tgt + n_est][n_fft / 2 + 1] or NULL */, void* workspace, size_t workspace_bytes, void* stream);

#endif /* SSR_HIP_SPECTRUM_H_ */
