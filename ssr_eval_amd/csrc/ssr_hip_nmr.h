/* Part of the C ABI of libssrhip.so: the noise-to-mask family.  Included by include/ssr_hip.h (which supplies the error codes and
 * the integer types); valid C99. */
#ifndef SSR_HIP_NMR_H_
#define SSR_HIP_NMR_H_

#define SSR_NMR_BANDS 128  /* the most bands a call takes (109 bands of a quarter Bark reach 18 kHz) */
#define SSR_NMR_COLUMNS 6  /* columns of out */
#define SSR_NMR_TABLE 8    /* doubles per band of `table` */

/* The noise-to-mask ratio of an estimate against its target: the error spectrum per critical band over the masking threshold the
 * target itself produces (not in the reference; the FFT ear model of ITU-R BS.1387 after Kabal 2002, restated - no
 * conformance is claimed).  Estimate e is scored against target tgt_index[e] and is as long as it.  Frames of N = n_fft samples
 * (256, 512, 1024 or 2048) every N / 2 samples, periodic Hann window, no padding, K = 1 + (len - N) / (N / 2) frames for len >= N,
 * else 0.  With the caller's tables - weights[k] = G W2[k], and per band i its bins bins[i] = (k_lo, k_hi), and table[i] = (u_lo,
 * u_hi, Ein, c_up, ad, 1 / Bs, a, mgain) -
 *   Eb[t][i] = u_lo Px[k_lo] + Px[k_lo + 1 .. k_hi - 1] + u_hi Px[k_hi] + Ein, Px = weights |X|^2 (k_lo == k_hi: u_lo Px[k_lo] + Ein),
 *   Pn[t][i] = the same sum of weights (|X| - |Y|)^2, without Ein,
 *   Es[t][i] = (sum_l (Eb[l] S[i][l])^0.4)^2.5 / Bs[i], S[i][l] = r_l^(i - l) for i >= l with r_l = 10^((c_up[l] + 2 log10 Eb[l]) / 40),
 *              10^(-0.675 (l - i)) below, each column divided by its sum over the bands (ad[l] = sum_{j = 1 .. l} 10^(-0.675 j)),
 *   Ef[t] = a Ef[t - 1] + (1 - a) Es[t], Ef[-1] = 0; M[t][i] = max(Ef, Es) mgain; R = Pn / M.
 * A target's mask depends on the target alone and is made once for all its estimates.  All arithmetic is float64.
 * tgt / est: float32, or float64 where tgt_f64 / est_f64, read where they lie; tgt_off / est_off: DEVICE int64 sample offsets.
 * weights: DEVICE double [n_fft / 2 + 1] (the caller's table: finite, >= 0), only read.
 * tgt_len, tgt_index, bins, table and split are HOST arrays: validated before anything is enqueued (lengths in [0, 2^29), indices in
 * [0, n_tgt), 1 <= n_bands <= SSR_NMR_BANDS, 0 <= k_lo <= k_hi <= n_fft / 2, u_lo and u_hi in [0, 1], Ein, 1 / Bs and mgain finite
 * and > 0, c_up and ad finite, ad >= 0, a in [0, 1), split [n_est] = -1 (no split: nmr_hf and nmr_lf NaN) or the first band of the
 * upper part in [0, n_bands]) and copied into the workspace on `stream` (from page-locked memory the copy is asynchronous: keep the
 * values until the stream has reached it).  n_est = 0: nothing is enqueued.
 * out: DEVICE double [n_est][SSR_NMR_COLUMNS] = nmr (10 log10 max(mean_{t,i} R, 1e-20)), nmr_seg (the mean over frames of 10 log10
 * max(mean_i R[t], 1e-20)), rdf (the share of frames with max_i R[t][i] >= 10^0.15), nmr_hf / nmr_lf (nmr over the bands from the
 * split up / below it; NaN without a split and for an empty side), frames (K).  K = 0: NaN, frames 0.  A mean at or under 1e-20 is
 * -200 exactly; no value is infinite.  bands_out: DEVICE double [n_est][n_bands], mean_t R (NaN for K = 0), or NULL; mask_out: DEVICE
 * double [sum of K over the targets][n_bands], M of every frame of every target in target order, or NULL; passing either changes no
 * bit of out.  Deterministic: fixed-order sums, no atomics; a pair gives the same bits alone, in any batch and at any position.
 * workspace: ssr_nmr_workspace_bytes (0 for invalid arguments).  A launch holds a workgroup of n_fft / 8 threads per chunk of 32
 * frames, or one of 128 threads per target or per estimate: SSR_ERR_UNSUPPORTED when any of these is 2^32 threads or more (checked
 * before anything is enqueued). */
size_t ssr_nmr_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft, int n_bands);
int ssr_nmr(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est, int est_f64,
            const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_fft, int n_bands,
            const double* weights /* [n_fft / 2 + 1] */, const int32_t* bins /* [n_bands][2] */,
            const double* table /* [n_bands][SSR_NMR_TABLE] */, const int32_t* split /* [n_est] */,
            double* out /* [n_est][SSR_NMR_COLUMNS] */, double* bands_out /* [n_est][n_bands] or NULL */,
            double* mask_out /* [frames][n_bands] or NULL */, void* workspace, size_t workspace_bytes, void* stream);

#endif /* SSR_HIP_NMR_H_ */
