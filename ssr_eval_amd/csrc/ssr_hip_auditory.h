/* Part of the C ABI of libssrhip.so: the auditory family - neurogram similarity (NSIM) of gammatone spectrograms.
 * Included by include/ssr_hip.h (which supplies the error codes and the integer types); valid C99. */
#ifndef SSR_HIP_AUDITORY_H_
#define SSR_HIP_AUDITORY_H_

#define SSR_AUDITORY_MIN_BANDS 3      /* one interior band */
#define SSR_AUDITORY_MAX_BANDS 64
#define SSR_AUDITORY_MAX_BLOCKS 65536 /* hop-blocks per signal: 10 min 55 s at hop = rate / 100 */
#define SSR_AUDITORY_PAIR_COLS 3      /* columns of pair_out */

/* How alike do two signals look to the ear's filterbank?  The neurogram similarity index (Hines & Harte 2012; the core of ViSQOL) of
 * the gammatone spectrograms of every estimate and its target.  The signals are the n_tgt targets followed by the n_est
 * estimates; estimate e belongs to target tgt_index[e] and is as long as it.  All arithmetic is float64.
 *   filterbank  Hohmann's complex all-pole gammatone of order 4, band c from coef[c] = (Re a, Im a, g), |a| < 1:
 *               y_0[n] = g x[n], y_s[n] = y_{s-1}[n] + a y_s[n - 1] for s = 1 .. 4 from the zero state, z = y_4
 *   image       win = 2 hop, no padding: T = 1 + (len - win) / hop rows for len >= win, else 0;  B[j][c] = sum of |z_c[n]|^2 over the
 *               samples j hop .. (j + 1) hop - 1 in sample order;  P[t][c] = (B[t][c] + B[t + 1][c]) / (2 win)
 *   level       match_level: the estimate's P times sum P_target / sum P_estimate (1 where sum P_estimate = 0); else 1
 *   dB          top = max P_target, floor_db = 10 log10(top) - range_db;  D = max(10 log10 P, floor_db), G = D - floor_db, of both
 *               signals on the target's floor (P = 0: G = 0)
 *   nsim        w = g3 g3^T, g3 = (e^-2, 1, e^-2) / (1 + 2 e^-2), over the cells 1 <= t <= T - 2, 1 <= c <= n_bands - 2, centred:
 *               mu = sum w G, v = sum w (G - mu)^2, cov = sum w (G_r - mu_r)(G_d - mu_d),
 *               nsim[t][c] = (2 mu_r mu_d + C1) / (mu_r^2 + mu_d^2 + C1) (cov + C3) / (sqrt(v_r v_d) + C3),
 *               C1 = (0.01 range_db)^2, C3 = (0.03 range_db)^2 / 2
 * T < 3 and a digitally silent target (top = 0) give NaN in every value, and so does, for its pair, a level factor that is not finite
 * (sum P_estimate denormal); no infinity leaves the library.
 * tgt / est: float32, or float64 where tgt_f64 / est_f64, read where they lie; tgt_off / est_off: DEVICE int64 sample offsets.
 * tgt_len, tgt_index, split_band and coef are HOST arrays: validated before anything is enqueued (lengths in [0, 2^29) and at most
 * SSR_AUDITORY_MAX_BLOCKS hop-blocks - more is SSR_ERR_UNSUPPORTED -, indices in [0, n_tgt), hop >= 1, 3 <= n_bands <= 64, every
 * coef finite with |a| < 1, 0 < range_db <= 150, split_band[e] = -1 or in [1, n_bands - 1]) and copied into the workspace on `stream`
 * (from page-locked memory the copy is asynchronous: keep the values until the stream has reached it).  split_band[e]: the first
 * interior band at or above the pair's split (n_bands - 1: the split lies above every interior band), or -1 for none.
 * pair_out: DEVICE double [n_est][3] = nsim (the mean over the valid cells), nsim_hf and nsim_lf (the means over the valid cells of
 * the interior bands c >= split_band[e] and c < split_band[e]; NaN where split_band[e] = -1 or no such band exists).  band_out: DEVICE
 * double [n_est][n_bands], the mean over t of every interior band (NaN in the two edge bands), or NULL.  image_out: DEVICE double, the
 * images D of the signals in signal order, signal s as [T_s][n_bands] behind those of the signals before it (an estimate's: level
 * matched, on its target's floor; NaN where the target is silent), or NULL; passing band_out or image_out changes no bit of the other
 * outputs.  n_est = 0 with n_tgt > 0 yields the targets' images (est, est_off, tgt_index, split_band and pair_out may be NULL);
 * n_tgt = n_est = 0: nothing is enqueued.  Deterministic: fixed-order sums, no atomics; a signal and a pair give the same bits alone,
 * in any batch and at any position.  workspace: ssr_auditory_workspace_bytes (0 for invalid arguments).  SSR_ERR_UNSUPPORTED with
 * more than 2^24 signals or a launch of 2^32 threads or more (checked before anything is enqueued).  The table built from (coef, hop)
 * is kept for the life of the process, one entry of about 120 n_bands bytes per distinct design and hop (the asynchronous copy reads it after
 * the call has returned): a caller that sweeps thousands of designs pays that memory. */
size_t ssr_auditory_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int hop, int n_bands);
int ssr_auditory(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est, int est_f64,
                 const int64_t* est_off, const int32_t* tgt_index, int n_est, int hop, int n_bands, const double* coef /* [n_bands][3] */,
                 double range_db, int match_level, const int32_t* split_band /* [n_est] */, double* pair_out /* [n_est][3] */,
                 double* band_out /* [n_est][n_bands] or NULL */, double* image_out /* or NULL */, void* workspace,
                 size_t workspace_bytes, void* stream);

#endif /* SSR_HIP_AUDITORY_H_ */
