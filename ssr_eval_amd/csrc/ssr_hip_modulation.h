/* Part of the C ABI of libssrhip.so: the modulation family - the speech-to-reverberation modulation energy ratio (SRMR) and a
 * modulation-spectrum distance.  Included by include/ssr_hip.h (which supplies the error codes and the integer types) after
 * ssr_hip_auditory.h, whose band limits it shares; valid C99. */
#ifndef SSR_HIP_MODULATION_H_
#define SSR_HIP_MODULATION_H_

#define SSR_MODULATION_BANDS 8          /* modulation bands per gammatone band */
#define SSR_MODULATION_MAX_BLOCKS 65536 /* envelope samples (blocks of hop_e samples) per signal: about 41 s at 1600 Hz */
#define SSR_MODULATION_MAX_STEP 1024    /* S, the frame step in envelope samples */
#define SSR_MODULATION_SIGNAL_COLS 4    /* columns of signal_out */
#define SSR_MODULATION_PAIR_COLS 4      /* columns of pair_out */

/* Does a signal move like speech?  How its sub-band envelopes are distributed over modulation frequency: SRMR (Falk, Zheng & Chan
 * 2010) of every signal on its own, and the distance of the modulation spectra of every estimate and its target.  The
 * signals are the n_tgt targets followed by the n_est estimates; estimate e belongs to target tgt_index[e] and is as long as it.
 * All arithmetic is float64.
 *   filterbank  ssr_auditory's: band c from coef[c] = (Re a, Im a, g), |a| < 1; z_c is complex, |z_c| the band's Hilbert envelope
 *   envelope    NB = len / hop_e blocks for len >= 2 hop_e, else 0;  env[m][c] = sqrt(B[m][c] / hop_e), B[m][c] the sum of |z_c[n]|^2
 *               over the samples m hop_e .. (m + 1) hop_e - 1 in sample order
 *   bank        8 biquads mod[k] = (b0, b1, b2, a1, a2) on env[.][c] from the zero state (transposed direct form II):
 *               y = b0 x + z0, z0 = b1 x - a1 y + z1, z1 = b2 x - a2 y
 *   frames      W = 4 S, w[i] = 0.54 - 0.46 cos(2 pi i / (W - 1)): F = 1 + (NB - W) / S frames for NB >= W, else 0;
 *               E_f[c][k] = sum_i (w[i] y_ck[f S + i])^2 in sample order, Ebar[c][k] = (sum_f E_f[c][k]) / F in frame order
 *   srmr        e_c = sum_k Ebar[c][k]; c90 = the lowest band whose running sum of e_c, low to high, exceeds 0.9 of the total;
 *               K* = kstar[c90]; srmr = sum_c sum_{k < 4} Ebar[c][k] / sum_c sum_{4 <= k < K*} Ebar[c][k]
 *   pair        f = sum Ebar_target / sum Ebar_estimate; top = max Ebar_target, floor = 10 log10 top - range_db;
 *               D = max(10 log10 Ebar, floor) of the target and of the estimate times f; mod_dist = sqrt(mean (D_e - D_t)^2) in dB
 * F = 0, a digitally silent signal and a zero denominator give NaN for that signal's srmr; a target without frames or energy and a
 * level factor that is not finite (a silent estimate included) give NaN in every value of the pair; no infinity leaves the library.
 * tgt / est: float32, or float64 where tgt_f64 / est_f64, read where they lie; tgt_off / est_off: DEVICE int64 sample offsets.
 * tgt_len, tgt_index, coef, mod, kstar and split_band are HOST arrays: validated before anything is enqueued (lengths in [0, 2^29)
 * and at most SSR_MODULATION_MAX_BLOCKS blocks - more is SSR_ERR_UNSUPPORTED -, indices in [0, n_tgt), hop_e >= 1, 3 <= n_bands <= 64,
 * every coef finite with |a| < 1, every mod finite and stable, 1 <= S <= SSR_MODULATION_MAX_STEP, 5 <= kstar[c] <= 8,
 * 0 < range_db <= 150, -1 <= split_band[e] <= n_bands) and copied into the workspace on `stream` (from page-locked memory the copy
 * is asynchronous: keep the values until the stream has reached it).  split_band[e]: the first band of the pair's upper part (0:
 * every band, n_bands: none), or -1 for no split.
 * signal_out: DEVICE double [n_tgt + n_est][4] = srmr, K*, c90, sum Ebar (K* and c90 as whole numbers; NaN with srmr where the signal
 * has no frame or no energy - sum Ebar is then NaN or 0).  pair_out: DEVICE double [n_est][4] = srmr_diff (the estimate's srmr minus
 * the target's), mod_dist over all n_bands x 8 cells, mod_dist_hf over the bands c >= split_band[e] and mod_dist_lf over those below
 * (NaN where split_band[e] = -1 or the side is empty).  spectrum_out: DEVICE double [n_tgt + n_est][n_bands][8], Ebar of every signal,
 * or NULL; passing it changes no bit of the other outputs.  n_est = 0 is the non-intrusive call (est, est_off, tgt_index, split_band
 * and pair_out may be NULL); n_tgt = n_est = 0: nothing is enqueued.  Deterministic: fixed-order sums, no atomics; a signal and a pair
 * give the same bits alone, in any batch and at any position.  workspace: ssr_modulation_workspace_bytes (0 for invalid arguments),
 * about 16 n_bands bytes per envelope sample.  SSR_ERR_UNSUPPORTED with more than 2^24 signals or a launch of 2^32 threads or more
 * (checked before anything is enqueued).  The tables built from (coef, hop_e) and (mod, S) are kept for the life of the process, about
 * 120 n_bands and 32 S bytes per distinct design (the asynchronous copies read them after the call has returned). */
size_t ssr_modulation_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int hop_e, int n_bands);
int ssr_modulation(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est, int est_f64,
                   const int64_t* est_off, const int32_t* tgt_index, int n_est, int hop_e, int n_bands, const double* coef /* [n_bands][3] */,
                   const double* mod /* [8][5] */, int S, const int32_t* kstar /* [n_bands] */, double range_db,
                   const int32_t* split_band /* [n_est] */, double* signal_out /* [n_tgt + n_est][4] */, double* pair_out /* [n_est][4] */,
                   double* spectrum_out /* [n_tgt + n_est][n_bands][8] or NULL */, void* workspace, size_t workspace_bytes, void* stream);

#endif /* SSR_HIP_MODULATION_H_ */
