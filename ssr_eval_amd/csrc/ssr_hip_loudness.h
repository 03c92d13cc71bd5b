/* Part of the C ABI of libssrhip.so: the loudness family, the first that describes ONE signal.  Included by include/ssr_hip.h
 * (which supplies the error codes and the integer types); valid C99. */
#ifndef SSR_HIP_LOUDNESS_H_
#define SSR_HIP_LOUDNESS_H_

/* EBU R128 meter quantities of mono signals (not in the reference): ITU-R BS.1770-4 integrated loudness with gating,
 * the largest momentary and short-term loudness (EBU Tech 3341), the loudness range (EBU Tech 3342), the sample peak and the 4x
 * oversampled peak.  Signal i has len[i] samples at the integer `rate` (8000 .. 192000 Hz) and channel weight 1.  With y the
 * K-weighted signal (two biquads designed at `rate`, from the zero state), h = (rate + 5) / 10 samples per sub-block and
 * E[s] = sum y^2 over sub-block s < S = len / h (samples past S h do not count):
 *   a momentary block j <= S - 4 has z = (E[j] + .. + E[j + 3]) / (4 h), a short-term block j <= S - 30 the same over 30 sub-blocks;
 *   L(z) = -0.691 + 10 log10 z
 *   lufs = L(mean z of the momentary blocks with L > -70 and L > G), G = L(mean z of those with L > -70) - 10
 *   lufs_m_max, lufs_s_max = the largest L of the momentary / short-term blocks with L > -70
 *   lra = v[r(95)] - v[r(10)]: v the L of the short-term blocks with L > -70 and L > L(their mean z) - 20, ascending, m of them,
 *   r(p) = ((m - 1) p + 50) / 100
 *   peak_db = 20 log10 max |x|, true_peak_db = 20 log10 max |u|, u = scipy.signal.resample_poly(x, 4, 1) (81-tap Kaiser filter)
 * An empty block set (S < 4, S < 30, nothing above -70) gives NaN, and so do both peaks of an all-zero or empty signal: no
 * infinity leaves the library.  All arithmetic is float64.
 * sig: float32, or float64 where sig_f64, read where they lie; off: DEVICE int64 sample offsets.  len and blocks_off are HOST
 * arrays: validated before anything is enqueued (lengths in [0, 2^29), at most 6144 sub-blocks - 10 minutes - per signal, else
 * SSR_ERR_UNSUPPORTED) and copied into the workspace on `stream` (from page-locked memory the copy is asynchronous: keep the
 * values until the stream has reached it).  n_sig = 0: nothing is enqueued.
 * out: DEVICE double [n_sig][6] = lufs, lra, lufs_m_max, lufs_s_max, peak_db, true_peak_db.  blocks_out: NULL, or a DEVICE ragged
 * array that receives E[s] of signal i at blocks_out + blocks_off[i] (HOST int64 [n_sig], >= 0); passing it changes no bit of
 * out.  Deterministic: fixed-order sums, no atomics; a signal gives the same bits alone, in any batch and at any position.
 * workspace: ssr_loudness_workspace_bytes (0 for invalid arguments). */
size_t ssr_loudness_workspace_bytes(const int32_t* len, int n_sig, int rate);
int ssr_loudness(const void* sig, int sig_f64, const int64_t* off, const int32_t* len, int n_sig, int rate,
                 double* out /* [n_sig][6] */, const int64_t* blocks_off /* [n_sig] or NULL */, double* blocks_out /* or NULL */,
                 void* workspace, size_t workspace_bytes, void* stream);

#endif /* SSR_HIP_LOUDNESS_H_ */
