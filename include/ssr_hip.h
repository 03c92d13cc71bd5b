/* libssrhip - C ABI of the MI355X (gfx950) implementation of the ssr_eval DSP / metric hot path.
 *
 * This header is the drop-in boundary.  Every entry point names the reference interface
 * (haoheliu/ssr_eval v0.0.6, file:line) whose arithmetic it replaces; the Python classes in
 * ssr_eval_amd/ (AudioMetrics, FDomainHelper, lowpass, SSR_Eval_Helper) bind these symbols through
 * ctypes and nothing else (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - plain C, no exceptions, no ownership transfer; every function returns SSR_OK (0) or a negative
 *    error code, with a thread-local message available from ssr_last_error();
 *  - every `const float*`, `float*`, `double*`, offset and length ARRAY argument is a DEVICE pointer
 *    (HBM) valid on the current HIP device; scalar arguments are host values;
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); all work is enqueued on it and
 *    nothing synchronises with the host;
 *  - batches are ragged: item i occupies elements [off[i], off[i] + len[i]) of its buffer; spectrogram
 *    rows of item i start at row frame_off[i] of a [total_rows, n_bins] float32 matrix;
 *  - a plan is immutable after creation and may be shared between host threads.
 */
#ifndef SSR_HIP_H_
#define SSR_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSR_OK 0
#define SSR_ERR_INVALID_ARG (-1)
#define SSR_ERR_UNSUPPORTED (-2)
#define SSR_ERR_HIP (-3)
#define SSR_ERR_WORKSPACE (-4)

/* transform precision: SSR_F64 reproduces librosa's float64 pocketfft -> complex64 rounding (parity
 * mode, default); SSR_F32 is a float32 transform (faster, not parity-safe on band-limited input). */
#define SSR_F32 0
#define SSR_F64 1

/* metric_mask bits; outputs are always laid out [n_items][4] = lsd, log_sispec, sispec, ssim
 * (key order of ssr_eval/metrics.py:98-103); unrequested entries are NaN. */
#define SSR_METRIC_LSD 1u
#define SSR_METRIC_LOG_SISPEC 2u
#define SSR_METRIC_SISPEC 4u
#define SSR_METRIC_SSIM 8u
#define SSR_METRIC_ALL 15u

/* ssr_stft output kinds */
#define SSR_STFT_MAG 1     /* out_a = |X|                       (ssr_eval/metrics.py:27) */
#define SSR_STFT_COMPLEX 2 /* out_a = Re X, out_b = Im X        (ssr_eval/dsp.py:64,73,77) */

typedef struct ssr_plan ssr_plan;

const char* ssr_last_error(void);
int ssr_version(void);

/* STFT plan: centred, reflect-padded, periodic-Hann, win_length = n_fft.
 * Replaces the parameter choice of AudioMetrics.__init__ (ssr_eval/metrics.py:16-19: rate -> n_fft, hop),
 * FDomainHelper.__init__ (ssr_eval/dsp.py:7-59: 2048 / 441) and librosa.stft defaults (eval.py:29: 2048 / 512).
 * Any 2 <= n_fft <= 4096 is accepted: powers of two in [256, 4096] run a direct FFT; n_fft = R q with R in {1, 2, 3} and
 * q <= 768 - every AudioMetrics(rate) size: 2229 = 3 * 743, 1486 = 2 * 743, 1114 = 2 * 557, 743 - runs one radix-R step over R
 * chirp-z (Bluestein) transforms of length 1536 on float32 pairs (q up to 1024: length 2048); everything else, float64 signals
 * and single-signal mode run Bluestein over a power of two >= 2 n_fft - 1 (radix 3 over three 2048-point ones for 2229). */
int ssr_plan_create(int n_fft, int hop, int precision, ssr_plan** plan);
/* FDomainHelper(window_size, hop_size, center, pad_mode, window) with anything but the defaults (ssr_eval/dsp.py:7-59 passes the
 * five straight to torchlibrosa's STFT / ISTFT, win_length = n_fft).  window: HOST pointer to n_fft float64 values - what
 * librosa.filters.get_window(name, n_fft, fftbins=True) returns for the caller's window name - or NULL for the periodic Hann;
 * center: 0 = no padding, frames start at sample 0, T = 1 + (n - n_fft) / hop, ISTFT trims nothing at the front;
 * pad_mode: torch's F.pad mode when center != 0 (SSR_PAD_REFLECT, SSR_PAD_CONSTANT = zeros).
 * Such a plan has the SSR_LOWPASS_CONV engine only (n_fft = 32 m <= 4096; torchlibrosa's own construction - conv weights from any
 * window - is the only one defined for it) and serves ssr_stft(SSR_STFT_COMPLEX), ssr_istft, ssr_fft_lowpass, ssr_num_frames,
 * ssr_ola_workspace_bytes and ssr_plan_query; every other entry point returns SSR_ERR_UNSUPPORTED for it.
 * Per item: center + reflect needs len > n_fft / 2, center + constant len >= 1, center = 0 len >= n_fft (an item that cannot be
 * framed gets 0 rows and a zeroed output; the LONGEST item failing is SSR_ERR_INVALID_ARG).  With center = 0 the overlap-added signal
 * is (T - 1) hop + n_fft samples long; torch's slice ends there, the C ABI's fixed-size output is zero-filled beyond it.
 * Parity: bit-exact against oracle/tl_chain.c; the non-default branches of that oracle are restated from the published torchlibrosa
 * module without a reference-generated vector (the reference only ever constructs FDomainHelper(), lowpass.py:18): "parity unpinned". */
#define SSR_PAD_REFLECT 0
#define SSR_PAD_CONSTANT 1
int ssr_plan_create_ex(int n_fft, int hop, const double* window, int center, int pad_mode, ssr_plan** plan);
int ssr_plan_destroy(ssr_plan* plan);
int ssr_plan_query(const ssr_plan* plan, int* n_fft, int* hop, int* n_bins, int* fft_len, int* bluestein,
                   int* precision);
/* Engine of ssr_fft_lowpass / ssr_istft for this plan (set it before the plan is shared between threads):
 *   SSR_LOWPASS_SEGMENTS (default): the frame kernel writes frames / paired segments to the workspace, a second kernel overlap-adds;
 *   SSR_LOWPASS_FUSED: transforms AND overlap-add in one kernel, no workspace traffic (HBM bytes = signal in + signal out).
 *     Float64 2048-point plans with 228 <= hop <= 914 only (SSR_ERR_UNSUPPORTED otherwise).  Measured on MI355X: 3 % faster when
 *     the call runs alone, 8 % slower inside a pipeline of other FP64-heavy kernels (it needs more cycles at a lower power
 *     density) - hence not the default.  Both give the reference's result to float32 resolution; the
 *     fused engine rounds to float32 once (sums in float64 from the unrounded frames).
 *   SSR_LOWPASS_CONV: the REFERENCE'S ARITHMETIC CLASS.  torchlibrosa (ssr_eval/dsp.py:1,21-39) evaluates STFT / ISTFT as dense float32
 *     DFT convolutions (nn.Conv1d with DFT x Hann weights computed in float64, stored float32); a hard-low-passed signal's stop band is
 *     that transform's round-off floor, and LSD / log-SISpec of the degraded input take its logarithm: against the float64 FFT engines
 *     above they differ by 2-7 % (LSD).  This engine runs the same dense products on the fp32 matrix cores (v_mfma_f32_32x32x2_f32 =
 *     a float32 fused-multiply-add chain) IN THE ACCUMULATION ORDER OF TORCH-CPU'S F.conv1d (oneDNN, AVX-512, >= 2 threads,
 *     established bit for bit: tests/test_oracle.py::test_tl_chain_is_torch_conv1d_bit_for_bit): forward one chain of n_fft terms
 *     per output (what torch runs for signals of >= 55 frames), inverse one chain per block of 256 channels of the mirrored
 *     spectrum, the blocks added in float32 in order - oracle/tl_chain.c restates it, the kernels reproduce it bit for bit -
 *     followed by F.fold's float32 overlap-add and window-sum division.  With the reference's own weight tables
 *     (ssr_plan_set_tl_weights) a low-passed waveform of >= 55 frames IS the reference's, sample for sample.  ssr_fft_lowpass(_multi),
 *     ssr_istft and ssr_stft(SSR_STFT_COMPLEX) of such a plan all run it.  n_fft = 32 m.  Cost: 2 n_fft (2 cut) + 2 n_fft (4 cut)
 *     flops per frame instead of two FFTs (10-30x the time of the default engine), and ssr_ola_workspace_bytes grows to
 *     ~(2 n_fft + 2 n_bins + hop) floats per frame.  The Python mirror makes it the default of lowpass(_type="stft_hard") and
 *     FDomainHelper. */
#define SSR_LOWPASS_SEGMENTS 0
#define SSR_LOWPASS_FUSED 1
#define SSR_LOWPASS_CONV 2
int ssr_plan_set_lowpass_engine(ssr_plan* plan, int engine);
/* The float32 weight tables of SSR_LOWPASS_CONV as the library builds them (torchlibrosa's DFTBase.dft_matrix / idft_matrix x
 * periodic Hann: STFT.__init__, ISTFT.init_real_imag_conv), TRANSPOSED: fwd_*_t [n_fft][n_fft/2+1] (row = sample, column = bin),
 * inv_*_t [n_fft][n_fft] (row = channel of the mirrored spectrum, column = output sample), w2 = hann^2 [n_fft].
 * HOST pointers (the one exception to the device-pointer convention; any may be NULL): a host-only introspection call, needs no GPU;
 * the parity tests feed these tables to oracle/tl_chain.c. */
int ssr_tl_weights(int n_fft, float* fwd_re_t, float* fwd_im_t, float* inv_re_t, float* inv_im_t, float* w2);
/* Replace the SSR_LOWPASS_CONV tables of a plan by the caller's (HOST pointers, torchlibrosa's own module layout):
 *   fwd_re / fwd_im [n_bins][n_fft] = STFT.conv_real / conv_imag .weight[:, 0, :]   (torchlibrosa stft.py STFT.__init__)
 *   inv_re / inv_im [n_fft][n_fft]  = ISTFT.conv_real / conv_imag .weight[:, :, 0]  (row = output sample, column = channel)
 *   w2 [n_fft] = float32(window ** 2)                                              (ISTFT._get_ifft_window_sum_onnx / fold input)
 * The Python mirror evaluates DFTBase.dft_matrix / idft_matrix with the module's own numpy expressions (np.power(omega, x * y) in
 * complex128) and hands the float32 results over, so that the engine multiplies by the REFERENCE'S weights to the last bit (the
 * library's own tables - exact phase reduction in long double - differ from numpy's in 1 ulp of ~0.5 % of the entries).
 * Call it before the plan is shared between threads / before launches that should see the tables are enqueued.  The library's own
 * tables are only built by the first conv launch that finds none, so a caller that sets its tables first never pays for them; a set
 * that IS superseded (this call twice, or after such a launch) is released after a hipDeviceSynchronize(). */
int ssr_plan_set_tl_weights(ssr_plan* plan, const float* fwd_re, const float* fwd_im, const float* inv_re, const float* inv_im,
                            const float* w2);
/* The same for a caller-supplied window (HOST float64 [n_fft], NULL = periodic Hann): the tables of an ssr_plan_create_ex plan. */
int ssr_tl_weights_ex(int n_fft, const double* window, float* fwd_re_t, float* fwd_im_t, float* inv_re_t, float* inv_im_t, float* w2);
/* T = 1 + (n + 2 pad - n_fft) / hop, pad = n_fft / 2 (0 for a center = 0 plan; then T = 0 when n < n_fft)
 * (librosa / torchlibrosa frame count; bit-exact integer) */
int64_t ssr_num_frames(const ssr_plan* plan, int64_t n_samples);

/* K1+K2.  Batched STFT of ragged float32 waveforms -> [total_rows, n_bins] float32.
 * Replaces AudioMetrics.wav_to_spectrogram (ssr_eval/metrics.py:26-30 -> librosa.stft + abs + transpose)
 * and FDomainHelper.complex_spectrogram / spectrogram / spectrogram_phase (ssr_eval/dsp.py:61-81 ->
 * torchlibrosa STFT).  Reflect padding follows numpy.pad (what librosa calls): items shorter than n_fft/2 are reflected
 * repeatedly; every item needs len >= 1.  (torch's reflect padding, used by torchlibrosa, refuses such items - the Python
 * FDomainHelper mirror raises for them before calling in.) */
int ssr_stft(const ssr_plan* plan, const float* wav, const int64_t* wav_off, const int32_t* wav_len,
             const int64_t* frame_off, int n_items, int max_len, int out_kind, float* out_a, float* out_b,
             void* stream);

/* K2'.  mag = sqrt(max(re^2 + im^2, eps)), cos = re / mag, sin = im / mag   (ssr_eval/dsp.py:76-81). */
int ssr_magphase(const float* re, const float* im, int64_t n, float eps, float* mag, float* cosv, float* sinv,
                 void* stream);

/* K1-K5 fused driver: the four metrics of AudioMetrics.evaluation (ssr_eval/metrics.py:51-107) for a
 * ragged batch of (est, target) waveform pairs already truncated to a common length len[i]
 * (metrics.py:89-90).  out: double [n_items][4].  total_rows = sum_i T_i, frame_off = exclusive prefix
 * sum of T_i.  workspace: at least ssr_pair_metrics_workspace_bytes(...) bytes of device memory. */
size_t ssr_pair_metrics_workspace_bytes(const ssr_plan* plan, int n_items, int max_len, int64_t total_rows);
/* The same for a given metric_mask: without SSIM the two [total_rows, n_bins] magnitude images are never materialised and the
 * workspace shrinks from 8 bytes per bin of the batch to the partial records (a few hundred bytes per item).  A workspace
 * sized for a mask serves every call whose mask is a subset of it. */
size_t ssr_pair_metrics_workspace_bytes_for(const ssr_plan* plan, int n_items, int max_len, int64_t total_rows,
                                            unsigned metric_mask);
int ssr_pair_metrics(const ssr_plan* plan, const float* est, const int64_t* est_off, const float* tgt,
                     const int64_t* tgt_off, const int32_t* len, const int64_t* frame_off, int n_items, int max_len,
                     int64_t total_rows, unsigned metric_mask, double* out, void* workspace, size_t workspace_bytes,
                     void* stream);

/* The same for an estimate held as a FLOAT64 signal against a float32 target.  This is what
 * AudioMetrics.evaluation receives from SSR_Eval_Helper.evaluate_single (ssr_eval/eval.py:128-156) whenever the
 * degradation was an IIR low-pass: scipy.signal.sosfiltfilt returns float64 (ssr_eval/lowpass.py:54-131), the
 * testee output and librosa.resample keep it, librosa.stft then yields complex128, and torch promotes every
 * est-side operation of metrics.py:109-121 to float64.  Same workspace size, same output layout. */
int ssr_pair_metrics_est64(const ssr_plan* plan, const double* est, const int64_t* est_off, const float* tgt,
                           const int64_t* tgt_off, const int32_t* len, const int64_t* frame_off, int n_items,
                           int max_len, int64_t total_rows, unsigned metric_mask, double* out, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Both signals float64 (e.g. arrays read with soundfile's default dtype handed to AudioMetrics.evaluation): two
 * complex128 spectra, every tensor of metrics.py:109-121 float64. */
int ssr_pair_metrics_f64(const ssr_plan* plan, const double* est, const int64_t* est_off, const double* tgt,
                         const int64_t* tgt_off, const int32_t* len, const int64_t* frame_off, int n_items, int max_len,
                         int64_t total_rows, unsigned metric_mask, double* out, void* workspace, size_t workspace_bytes,
                         void* stream);

/* K1-K5 for ONE target and K estimates per item: SSR_Eval_Helper.evaluate_single scores every degradation key of a file against the
 * same target (ssr_eval/eval.py:136-154).  est_off is key-major, [n_keys][n_items]: estimate k of item i starts at element
 * est_off[k * n_items + i] of est; all K estimates and the target of item i share the truncated length len[i] (metrics.py:89-90);
 * out: double [n_items][n_keys][4].  The target is transformed once (with estimate 0: that key is bit-identical to ssr_pair_metrics)
 * and its magnitude image stored once; estimates 1 .. K-1 are transformed two per complex transform and reduced against the stored
 * image - the same per-bin arithmetic on the same float32 magnitudes, so the metrics agree with K calls of ssr_pair_metrics to
 * <= 1e-6 relative (not bit for bit: an estimate separated from another estimate instead of the target keeps ~1e-16 of its
 * partner's spectrum, a last-bit flip of a float32 magnitude now and then; float64 partial sums are added in another order).
 * K + 1 real transforms and K + 1 magnitude images per item instead of 2 K and 2 K.  Plans whose pair transform runs a block engine
 * take K plain passes (bit-identical to ssr_pair_metrics). */
size_t ssr_pair_metrics_multi_workspace_bytes(const ssr_plan* plan, int n_items, int n_keys, int max_len, int64_t total_rows,
                                              unsigned metric_mask);
int ssr_pair_metrics_multi(const ssr_plan* plan, const float* est, const int64_t* est_off, const float* tgt, const int64_t* tgt_off,
                           const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len, int64_t total_rows,
                           unsigned metric_mask, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* The same for K FLOAT64 estimates per float32 target: what SSR_Eval_Helper.evaluate_single holds when `setting_lowpass_filtering` is on -
 * every IIR key of a file is a float64 signal (scipy.signal.sosfiltfilt, ssr_eval/lowpass.py:54-131) scored against the file's one
 * float32 target (ssr_eval/eval.py:136-154, 243-258).  est: double, key-major offsets as above.  Key 0 runs as ssr_pair_metrics_est64
 * (bit-identical to it) and stores the target's magnitude image; keys 1 .. K-1 are transformed two per complex float64 transform into
 * float32 magnitude rows - numpy.abs of the unrounded complex128 spectrum, rounded once - and reduced against the stored image (an odd
 * last key runs with the target again).  Against K calls of ssr_pair_metrics_est64: the estimate's magnitude enters the LSD / SISpec
 * terms rounded to float32 (6e-8 relative: <= 5e-8 absolute on an LSD term, the size of that entry point's own float32 logarithms)
 * and the terms are float32 sequences summed in float64 - metrics equal to <= 1e-6 relative, 1e-5 being the bar.  Plans without a
 * two-estimate wave kernel (today: every n_fft but 3 q <= 2304, i.e. every rate but AudioMetrics(48000)) take K plain passes,
 * bit-identical to ssr_pair_metrics_est64. */
size_t ssr_pair_metrics_multi_est64_workspace_bytes(const ssr_plan* plan, int n_items, int n_keys, int max_len, int64_t total_rows,
                                                    unsigned metric_mask);
int ssr_pair_metrics_multi_est64(const ssr_plan* plan, const double* est, const int64_t* est_off, const float* tgt, const int64_t* tgt_off,
                                 const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len, int64_t total_rows,
                                 unsigned metric_mask, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* Same, restricted to a subset of its three launches (bit 0: STFT + fused LSD/SISpec epilogue, bit 1:
 * SSIM, bit 2: finalisation) so that bench.py can time the dominant kernel on its own stream with
 * HIP events.  stages = 7 is ssr_pair_metrics. */
int ssr_pair_metrics_stages(const ssr_plan* plan, const float* est, const int64_t* est_off, const float* tgt,
                            const int64_t* tgt_off, const int32_t* len, const int64_t* frame_off, int n_items,
                            int max_len, int64_t total_rows, unsigned metric_mask, double* out, void* workspace,
                            size_t workspace_bytes, void* stream, int stages);

/* K3-K5 on precomputed [T_i, n_bins] magnitude spectrograms: AudioMetrics.lsd / .sispec (incl. the
 * to_log variant) / .ssim (ssr_eval/metrics.py:109-132, ssr_eval/utils.py:43-92).  est first, target second.
 * SSIM needs T_i >= 7 and n_bins >= 7. */
size_t ssr_spectrogram_metrics_workspace_bytes(int n_items, int max_rows, int n_bins);
int ssr_spectrogram_metrics(const float* est_sp, const float* tgt_sp, const int64_t* frame_off, const int32_t* n_rows,
                            int n_items, int max_rows, int n_bins, unsigned metric_mask, double* out, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Band-split LSD: AudioMetrics.lsd (ssr_eval/metrics.py:109-112) applied to the columns [a, b) of each band - e.g. LSD-LF / LSD-HF
 * on either side of a degradation's cutoff bin,
 *   lsd_band(E, T, a, b) = mean_t sqrt( mean_{a <= k < b} log10( T^2 / (E + 1e-12)^2 + 1e-12 )^2 ).
 * The per-bin term is the float32 sequence of the fused LSD epilogue; per-band row sums and frame totals are float64.
 * edges: HOST int32 [n_images][n_bands + 1] (the one other exception to the device-pointer convention, like ssr_tl_weights):
 * strictly ascending, 0 <= edges[0], edges[n_bands] <= n_bins; band j of image v is [edges[v][j], edges[v][j + 1]).  They are
 * validated before anything is enqueued and copied into the workspace on `stream` - from page-locked memory that copy is
 * asynchronous, and the caller keeps the values unchanged until the stream has reached it.  1 <= n_bands <= SSR_MAX_BANDS. */
#define SSR_MAX_BANDS 8
/* Image level, backs AudioMetrics.lsd_bands on [B, C, T, F] tensors: image v is the est rows [est_frame_off[v], + n_rows[v]) of
 * est_sp and the target rows [tgt_frame_off[v], + n_rows[v]) of tgt_sp, both [*, n_bins] float32 matrices (several images may
 * share one target).  max_rows >= every n_rows[v].  out: double [n_images][n_bands].
 * workspace: ssr_spectrogram_lsd_bands_workspace_bytes(n_images, max_rows, n_bands). */
size_t ssr_spectrogram_lsd_bands_workspace_bytes(int n_images, int max_rows, int n_bands);
int ssr_spectrogram_lsd_bands(const float* est_sp, const int64_t* est_frame_off, const float* tgt_sp, const int64_t* tgt_frame_off,
                              const int32_t* n_rows, int n_images, int max_rows, int n_bins, const int32_t* edges, int n_bands,
                              double* out, void* workspace, size_t workspace_bytes, void* stream);
/* Waveform level: K float32 estimates per float32 target with the key-major [n_keys][n_items] estimate offsets and the length /
 * frame descriptors of ssr_pair_metrics_multi; edges [n_keys][n_items][n_bands + 1] (image v = k * n_items + i).  The target is
 * transformed once per item (with estimate 0, as ssr_pair_metrics does) into a magnitude image; the other estimates go into
 * magnitude images two per complex transform where the plan's pair transform is a wave kernel (else one per transform with the
 * target, whose image is not rewritten) - the magnitudes of ssr_pair_metrics_multi - and the band reduction runs on the images.
 * Bands [0, n_bins) give ssr_pair_metrics' LSD to <= 1e-6 relative.  out: double [n_items][n_keys][n_bands].
 * The workspace holds K + 1 magnitude images of the batch (8 (K + 1) * total_rows * n_bins bytes, rows padded to 16 bytes): callers
 * with many keys run them in chunks.  ssr_pair_lsd_bands_workspace_bytes serves both entry points, and both ask for all of it
 * (SSR_ERR_WORKSPACE for a byte less, whichever layout the call at hand uses). */
size_t ssr_pair_lsd_bands_workspace_bytes(const ssr_plan* plan, int n_items, int n_keys, int max_len, int64_t total_rows, int n_bands);
int ssr_pair_lsd_bands(const ssr_plan* plan, const float* est, const int64_t* est_off, const float* tgt, const int64_t* tgt_off,
                       const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len, int64_t total_rows,
                       const int32_t* edges, int n_bands, double* out, void* workspace, size_t workspace_bytes, void* stream);
/* The same for FLOAT64 estimates (IIR keys, as ssr_pair_metrics_multi_est64): transformed at float64, |.| rounded once to float32. */
int ssr_pair_lsd_bands_est64(const ssr_plan* plan, const double* est, const int64_t* est_off, const float* tgt, const int64_t* tgt_off,
                             const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len, int64_t total_rows,
                             const int32_t* edges, int n_bands, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* Intelligibility (not in the reference): STOI (Taal, Hendriks, Heusdens, Jensen, IEEE TASLP 19(7), 2011) and ESTOI (Jensen &
 * Taal, IEEE/ACM TASLP 24(11), 2016) as the pystoi package (0.3.x) computes them - a restatement of that algorithm, not a copy
 * pinned against it: silent frames of the target (40 dB below its loudest 256-sample frame) removed from both
 * signals, 512-point STFT, 15 one-third-octave bands from 150 Hz, 30-frame segments; ESTOI without pystoi's EPS-scale random
 * noise (deterministic), each normalisation divided by (norm + EPS).  Fewer than 30 frames left: 1e-5, as pystoi.
 * Signals are 10 kHz float64 (resample first: ssr_resample_poly_f64 with the Octave-compatible taps of pystoi.utils.resample_oct).
 * Pair e scores estimate e (est + est_off[e], est_len[e] samples) against target tgt_index[e]; K estimates of one target share
 * its voice-activity mask and band image, computed once.  tgt_len, est_len and tgt_index are HOST int32 arrays (like the band
 * edges of ssr_*_lsd_bands): validated before anything is enqueued - lengths in [0, 2^29), indices in [0, n_tgt), every estimate
 * as long as its target - and copied into the workspace on `stream`; from page-locked memory the copy is asynchronous and the
 * caller keeps the values unchanged until the stream has reached it.  which: SSR_STOI, SSR_ESTOI or SSR_STOI_BOTH.
 * out: double [n_est][1] ([n_est][2] = STOI, ESTOI for SSR_STOI_BOTH).  Deterministic: fixed-order sums, no atomics.
 * workspace: ssr_stoi_workspace_bytes (0 for invalid lengths or indices). */
#define SSR_STOI 1
#define SSR_ESTOI 2
#define SSR_STOI_BOTH 3
size_t ssr_stoi_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est);
int ssr_stoi(const double* tgt, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const double* est, const int64_t* est_off,
             const int32_t* est_len, const int32_t* tgt_index, int n_est, int which, double* out, void* workspace,
             size_t workspace_bytes, void* stream);
/* The band matrix of pystoi.utils.thirdoct(10000, 512, 15, 150) as bin ranges: band k sums |X|^2 over bins [lo[k], hi[k]).
 * lo / hi: HOST int32 [15]. */
int ssr_stoi_band_edges(int32_t* lo, int32_t* hi);

/* Waveform metrics (not in the reference), float64 throughout, EPS = DBL_EPSILON, x = target, y = estimate:
 *   SSR_WAVE_SNR      10 log10((Σx² + EPS) / (Σ(x - y)² + EPS))
 *   SSR_WAVE_SI_SDR   zero-mean SI-SDR (Le Roux et al. 2019): x0 = x - mean(x), y0 = y - mean(y), alpha = (Σx0 y0 + EPS) / (Σx0² + EPS),
 *                     s = alpha x0, 10 log10((Σs² + EPS) / (Σ(s - y0)² + EPS)), the residual formed sample by sample
 *   SSR_WAVE_SEG_SNR  Loizou's comp_snr.m: L = (3 fs + 50) / 100, R = L / 4, M = max(0, (n - L) / R) frames [jR, jR + L) under the
 *                     window 0.5 (1 - cos(2 pi (i + 1) / (L + 1))), seg_j = 10 log10(S_j / (N_j + EPS) + EPS) clamped to [-10, 35],
 *                     the mean over j; M = 0: NaN
 * n = 0: NaN for all three.  Pair e scores estimate e (est + est_off[e], as long as its target) against target tgt_index[e];
 * pairs next to each other that name one target read its tiles once.  tgt / est: float32, or float64 where tgt_f64 / est_f64;
 * tgt_off / est_off: DEVICE int64 sample offsets.  tgt_len and tgt_index are HOST int32 arrays: validated before anything is
 * enqueued (which a non-empty subset of 7, fs > 0, lengths >= 0, indices in [0, n_tgt)) and copied into the workspace on `stream`
 * (from page-locked memory the copy is asynchronous: keep the values until the stream has reached it).  n_est = 0: nothing is
 * enqueued.  out: double [n_est][popcount(which)], columns in bit order.  Deterministic: fixed-order sums, no atomics; a pair
 * gives the same bits alone and in any batch.  workspace: ssr_wave_metrics_workspace_bytes (0 for invalid arguments). */
#define SSR_WAVE_SNR 1
#define SSR_WAVE_SI_SDR 2
#define SSR_WAVE_SEG_SNR 4
size_t ssr_wave_metrics_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int fs, int which);
int ssr_wave_metrics(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt,
                     const void* est, int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est,
                     int fs, int which, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* Filter-invariant SDR (not in the reference): the SDR of BSS Eval (Vincent, Gribonval & Fevotte, "Performance
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
#define SSR_BSS_MAX_TAPS 512
size_t ssr_bss_sdr_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int taps);
int ssr_bss_sdr(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt,
                const void* est, int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est,
                int taps, double* out /* [n_est][2]: sdr, sdr_lag */, double* filt /* [n_est][taps] or NULL */,
                void* workspace, size_t workspace_bytes, void* stream);

/* Mel-spectrogram distances (not in the reference) on magnitude images S [T][n_bins] (power 1):
 *   M[t][m] = Σ_f S[t][f] fb[f][m]           (float64 sums; E / G: the estimate's / target's mel image)
 *   SSR_MEL_LSD  mel_lsd = mean_t sqrt( mean_m log10( G² / (E + 1e-12)² + 1e-12 )² )        (AudioMetrics.lsd on mel magnitudes)
 *   SSR_MEL_L1   mel_l1  = mean_{t,m} | ln⁺E - ln⁺G |,  ln⁺x = ln(max(x, 1e-5))
 *   SSR_MEL_MCD  mcd     = mean_t (10 / ln 10) sqrt( 2 Σ_{d=1..n_cep} c_d² ),  c = orthonormal DCT-II over m of ln⁺E - ln⁺G
 *                (MFCC-based, frame t against frame t: not an SPTK mel-cepstrum MCD; the warped measure is ssr_*_mel_dtw below)
 * fb: HOST float32 [n_bins][n_mels], row-major (torchaudio's melscale_fbanks layout).  It is validated before anything is
 * enqueued - finite, >= 0, every filter one contiguous run of non-zero weights and none all zero, 1 <= n_mels <= SSR_MEL_MAX,
 * 1 <= n_cep < n_mels - then copied into the workspace on `stream` (from page-locked memory asynchronously: keep it unchanged
 * until the stream has reached it) and packed there as per-filter bin ranges.  which: a non-empty subset of the three bits;
 * out: double [n_items][n_keys][3] = mel_lsd, mel_l1, mcd, NaN where not asked for.  Deterministic: runs of 16 frames per
 * image, fixed-order sums, no atomics - a pair gives the same bits alone and in any batch. */
#define SSR_MEL_LSD 1
#define SSR_MEL_L1 2
#define SSR_MEL_MCD 4
#define SSR_MEL_MAX 256
/* Projection only (AudioMetrics.mel_spectrogram): image v is the rows [frame_off[v], + n_rows[v]) of sp [*, n_bins]; its mel
 * rows go to out + (frame_off[v] + r) * n_mels, float32.  workspace: ssr_spectrogram_mel_workspace_bytes(n_bins, n_mels). */
size_t ssr_spectrogram_mel_workspace_bytes(int n_bins, int n_mels);
int ssr_spectrogram_mel(const float* sp, const int64_t* frame_off, const int32_t* n_rows, int n_images, int max_rows, int n_bins,
                        const float* fb, int n_mels, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* Image level, the descriptors of ssr_spectrogram_lsd_bands (n_keys = 1): out double [n_images][3]. */
size_t ssr_spectrogram_mel_metrics_workspace_bytes(int n_images, int max_rows, int n_bins, int n_mels, int n_cep);
int ssr_spectrogram_mel_metrics(const float* est_sp, const int64_t* est_frame_off, const float* tgt_sp, const int64_t* tgt_frame_off,
                                const int32_t* n_rows, int n_images, int max_rows, int n_bins, const float* fb, int n_mels, int n_cep,
                                int which, double* out, void* workspace, size_t workspace_bytes, void* stream);
/* Waveform level, the descriptors of ssr_pair_lsd_bands: the K + 1 magnitude images of ssr_pair_lsd_bands (n_bins = the plan's),
 * then the reduction.  ssr_pair_mel_metrics_workspace_bytes serves both entry points, and both ask for all of it. */
size_t ssr_pair_mel_metrics_workspace_bytes(const ssr_plan* plan, int n_items, int n_keys, int max_len, int64_t total_rows, int n_mels,
                                            int n_cep);
int ssr_pair_mel_metrics(const ssr_plan* plan, const float* est, const int64_t* est_off, const float* tgt, const int64_t* tgt_off,
                         const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len, int64_t total_rows,
                         const float* fb, int n_mels, int n_cep, int which, double* out, void* workspace, size_t workspace_bytes,
                         void* stream);
int ssr_pair_mel_metrics_est64(const ssr_plan* plan, const double* est, const int64_t* est_off, const float* tgt, const int64_t* tgt_off,
                               const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len, int64_t total_rows,
                               const float* fb, int n_mels, int n_cep, int which, double* out, void* workspace, size_t workspace_bytes,
                               void* stream);

/* DTW-aligned mel-cepstral distortion (not in the reference), for testees whose output drifts by a few frames against
 * the target.  Inputs as above (magnitude images [T][n_bins], fb, ln⁺).  For every image on its own
 *   c[t][d] = orthonormal DCT-II over m of ln⁺((S fb)[t][m]),  d = 1 .. n_cep            (float64; not the DCT of a difference)
 * and for an (estimate E, target G) pair of T frames each (the min_len truncation of evaluation()) and a radius R in frames:
 *   δ(i, j) = (10 / ln 10) sqrt( 2 Σ_d (c_E[i][d] - c_G[j][d])² )   for |i - j| <= R (Sakoe-Chiba band), +inf outside
 *   D[0][0] = 2 δ(0, 0)
 *   D[i][j] = min( D[i-1][j-1] + 2 δ(i, j),  D[i-1][j] + δ(i, j),  D[i][j-1] + δ(i, j) )
 *             the candidates formed in that order, a later one replacing an earlier one only when strictly smaller (a tie keeps the
 *             diagonal, then (i-1, j))
 *   mcd_dtw = D[T-1][T-1] / (2 T)          (the normaliser does not depend on the path: the value is continuous in the images)
 *   dtw_len = cells on the chosen path,  dtw_dev = ( Σ |i - j| over them ) / dtw_len   (mean drift in frames)
 * R = 0: mean_t δ(t, t), i.e. mcd up to float64 rounding; R >= T behaves as R = T - 1; a wider band never gives a larger value,
 * bit for bit (every δ is computed the same way whatever R).  0 <= radius <= SSR_DTW_MAX_RADIUS (one band offset per lane),
 * 1 <= n_cep < n_mels and the filterbank are checked before anything is enqueued (SSR_ERR_INVALID_ARG); the workspace queries
 * return 0 for such arguments; n_items = 0 enqueues nothing.
 * out: double [n_items][n_keys][3] = mcd_dtw, dtw_dev, dtw_len.  Deterministic: a pair gives the same bits alone and in any batch. */
#define SSR_DTW_MAX_RADIUS 31
/* Image level, the descriptors of ssr_spectrogram_mel_metrics with `radius` for `which`: out double [n_images][3]. */
size_t ssr_spectrogram_mel_dtw_workspace_bytes(int n_images, int max_rows, int n_bins, int n_mels, int n_cep, int radius);
int ssr_spectrogram_mel_dtw(const float* est_sp, const int64_t* est_frame_off, const float* tgt_sp, const int64_t* tgt_frame_off,
                            const int32_t* n_rows, int n_images, int max_rows, int n_bins, const float* fb, int n_mels, int n_cep,
                            int radius, double* out, void* workspace, size_t workspace_bytes, void* stream);
/* Waveform level, the descriptors of ssr_pair_mel_metrics with `radius` for `which` (the images are ssr_pair_mel_metrics' own).
 * ssr_pair_mel_dtw_workspace_bytes serves both entry points, and both ask for all of it. */
size_t ssr_pair_mel_dtw_workspace_bytes(const ssr_plan* plan, int n_items, int n_keys, int max_len, int64_t total_rows, int n_mels,
                                        int n_cep, int radius);
int ssr_pair_mel_dtw(const ssr_plan* plan, const float* est, const int64_t* est_off, const float* tgt, const int64_t* tgt_off,
                     const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len, int64_t total_rows,
                     const float* fb, int n_mels, int n_cep, int radius, double* out, void* workspace, size_t workspace_bytes,
                     void* stream);
int ssr_pair_mel_dtw_est64(const ssr_plan* plan, const double* est, const int64_t* est_off, const float* tgt, const int64_t* tgt_off,
                           const int32_t* len, const int64_t* frame_off, int n_items, int n_keys, int max_len, int64_t total_rows,
                           const float* fb, int n_mels, int n_cep, int radius, double* out, void* workspace, size_t workspace_bytes,
                           void* stream);

/* Objective quality measures (not in the reference): Loizou's comp_llr.m, comp_cep.m, comp_wss.m and comp_fwseg.m
 * (Speech Enhancement: Theory and Practice, §11.1-11.2), restated.  Both signals widened to float64 with EPS added to every
 * sample; frames of §10: L = (3 fs + 50) / 100, R = L / 4, M = max(0, (n - L) / R) frames [jR, jR + L) under the window
 * 0.5 (1 - cos(2 pi (i + 1) / (L + 1))).
 *   SSR_QUAL_LLR    per frame min(2, ln(a_y' R_x a_y / a_x' R_x a_x)), order-P LPC by Levinson-Durbin on the autocorrelation
 *                   (P = 10 below 10 kHz, else 16; lpc_order overrides); mean of the round(0.95 M) smallest frame values
 *   SSR_QUAL_CEP    per frame min(10, (10 sqrt 2 / ln 10) ||c_x - c_y||), c the LPC cepstrum c_1 .. c_P; the same trimmed mean
 *   SSR_QUAL_WSS    Klatt's weighted spectral slope on Loizou's 25 critical bands (50 Hz .. about 3.9 kHz at EVERY rate: a
 *                   measure of the band below 4 kHz), N = 2^ceil(log2(2 L))-point spectra; the same trimmed mean
 *   SSR_QUAL_FWSEG  frequency-weighted segmental SNR on the same bands (weights B_x^0.2, frame values clamped to [-10, 35]);
 *                   the plain mean
 * Guards (the frame value stays finite): Levinson stops at an order whose prediction error is not finite and positive; a
 * non-finite or non-positive LLR ratio gives 2; fwSNRseg skips bands with B_x = 0 (none left: -10).  M = 0 or n = 0: NaN.
 * Pair e scores estimate e (est + est_off[e], as long as its target) against target tgt_index[e]; pairs next to each other
 * that name one target analyse its frames once.  tgt / est: float32, or float64 where tgt_f64 / est_f64; tgt_off / est_off:
 * DEVICE int64 sample offsets.  tgt_len and tgt_index are HOST int32 arrays: validated before anything is enqueued (which a
 * non-empty subset of 15, fs in [8000, 48000], lpc_order 0 = default or in [1, 32], lengths >= 0, indices in [0, n_tgt)) and
 * copied into the workspace on `stream` (from page-locked memory the copy is asynchronous: keep the values until the stream has
 * reached it).  n_est = 0: nothing is enqueued.  out: double [n_est][popcount(which)], columns in bit order.  No LPC kernel
 * runs without SSR_QUAL_LLR / SSR_QUAL_CEP, no transform without SSR_QUAL_WSS / SSR_QUAL_FWSEG.  Deterministic: fixed-order
 * float sums, no floating-point atomics; a pair gives the same bits alone and in any batch.  workspace:
 * ssr_quality_metrics_workspace_bytes (0 for invalid arguments).
 * ssr_quality_bands: the transform size at fs, the band centres and widths (Hz, 25 each) and the float64 filters [25][n_fft / 2]
 * (filters_len doubles at least); any output may be null. */
#define SSR_QUAL_LLR 1
#define SSR_QUAL_CEP 2
#define SSR_QUAL_WSS 4
#define SSR_QUAL_FWSEG 8
size_t ssr_quality_metrics_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int fs,
                                           int lpc_order, int which);
int ssr_quality_metrics(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt,
                        const void* est, int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est,
                        int fs, int lpc_order, int which, double* out, void* workspace, size_t workspace_bytes, void* stream);
int ssr_quality_bands(int fs, int32_t* n_fft, double* cent, double* bw, double* filters, size_t filters_len);

/* Pitch metrics (not in the reference): YIN F0 tracking (de Cheveigné & Kawahara, JASA 2002), restated, on 16 kHz
 * float64 signals (the caller resamples: scipy.signal.resample_poly(x, 16000 / g, fs / g) with ssr_resample_poly_f64).
 * Frames: hop H = 160, window W = 400; a signal of n > 0 samples has T = n / H + 1 frames (0 for n = 0), frame t covers samples
 * [t H - W / 2, t H + W / 2) (zeros outside [0, n)).  Lags tau_lo = floor(16000 / fmax) .. tau_hi = ceil(16000 / fmin); the
 * difference d_t(tau) = Σ_j<W (x[s+j] - x[s+j+tau])^2 in float64, in the direct form, for tau = 1 .. tau_hi;
 * d'(tau) = tau d(tau) / Σ_k<=tau d(k) (1 where that sum is 0).  tau* = the smallest trough of d' in [tau_lo, tau_hi] below 0.1,
 * else the smallest tau with the minimum d'; a parabola through d'(tau* - 1 .. tau* + 1) refines it strictly inside the range
 * (when its denominator is > 0 and |delta| <= 1).  f0 = 16000 / (tau* + delta) (NaN where E_t = 0), aperiodicity d'(tau*),
 * E_t = Σ_j<W x[s+j]^2; voiced: E_t > 0, E_t >= 1e-4 max_t E_t and aperiodicity < 0.2.
 * ssr_f0_track: signal i (sig + off[i], len[i] samples) -> its T frames at f0 / aperiodicity / energy / voiced + frame_off[i]
 * (frame_off: DEVICE int64 [n]).
 * ssr_f0_metrics: pair e tracks estimate e (est + est_off[e], as long as its target) and target tgt_index[e]; every target
 * is tracked once, whatever number of estimates name it.  Over the frames voiced in both (B), N_V frames whose voicing differs
 * and N_G frames of B with |f_y / f_x - 1| > 0.2:
 *   SSR_PITCH_F0_RMSE  sqrt(mean_B (1200 log2(f_y / f_x))^2), cents (NaN: B empty)
 *   SSR_PITCH_F0_CORR  Pearson correlation of f_x, f_y over B (NaN: |B| < 2, or every f_x or every f_y of B equal)
 *   SSR_PITCH_GPE      N_G / |B| (NaN: B empty)
 *   SSR_PITCH_VDE      N_V / T (NaN: T = 0)
 *   SSR_PITCH_FFE      (N_V + N_G) / T (NaN: T = 0)
 * Lengths (len, tgt_len) and tgt_index are HOST int32 arrays: validated before anything is enqueued (which a non-empty subset of
 * 31, 40 <= fmin < fmax <= 1000 with tau_hi - tau_lo >= 2, lengths in [0, 2^29), indices in [0, n_tgt)) and copied into the
 * workspace on `stream` (from page-locked memory the copy is asynchronous: keep the values until the stream has reached it).
 * n = 0 / n_est = 0: nothing is enqueued.  out: double [n_est][popcount(which)], columns in bit order.  Deterministic: fixed-order
 * float sums, no floating-point atomics; a signal's track and a pair's values are the same bits alone and in any batch.
 * workspace: the _workspace_bytes queries (0 for invalid arguments). */
#define SSR_PITCH_F0_RMSE 1
#define SSR_PITCH_F0_CORR 2
#define SSR_PITCH_GPE 4
#define SSR_PITCH_VDE 8
#define SSR_PITCH_FFE 16
size_t ssr_f0_track_workspace_bytes(const int32_t* len, int n, double fmin, double fmax);
int ssr_f0_track(const double* sig, const int64_t* off, const int32_t* len, int n, double fmin, double fmax, double* f0,
                 double* aperiodicity, double* energy, uint8_t* voiced, const int64_t* frame_off, void* workspace,
                 size_t workspace_bytes, void* stream);
size_t ssr_f0_metrics_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, double fmin,
                                      double fmax, int which);
int ssr_f0_metrics(const double* tgt, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const double* est,
                   const int64_t* est_off, const int32_t* tgt_index, int n_est, double fmin, double fmax, int which,
                   double* out, void* workspace, size_t workspace_bytes, void* stream);

/* Anti-wrapping phase distances (not in the reference): the instantaneous-phase, group-delay and instantaneous-
 * angular-frequency losses of the bandwidth-extension literature with explicit phase modelling (Ai & Ling 2023; AP-BWE, Lu et
 * al. 2024), restated as metrics.  Both signals widened to float64.  N = n_fft in {256, 512, 1024, 2048}, hop H in [1, N],
 * periodic Hann window 0.5 - 0.5 cos(2 pi i / N), frames centred with reflect padding of N / 2 samples: T = 1 + n / H frames,
 * frame t over padded samples [t H, t H + N).  X[t][k], Y[t][k]: the N-point DFTs of the target's and the estimate's windowed
 * frames, C = Y conj(X); a(z) = |atan2(Im z, Re z)| in [0, pi], and a(z) = 0 where Re z = Im z = 0 whatever their signs (digital
 * silence scores 0 and is counted).  With f(u) = |u - 2 pi round(u / 2 pi)| the papers' anti-wrapping function,
 * f(arg Y - arg X) = a(C), and their differences along frequency and time are arguments of products:
 *   SSR_PHASE_IP    mean over t < T, bin_lo <= k <= bin_hi of a(C[t][k])
 *   SSR_PHASE_GD    mean over t < T, bin_lo <= k < bin_hi of a(C[t][k + 1] conj(C[t][k]))          (NaN: bin_hi = bin_lo)
 *   SSR_PHASE_IAF   mean over t < T - 1, bin_lo <= k <= bin_hi of a(C[t + 1][k] conj(C[t][k]))     (NaN: T < 2)
 * n <= N / 2 (reflect padding undefined) or n = 0: NaN.  Nothing is rescaled: a product that underflows to zero scores 0 (none
 * does for float32 signals) and the definition does not depend on the level of either signal; the two frames of a pair share one
 * complex transform, so a spectrum value is accurate to about 1e-16 log2(N) of the larger of the two frames' largest bins, and
 * multiplying BOTH signals by one power of two changes no bit.  A frame in which either signal is digitally silent has C = 0
 * exactly.  Values in radians.
 * Pair e scores estimate e (est + est_off[e], as long as its target) against target tgt_index[e].  tgt / est: float32, or
 * float64 where tgt_f64 / est_f64; tgt_off / est_off: DEVICE int64 sample offsets.  tgt_len and tgt_index are HOST int32 arrays:
 * validated before anything is enqueued (which a non-empty subset of 7, n_fft in the set, 1 <= hop <= n_fft,
 * 0 <= bin_lo <= bin_hi <= n_fft / 2, lengths in [0, 2^29), indices in [0, n_tgt)) and copied into the workspace on `stream`
 * (from page-locked memory the copy is asynchronous: keep the values until the stream has reached it).  n_est = 0: nothing is
 * enqueued.  out: double [n_est][popcount(which)], columns in bit order.  Without SSR_PHASE_IAF no warm-up frame is
 * transformed; the IP and GD bits are the same either way.  Deterministic: fixed-order float sums, no floating-point atomics; a
 * pair gives the same bits alone, in any batch and at any position.  workspace: ssr_phase_metrics_workspace_bytes (0 for
 * invalid arguments).  One launch holds a workgroup of n_fft / 8 threads per chunk of 16 frames: SSR_ERR_UNSUPPORTED when that is
 * 2^32 threads or more (checked before anything is enqueued). */
#define SSR_PHASE_IP 1
#define SSR_PHASE_GD 2
#define SSR_PHASE_IAF 4
size_t ssr_phase_metrics_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_fft, int hop,
                                         int which);
int ssr_phase_metrics(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                      int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_fft, int hop, int bin_lo,
                      int bin_hi, int which, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* Multi-resolution STFT distance (not in the reference): the spectral convergence and the log-magnitude distance of
 * Parallel WaveGAN's training loss (Yamamoto et al. 2020), restated as metrics, at n_res resolutions (N, H, W) = (n_fft[r], hop[r],
 * win[r]) and their means.  Both signals widened to float64.  N in {256, 512, 1024, 2048}, 1 <= H <= N, 2 <= W <= N; the window is
 * w[l + i] = 0.5 - 0.5 cos(2 pi i / W) for 0 <= i < W with l = (N - W) / 2 rounded down and zero elsewhere (torch.stft's placement
 * of a periodic Hann window of win_length W); frames centred with reflect padding of N / 2 samples: T = 1 + n / H frames, none
 * where n <= N / 2.  X[t][k], Y[t][k]: the N-point DFTs of the target's and the estimate's windowed frames on the bins
 * bin_lo[r] <= k <= bin_hi[r]; p = max(|.|^2, eps), m = sqrt(p).  Per resolution
 *   sc  = sqrt(sum (m_x - m_y)^2 / sum m_x^2)   over all scored cells of the signal
 *   mag = mean |log m_x - log m_y|              over the same cells (evaluated as 0.5 |log(p_x / p_y)|)
 * and NaN for both where the resolution has no frame.  A frame whose windowed samples are all zero has |.|^2 = 0 exactly, so
 * m = sqrt(eps) in each of its bins; a frame whose windowed estimate equals its windowed target sample for sample has m_y = m_x
 * exactly: an estimate equal to its target scores 0 / 0.
 * Pair e scores estimate e (est + est_off[e], as long as its target) against target tgt_index[e].  tgt / est: float32, or
 * float64 where tgt_f64 / est_f64; tgt_off / est_off: DEVICE int64 sample offsets.  tgt_len, tgt_index, n_fft, hop, win, bin_lo
 * and bin_hi are HOST int32 arrays: validated before anything is enqueued (n_res in [1, SSR_MRSTFT_MAX_RES], each n_fft in the
 * set, 1 <= hop <= n_fft, 2 <= win <= n_fft, 0 <= bin_lo <= bin_hi <= n_fft / 2, eps finite and > 0, lengths in [0, 2^29),
 * indices in [0, n_tgt)); the first two are copied into the workspace on `stream` (from page-locked memory the copy is
 * asynchronous: keep the values until the stream has reached it).  n_est = 0: nothing is enqueued.
 * out: double [n_est][n_res + 1][2]: (sc, mag) of resolution r in row r, their means over the resolutions (added in index order;
 * NaN where any resolution is NaN) in row n_res.  A resolution's row does not depend on the other resolutions of the call.
 * Deterministic: fixed-order float sums, no atomics; a pair gives the same bits alone, in any batch and at any position.  Every
 * launch is on `stream`, without a host wait in between.  workspace: ssr_mrstft_workspace_bytes (0 for invalid arguments).  A
 * resolution's launch holds a workgroup of n_fft / 8 threads per chunk of 16 frames: SSR_ERR_UNSUPPORTED when that is 2^32 threads
 * or more (checked before anything is enqueued). */
#define SSR_MRSTFT_MAX_RES 8
size_t ssr_mrstft_workspace_bytes(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int n_res,
                                  const int32_t* n_fft, const int32_t* hop, const int32_t* win);
int ssr_mrstft_metrics(const void* tgt, int tgt_f64, const int64_t* tgt_off, const int32_t* tgt_len, int n_tgt, const void* est,
                       int est_f64, const int64_t* est_off, const int32_t* tgt_index, int n_est, int n_res, const int32_t* n_fft,
                       const int32_t* hop, const int32_t* win, const int32_t* bin_lo, const int32_t* bin_hi, double eps, double* out,
                       void* workspace, size_t workspace_bytes, void* stream);

/* A6.  The tensor helpers of ssr_eval/utils.py as stand-alone calls (inside ssr_pair_metrics /
 * ssr_spectrogram_metrics they are fused; these back `from ssr_eval.utils import to_log, pow_p_norm, ...`).
 *   ssr_to_log      out = log10(x + 1e-12)                       utils.py:43-44
 *   ssr_from_log    out = 10 ** min(x, 5)                        utils.py:47-49
 *   ssr_energy_sums sums[i] = {sum a^2, sum b^2, sum a*b} over item i's per_item contiguous elements (float64):
 *                   pow_p_norm = (float)sqrt(sum)^2 (utils.py:68-76), pow_norm = sum a*b (utils.py:85-92)
 *   ssr_scale_items out[i][j] = (x[i][j] * mul[i]) / div[i]      the rescaled target of energy_unify, utils.py:79-82 */
int ssr_to_log(const float* x, int64_t n, float* out, void* stream);
int ssr_from_log(const float* x, int64_t n, float* out, void* stream);
int ssr_energy_sums(const float* a, const float* b, int n_items, int64_t per_item, double* sums, void* stream);
int ssr_scale_items(const float* x, const float* mul, const float* div, int n_items, int64_t per_item, float* out,
                    void* stream);

/* A5 on [B, C, T, F] tensors with C > 1: AudioMetrics.sispec / its to_log variant (ssr_eval/metrics.py:114-121 with
 * energy_unify, utils.py:79-82).  pow_norm (utils.py:85-92) is per (b, c), pow_p_norm (utils.py:68-76) over every dimension
 * but the batch, so the per-channel projections share one all-channel target energy and there is one ratio per batch item.
 * est / tgt: contiguous [n_batch, n_channels, per_image] float32; log_domain != 0 applies to_log (utils.py:43-44) to both
 * first.  out: [n_batch + 1] float64 = the per-item values, then their mean (metrics.py:121: sum / B).  Energies are
 * accumulated in float64 on the difference est - tgt (accurate at any SNR).  workspace: n_batch * n_channels * 24 bytes. */
int ssr_sispec_multichannel(const float* est, const float* tgt, int n_batch, int n_channels, int64_t per_image,
                            int log_domain, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* K6.  STFT-domain hard low-pass: stft_hard_lowpass_v0 (ssr_eval/lowpass.py:17-28) through
 * FDomainHelper.wav_to_spectrogram_phase / spectrogram_phase_to_wav (ssr_eval/dsp.py:83-119).
 * cut[i] = first zeroed bin = int(n_bins * highcut / int(fs/2)) (lowpass.py:24,193-194; computed by the
 * caller, bit-exact integer).  Output has the input's layout (same off / len).  Power-of-two n_fft only.
 * workspace: ssr_ola_workspace_bytes(plan, total_rows).
 * Precondition, PER ITEM: len[i] > n_fft / 2 (torch's reflect padding inside torchlibrosa's STFT refuses anything
 * shorter, dsp.py:21-59).  max_len <= n_fft / 2 is SSR_ERR_INVALID_ARG; lengths live on the device, so a short item in a
 * batch whose max_len passes cannot be reported - it is skipped and its output samples are set to 0 (no out-of-range
 * access); the Python mirror checks every item on the host and raises ValueError.  Same for ssr_istft. */
size_t ssr_ola_workspace_bytes(const ssr_plan* plan, int64_t total_rows);
int ssr_fft_lowpass(const ssr_plan* plan, const float* in, const int64_t* off, const int32_t* len, const int32_t* cut,
                    const int64_t* frame_off, int n_items, int max_len, int64_t total_rows, float* out,
                    void* workspace, size_t workspace_bytes, void* stream);

/* K6 for ONE batch and K cut-offs: SSR_Eval_Helper.lowpass_stft_hard (ssr_eval/eval.py:401-410) loops stft_hard_lowpass_v0 over the
 * cutoffs of setting_fft on the same waveform.  cuts: HOST array of n_keys cut bins, each applied to every item of the batch
 * (int(n_bins * (cutoff // 2) / int(fs / 2)) with the evaluator's one fs).  Key k's output goes to out + k * key_stride (elements),
 * in the input's layout (same off / len).  On the SSR_LOWPASS_CONV engine the padded copy and the forward dense-DFT product are
 * computed ONCE, at the largest cut (spectrogram_phase and mag * cos / mag * sin of a bin do not depend on the cut: every output is
 * bit-identical to K ssr_fft_lowpass calls), followed by one inverse product per key over that key's channels; row tiles run over
 * the whole batch (one cut per launch).  The FFT engines run K plain calls.  workspace: ssr_ola_workspace_bytes(plan, total_rows). */
int ssr_fft_lowpass_multi(const ssr_plan* plan, const float* in, const int64_t* off, const int32_t* len, const int32_t* cuts,
                          int n_keys, const int64_t* frame_off, int n_items, int max_len, int64_t total_rows, float* out,
                          int64_t key_stride, void* workspace, size_t workspace_bytes, void* stream);

/* K6'.  Inverse STFT: torchlibrosa ISTFT.forward(real, imag, length) as used by
 * FDomainHelper.spectrogram_phase_to_wav / reverse_complex_spectrogram (ssr_eval/dsp.py:67-70,107-119).
 * re/im: [total_rows, n_bins]; item i has ssr_num_frames(len[i]) rows. */
int ssr_istft(const ssr_plan* plan, const float* re, const float* im, const int64_t* frame_off, const int32_t* len,
              const int64_t* out_off, int n_items, int max_len, int64_t total_rows, float* out, void* workspace,
              size_t workspace_bytes, void* stream);

/* K7.  Polyphase resampler = scipy.signal.resample_poly(x, up, down) for float32 x, i.e.
 * librosa.resample(..., res_type="polyphase") (ssr_eval/eval.py:145-150) and subsampling()
 * (ssr_eval/lowpass.py:134-144).  ssr_resample_plan reproduces SciPy's integer plan on the host;
 * `taps` is the DEVICE copy of zeros(n_pre_pad) ++ firwin(2*half_len+1, 1/max(up,down), kaiser 5.0)*up
 * as float32 (the caller designs the taps exactly as SciPy does).  Output bit-identical to SciPy. */
int ssr_resample_plan(int64_t n_in, int up, int down, int* up_reduced, int* down_reduced, int64_t* n_out,
                      int* half_len, int* n_pre_pad, int* n_pre_remove);
int ssr_resample_poly(const float* in, const int64_t* in_off, const int32_t* in_len, const int64_t* out_off,
                      const int32_t* out_len, int n_items, int max_out_len, int up, int down, const float* taps,
                      int n_taps, int n_pre_remove, float* out, void* stream);

/* K7 twice in one kernel (round 4): resample_poly(resample_poly(x, up1, down1), up2, down2) for float32 signals with the INTERMEDIATE
 * signal held in LDS only - BASELINE cfg-5's 16 kHz -> 44.1 kHz -> 48 kHz chain (librosa.resample(res_type="polyphase") at
 * ssr_eval/eval.py:144-150 behind a testee that itself up-sampled).  Both stages are the bit-exact kernel of ssr_resample_poly: the
 * intermediate has SciPy's bits and so has the output - bit-identical to two ssr_resample_poly calls, at 12.8 GB of HBM traffic per
 * 12,500 utterances of 4 s instead of 30.6 GB.  mid_len[i] (device) = the intermediate length of item i (ssr_resample_plan's n_out
 * for stage 1); out_len / max_out_len refer to the final signal.  Plans (reduced up / down, taps, n_pre_remove) as for
 * ssr_resample_poly.  SSR_ERR_UNSUPPORTED unless both plans have 21 taps per phase and 8 up1 = 24 down2 with up1 <= 448,
 * up2 <= 160 (441/160 then 160/147 and its multiples): the caller then runs the two stages through ssr_resample_poly. */
int ssr_resample_poly_chain(const float* in, const int64_t* in_off, const int32_t* in_len, const int32_t* mid_len,
                            const int64_t* out_off, const int32_t* out_len, int n_items, int max_out_len, int up1, int down1,
                            const float* taps1, int n_taps1, int n_pre_remove1, int up2, int down2, const float* taps2,
                            int n_taps2, int n_pre_remove2, float* out, void* stream);

/* K7 on the matrix cores (round 3): the same sums as ssr_resample_poly, evaluated as a dense (outputs x input window) by
 * (input window x 32 utterances) product on v_mfma_f32_32x32x2_f32 - float32 FUSED multiply-adds in ascending input index, one
 * rounding per tap where SciPy's upfirdn rounds product and sum separately.  NOT bit-identical to scipy.signal.resample_poly:
 * within ~1 ulp per tap of it.  Metrics of a resampled signal whose upper band is the resampler's own leakage move with those
 * ulps: LSD by up to 1.2e-5 relative over 12,500 white-noise utterances (typically 1e-6), log-SISpec by 2.5e-5 - a caller that needs
 * the 1e-5 bar against SciPy-resampled references uses ssr_resample_poly; 1.2-1.5x the rate of the bit-exact kernel (measured: 441/160 1.45 against 2.23 ms, 160/147
 * 1.93 against 2.27 ms per 4096 utterances of 4 s).  Same
 * arguments and sample indices.  SSR_ERR_UNSUPPORTED for plans whose tap table (> 96 KB) or 32-output window (> 446 samples)
 * do not fit - ssr_resample_poly serves every plan. */
int ssr_resample_poly_mfma(const float* in, const int64_t* in_off, const int32_t* in_len, const int64_t* out_off,
                           const int32_t* out_len, int n_items, int max_out_len, int up, int down, const float* taps,
                           int n_taps, int n_pre_remove, float* out, void* stream);

/* K7 for a float64 signal (what the reference has after an IIR degradation or a float64-returning testee):
 * SciPy then keeps the taps in float64 and accumulates in float64; same plan, same ordering, bit-identical. */
int ssr_resample_poly_f64(const double* in, const int64_t* in_off, const int32_t* in_len, const int64_t* out_off,
                          const int32_t* out_len, int n_items, int max_out_len, int up, int down, const double* taps,
                          int n_taps, int n_pre_remove, double* out, void* stream);

/* N2.  Band-limited windowed-sinc resampler: the arithmetic of resampy.resample(x, sr_orig, sr_new, filter="kaiser_best"),
 * i.e. of librosa.load(file, sr=...) / librosa.resample(res_type="kaiser_best") at the reference's ingest call sites
 * (ssr_eval/eval.py:242 preprocess -> librosa.load(file, sr=sr); ssr_eval/metrics.py:22-23 AudioMetrics.read; and in place of
 * the `sox -r` target resampling of eval.py:133-134).  The caller supplies, as DEVICE arrays, the interpolation filter
 * (interp_win, already scaled by the ratio when downsampling, and interp_delta = its forward differences), resampy's
 * `precision` as num_table = 2^precision, index_step = int(scale * num_table), scale = min(1, ratio), and the time register of
 * every output index (t / ratio, accumulated sequentially as resampy does; time_register_len entries, at least max_out_len -
 * checked).  out_len[i] = int(in_len[i] * ratio), ratio = sr_new / sr_orig.  phase_period: a of the reduced fraction
 * sr_new / sr_orig = a / b when the rates are integers (the filter phase repeats every a outputs: a wave then works on one
 * phase across 64 consecutive periods and its table reads coalesce), or 0 / 1 when unknown - a work-mapping hint only, the
 * result does not depend on it.  float64 weights, float32 running sum rounded after every tap, no fused multiply-add:
 * bit-identical to the NumPy restatement in oracle/resampy.py.  (resampy itself is absent from the reference tree and the
 * image: parity with the package is unpinned.)  n_items * ceil(max_out_len / block) must stay below 2^31 (checked). */
int ssr_resample_sinc(const float* in, const int64_t* in_off, const int32_t* in_len, const int64_t* out_off,
                      const int32_t* out_len, int n_items, int max_out_len, const double* time_register,
                      int64_t time_register_len, const double* interp_win, const double* interp_delta, int n_win,
                      int num_table, int index_step, double scale, double ratio, int phase_period, float* out, void* stream);

/* N2 (decode side).  16-bit PCM frames -> float32 mono, the values librosa.load(file, sr=None) returns for a PCM_16 file
 * (ssr_eval/eval.py:242, metrics.py:21-24: soundfile's float32 read = sample / 32768, then the channel mean): the host decoder
 * hands over the raw interleaved int16 frames (half the bytes across PCIe, no float pass on the host).
 * pcm_off[i]: element offset of item i in `pcm`; item i holds n_frames[i] * n_channels[i] samples (1 <= n_channels <= 8);
 * out_off[i]: element offset of its n_frames[i] float32 outputs. */
int ssr_pcm16_to_float(const int16_t* pcm, const int64_t* pcm_off, const int32_t* n_frames, const int32_t* n_channels,
                       int n_items, int max_frames, float* out, const int64_t* out_off, void* stream);

/* N2.  FLAC ingest: the decode half of librosa.load(file) for the format the reference's data set ships in
 * (ssr_eval/eval.py:158-169 lists ".wav" / ".flac"; eval.py:242, ssr_eval/metrics.py:21-24).  HOST entry points (paths and
 * buffers are host memory; no GPU needed): the decoder threads of the Python mirror call them with the pinned staging arena as
 * `out`, so 16-bit files cross PCIe as int16 exactly like PCM .wav files (ssr_pcm16_to_float then yields librosa's float32 values).
 * Full format support (RFC 9639: CONSTANT / VERBATIM / FIXED / LPC subframes, Rice partitions incl. escapes, wasted bits, the three
 * stereo decorrelations, 4-32 bits, CRC-8 / CRC-16 checked).  verify_md5 != 0: the MD5 of the decoded PCM is compared with the
 * signature STREAMINFO carries (when the encoder stored one) - a bit-exact self-check; mismatch = SSR_ERR_INVALID_ARG.
 * out: interleaved frames, capacity in SAMPLES (frames x channels); out == NULL only counts (and verifies); *frames_out = frames
 * per channel.  ssr_flac_decode_pcm16 takes streams of <= 16 bits per sample (SSR_ERR_UNSUPPORTED otherwise); _i32 takes any. */
int ssr_flac_info(const char* path, int* sample_rate, int* channels, int* bits, int64_t* total_samples, int* has_md5);
int ssr_flac_decode_pcm16(const char* path, int16_t* out, int64_t capacity, int verify_md5, int64_t* frames_out);
int ssr_flac_decode_i32(const char* path, int32_t* out, int64_t capacity, int verify_md5, int64_t* frames_out);

/* N4.  Position of the maximum of the full cross-correlation of two equal-length signals,
 *   z[k] = sum_l a[l] * b[l - k + n - 1],  k = 0 .. 2n-2   (scipy.signal.correlate(a, b, "full")),
 * first maximum on ties (numpy.argmax): the alignment step of SSR_Eval_Helper.mp3_encoding
 * (ssr_eval/eval.py:319  shift = argmax(correlate(decoded, x)) - len(x)).  argmax_out: int64 [n_items]. */
size_t ssr_xcorr_workspace_bytes(int n_items, int max_len);
int ssr_xcorr_argmax(const float* a, const int64_t* a_off, const float* b, const int64_t* b_off, const int32_t* len,
                     int n_items, int max_len, int64_t* argmax_out, void* workspace, size_t workspace_bytes,
                     void* stream);

/* N1.  Zero-phase IIR: scipy.signal.sosfiltfilt(sos, x) (padtype "odd", padlen 3*ntaps) for float32 x, float64
 * arithmetic and output - the arithmetic of lowpass_filter / bandpass_filter (ssr_eval/lowpass.py:54-131, called
 * from lowpass()/bandpass() :175-190,:215-254 and SSR_Eval_Helper.lowpass_butterworth/... eval.py:334-399).
 * sos: DEVICE [n_sections][6] float64 (b0 b1 b2 1 a1 a2, designed by the caller as the reference does with
 * scipy.signal.butter/cheby1/ellip/bessel(output="sos")); zi: DEVICE [n_sections][2] = scipy.signal.sosfilt_zi(sos);
 * edge = 3 * (2*n_sections + 1 - min(#(b2 == 0), #(a2 == 0))); every item needs len > edge.  n_sections <= 16.
 * y: float64, same ragged layout as x.  workspace: ssr_sosfiltfilt_workspace_bytes(total_len, n_items, edge).
 * Bit-identical to SciPy (same operation order, no fused multiply-add). */
size_t ssr_sosfiltfilt_workspace_bytes(int64_t total_len, int n_items, int edge);
int ssr_sosfiltfilt(const float* x, const int64_t* off, const int32_t* len, int n_items, int64_t total_len,
                    const double* sos, const double* zi, int n_sections, int edge, double* y, void* workspace,
                    size_t workspace_bytes, void* stream);
/* The same for a float64 signal (odd extension and filtering on the float64 values, as SciPy does). */
int ssr_sosfiltfilt_f64(const double* x, const int64_t* off, const int32_t* len, int n_items, int64_t total_len,
                    const double* sos, const double* zi, int n_sections, int edge, double* y, void* workspace,
                    size_t workspace_bytes, void* stream);

/* The same for n_designs filters over ONE batch in one launch (round 5): SSR_Eval_Helper.preprocess applies every
 * (filter type, cutoff, order) of setting_lowpass_filtering to the same waveform (ssr_eval/eval.py:243-258, three nested loops).
 * The recurrence is serial in time - a launch lasts as long as its longest utterance's chain (35-39 ns per sample step since round 6:
 * ssr_iir.h) whatever runs beside it - so 36 designs one after the other took 36 x that latency (94 % of an evaluate() pass with IIR
 * settings in round 4); side by side they take it once.  A design of S sections occupies the smallest power of two >= S lanes per utterance.
 * sos: DEVICE [n_designs][8][6] (rows >= n_sections[d] unused), zi: DEVICE [n_designs][8][2]; n_sections, edge: HOST [n_designs]
 * (n_sections <= 8, n_designs <= 48); y: [n_designs][y_stride] float64, design d's output in x's ragged layout from d * y_stride.
 * Every output bit-identical to the single-design call. */
size_t ssr_sosfiltfilt_multi_workspace_bytes(int64_t total_len, int n_items, const int32_t* edge, int n_designs);
int ssr_sosfiltfilt_multi(const float* x, const int64_t* off, const int32_t* len, int n_items, int64_t total_len,
                          const double* sos, const double* zi, const int32_t* n_sections, const int32_t* edge, int n_designs,
                          double* y, int64_t y_stride, void* workspace, size_t workspace_bytes, void* stream);

/* N1-fast.  The same n_designs filters over one batch PARALLEL IN TIME - the opt-in second arithmetic of the IIR keys
 * (backend.sosfiltfilt_multi(exact=False), SSR_Eval_Helper(iir_exact=False)); ssr_sosfiltfilt_multi stays the default everywhere.
 * Method (ssr_iir_pit.h): the cascade of S sections is one linear system with 2S states, so every utterance's odd-extended signal is
 * cut into segments of 128 samples, counted from its first extended sample, that run side by side - one lane per (design, utterance,
 * segment) filters its segment from the zero state; a short scan per (design, utterance) hands the states on,
 * z_in[k+1] = z_end[k] + M z_in[k], from SciPy's zi * ext[0]; the zero-input response H[n mod 128] z_in[n / 128] is added in a fixed
 * order where the backward pass reads the forward output; the backward pass does the same over the same segments downwards from
 * zi * fwd[-1], its second sweep starting every segment from its handed-on state and writing y once.  H (128 x 2S) and M (2S x 2S)
 * are built on the device by this call, on `stream`, inside `workspace`: no allocation, no host synchronisation.
 * Accuracy contract: float64 throughout, max|y - scipy.signal.sosfiltfilt| <= 1e-10 max|scipy| per signal (measured: below 1e-12 for
 * butter / cheby1 / ellip / bessel of order 2-10 at 1-12 kHz, fs 44.1 kHz) - NOT SciPy's bits: the sums are re-associated across
 * segments and multiply-adds may be fused.  No atomics and no order that depends on the launch: two calls give the same bits, and a
 * signal alone gives the same bits as inside a batch or beside other designs.
 * Arguments as ssr_sosfiltfilt_multi's (sos [n_designs][8][6], zi [n_designs][8][2] DEVICE; n_sections, edge HOST; n_sections <= 8,
 * n_designs <= 48, every item len > edge, items back to back or apart but not overlapping), the same error codes for the same
 * argument faults, returned before any launch.  ONE RESTRICTION ssr_sosfiltfilt_multi DOES NOT MAKE: off[] must ascend with the item
 * index (what Ragged packs) - the segment-to-item map is a binary search over it, and it is on the device where this call cannot
 * check it: descending or shuffled offsets give wrong output, not an error.  A batch with items needs total_len > 0
 * (SSR_ERR_INVALID_ARG).  _f64: float64 signals (extended and filtered as float64). */
size_t ssr_sosfiltfilt_fast_workspace_bytes(int64_t total_len, int n_items, const int32_t* edge, int n_designs);
int ssr_sosfiltfilt_fast(const float* x, const int64_t* off, const int32_t* len, int n_items, int64_t total_len,
                         const double* sos, const double* zi, const int32_t* n_sections, const int32_t* edge, int n_designs,
                         double* y, int64_t y_stride, void* workspace, size_t workspace_bytes, void* stream);
int ssr_sosfiltfilt_fast_f64(const double* x, const int64_t* off, const int32_t* len, int n_items, int64_t total_len,
                             const double* sos, const double* zi, const int32_t* n_sections, const int32_t* edge, int n_designs,
                             double* y, int64_t y_stride, void* workspace, size_t workspace_bytes, void* stream);

/* Not in the reference.  Bootstrap of the aggregate: replicates of SSR_Eval_Helper.evaluate's "averaged" - the
 * mean over speakers of each speaker's mean over its files (ssr_eval/eval.py:200-216 computes the point estimate only) - for
 * every column of the per-file table at once, and a per-column summary of the replicates.
 * table: DEVICE [n_rows][n_cols] float64, one row per file, the rows of speaker s at spk_off[s] .. spk_off[s + 1] - 1; spk_off:
 * HOST [n_spk + 1], from 0 to n_rows, strictly ascending (no empty speaker); n_spk <= SSR_BOOTSTRAP_MAX_SPEAKERS (it travels in
 * the kernel arguments: no workspace, no copy).  scheme SSR_BOOTSTRAP_UTTERANCE: slot t = speaker t; SSR_BOOTSTRAP_SPEAKER: the
 * speaker of every slot is drawn with replacement first.  Either way slot t then draws as many files of its speaker as the speaker
 * has, with replacement, and the SAME files serve every column of the replicate.  Draws are Philox4x32-10 words with the key
 * (seed & 0xffffffff, seed >> 32): file draw j of slot t of replicate b = word j % 4 of counter (b, j / 4, t, 0), the speaker of
 * slot t = word t % 4 of counter (b, t / 4, 0, 1); a word u picks index (u * n) >> 32.  A replicate therefore depends on
 * (seed, b, spk_off, the table) only.  Each replicate of each column is ONE sequential float64 chain (file sums in draw order, slot
 * means in slot order), so a column gives the same bits alone and inside a wider table.  A column with a non-finite table entry
 * gets NaN in every replicate.  reps: DEVICE [n_boot][n_cols] float64.  1 <= n_boot <= 16384 (SSR_ERR_UNSUPPORTED above). */
#define SSR_BOOTSTRAP_UTTERANCE 0
#define SSR_BOOTSTRAP_SPEAKER 1
#define SSR_BOOTSTRAP_MAX_Q 8
#define SSR_BOOTSTRAP_MAX_SPEAKERS 512
int ssr_bootstrap_means(const double* table, int64_t n_rows, int n_cols, const int32_t* spk_off, int n_spk, int n_boot,
                        uint64_t seed, int scheme, double* reps, void* stream);
/* Not in the reference.  Per column of reps (DEVICE [n_boot][n_cols], n_boot <= 16384: one workgroup sorts a column in LDS):
 * out (DEVICE [n_cols][2 + n_q] float64) = the mean of the replicates, their standard error (two-pass, ddof = 1; NaN for
 * n_boot = 1) and the n_q <= SSR_BOOTSTRAP_MAX_Q quantiles q (HOST, each in [0, 1]) by NumPy's default linear rule,
 * pos = q (n_boot - 1); counts (DEVICE [n_cols][2] int32) = the replicates <= 0 and the replicates >= 0.  A column holding a
 * non-finite replicate gets NaN in every float output and -1 in both counts. */
int ssr_bootstrap_summary(const double* reps, int n_boot, int n_cols, const double* q, int n_q, double* out, int32_t* counts,
                          void* stream);
/* Not in the reference.  *index_tile = the file draws a workgroup generates at a time (speakers with more files take several tiles),
 * *max_boot = the largest n_boot. */
int ssr_bootstrap_geometry(int* index_tile, int* max_boot);

/* A12 / SURVEY 8(e).  The path's one collective: the per-speaker [metric sums ..., count] buffer summed over ranks in
 * float64 (what SSR_Eval_Helper.evaluate's mean-of-speaker-means needs from the other shards, ssr_eval/eval.py:200-216) -
 * ncclAllReduce(sum, double) over RCCL / xGMI, in place, on `stream`.  RCCL is resolved with dlopen at the first call
 * (SSR_ERR_UNSUPPORTED when it is absent); one communicator per rank / GPU:
 *   rank 0: ssr_comm_unique_id(uid) -> hand the 128 bytes to every rank (any side channel) -> all: ssr_comm_init_rank.
 * The Python mirror uses torch.distributed (the same RCCL) instead: ssr_eval_amd/dist.py. */
int ssr_comm_unique_id(void* uid128);
int ssr_comm_init_rank(const void* uid128, int n_ranks, int rank, void** comm);
int ssr_comm_destroy(void* comm);
int ssr_allreduce_sums(double* buf, int n, void* comm, void* stream);

#include "../ssr_eval_amd/csrc/ssr_hip_coherence.h"
#include "../ssr_eval_amd/csrc/ssr_hip_loudness.h"
#include "../ssr_eval_amd/csrc/ssr_hip_spectrum.h"
#include "../ssr_eval_amd/csrc/ssr_hip_auditory.h"
#include "../ssr_eval_amd/csrc/ssr_hip_modulation.h"
#include "../ssr_eval_amd/csrc/ssr_hip_distribution.h"
#include "../ssr_eval_amd/csrc/ssr_hip_align.h"
#include "../ssr_eval_amd/csrc/ssr_hip_nmr.h"
#include "../ssr_eval_amd/csrc/ssr_hip_csii.h"

#ifdef __cplusplus
}
#endif
#endif /* SSR_HIP_H_ */
