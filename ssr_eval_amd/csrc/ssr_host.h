// Host-side glue shared by the translation units of libssrhip.so (not part of the C ABI; see include/ssr_hip.h).
// The library is compiled as several .hip files (one per kernel family / precision) so that the few hundred kernel
// instantiations build in parallel; this header carries what they share: the error state, the plan object, launch
// geometry and the launcher entry points each unit defines.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ssr_hip.h"
#include "ssr_block.h"
#include "ssr_fft.h"
#include "ssr_tables.h"

int ssr_fail(int code, const std::string& msg);   // records the thread-local message behind ssr_last_error()
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return ssr_fail(SSR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
// a kernel launch and its error check: SSR_LAUNCH((k_name<A, B>), grid, block, stream, args...) - no dynamic LDS
#define SSR_LAUNCH(kernel, grid, block, stream, ...)                                               \
  do {                                                                                             \
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);                               \
    HIP_TRY(hipGetLastError());                                                                    \
  } while (0)

template <typename T> struct DevTables {
  T* window = nullptr;
  T* window_h = nullptr;
  cx<T>*tw = nullptr, *wchirp = nullptr, *bfilt = nullptr, *chirp = nullptr;
};

struct ssr_plan {
  int n_fft, hop, n_bins, precision, device;
  SsrEngine eng;
  DevTables<float> f32;
  DevTables<double> f64;
  SsrEngine weng;              // the wave engine's variant for float32 pairs (ssr_pick_wave_engine; !ok: none)
  DevTables<float> f32w;       // its tables where they differ from the block engine's (radix 2), else copies of the pointers
  DevTables<double> f64w;
  double* window64 = nullptr;  // always present (OLA normalisation)
  double* wss_tab = nullptr;   // [hop] overlap-added squared window where every overlapping frame exists (hop <= n_fft)
  double* wss_rcp_tab = nullptr;   // [hop] its reciprocal
  int lowpass_engine = 0;      // SSR_LOWPASS_SEGMENTS / SSR_LOWPASS_FUSED / SSR_LOWPASS_CONV (ssr_plan_set_lowpass_engine)
  // SSR_LOWPASS_CONV: torchlibrosa's float32 Conv1d weights, transposed (tu_tlconv.hip; built when the engine is selected)
  float *tl_wre_t = nullptr, *tl_wim_t = nullptr, *tl_ire_t = nullptr, *tl_iim_t = nullptr, *tl_w2 = nullptr;
  int tl_ldw = 0;
  // ssr_plan_create_ex: a caller-supplied analysis / synthesis window, center = False, constant padding - conv engine only
  std::vector<double> ex_window;     // empty: periodic Hann
  int ex_center = 1, ex_pad_reflect = 1;
  bool ex = false;                   // true: only ssr_stft(COMPLEX) / ssr_istft / ssr_fft_lowpass on the conv engine exist for this plan
  std::vector<void*> allocs;
};

template <typename T> inline const DevTables<T>& ssr_tables_of(const ssr_plan* pl);
template <> inline const DevTables<float>& ssr_tables_of<float>(const ssr_plan* pl) { return pl->f32; }
template <> inline const DevTables<double>& ssr_tables_of<double>(const ssr_plan* pl) { return pl->f64; }
template <typename T> inline const DevTables<T>& ssr_wave_tables_of(const ssr_plan* pl);
template <> inline const DevTables<float>& ssr_wave_tables_of<float>(const ssr_plan* pl) { return pl->f32w; }
template <> inline const DevTables<double>& ssr_wave_tables_of<double>(const ssr_plan* pl) { return pl->f64w; }

// Every entry point that takes a plan runs on the plan's device: its tables live there.  (The Python mirror selects
// the device before calling in; a C caller that forgot gets an error instead of an illegal address.)
int ssr_check_plan_device(const ssr_plan* pl, bool ex_ok = false);      // ex_ok: the entry point serves ssr_plan_create_ex plans

// Opt a kernel into more than 48 KiB of dynamic LDS, once per (kernel, device, largest size so far) instead of once per
// launch.  `slot` is a per-kernel static the caller owns (one per template instantiation): the largest size each device has
// been opted into - a kernel whose LDS size depends on the call (resampler rate pair, radix-3 q) grows it per device.
struct SsrLdsSlot { enum { MAX_DEV = 32 }; size_t opted[MAX_DEV] = {}; };
inline int ssr_allow_lds(const void* fn, size_t lds, SsrLdsSlot* slot) {
  if (lds <= 48 * 1024) return SSR_OK;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  const bool tracked = dev >= 0 && dev < SsrLdsSlot::MAX_DEV;
  if (tracked && slot->opted[dev] >= lds) return SSR_OK;
  HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (tracked) slot->opted[dev] = lds;
  return SSR_OK;
}

// ---- launch geometry (deterministic functions of the batch shape; they also define the workspace layout) ----
inline int ssr_ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
inline size_t ssr_align256(size_t x) { return (x + 255) & ~(size_t)255; }
int ssr_target_wgs();                                  // workgroups per launch aimed for when chunking items
int ssr_units_per_chunk_for(int max_units, int n_items, int target_wgs = 0);
// Pair transform of this plan on float32 (in64 = false) signals runs the wave-autonomous engine (ssr_stft_wave.h: one
// wave per workgroup) -> the chunking aims for 4x as many (one-wave) workgroups.
bool ssr_stft_uses_wave_engine(const ssr_plan* pl, bool in64);
int ssr_stft_rn_wave_radix(const ssr_plan* pl);            // 1 / 2 / 3: n_fft = R q over M = 2048, float32 pairs (ssr_stft_rn_wave.h); 0: none
int ssr_pair_units_per_chunk(const ssr_plan* pl, int max_units, int n_items, bool in64);
// chunks per interleaving group of the pair transform (1: none).  The wave engine's chunks interleave in groups of 8 so that
// the frames whose samples overlap are transformed at the same time on one XCD (ssr_stft_wave.h); n_chunks is a multiple of it.
int ssr_pair_interleave(const ssr_plan* pl, bool in64);

// row pitch of the pair pipeline's magnitude images: rows padded to 16 bytes (k_ssim's aligned loads, ssr_metrics.h CONTIG)
inline int ssr_mag_pitch(int n_bins) { return (n_bins + 3) & ~3; }
// such images through 16-byte loads: rows, both bases and the stride between estimate planes 16-byte aligned
inline bool ssr_images_vec16(const float* x, const float* y, int pitch, int64_t x_plane) {
  return pitch % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0 && (x_plane % 4) == 0;
}
// The reductions on K + 1 images run one wave per workgroup over a run of rows.  Estimate keys per wave sharing the target's
// rows: three where they divide by three, else two, else one (k_specred_wave measured 3 and 2 best on the four-metric reduction).
inline int ssr_keys_per_wave(int n_keys) { return n_keys % 3 == 0 ? 3 : (n_keys % 2 == 0 ? 2 : 1); }
// Rows per workgroup: ~16 k workgroups per launch over `groups` (item, key group) pairs, at least 8 rows each
inline int ssr_wave_rows_per_wg(int max_rows, int64_t groups) {
  int64_t spc = ((int64_t)16384 + groups - 1) / groups;
  if (spc > max_rows / 8) spc = max_rows / 8;
  if (spc < 1) spc = 1;
  return ssr_ceil_div(max_rows, spc);
}
// Estimates of a multi-key call go two per complex transform (images only) where the plan has a wave kernel for that
// (ssr_pair_metrics_multi, ssr_pair_lsd_bands).  est64: float64 estimates - n_fft = 3 q on the rotating four-wave engine
// (AudioMetrics(48000), ssr_stft_r3_rot.h SSR_IN_EST64X2).
inline bool ssr_multi_fast_path(const ssr_plan* pl, bool est64) {
  if (est64) return pl->precision == SSR_F64 && ssr_stft_rn_wave_radix(pl) == 3 && pl->weng.m == 1536;
  return ssr_stft_uses_wave_engine(pl, false) || ssr_stft_rn_wave_radix(pl) != 0;
}

// ---- the per-pair families (tu_stoi / tu_wave_metrics / tu_quality / tu_pitch / tu_phase / tu_mrstft / tu_bss / tu_coherence / tu_spectrum / tu_auditory): estimate e is scored
// against target tgt_index[e].  The device side of what they share is ssr_pairs.h ----
// host-side validation of the two descriptor arrays (host memory): lengths in [0, len_limit), indices in [0, n_tgt)
inline int ssr_check_pair_index(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int64_t len_limit,
                                const char* len_msg, const char* count_msg = "n_tgt and n_est must be >= 0") {
  if (n_tgt < 0 || n_est < 0) return ssr_fail(SSR_ERR_INVALID_ARG, count_msg);
  if ((n_tgt > 0 && !tgt_len) || (n_est > 0 && !tgt_index)) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  for (int t = 0; t < n_tgt; ++t)
    if (tgt_len[t] < 0 || tgt_len[t] >= len_limit) return ssr_fail(SSR_ERR_INVALID_ARG, len_msg);
  for (int e = 0; e < n_est; ++e)
    if (tgt_index[e] < 0 || tgt_index[e] >= n_tgt) return ssr_fail(SSR_ERR_INVALID_ARG, "tgt_index out of range");
  return SSR_OK;
}
// the two arrays -> the head of the workspace (host arrays: from page-locked memory these copies are asynchronous - the caller
// keeps them until the stream has passed)
inline int ssr_upload_pair_index(const int32_t* tgt_len, int n_tgt, const int32_t* tgt_index, int n_est, int32_t* len_dev,
                                 int32_t* idx_dev, hipStream_t s) {
  if (n_tgt) HIP_TRY(hipMemcpyAsync(len_dev, tgt_len, (size_t)n_tgt * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(idx_dev, tgt_index, (size_t)n_est * sizeof(int32_t), hipMemcpyHostToDevice, s));
  return SSR_OK;
}
// the signal buffers of an entry point that reads float32 or float64 signals where they lie (checked after the descriptors:
// an empty batch has returned by then); the signals themselves may be absent where no target has a sample
inline int ssr_check_pair_buffers(const void* tgt, const int64_t* tgt_off, const void* est, const int64_t* est_off, const void* out,
                                  const int32_t* tgt_len, int n_tgt) {
  int64_t samples = 0;
  for (int t = 0; t < n_tgt; ++t) samples += tgt_len[t];
  if (!tgt_off || !est_off || !out || (samples > 0 && (!tgt || !est))) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  return SSR_OK;
}
// f(TT{}, TE{}) with the element types of the target and estimate buffers: (float | double) x (float | double); -> f's value
template <typename F> inline auto ssr_dispatch_pair_dtypes(bool tgt_f64, bool est_f64, F&& f) {
  if (!tgt_f64 && !est_f64) return f(float{}, float{});
  if (!tgt_f64) return f(float{}, double{});
  if (!est_f64) return f(double{}, float{});
  return f(double{}, double{});
}
// a workspace carved area after area, each rounded to 256 bytes: take() -> the area's offset; o: the bytes so far
struct SsrWsLayout {
  size_t o = 0;
  size_t take(size_t bytes) { const size_t at = o; o += ssr_align256(bytes); return at; }
};
// host tables by key: built on first use under a lock, never written again - the reference holds for the life of the process
// (the asynchronous copies into a workspace read them after the entry point has returned)
template <typename K, typename V> struct SsrHostTables {
  std::mutex mu;
  std::map<K, V> cache;
  template <typename B> const V& get(const K& key, B&& build) {
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it == cache.end()) {
      it = cache.emplace(key, V{}).first;
      build(it->second);
    }
    return it->second;
  }
};
// the twiddles of an n_fft-point transform (ssr_phase_twiddles_host): one cache for every family that transforms frames
inline const std::vector<cx<double>>& ssr_twiddles_cached(int n_fft) {
  static SsrHostTables<int, std::vector<cx<double>>> tables;
  return tables.get(n_fft, [&](std::vector<cx<double>>& tw) { ssr_phase_twiddles_host(n_fft, tw); });
}

// ---- launchers defined by the kernel translation units --------------------------------------------------------
template <typename T> struct SsrStftParams;
template <typename T> struct SsrLowpassParams;
// tu_stft_*.hip: direct / Bluestein engines.  part 0: float32 pairs, part 1: float64-signal pairs, part 2: single
template <typename T> int ssr_launch_stft_pair(const ssr_plan*, SsrStftParams<T>&, int grid, hipStream_t);
template <typename T> int ssr_launch_stft_pair64(const ssr_plan*, SsrStftParams<T>&, int grid, hipStream_t);
template <typename T> int ssr_launch_stft_single(const ssr_plan*, SsrStftParams<T>&, int grid, hipStream_t);
// radix-3 engine (n_fft = 3q)
template <typename T> int ssr_launch_stft_r3(const ssr_plan*, SsrStftParams<T>&, int grid, hipStream_t);
// R autonomous waves per workgroup (n_fft = R q, float32 pairs); defined next to the radix-3 engine
template <typename T> int ssr_launch_stft_rn_wave(const ssr_plan*, SsrStftParams<T>&, int grid, hipStream_t);
template <typename T> int ssr_launch_stft_r3_64(const ssr_plan*, SsrStftParams<T>&, int grid, hipStream_t);
// dispatcher (tu_core.hip): fills the plan tables into p and picks the unit
template <typename T> int ssr_launch_stft(const ssr_plan*, SsrStftParams<T>&, int grid, hipStream_t);
// tu_metrics.hip: rows[i] = the frames of item i, from the lengths on the device (what the reductions and finalisations read as T_i)
int ssr_launch_rows_from_len(const ssr_plan* pl, const int32_t* len, int n_items, int32_t* rows, hipStream_t s);
// tu_mel.hip: the filterbank area of a mel workspace - the table's host-side validation (n_cep = 0: projection only; -> *nnz), the
// area's bytes, and the copy + k_mel_schedule on `s` that packs it at `ws` (-> *f)
struct SsrMelFb;
int ssr_mel_check_fb(const float* fb, int n_bins, int n_mels, int n_cep, int* nnz);
size_t ssr_mel_fb_bytes(int n_bins, int n_mels, int n_cep);
int ssr_mel_upload_fb(const float* fb, int n_bins, int n_mels, int n_cep, int nnz, char* ws, hipStream_t s, SsrMelFb* f);
// tu_lowpass.hip
template <typename T> int ssr_launch_lowpass(const ssr_plan*, SsrLowpassParams<T>&, int grid, hipStream_t);
// tu_tlconv.hip: the reference-arithmetic engine (dense float32 DFT products on the matrix cores)
int ssr_tl_build(ssr_plan* pl);
int ssr_tl_supported(const ssr_plan* pl);       // the conv engine can serve this n_fft (tables are built at the first launch)
inline int ssr_plan_pad(const ssr_plan* pl) { return pl->ex_center ? pl->n_fft / 2 : 0; }
// the longest item must be transformable (lengths live on the device: a shorter item in a batch is skipped and its output zeroed)
inline int ssr_check_max_len(const ssr_plan* pl, int max_len) {
  const int pad = ssr_plan_pad(pl);
  if (pad && pl->ex_pad_reflect && max_len <= pad) return ssr_fail(SSR_ERR_INVALID_ARG, "reflect padding needs len > n_fft/2");
  if ((int64_t)max_len + 2 * pad < pl->n_fft || max_len < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "signals shorter than one frame");
  return SSR_OK;
}
size_t ssr_tl_workspace_bytes(const ssr_plan* pl, int64_t total_rows);
int ssr_tl_run_inverse(const ssr_plan* pl, const float* in, const int64_t* in_off, const int32_t* len, const int32_t* cut,
                       const float* re, const float* im, const int64_t* frame_off, const int64_t* out_off, int n_items,
                       int max_len, int64_t total_rows, float* out, void* workspace, size_t workspace_bytes, hipStream_t s);
int ssr_tl_run_multi(const ssr_plan* pl, const float* in, const int64_t* in_off, const int32_t* len, const int32_t* cuts_host,
                     int n_keys, const int64_t* frame_off, int n_items, int max_len, int64_t total_rows, float* out,
                     int64_t key_stride, void* workspace, size_t workspace_bytes, hipStream_t s);
int ssr_tl_stft(const ssr_plan* pl, const float* wav, const int64_t* wav_off, const int32_t* wav_len, const int64_t* frame_off,
                int n_items, int max_len, float* out_re, float* out_im, hipStream_t s);
