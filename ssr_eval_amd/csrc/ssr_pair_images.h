// Host-side producer of the K + 1 magnitude images of a multi-key pair batch, shared by the waveform-level reductions on
// images (ssr_pair_lsd_bands, ssr_pair_mel_metrics): the pair transform of ssr_pair_metrics_multi with no metric epilogue.
// Key 0 is transformed with the target (both images written, the target's once); the other keys go two per complex transform
// where the plan's pair transform is a wave kernel, else one per transform with the target, whose image is not rewritten.
#pragma once
#include "ssr_host.h"
#include "ssr_stft.h"

// workspace head: n_keys estimate planes, the target plane, the block engines' scratch plane; callers append their own areas at
// `end`.  Every plane is total_rows rows of ssr_mag_pitch(n_bins) floats, item i from row frame_off[i].
struct SsrPairImages { size_t plane, off_est, off_tgt, off_scratch, end; int units_per_chunk, n_chunks; };

inline SsrPairImages ssr_pair_images_layout(const ssr_plan* pl, int n_items, int n_keys, int max_len, int64_t total_rows, bool in64) {
  SsrPairImages w;
  const int max_T = (int)ssr_num_frames(pl, max_len);
  w.units_per_chunk = ssr_pair_units_per_chunk(pl, max_T, n_items, in64);
  w.n_chunks = ssr_ceil_div(max_T, w.units_per_chunk);
  const int S = ssr_pair_interleave(pl, in64);
  w.n_chunks = ssr_ceil_div(w.n_chunks, S) * S;
  w.plane = ssr_align256((size_t)total_rows * ssr_mag_pitch(pl->n_bins) * sizeof(float));
  size_t o = 0;
  w.off_est = o; o += (size_t)n_keys * w.plane;
  w.off_tgt = o; o += w.plane;
  // the block engines store both images of a pair (they take no null out_b): keys 1 .. K-1 paired with the target put the target's
  // rows here, so that the image key 0 wrote stays the one every key is reduced against
  w.off_scratch = o; o += (n_keys > 1 && !ssr_multi_fast_path(pl, in64)) ? w.plane : 0;
  w.end = o;
  return w;
}

template <typename T>
static int ssr_pair_images_stft(const ssr_plan* pl, const float* a, const double* a64, const int64_t* a_off, const float* b, const double* b64,
                                const int64_t* b_off, const int32_t* len, const int64_t* frame_off, int n_items, float* out_a, float* out_b,
                                const SsrPairImages& w, hipStream_t s) {
  SsrStftParams<T> p{};
  p.a = a; p.a64 = a64; p.b = b; p.b64 = b64; p.a_off = a_off; p.b_off = b_off; p.len = len; p.frame_off = frame_off;
  p.mode = SSR_MODE_PAIR; p.out_kind = SSR_OUT_MAG; p.metric_mask = 0;     // images only, no metric epilogue
  p.n_fft = pl->n_fft; p.hop = pl->hop; p.n_bins = pl->n_bins;
  p.units_per_chunk = w.units_per_chunk; p.n_chunks = w.n_chunks; p.interleave = ssr_pair_interleave(pl, a64 != nullptr);
  p.out_a = out_a; p.out_b = out_b; p.out_pitch = ssr_mag_pitch(pl->n_bins); p.part = nullptr;
  return ssr_launch_stft<T>(pl, p, n_items * w.n_chunks, s);
}

// the images of every key and the target into the workspace planes of `w` (est xor est64; float32 targets)
static int ssr_pair_images(const ssr_plan* pl, const float* est, const double* est64, const int64_t* est_off, const float* tgt,
                           const int64_t* tgt_off, const int32_t* len, const int64_t* frame_off, int n_items, int n_keys,
                           const SsrPairImages& w, char* ws, hipStream_t s) {
  auto plane_of = [&](int k) { return (float*)(ws + w.off_est + (size_t)k * w.plane); };
  float* tgt_plane = (float*)(ws + w.off_tgt);
  auto stft = [&](const float* a, const double* a64, const int64_t* a_off, const float* b, const double* b64, const int64_t* b_off,
                  float* oa, float* ob) {
    return pl->precision == SSR_F64 ? ssr_pair_images_stft<double>(pl, a, a64, a_off, b, b64, b_off, len, frame_off, n_items, oa, ob, w, s)
                                    : ssr_pair_images_stft<float>(pl, a, a64, a_off, b, b64, b_off, len, frame_off, n_items, oa, ob, w, s);
  };
  // key 0 with the target: both images (the target's written once, here)
  int rc = stft(est, est64, est_off, tgt, nullptr, tgt_off, plane_of(0), tgt_plane);
  if (rc) return rc;
  int k = 1;
  const bool fast = ssr_multi_fast_path(pl, est64 != nullptr);
  if (fast)                                  // two estimates per complex transform (wave engines)
    for (; k + 1 < n_keys; k += 2)
      if ((rc = stft(est, est64, est_off + (size_t)k * n_items, est, est64, est_off + (size_t)(k + 1) * n_items, plane_of(k), plane_of(k + 1))))
        return rc;
  // the rest with the target, whose image is not rewritten: the wave engines skip a null out_b, the block engines get the scratch plane
  float* tgt_sink = fast ? nullptr : (float*)(ws + w.off_scratch);
  for (; k < n_keys; ++k)
    if ((rc = stft(est, est64, est_off + (size_t)k * n_items, tgt, nullptr, tgt_off, plane_of(k), tgt_sink))) return rc;
  return SSR_OK;
}
