// Host side of the pair transform, shared by the waveform-level spectral entry points (ssr_pair_metrics*, ssr_pair_metrics_multi*,
// ssr_pair_lsd_bands*, ssr_pair_mel_metrics*): their argument checks, the chunk geometry, the one launch of the plan's pair STFT, and
// the walk over the K estimates of a multi-key batch that leaves K + 1 magnitude images in the workspace.
#pragma once
#include "ssr_host.h"
#include "ssr_stft.h"

// The checks every waveform-level entry point makes before it sizes its workspace.  args_ok: no required pointer but the plan is
// null; family(): the family's own argument checks, which hold for an empty batch too; images: the call materialises magnitude
// images.  -> *max_T: the frames of the longest item, 0 for an empty batch (nothing to do).
template <typename F>
inline int ssr_check_pair_batch(const ssr_plan* pl, bool args_ok, int n_items, int n_keys, int max_len, bool images, int* max_T, F&& family) {
  *max_T = 0;
  if (!pl || !args_ok) return ssr_fail(SSR_ERR_INVALID_ARG, "null argument");
  if (int rc = family()) return rc;
  if (n_items <= 0 || n_keys <= 0) return SSR_OK;
  if (int rc_dev = ssr_check_plan_device(pl)) return rc_dev;
  if (max_len < 1) return ssr_fail(SSR_ERR_INVALID_ARG, "empty signals");
  if (max_len >= (1 << 29)) return ssr_fail(SSR_ERR_UNSUPPORTED, "signals of 2^29 samples or more (4 GiB buffer views)");
  if ((int64_t)n_items * n_keys > 0x3fffffff) return ssr_fail(SSR_ERR_UNSUPPORTED, "batch too large for one launch");
  const int T = (int)ssr_num_frames(pl, max_len);
  if (images && (int64_t)T * pl->n_bins >= ((int64_t)1 << 30))
    return ssr_fail(SSR_ERR_UNSUPPORTED, "spectrogram of 2^30 elements or more (4 GiB buffer views)");
  *max_T = T;
  return SSR_OK;
}
inline int ssr_check_pair_batch(const ssr_plan* pl, bool args_ok, int n_items, int n_keys, int max_len, bool images, int* max_T) {
  return ssr_check_pair_batch(pl, args_ok, n_items, n_keys, max_len, images, max_T, [] { return SSR_OK; });
}

// chunking of one transform pass over the batch
struct SsrPairGeom { int units_per_chunk, n_chunks, interleave; };
inline SsrPairGeom ssr_pair_geom(const ssr_plan* pl, int n_items, int max_len, bool in64) {
  SsrPairGeom g;
  const int max_T = (int)ssr_num_frames(pl, max_len);
  g.units_per_chunk = ssr_pair_units_per_chunk(pl, max_T, n_items, in64);     // depends on the engine that will run
  g.interleave = ssr_pair_interleave(pl, in64);                                // whole interleaving groups (empty chunks write zeros)
  g.n_chunks = ssr_ceil_div(ssr_ceil_div(max_T, g.units_per_chunk), g.interleave) * g.interleave;
  return g;
}

struct SsrPairBatch {            // fixed per batch
  const int32_t* len; const int64_t* frame_off; int n_items; SsrPairGeom g;
};
struct SsrPairLaunch {           // one transform of two signals per item, each as float32 OR float64 samples (the other pointer null)
  const float* a; const double* a64; const int64_t* a_off;
  const float* b; const double* b64; const int64_t* b_off;
  unsigned metric_mask;          // the metric epilogue of (a, b) into `part` (0: none)
  int out_kind;                  // SSR_OUT_MAG: magnitude rows into out_a / out_b (the wave engines skip a null out_b)
  float *out_a, *out_b;
  double* part;
};
inline int ssr_pair_transform(const ssr_plan* pl, const SsrPairBatch& bt, const SsrPairLaunch& l, hipStream_t s) {
  auto run = [&](auto t) {
    SsrStftParams<decltype(t)> p{};
    p.a = l.a; p.a64 = l.a64; p.b = l.b; p.b64 = l.b64; p.a_off = l.a_off; p.b_off = l.b_off; p.len = bt.len; p.frame_off = bt.frame_off;
    p.mode = SSR_MODE_PAIR; p.out_kind = l.out_kind; p.metric_mask = (int)l.metric_mask;
    p.n_fft = pl->n_fft; p.hop = pl->hop; p.n_bins = pl->n_bins;
    p.units_per_chunk = bt.g.units_per_chunk; p.n_chunks = bt.g.n_chunks; p.interleave = bt.g.interleave;
    p.out_a = l.out_a; p.out_b = l.out_b; p.out_pitch = ssr_mag_pitch(pl->n_bins); p.part = l.part;
    return ssr_launch_stft<decltype(t)>(pl, p, bt.n_items * bt.g.n_chunks, s);
  };
  return pl->precision == SSR_F64 ? run(double{}) : run(float{});
}

// workspace head: n_keys estimate planes, the target plane, the block engines' scratch plane; callers append their own areas at
// `end`.  Every plane is total_rows rows of ssr_mag_pitch(n_bins) floats, item i from row frame_off[i].
struct SsrPairImages { size_t plane, off_est, off_tgt, off_scratch, end; };
// planes = false: a caller that materialises no images (empty areas); scratch = false: one that never pairs keys 1 .. with the target
inline SsrPairImages ssr_pair_images_layout(const ssr_plan* pl, int n_keys, int64_t total_rows, bool in64, bool planes = true,
                                            bool scratch = true) {
  SsrPairImages w;
  w.plane = planes ? ssr_align256((size_t)total_rows * ssr_mag_pitch(pl->n_bins) * sizeof(float)) : 0;
  size_t o = 0;
  w.off_est = o; o += (size_t)n_keys * w.plane;
  w.off_tgt = o; o += w.plane;
  // the block engines store both images of a pair (they take no null out_b): keys 1 .. K-1 paired with the target put the target's
  // rows here, so that the image key 0 wrote stays the one every key is reduced against
  w.off_scratch = o; o += (scratch && n_keys > 1 && !ssr_multi_fast_path(pl, in64)) ? w.plane : 0;
  w.end = o;
  return w;
}

// The images of every key and the target into the workspace planes of `w` (est xor est64; float32 targets).  Key 0 is transformed
// with the target (both images written, the target's once); the other keys go two per complex transform where the plan's pair
// transform is a wave kernel, else one per transform with the target, whose image is not rewritten.  mask / part0 / part_last: the
// metric epilogue of the transforms that see the target on the wave engines - key 0 and an odd last key (ssr_pair_metrics_multi).
static int ssr_pair_images(const ssr_plan* pl, const SsrPairBatch& bt, const float* est, const double* est64, const int64_t* est_off,
                           const float* tgt, const int64_t* tgt_off, int n_keys, const SsrPairImages& w, char* ws, hipStream_t s,
                           unsigned mask = 0, double* part0 = nullptr, double* part_last = nullptr) {
  auto plane_of = [&](int k) { return (float*)(ws + w.off_est + (size_t)k * w.plane); };
  auto key = [&](int k) { return est_off + (size_t)k * bt.n_items; };
  // key 0 with the target: both images (the target's written once, here)
  int rc = ssr_pair_transform(pl, bt, {est, est64, key(0), tgt, nullptr, tgt_off, mask, SSR_OUT_MAG, plane_of(0), (float*)(ws + w.off_tgt), part0}, s);
  if (rc) return rc;
  int k = 1;
  const bool fast = ssr_multi_fast_path(pl, est64 != nullptr);
  if (fast)                                  // two estimates per complex transform (wave engines), images only
    for (; k + 1 < n_keys; k += 2)
      if ((rc = ssr_pair_transform(pl, bt, {est, est64, key(k), est, est64, key(k + 1), 0u, SSR_OUT_MAG, plane_of(k), plane_of(k + 1), nullptr}, s)))
        return rc;
  // the rest with the target, whose image is not rewritten: the wave engines (an odd last key) skip a null out_b, the block engines
  // get the scratch plane
  float* tgt_sink = fast ? nullptr : (float*)(ws + w.off_scratch);
  for (; k < n_keys; ++k)
    if ((rc = ssr_pair_transform(pl, bt, {est, est64, key(k), tgt, nullptr, tgt_off, mask, SSR_OUT_MAG, plane_of(k), tgt_sink, part_last}, s)))
      return rc;
  return SSR_OK;
}
