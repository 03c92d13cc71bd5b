// Host emulation of k_stft_wave's body for tests/test_wave_flush_host.py: ssr_stft_wave_body with the one-lane work stashed per frame and
// flushed every 64 frames (STASH = true, the product) next to the frame-by-frame code it replaces (STASH = false), with the chunk
// geometry (units_per_chunk, n_chunks, interleave), the row pitch and the output pointers set directly.
// Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libwave_flush_emu.so wave_flush_emu.cpp
#define SSR_HOST_EMU 1
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_tables.h"
#include "../../ssr_eval_amd/csrc/ssr_stft_wave.h"

template <typename T, bool SUMS, int MAG, bool STASH>
static void run_chunks(const SsrStftParams<T>& p, int n_items) {
  SsrBlk blk{64};
  for (int item = 0; item < n_items; ++item)
    for (int c = 0; c < p.n_chunks; ++c) {
      std::vector<char> lds(ssr_stft_wave_lds_bytes<T, true, true>() + 16, (char)0xA5);     // poisoned: nothing may be read before it is written
      ssr_stft_wave_body<T, SUMS, true, MAG, STASH>(p, blk, c, item, lds.data());
    }
}

// stash: 1 = the product's path, 0 = frame by frame.  mag: -1 = rows decided by out_kind at run time, 0 / 1 = at compile time (stash = 1).
template <typename T>
static int run(int stash, int mag, int hop, int out_kind, int mask, int interleave, const float* a, const float* b, const int64_t* a_off,
               const int64_t* b_off, const int32_t* len, const int64_t* frame_off, int n_items, int units_per_chunk, int n_chunks,
               int64_t out_pitch, float* out_a, float* out_b, double* part) {
  SsrTables<T> t;
  if (!ssr_build_tables<T>(SSR_W_N, t)) return -3;
  SsrStftParams<T> p{};
  p.a = a; p.b = b; p.a_off = a_off; p.b_off = b_off; p.len = len; p.frame_off = frame_off;
  p.mode = SSR_MODE_PAIR; p.out_kind = out_kind; p.metric_mask = mask;
  p.n_fft = SSR_W_N; p.hop = hop; p.n_bins = SSR_W_N / 2 + 1;
  p.units_per_chunk = units_per_chunk; p.n_chunks = n_chunks; p.interleave = interleave;
  if (interleave > 1 && n_chunks % interleave) return -5;
  p.window = t.window_h.data(); p.tw = t.tw.data();
  p.out_a = out_a; p.out_b = out_b; p.out_pitch = out_pitch; p.part = part;
  const bool sums = mask & (SSR_M_SISPEC | SSR_M_LOG_SISPEC);
  if (mag == 1 && out_kind != SSR_OUT_MAG) return -6;
  if (mag == 0 && out_kind == SSR_OUT_MAG) return -6;
  if (!stash) {
    if (mag != -1) return -6;
    if (sums) run_chunks<T, true, -1, false>(p, n_items); else run_chunks<T, false, -1, false>(p, n_items);
    return 0;
  }
#define RUN(M) if (sums) run_chunks<T, true, M, true>(p, n_items); else run_chunks<T, false, M, true>(p, n_items)
  if (mag == -1) { RUN(-1); } else if (mag == 0) { RUN(0); } else { RUN(1); }
#undef RUN
  return 0;
}

extern "C" int wave_flush_run(int precision, int stash, int mag, int hop, int out_kind, int mask, int interleave, const float* a,
                              const float* b, const int64_t* a_off, const int64_t* b_off, const int32_t* len, const int64_t* frame_off,
                              int n_items, int units_per_chunk, int n_chunks, int64_t out_pitch, float* out_a, float* out_b, double* part) {
  if (precision == 1)
    return run<double>(stash, mag, hop, out_kind, mask, interleave, a, b, a_off, b_off, len, frame_off, n_items, units_per_chunk, n_chunks,
                       out_pitch, out_a, out_b, part);
  return run<float>(stash, mag, hop, out_kind, mask, interleave, a, b, a_off, b_off, len, frame_off, n_items, units_per_chunk, n_chunks,
                    out_pitch, out_a, out_b, part);
}
extern "C" int wave_flush_out_mag() { return SSR_OUT_MAG; }
