// Host emulation of the wave engines' radix-8 passes for tests/test_fft_fma_host.py: the twiddled butterfly ssr_bfly8_tw on its
// own, next to the multiply-then-ssr_bfly8 sequence the block engines keep, and the two shared tails (2048 points after
// ssr_dft32, 1536 points after ssr_dft24) as complex transforms in natural order.  Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libfft_fma_emu.so fft_fma_emu.cpp
#define SSR_HOST_EMU 1
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_tables.h"
#include "../../ssr_eval_amd/csrc/ssr_stft_rn_wave.h"

// ---- one butterfly: v[8] complex (interleaved), base twiddle t given as t, t^2, t^4 (each rounded from the exact value, as the
// tables hold them).  which = 0: ssr_bfly8_tw;  1: the seven multiplies (powers 3, 5, 6, 7 formed by products) + ssr_bfly8
template <typename T> static void bfly(int which, const T* in, const T* tw, T* out) {
  cx<T> v[8];
  for (int q = 0; q < 8; ++q) v[q] = {in[2 * q], in[2 * q + 1]};
  const cx<T> w[3] = {{tw[0], tw[1]}, {tw[2], tw[3]}, {tw[4], tw[5]}};
  if (which == 0) ssr_bfly8_tw(v, w[0], w[1], w[2], ssr_tw_w8(w[0]));
  else ssr_fft_compute_tw<T, 9, 1, 8>(v, w);          // pass 1 of a 512-point plan: one radix-8 butterfly with table twiddles
  for (int q = 0; q < 8; ++q) { out[2 * q] = v[q].x; out[2 * q + 1] = v[q].y; }
}
extern "C" void fma_bfly8_f64(int which, const double* in, const double* tw, double* out) { bfly<double>(which, in, tw, out); }
extern "C" void fma_bfly8_f32(int which, const float* in, const float* tw, float* out) { bfly<float>(which, in, tw, out); }

// ---- the 2048-point transform of one wave: in / out [2048] complex, natural order.  paired: k_stft_wave's output order
template <typename T, bool SPLIT, bool PAIRED> static int tail2048(const T* in, T* out) {
  SsrTables<T> t;
  if (!ssr_build_tables<T>(SSR_W_N, t)) return -3;
  std::vector<double> lds(SsrWaveLds<T, SPLIT>::bytes() / sizeof(double) + 1);
  SsrWaveLds<T, SPLIT> L(reinterpret_cast<char*>(lds.data()));
  const SsrView<cx<T>> vt(t.tw.data(), SSR_W_N + SSR_W_TWP);
  SsrBlk blk{SSR_W_L};
  const SsrBlk blk0 = blk;
  using Regs = SsrWaveRegs<T, false>;
  SSR_REGS(Regs, regs, blk);
  SSR_WPHASE(blk, regs, {
    for (int r = 0; r < SSR_W_P; ++r) R.v[r] = {in[2 * (tid + 64 * r)], in[2 * (tid + 64 * r) + 1]};
    ssr_dft32(R.v);
  });
#define VT vt
  if constexpr (PAIRED) { SSR_W_FFT_TAIL_PAIRED(blk, blk0, regs, L); } else { SSR_W_FFT_TAIL(blk, blk0, regs, L, ); }
#undef VT
  SSR_WPHASE(blk, regs, {
    const int jp[4] = {tid, 64 + tid, 192 - tid, ssr_wave_pj3(tid)};
    for (int b = 0; b < 4; ++b) for (int q = 0; q < 8; ++q) {
      const int k = (PAIRED ? jp[b] : tid + 64 * b) + 256 * q;
      out[2 * k] = R.v[8 * b + q].x; out[2 * k + 1] = R.v[8 * b + q].y;
    }
  });
  return 0;
}

// ---- the 1536-point transform of one wave (ssr_fft24.h)
template <typename T> static int tail1536(const T* in, T* out) {
  SsrTables<T> t;
  if (!ssr_build_tables_for<T>(2229, ssr_pick_wave_engine(2229), t) || t.eng.m != SSR_W24_N) return -3;
  std::vector<T> ex(SSR_W24_PN);
  SsrWaveBuf<T> L{ex.data(), ex.data()};
  const SsrView<cx<T>> vt(t.tw.data(), SSR_W24_N + SSR_W24_TWP);
  SsrBlk blk{SSR_W_L};
  const SsrBlk blk0 = blk;
  using Regs = SsrRnWaveRegs<T, false, 3, 24>;
  SSR_REGS(Regs, regs, blk);
  SSR_WPHASE(blk, regs, {
    for (int r = 0; r < SSR_W24_P; ++r) R.v[r] = {in[2 * (tid + 64 * r)], in[2 * (tid + 64 * r) + 1]};
    ssr_dft24(R.v);
  });
#define VT vt
  SSR_W24_FFT_TAIL(blk, blk0, regs, L, );
#undef VT
  SSR_WPHASE(blk, regs, {
    for (int b = 0; b < 3; ++b) for (int m = 0; m < 8; ++m) {
      const int k = tid + 64 * b + 192 * m;
      out[2 * k] = R.v[8 * b + m].x; out[2 * k + 1] = R.v[8 * b + m].y;
    }
  });
  return 0;
}

// n: 2048 or 1536; mode (2048 only): 0 = split exchange, 1 = full exchange, 2 = split exchange with the paired output order
extern "C" int fma_tail_f64(int n, int mode, const double* in, double* out) {
  if (n == SSR_W24_N) return tail1536<double>(in, out);
  if (n != SSR_W_N) return -2;
  return mode == 0 ? tail2048<double, true, false>(in, out) : mode == 1 ? tail2048<double, false, false>(in, out)
                                                                       : tail2048<double, true, true>(in, out);
}
extern "C" int fma_tail_f32(int n, int mode, const float* in, float* out) {
  if (n == SSR_W24_N) return tail1536<float>(in, out);
  if (n != SSR_W_N) return -2;
  return mode == 0 ? tail2048<float, true, false>(in, out) : mode == 1 ? tail2048<float, false, false>(in, out)
                                                                      : tail2048<float, true, true>(in, out);
}
