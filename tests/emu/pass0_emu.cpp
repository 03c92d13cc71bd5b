// Host emulation of k_stft_wave's first pass for tests/test_pass0_host.py: the windowed in-register radix-32 DFT ssr_dft32_win next
// to the sequence it replaces (window, then ssr_dft32), and the whole windowed 2048-point transform of one wave in natural order.
// Test infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libpass0_emu.so pass0_emu.cpp
#define SSR_HOST_EMU 1
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_tables.h"
#include "../../ssr_eval_amd/csrc/ssr_stft_wave.h"

// which = 0: ssr_dft32_win;  1: window (w[r + 16] = 1/2 - wl[r]), then ssr_dft32 - the parent's pass 0
template <typename T> static void pass0(int which, cx<T>* v, const float* pa, const float* pb, const T* wl) {
  if (which == 0) {
    ssr_dft32_win(v, pa, pb, wl);
  } else {
    for (int r = 0; r < SSR_W_P; ++r) {
      const T w = (r < SSR_W_P / 2) ? wl[r] : (T)0.5 - wl[r - SSR_W_P / 2];
      v[r] = {(T)pa[r] * w, (T)pb[r] * w};
    }
    ssr_dft32(v);
  }
}

// ---- one lane: pa, pb [32] samples, wl [16] half-window values -> out [32] complex (interleaved), out[k] = DFT32(x w)[k]
template <typename T> static void dft32(int which, const float* pa, const float* pb, const T* wl, T* out) {
  cx<T> v[SSR_W_P];
  pass0<T>(which, v, pa, pb, wl);
  for (int rho = 0; rho < SSR_W_P; ++rho) { out[2 * ssr_dft32_freq(rho)] = v[rho].x; out[2 * ssr_dft32_freq(rho) + 1] = v[rho].y; }
}
extern "C" void pass0_dft32_f64(int which, const float* pa, const float* pb, const double* wl, double* out) { dft32<double>(which, pa, pb, wl, out); }
extern "C" void pass0_dft32_f32(int which, const float* pa, const float* pb, const float* wl, float* out) { dft32<float>(which, pa, pb, wl, out); }

// ---- the windowed 2048-point transform of one wave (split exchange, paired output order: k_stft_wave's): a, b [2048] samples
// -> out [2048] complex of FFT((a + i b) w_h), natural order; win [2048]: the half window w_h that pass 0 multiplied by (which = 0: formed
// per lane by ssr_window_from_lane, which = 1: the plan's table)
template <typename T> static int frame2048(int which, const float* a, const float* b, T* out, T* win) {
  SsrTables<T> t;
  if (!ssr_build_tables<T>(SSR_W_N, t)) return -3;
  for (int l = 0; l < SSR_W_L; ++l) {
    T wl[SSR_W_P / 2];
    ssr_window_from_lane(wl, t.tw[SSR_W_N + SSR_W_WCS_OFF + l]);
    for (int r = 0; r < SSR_W_P / 2; ++r) {
      win[l + 64 * r] = which == 0 ? wl[r] : t.window_h[l + 64 * r];
      win[SSR_W_N / 2 + l + 64 * r] = (T)0.5 - win[l + 64 * r];
    }
  }
  std::vector<double> lds(SsrWaveLds<T, true>::bytes() / sizeof(double) + 1);
  SsrWaveLds<T, true> L(reinterpret_cast<char*>(lds.data()));
  constexpr bool SPLIT = true;
  const SsrView<cx<T>> vt(t.tw.data(), SSR_W_N + SSR_W_TWP);
  SsrBlk blk{SSR_W_L};
  const SsrBlk blk0 = blk;
  using Regs = SsrWaveRegs<T, false>;
  SSR_REGS(Regs, regs, blk);
#define VT vt
  SSR_WPHASE(blk, regs, {
    for (int r = 0; r < SSR_W_P; ++r) { R.pa[r] = a[tid + 64 * r]; R.pb[r] = b[tid + 64 * r]; }
    T wl[SSR_W_P / 2];
    if (which == 0) ssr_window_from_lane(wl, t.tw[SSR_W_N + SSR_W_WCS_OFF + tid]);          // as the kernel forms them
    else for (int r = 0; r < SSR_W_P / 2; ++r) wl[r] = t.window_h[tid + 64 * r];   // the parent: from the plan's table
    pass0<T>(which, R.v, R.pa, R.pb, wl);
    SSR_W_LOAD_TW1;
  });
  SSR_W_FFT_TAIL_PAIRED_EARLY(blk, blk0, regs, L);
#undef VT
  SSR_WPHASE(blk, regs, {
    const int jp[4] = {tid, 64 + tid, 192 - tid, ssr_wave_pj3(tid)};
    for (int bb = 0; bb < 4; ++bb) for (int q = 0; q < 8; ++q) {
      const int k = jp[bb] + 256 * q;
      out[2 * k] = R.v[8 * bb + q].x; out[2 * k + 1] = R.v[8 * bb + q].y;
    }
  });
  return 0;
}
extern "C" int pass0_frame_f64(int which, const float* a, const float* b, double* out, double* win) { return frame2048<double>(which, a, b, out, win); }
extern "C" int pass0_frame_f32(int which, const float* a, const float* b, float* out, float* win) { return frame2048<float>(which, a, b, out, win); }
