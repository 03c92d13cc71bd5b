// Kernel body K1-K4, wave-autonomous engine: the 2048-point pair STFT + fused LSD / SISpec epilogue with ONE WAVE PER
// FRAME and no workgroup barrier anywhere.
//
// Why: the 256-thread engine of ssr_stft.h runs a frame on four waves in lock step - eight s_barrier per frame (14 % of
// the kernel, measured), three LDS exchanges, and four waves that all stall together.  Here a frame belongs to one wave:
//   * 64 lanes x 32 points.  The first pass is a radix-32 DFT done entirely IN the lane's registers (4 x 8 with
//     compile-time twiddles), so the transform is 32 x 8 x 8 = three passes and only TWO exchanges through LDS; k_stft_wave
//     folds the window into its first radix-4 layer and the inner twiddles into its radix-8 butterflies (ssr_dft32_win);
//   * exchanges are ordered by the hardware (the DS operations of one wave execute in order), so a "phase boundary" is a
//     compiler-only wave-scope fence: no s_barrier, no s_waitcnt between a wave's writes and its reads;
//   * what a lane needs every frame is loop-invariant: its 16 window values (w[m + N/2] = 1/2 - w[m]; k_stft_wave forms them
//     from two per-lane constants, ssr_window_from_lane) and the 3 twiddles of the second pass (t, t^2, t^4 of t = w^(8 (l mod 32)), which does not
//     depend on the butterfly); the first pass needs none.  Only the third pass loads 3 table twiddles per butterfly.
//     Both radix-8 passes run the twiddles INSIDE the butterfly (ssr_bfly8_tw: three layers of fused radix-2 butterflies);
//   * the per-frame LSD reduction is a wave shuffle, the silent-frame vote a ballot.
// Occupancy is bounded by LDS, not by registers: one wave owns one 2048-point buffer (33 KB float64: 4 waves per CU, one
// per SIMD, up to 512 VGPRs each) - or, with the re / im parts exchanged one after the other through a single array
// (SPLIT = true), 17 KB: 8 waves per CU at <= 256 VGPRs.
//
// Arithmetic (window, two-for-one packing, separation, magnitudes, metric terms) is the one of ssr_stft.h; the parity
// tests run both engines against the oracle and against each other.  Reference semantics: ssr_eval/metrics.py:26-30,
// 109-121 (see ssr_stft.h).
#pragma once
#include "ssr_stft.h"

// (SSR_WPHASE / SSR_WAVE_SYNC: ssr_block.h)

constexpr int SSR_W_N = 2048, SSR_W_L = 64, SSR_W_P = 32;     // points, lanes, points per lane
constexpr int SSR_W_WCS_OFF = 7 * 32 + 12 * 64;               // lane-ordered twiddle copies behind the table, then the 64 window constants
constexpr int SSR_W_TWP = SSR_W_WCS_OFF + 64;                 // (= SSR_WAVE_WCS_OFF, SSR_WAVE_TWP of ssr_tables.h: tu_stft.inc asserts it)
SSR_DEV int ssr_wpad(int i) { return i + (i >> 5); }            // lane stride 32 -> 33 doubles: conflict-free ds_*_b64
constexpr int SSR_W_PN = SSR_W_N + (SSR_W_N >> 5) + 1;

// exp(-2 pi i m / 32), m = 0..21 (the exponents n2 * k1 of the in-lane 4 x 8 decomposition)
template <typename T> SSR_DEV cx<T> ssr_w32(int m) {
  constexpr double c[22] = {1.0, 0.98078528040323044913, 0.92387953251128675613, 0.83146961230254523708, 0.70710678118654752440,
                            0.55557023301960222474, 0.38268343236508977173, 0.19509032201612826785, 0.0,
                            -0.19509032201612826785, -0.38268343236508977173, -0.55557023301960222474, -0.70710678118654752440,
                            -0.83146961230254523708, -0.92387953251128675613, -0.98078528040323044913, -1.0,
                            -0.98078528040323044913, -0.92387953251128675613, -0.83146961230254523708, -0.70710678118654752440,
                            -0.55557023301960222474};
  constexpr double s[22] = {0.0, -0.19509032201612826785, -0.38268343236508977173, -0.55557023301960222474, -0.70710678118654752440,
                            -0.83146961230254523708, -0.92387953251128675613, -0.98078528040323044913, -1.0,
                            -0.98078528040323044913, -0.92387953251128675613, -0.83146961230254523708, -0.70710678118654752440,
                            -0.55557023301960222474, -0.38268343236508977173, -0.19509032201612826785, 0.0,
                            0.19509032201612826785, 0.38268343236508977173, 0.55557023301960222474, 0.70710678118654752440,
                            0.83146961230254523708};
  return {(T)c[m], (T)s[m]};
}

// v[r], r = 8 n1 + n2  (n1 < 4, n2 < 8)   ->   v[8 k1 + k2] = DFT32(v)[k1 + 4 k2]      (in place, registers only)
// NZ: only v[0 .. NZ) can be non-zero (a zero-padded Bluestein input: NZ = 12 or 16 rows of 64 samples); the first
// radix-4 stage then skips the additions of zeros - the same values, 96 fewer instructions at NZ = 12.
template <typename T, int NZ = 32> SSR_DEV void ssr_dft32(cx<T>* v) {
  const T h = (T)0.70710678118654752440;
  static_assert(NZ == 32 || (NZ > 8 && NZ <= 16), "full, or two non-zero row groups");
  SSR_UNROLL for (int n2 = 0; n2 < 8; ++n2) {
    cx<T> t[4] = {v[n2], v[8 + n2], v[16 + n2], v[24 + n2]};
    if (NZ == 32) {
      ssr_bfly4(t);
    } else if (8 + n2 < NZ) {                       // t[2] = t[3] = 0
      const cx<T> r = cmul_negi(t[1]);
      t[2] = csub(t[0], t[1]); t[3] = csub(t[0], r);
      t[1] = cadd(t[0], r);    t[0] = cadd(t[0], v[8 + n2]);
    } else {                                        // only t[0]
      t[1] = t[0]; t[2] = t[0]; t[3] = t[0];
    }
    SSR_UNROLL for (int k1 = 0; k1 < 4; ++k1) {
      const int m = n2 * k1;                       // compile-time after unrolling: the special angles cost no multiply
      cx<T> x = t[k1];
      if (m == 0) {
      } else if (m == 8) {
        x = cmul_negi(x);
      } else if (m == 16) {
        x = {-x.x, -x.y};
      } else if (m == 4) {
        x = {h * (x.x + x.y), h * (x.y - x.x)};
      } else if (m == 12) {
        x = {h * (x.y - x.x), -h * (x.x + x.y)};
      } else if (m == 20) {
        x = {-h * (x.x + x.y), h * (x.x - x.y)};
      } else {
        x = cmul(x, ssr_w32<T>(m));
      }
      v[8 * k1 + n2] = x;
    }
  }
  SSR_UNROLL for (int k1 = 0; k1 < 4; ++k1) ssr_bfly8(v + 8 * k1);
}

// Radix-2 butterfly with the COMPILE-TIME twiddle W = W32^M on the second input:  a, b  <-  a + W b,  a - W b.
// W = -i (M = 8, the only trivial one among the exponents in use) is plain additions, selected on the exponent: an fma with a literal
// 0 or 1 does not fold without fast-math; every other exponent is ssr_bfly2_tw with literal operands.
template <int M, typename T> SSR_DEV void ssr_bfly2_w32(cx<T>& a, cx<T>& b) {
  static_assert(M > 0 && M < 16, "the exponents of ssr_bfly8_w32<1..3> are 1..15 (ssr_w32 holds 0..21)");
  if constexpr (M == 8) { const cx<T> r = cmul_negi(b); const cx<T> p = cadd(a, r); b = csub(a, r); a = p; }
  else ssr_bfly2_tw(a, b, ssr_w32<T>(M));
}
// ssr_bfly8_tw (ssr_fft.h) with the compile-time base twiddle t = W32^K1:  t^4, t^2, -i t^2, t, -i t, s = t W8, -i s
template <int K1, typename T> SSR_DEV void ssr_bfly8_w32(cx<T>* v) {
  cx<T> a0 = v[0], a1 = v[1], a2 = v[2], a3 = v[3], b0 = v[4], b1 = v[5], b2 = v[6], b3 = v[7];
  ssr_bfly2_w32<4 * K1>(a0, b0);
  ssr_bfly2_w32<4 * K1>(a1, b1);
  ssr_bfly2_w32<4 * K1>(a2, b2);
  ssr_bfly2_w32<4 * K1>(a3, b3);
  ssr_bfly2_w32<2 * K1>(a0, a2);          // c0, d0
  ssr_bfly2_w32<2 * K1>(a1, a3);          // c1, d1
  ssr_bfly2_w32<2 * K1 + 8>(b0, b2);      // e0, f0
  ssr_bfly2_w32<2 * K1 + 8>(b1, b3);      // e1, f1
  ssr_bfly2_w32<K1>(a0, a1);              // X0, X4
  ssr_bfly2_w32<K1 + 8>(a2, a3);          // X2, X6
  ssr_bfly2_w32<K1 + 4>(b0, b1);          // X1, X5
  ssr_bfly2_w32<K1 + 12>(b2, b3);         // X3, X7
  v[0] = a0; v[1] = b0; v[2] = a2; v[3] = b2; v[4] = a1; v[5] = b1; v[6] = a3; v[7] = b3;
}
// Lane l's 16 half-window values 0.5 hann[l + 64 r] = 1/4 - 1/4 cos(a_l + 2 pi r / 32) = 1/4 - (CA cos_r - SA sin_r), r < 16, from
// cs = (CA, SA) = (cos, sin)(a_l) / 4, a_l = 2 pi l / N (ssr_tables.h, long double) and the compile-time (cos_r, sin_r): two fused
// multiply-adds each, within 3 ulp of 1/4 of the exact value (two roundings below 1/2, the roundings of CA, SA, cos_r, sin_r; the
// table's values are within 1/2 ulp of THEIR size).  k_stft_wave computes them every frame instead of loading them: 16 vector-memory
// instructions per frame pair less on the CU-shared address unit, 30 FP64 instructions more on the SIMD's own pipe.
template <typename T> SSR_DEV void ssr_window_from_lane(T* wl, cx<T> cs) {
  SSR_UNROLL for (int r = 0; r < SSR_W_P / 2; ++r) {
    const cx<T> e = ssr_w32<T>(r);                     // (cos_r, -sin_r)
    if (r == 0) wl[r] = (T)0.25 - cs.x;
    else if (r == 8) wl[r] = (T)0.25 + cs.y;
    else wl[r] = ssr_fma(-cs.y, e.y, ssr_fma(-cs.x, e.x, (T)0.25));
  }
}
// ssr_dft32 of the WINDOWED packed frame v[r] = (pa[r] + i pb[r]) w[r], w[r] = wl[r] (r < 16), 1/2 - wl[r - 16] (r >= 16), with the
// window folded into the first radix-4 layer (t0 +- t2 = fma(+-x2, w2, x0 w0): 4 multiplies + 4 fused multiply-adds where the
// separate window pass costs 8 multiplies + 4 additions) and the inner twiddles W32^(n2 k1) folded into the radix-8 butterflies
// (ssr_bfly8_w32; k1 = 0 has none: ssr_bfly8).  The same register order as ssr_dft32 on exit.
// Two halves, so that a caller can issue work between them: once the first layer is done pa / pb / wl are dead (k_stft_wave requests
// the next pass's table values there).
template <typename T> SSR_DEV void ssr_dft32_win_layer1(cx<T>* v, const float* pa, const float* pb, const T* wl) {
  SSR_UNROLL for (int n2 = 0; n2 < 8; ++n2) {
    const T w0 = wl[n2], w1 = wl[8 + n2], w2 = (T)0.5 - w0, w3 = (T)0.5 - w1;              // w[m + N/2] = 1/2 - w[m]
    const cx<T> x2 = {(T)pa[16 + n2], (T)pb[16 + n2]}, x3 = {(T)pa[24 + n2], (T)pb[24 + n2]};
    const cx<T> t0 = {(T)pa[n2] * w0, (T)pb[n2] * w0}, t1 = {(T)pa[8 + n2] * w1, (T)pb[8 + n2] * w1};
    const cx<T> b0 = {ssr_fma(x2.x, w2, t0.x), ssr_fma(x2.y, w2, t0.y)};
    const cx<T> b1 = {ssr_fma(-x2.x, w2, t0.x), ssr_fma(-x2.y, w2, t0.y)};
    const cx<T> b2 = {ssr_fma(x3.x, w3, t1.x), ssr_fma(x3.y, w3, t1.y)};
    const cx<T> b3 = cmul_negi(cx<T>{ssr_fma(-x3.x, w3, t1.x), ssr_fma(-x3.y, w3, t1.y)});
    v[n2] = cadd(b0, b2); v[8 + n2] = cadd(b1, b3); v[16 + n2] = csub(b0, b2); v[24 + n2] = csub(b1, b3);
  }
}
template <typename T> SSR_DEV void ssr_dft32_win_rest(cx<T>* v) {
  ssr_bfly8(v);
  ssr_bfly8_w32<1>(v + 8);
  ssr_bfly8_w32<2>(v + 16);
  ssr_bfly8_w32<3>(v + 24);
}
template <typename T> SSR_DEV void ssr_dft32_win(cx<T>* v, const float* pa, const float* pb, const T* wl) {
  ssr_dft32_win_layer1(v, pa, pb, wl);
  ssr_dft32_win_rest(v);
}
// frequency held by register rho after ssr_dft32
SSR_DEV constexpr int ssr_dft32_freq(int rho) { return (rho >> 3) + 4 * (rho & 7); }

struct SsrTrue { static constexpr bool value = true; };
struct SsrFalse { static constexpr bool value = false; };

template <typename T, bool SUMS> struct SsrWaveRegs {
  cx<T> v[SSR_W_P];          // the lane's 32 points
  T tx[SSR_W_P];             // SPLIT exchange: real parts read back while the imaginary parts are still to be written
  float pa[SSR_W_P], pb[SSR_W_P];   // samples of the NEXT frame, requested one frame ahead
  cx<T> wcs;                 // (cos, sin)(2 pi tid / N) / 4, loaded once per chunk: the lane's window values come from it (ssr_window_from_lane)
  cx<T> tw1[3];              // t, t^2, t^4 of t = w^(8 (tid mod 32)): requested while the first exchange is in flight (k_stft_wave: in
                             // pass 0, behind its first layer)
  cx<T> tw2[12];             // w^j, w^2j, w^4j of the four third-pass butterflies: requested while the second one is (k_stft_wave: at
                             // the top of pass 1)
  double lsd_total;          // lane 0: sum over the chunk's frames of the per-frame LSD
  // STASH (ssr_stft_wave_body): frame `it` of a chunk belongs to lane it & 63, which holds what lane 0 used to finish frame by
  // frame until the next flush - the frame's wave sum of LSD terms without the Nyquist bin's, and the frame's Z[1024]
  double lsd_frame;
  cx<T> nyq;
};

template <typename T, bool SPLIT> struct SsrWaveLds {
  // scratch first (doubles), then the exchange array(s)
  static constexpr size_t bytes() { return sizeof(double) * 4 + sizeof(int) * 8 + sizeof(T) * (SPLIT ? 1 : 2) * SSR_W_PN; }
  double* sc1; int* nz; T* re; T* im;
  SSR_MEMBER explicit SsrWaveLds(char* base) {
    sc1 = reinterpret_cast<double*>(base);
    nz = reinterpret_cast<int*>(sc1 + 4);           // [2 signals][2 flag sets]
    re = reinterpret_cast<T*>(nz + 8);
    im = SPLIT ? re : re + SSR_W_PN;
  }
  SSR_MEMBER bool nonzero(int which, int par) const {
    int f = nz[which * 2 + par];
#ifndef SSR_HOST_EMU
    f = __builtin_amdgcn_readfirstlane(f);
#endif
    return f != 0;
  }
};

// a wave's exchange array(s) inside a workgroup of several autonomous waves (ssr_stft_rn_wave.h, ssr_lowpass_group.h)
template <typename T> struct SsrWaveBuf { T* re; T* im; };

// LDS of one k_stft_wave wave.  The six SISpec / log-SISpec running sums of a lane live behind the exchange array (6 x 64
// float64 = 3 KB: 16,968 + 3,072 B still makes eight waves per CU) and are updated with ds_add_f64 - as registers they
// were twelve more than the variant had (11 spilled to scratch: 0.9 GB of scratch traffic per launch).
// (offset of the accumulators: the float32 engine's arrays end on a 4-byte boundary, ds_add_f64 needs 8)
template <typename T, bool SPLIT> constexpr size_t ssr_stft_wave_sums_offset() { return (SsrWaveLds<T, SPLIT>::bytes() + 7) & ~(size_t)7; }
template <typename T, bool SPLIT, bool SUMS> constexpr size_t ssr_stft_wave_lds_bytes() {
  return SUMS ? ssr_stft_wave_sums_offset<T, SPLIT>() + 6 * 64 * sizeof(double) : SsrWaveLds<T, SPLIT>::bytes();
}

// LDS slots as (per-lane base) + (compile-time offset): the offsets fold into the DS instructions' immediate fields.
//  after pass 0 : register rho = frequency q = ssr_dft32_freq(rho) of sub-transform `tid` -> slot 32 tid + q, padded 33 tid + q
//  radix-8 load : register 8 b + q = input q of butterfly j = tid + 64 b -> slot j + 256 q, padded tid + tid/32 + 66 b + 264 q
//  after pass 1 : output q of butterfly j -> slot (j - k) 8 + k + 32 q, k = j mod 32,
//                 padded 264 (tid/32) + tid mod 32 + 528 b + 33 q
struct SsrWaveBase { int st0, ld8, st1; };
SSR_DEV SsrWaveBase ssr_wave_bases(int tid) {
  return {33 * tid, tid + (tid >> 5), 264 * (tid >> 5) + (tid & 31)};
}
SSR_DEV constexpr int ssr_w_off_st0(int i) { return ssr_dft32_freq(i); }
SSR_DEV constexpr int ssr_w_off_ld8(int i) { return 66 * (i >> 3) + 264 * (i & 7); }
SSR_DEV constexpr int ssr_w_off_st1(int i) { return 528 * (i >> 3) + 33 * (i & 7); }

// One exchange through LDS: R.v[i] goes to slot WB + WO(i), then R.v[i] is reloaded from slot RB + RO(i).
// SPLIT: real parts first, imaginary parts second, through the same array.
// EXTRA: statements issued right after the (first) write phase - the table loads of the NEXT pass: the registers of the
// values just written are free at that point, and the loads' latency overlaps the exchange.
// (the read side as (per-lane bases RBASES(lane), index RIDX(bases, i)): SSR_W_EXCHANGE reads slot RB + RO(i); the paired
// second exchange of k_stft_wave reads each butterfly's inputs from its own per-lane base)
#define SSR_W_EXCHANGE_G(blk, regs, L, WB, WO, RBASES, RIDX, EXTRA)                                       \
  if constexpr (!SPLIT) {                                                                                 \
    SSR_WPHASE(blk, regs, { const int w_ = ssr_wave_bases(tid & 63).WB;                                        \
      SSR_UNROLL for (int i = 0; i < SSR_W_P; ++i) { (L).re[w_ + WO(i)] = R.v[i].x; (L).im[w_ + WO(i)] = R.v[i].y; } }); \
    SSR_WPHASE(blk, regs, { SSR_SCHED_BARRIER(); EXTRA; const auto r_ = RBASES(tid & 63);                    \
      SSR_UNROLL for (int i = 0; i < SSR_W_P; ++i) R.v[i] = {(L).re[RIDX(r_, i)], (L).im[RIDX(r_, i)]}; });   \
  } else {                                                                                                \
    SSR_WPHASE(blk, regs, { const int w_ = ssr_wave_bases(tid & 63).WB;                                        \
      SSR_UNROLL for (int i = 0; i < SSR_W_P; ++i) (L).re[w_ + WO(i)] = R.v[i].x; });                     \
    SSR_WPHASE(blk, regs, { SSR_SCHED_BARRIER(); EXTRA; const auto r_ = RBASES(tid & 63);                    \
      SSR_UNROLL for (int i = 0; i < SSR_W_P; ++i) R.tx[i] = (L).re[RIDX(r_, i)]; });                     \
    SSR_WPHASE(blk, regs, { const int w_ = ssr_wave_bases(tid & 63).WB;                                        \
      SSR_UNROLL for (int i = 0; i < SSR_W_P; ++i) (L).re[w_ + WO(i)] = R.v[i].y; });                     \
    SSR_WPHASE(blk, regs, { const auto r_ = RBASES(tid & 63);                                                \
      SSR_UNROLL for (int i = 0; i < SSR_W_P; ++i) R.v[i] = {R.tx[i], (L).re[RIDX(r_, i)]}; });           \
  }
#define SSR_W_RIDX_LD8(b_, i) ((b_).ld8 + ssr_w_off_ld8(i))
#define SSR_W_EXCHANGE(blk, regs, L, WB, WO, RB, RO, EXTRA) SSR_W_EXCHANGE_G(blk, regs, L, WB, WO, ssr_wave_bases, SSR_W_RIDX_##RB##_##RO, EXTRA)
#define SSR_W_RIDX_ld8_ssr_w_off_ld8(b_, i) SSR_W_RIDX_LD8(b_, i)

// ---- PAIRED output order (k_stft_wave, round 6): the third pass's butterfly j emits Z[j + 256 q] and a bin's partner
// Z[2048 - k] = Z[(256 - j) + 256 (7 - q)] comes out of butterfly 256 - j.  A lane that runs BOTH butterflies of such a pair holds
// every (k, 2048 - k) couple it needs in its own registers: the upper halves no longer cross lanes through LDS (one exchange
// of 32 stores + 32 loads and one dependent LDS round trip per frame pair less; the same arithmetic on the same operands:
// magnitudes bit-identical to the ascending order).  Lane l runs j = l, 64 + l, 192 - l, 256 - l (registers 8 b + q, b = 0..3);
// j = 0 and j = 128 pair with themselves and both sit in lane 0, whose four butterflies are 0, 64, 192, 128.
//   partner of register (b, q), q < 4:  lane > 0: (3 - b, 7 - q);   lane 0: b = 0 -> (0, 8 - q) (q = 0: itself, q = 4: Nyquist,
//   itself), b = 3 -> (3, 7 - q), b = 1 <-> 2 as everywhere.
struct SsrWavePBase { int ld8, p2, p3; };
SSR_DEV int ssr_wave_pj3(int tid) { return tid == 0 ? 128 : 256 - tid; }
SSR_DEV SsrWavePBase ssr_wave_pbases(int tid) {
  return {tid + (tid >> 5), ssr_wpad(192 - tid), ssr_wpad(ssr_wave_pj3(tid))};
}
SSR_DEV int ssr_w_rd_paired(const SsrWavePBase& B, int i) {
  const int b = i >> 3, q = i & 7;
  return (b == 0 ? B.ld8 : b == 1 ? B.ld8 + 66 : b == 2 ? B.p2 : B.p3) + 264 * q;
}
#define SSR_W_RIDX_PAIRED(b_, i) ssr_w_rd_paired(b_, i)
// the lane-ordered copies [N + 224 + 64 (3 b + m) + l] = w^((l + 64 b) 2^m): butterfly 192 - l is copy b = 2 at lane 64 - l
// (lane 0: copy 3, lane 0), butterfly 256 - l copy b = 3 at lane 64 - l (lane 0, j = 128: copy 2, lane 0)
#define SSR_W_LOAD_TW2_PAIRED { const int t_ = tid & 63; const unsigned l_ = SSR_UIDX(t_);                       \
    const unsigned o2_ = SSR_UIDX(t_ == 0 ? 192 : 64 - t_); const unsigned o3_ = SSR_UIDX(t_ == 0 ? -192 : 64 - t_); \
    SSR_UNROLL for (int i = 0; i < 6; ++i) R.tw2[i] = VT.at(l_ + (SSR_W_N + 224 + 64 * i));                       \
    SSR_UNROLL for (int i = 6; i < 9; ++i) R.tw2[i] = VT.at(o2_ + (SSR_W_N + 224 + 64 * i));                      \
    SSR_UNROLL for (int i = 9; i < 12; ++i) R.tw2[i] = VT.at(o3_ + (SSR_W_N + 224 + 64 * i)); }

// The rest of the transform after the in-register radix-32 pass (ssr_dft32 applied to R.v): exchange, radix-8 pass with the
// lane's three twiddles, exchange, radix-8 pass with table twiddles.  On exit register 8 b + q holds Z[tid + 64 b + 256 q].
// BLK0: the untouched block descriptor (a fresh opaque lane index per stage: addresses are formed where they are used).
// The lane index is `tid & 63` throughout: a workgroup of several autonomous waves (ssr_stft_rn_wave.h) passes an L whose
// arrays are the calling wave's own.
// EXTRA2: further table loads to issue with the last pass's twiddles (the low-pass kernel's synthesis window).
// (VT: a view of the plan's twiddle table INCLUDING the lane-ordered copies behind it, SSR_W_N + SSR_W_TWP entries -
// ssr_tables.h: every load below is one contiguous run of 32 / 64 table entries)
#define SSR_W_LOAD_TW1 { const unsigned l_ = SSR_UIDX(tid & 31); \
                         SSR_UNROLL for (int m = 0; m < 3; ++m) R.tw1[m] = VT.at(l_ + (SSR_W_N + 32 * ((1 << m) - 1))); }
#define SSR_W_LOAD_TW2 { const unsigned l_ = SSR_UIDX(tid & 63); \
                         SSR_UNROLL for (int i = 0; i < 12; ++i) R.tw2[i] = VT.at(l_ + (SSR_W_N + 224 + 64 * i)); }
#define SSR_W_FFT_TAIL(blk, BLK0, regs, L, EXTRA2)                                                                        \
  SSR_W_FFT_TAIL_X(blk, BLK0, regs, L, SSR_W_LOAD_TW1, , SSR_W_EXCHANGE(blk, regs, L, st1, ssr_w_off_st1, ld8, ssr_w_off_ld8, SSR_W_LOAD_TW2 EXTRA2))
#define SSR_W_FFT_TAIL_PAIRED(blk, BLK0, regs, L)                                                                         \
  SSR_W_FFT_TAIL_X(blk, BLK0, regs, L, SSR_W_LOAD_TW1, , SSR_W_EXCHANGE_G(blk, regs, L, st1, ssr_w_off_st1, ssr_wave_pbases, SSR_W_RIDX_PAIRED, SSR_W_LOAD_TW2_PAIRED))
// The paired tail with both table requests A WHOLE PASS ahead of their waits (k_stft_wave): R.tw1 is requested by the CALLER's pass 0,
// once its first layer has consumed the prefetched samples (64 registers free), R.tw2 at the top of pass 1 (the 64
// registers of R.tx are dead from the end of the first exchange to the second one's first read).  Requested inside the exchanges
// (SSR_W_FFT_TAIL_PAIRED) the values are awaited some 65 instructions - nearly all of them DS operations - after they were asked for.
#define SSR_W_FFT_TAIL_PAIRED_EARLY(blk, BLK0, regs, L)                                                                   \
  SSR_W_FFT_TAIL_X(blk, BLK0, regs, L, , SSR_SCHED_BARRIER(); SSR_W_LOAD_TW2_PAIRED; SSR_SCHED_BARRIER(),                \
                    SSR_W_EXCHANGE_G(blk, regs, L, st1, ssr_w_off_st1, ssr_wave_pbases, SSR_W_RIDX_PAIRED, ))
// LOAD1: the request of R.tw1, issued in the first exchange (empty: the caller has requested it); EARLY2: statements at the top of
// pass 1 (the request of R.tw2, where EXCH2 does not make it)
#define SSR_W_FFT_TAIL_X(blk, BLK0, regs, L, LOAD1, EARLY2, EXCH2)                                                    \
  blk = BLK0; ssr_launder(blk);                                                                                       \
  SSR_W_EXCHANGE(blk, regs, L, st0, ssr_w_off_st0, ld8, ssr_w_off_ld8, LOAD1);                                        \
  /* pass 1: four radix-8 butterflies, base twiddle t = w^(8 (j mod 32)) - the same for every butterfly of the lane */\
  SSR_WPHASE(blk, regs, {                                                                                             \
    EARLY2;                                                                                                           \
    const cx<T> s1_ = ssr_tw_w8(R.tw1[0]);                                                                            \
    SSR_UNROLL for (int b = 0; b < 4; ++b) ssr_bfly8_tw(R.v + 8 * b, R.tw1[0], R.tw1[1], R.tw1[2], s1_);              \
  });                                                                                                                 \
  blk = BLK0; ssr_launder(blk);                                                                                       \
  EXCH2;                                                                                                              \
  /* pass 2: four radix-8 butterflies, base twiddle w^j, j = tid + 64 b: three table values each */                   \
  SSR_WPHASE(blk, regs, {                                                                                             \
    SSR_UNROLL for (int b = 0; b < 4; ++b)                                                                            \
      ssr_bfly8_tw(R.v + 8 * b, R.tw2[3 * b], R.tw2[3 * b + 1], R.tw2[3 * b + 2], ssr_tw_w8(R.tw2[3 * b]));           \
  });

// Request unit u's samples into the prefetch registers (branch-free, always valid addresses, reflection only at the ends).
// WHICH: 1 = the first signal's, 2 = the second's, 3 = both.  A wave can have 63 vector-memory instructions in flight (vmcnt is
// six bits); the 64th waits at issue for the oldest to return, so the body requests the two signals at different times.
template <typename T, int WHICH = 3, typename REGS>
SSR_DEV void ssr_wave_prefetch(const SsrStftParams<T>& p, REGS& R, int tid, const SsrView<float>& va, const SsrView<float>& vb,
                               int u, int n, int n_frames) {
  const int t_c = (u < n_frames) ? u : n_frames - 1;
  const int base = t_c * p.hop - SSR_W_N / 2;
  if (base >= 0 && base + SSR_W_N <= n) {            // wave-uniform: the frame lies fully inside the signal
    SSR_UNROLL for (int r = 0; r < SSR_W_P; ++r) {
      if (WHICH & 1) R.pa[r] = va.at(SSR_UIDX(tid + 64 * r), base);
      if (WHICH & 2) R.pb[r] = vb.at(SSR_UIDX(tid + 64 * r), base);
    }
  } else {
    SSR_UNROLL for (int r = 0; r < SSR_W_P; ++r) {
      const unsigned m = SSR_UIDX(ssr_reflect(base + tid + 64 * r, n));
      if (WHICH & 1) R.pa[r] = va.at(m);
      if (WHICH & 2) R.pb[r] = vb.at(m);
    }
  }
}

// Silent-frame votes of the unit whose samples sit in the prefetch registers, into flag set `par` (the body calls it at
// the top of the frame that consumes them; cf. ssr_stft_prefetched_flags).
template <typename REGS> SSR_DEV void ssr_wave_flags(REGS& R, int tid, int* nz, int par) {
  SSR_UNROLL for (int r = 0; r < SSR_W_P; ++r) { ssr_touch(R.pa[r]); ssr_touch(R.pb[r]); }
  unsigned ora = 0u, orb = 0u;
  SSR_UNROLL for (int r = 1; r < SSR_W_P; ++r) { ora |= ssr_mag_bits(R.pa[r]); orb |= ssr_mag_bits(R.pb[r]); }
  ora |= (tid == 0) ? 0u : ssr_mag_bits(R.pa[0]);    // sample m = 0 carries window weight exactly 0
  orb |= (tid == 0) ? 0u : ssr_mag_bits(R.pb[0]);
  SSR_WAVE_ANY_STORE(tid, ora != 0u, nz + par);
  SSR_WAVE_ANY_STORE(tid, orb != 0u, nz + 2 + par);
}

// ---- one-lane work taken out of the frame loop (STASH): lane 0's value for every lane, and wave sums that land in a register.
// Device: v_readfirstlane / a DPP sum handed to every lane by v_readlane (ssr_wave_sum_dpp).  Host emulation: the lanes of a phase run one after
// the other in ascending order, so lane 0 leaves its value in `slot` for the others, and a wave sum is complete only when the
// phase is over - it goes through LDS scratch and lands in a phase of its own (SSR_W_SUM_LAND; nothing on the device).
#ifdef SSR_HOST_EMU
template <typename V> SSR_DEV V ssr_wave_first(int tid, V v, V& slot) { if ((tid & 63) == 0) slot = v; return slot; }
// SSR_W_SUM(tid, val, sc, lane_ok, dst, OP), inside a phase, then SSR_W_SUM_LAND(blk, regs, cond, sc, lane_ok, dst, OP) right behind that
// phase with the same last four arguments: in the lanes where `lane_ok` holds, `dst OP (sum of val over the wave)` - OP is = or +=.
// The device does it in SSR_W_SUM and SSR_W_SUM_LAND is empty; the host sums into sc[0] in SSR_W_SUM and applies OP in SSR_W_SUM_LAND
// (where `cond` is the condition under which SSR_W_SUM was reached).
#define SSR_W_SUM(tid, val, sc, lane_ok, dst, OP) SSR_WAVE_SUM_STORE(tid, 64, val, sc)
#define SSR_W_SUM_LAND(blk, regs, cond, sc, lane_ok, dst, OP) SSR_WPHASE(blk, regs, if ((cond) && (lane_ok)) dst OP (sc)[0])
#else
SSR_DEV float ssr_wave_first(int, float v, float&) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
SSR_DEV double ssr_wave_first(int, double v, double&) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// The wave sum by data-parallel-primitive moves instead of ssr_wave_sum's six ds_bpermute round trips (each a dependent LDS access at
// the very end of a frame, with nothing left to cover it): an inclusive scan inside each row of 16 lanes (row_shr 1, 2, 4, 8, lanes
// without a source read 0), then lane 15 of rows 0 and 2 into rows 1 and 3 (row_bcast:15), then lane 31 into rows 2 and 3
// (row_bcast:31) - lane 63 holds the sum, and v_readlane hands it to every lane.  Two 32-bit moves and one addition per step.
template <int CTRL, int ROWS> SSR_DEV double ssr_wave_dpp(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, ROWS, 0xf, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, ROWS, 0xf, true);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
SSR_DEV double ssr_wave_sum_dpp(double v) {
  v += ssr_wave_dpp<0x111, 0xf>(v);
  v += ssr_wave_dpp<0x112, 0xf>(v);
  v += ssr_wave_dpp<0x114, 0xf>(v);
  v += ssr_wave_dpp<0x118, 0xf>(v);
  v += ssr_wave_dpp<0x142, 0xa>(v);
  v += ssr_wave_dpp<0x143, 0xc>(v);
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), 63);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
#define SSR_W_SUM(tid, val, sc, lane_ok, dst, OP) do { const double s_ = ssr_wave_sum_dpp(val); if (lane_ok) dst OP s_; } while (0)
#define SSR_W_SUM_LAND(blk, regs, cond, sc, lane_ok, dst, OP)
#endif

// log10(0 / e^2 + 1e-12)^2: the LSD term of a bin whose target magnitude is exactly 0 (log10 of float32 1e-12 is -12 to 2e-9)
constexpr double SSR_W_LSD_OF_ZERO = 144.0;

// grid = n_items * n_chunks workgroups of ONE wave; PAIR mode, direct 2048-point engine, float32 signals.
// MAG: 1 / 0 = magnitude rows are / are not written (p.out_kind == SSR_OUT_MAG known at compile time), -1 = decided at run time.
// STASH: what only lane 0 did in every frame - the float64 division and square root that close the previous frame's LSD, and the
// Nyquist bin Z[1024] with its two stores under a lane condition - is done once per 64 frames by all lanes at once.  Frame `it`
// belongs to lane it & 63: a frame leaves its wave sum of LSD terms (R.lsd_frame) and lane 0's register 4 (R.nyq) with its owner,
// and the FLUSH behind every block of 64 frames (and behind a chunk's last, shorter block) evaluates the 64 Nyquist bins, closes
// the 64 frames' LSD and stores column 1024 of the 64 rows, wave-uniformly.  The frame's LSD sum receives its Nyquist term last,
// and frame values are added by wave reduction: results move at round-off level, magnitude rows not at all.
// STASH = false is the frame-by-frame code (the host tests compare the two).  The float64 variants with running sums keep it: they
// stand at 256 VGPRs, and the stash's six more spill (7 and 13 registers, 32 and 48 B of scratch).
template <typename T, bool SUMS> constexpr bool ssr_stft_wave_stash() { return !(SUMS && sizeof(T) == 8); }
template <typename T, bool SUMS, bool SPLIT, int MAG = -1, bool STASH = ssr_stft_wave_stash<T, SUMS>(), typename BLK>
SSR_BODY void ssr_stft_wave_body(const SsrStftParams<T>& p, BLK& blk, int chunk, int item, char* lds_base) {
  constexpr int N = SSR_W_N, F = N / 2 + 1;
  // (the magnitude rows staged through LDS and stored as 16-byte writes instead - 136 -> 112 vector-memory instructions per frame
  // pair - measured the same time, 2.34 ms: the 0.5 ms the rows cost is not instruction count; profiles/r06_stft_wave_vmem_path.txt)
  using Regs = SsrWaveRegs<T, SUMS>;
  SsrWaveLds<T, SPLIT> L(lds_base);
  const int n = p.len[item], hop = p.hop;
  const int n_frames = ssr_num_frames_dev(n, N, hop);
  // Units of this chunk: u0, u0 + S, u0 + 2 S, ... (< u1).  S = 1: consecutive frames.  S > 1: the S chunks of a group
  // interleave over the group's span of S * units_per_chunk frames - they run at the same time on the same XCD (k_stft_wave's
  // block mapping), so the 75 % overlap of neighbouring frames is found in that XCD's L2 instead of being fetched again by the
  // same wave 13 us later, when it has long been evicted (2048 waves x 16 KB of live signal = the whole L2).
  const int S = p.interleave > 1 ? p.interleave : 1;
  const int span0 = (chunk / S) * S * p.units_per_chunk;
  const int u0 = span0 + chunk % S;
  const int u1 = (span0 + S * p.units_per_chunk < n_frames) ? span0 + S * p.units_per_chunk : n_frames;
  const float* sa = p.a + p.a_off[item];
  const float* sb = p.b + p.b_off[item];
  const int64_t row0 = p.frame_off[item];
  double* part = p.part ? p.part + ((int64_t)item * p.n_chunks + chunk) * SSR_NPART : nullptr;
  // the variant without running sums is only launched when no SISpec bit is set: say so, and their code disappears
  const int mask = SUMS ? p.metric_mask : (p.metric_mask & SSR_M_LSD);
  const bool want_lsd = mask & SSR_M_LSD;
  const SsrView<float> va(sa, n), vb(sb, n);
  const SsrView<cx<T>> vt(p.tw, N + SSR_W_TWP);

  double* lsum = reinterpret_cast<double*>(lds_base + ssr_stft_wave_sums_offset<T, SPLIT>());   // [6][64], SUMS only
  SSR_REGS(Regs, regs, blk);
  SSR_WPHASE(blk, regs, {
    R.lsd_total = 0.0;
    R.lsd_frame = 0.0; R.nyq = {(T)0, (T)0};
    if constexpr (SUMS) for (int q = 0; q < 6; ++q) lsum[64 * q + tid] = 0.0;
    if (tid == 0) L.sc1[0] = 0.0;
    if (u0 < u1) {
      ssr_wave_prefetch<T>(p, R, tid, va, vb, u0, n, n_frames);
      R.wcs = vt.at(SSR_UIDX(tid) + (SSR_W_N + SSR_W_WCS_OFF));
    }
    SSR_VMEM_DRAIN();
  });

  BLK blk0 = blk;
  const int64_t OP = p.out_pitch ? p.out_pitch : F;      // floats between output rows
  // STASH: blocks of 64 frames (units ub, ub + S, ... < ue; the chunk's frames it0 ...), a flush behind each.  Otherwise one block.
  for (int ub = u0, it0 = 0; ub < u1; it0 += 64) {
    const int ue = (STASH && ub + 64 * S < u1) ? ub + 64 * S : u1;
    // (only the host emulation's ssr_wave_first uses it: lane 0's register 4 on its way to the frame's owner)
    [[maybe_unused]] cx<T> nyq0 = {(T)0, (T)0};
    for (int u = ub, it = it0; u < ue; u += S, ++it) {
      // The lane's table values (twiddles) and addresses are loop-invariant, and 128 + 64 registers of data and
      // prefetched samples leave no room to keep them: with the lane index opaque the optimiser cannot hoist them out of the
      // loop (it would, and then shuffle some 250 values through the accumulator registers every frame).  Table values are
      // re-requested from L1 / L2 a pass before they are needed; LDS slots are four per-lane bases plus immediates.
      blk = blk0; ssr_launder(blk);
#define VT vt
      // ---- pass 0: window, radix-32 DFT in registers (Stockham pass with stride 1: no twiddle).  Without STASH lane 0 also closes the
      // previous frame's LSD.
      SSR_WPHASE(blk, regs, {
        ssr_wave_flags(R, tid, L.nz, it & 1);            // silent-frame votes of this unit, read by its epilogue
        // (lane 0's branch first: behind the transform it splits the phase, and the first layer sinks below the table request)
        if constexpr (!STASH) { if (want_lsd && it > 0 && tid == 0) R.lsd_total += sqrt(L.sc1[0] / (double)F); }
        T wl[SSR_W_P / 2];
        ssr_touch(R.wcs.x); ssr_touch(R.wcs.y);          // a product of this point: hoisted out of the loop the 64 window values spill
        ssr_window_from_lane(wl, R.wcs);
        ssr_dft32_win_layer1(R.v, R.pa, R.pb, wl);
        SSR_SCHED_BARRIER();                             // pa / pb are dead: pass 1's twiddles, a whole pass ahead of their wait
        SSR_W_LOAD_TW1;
        SSR_SCHED_BARRIER();
        ssr_dft32_win_rest(R.v);
      });
      SSR_W_FFT_TAIL_PAIRED_EARLY(blk, blk0, regs, L);
#undef VT
      // register 8 b + q holds Z[j_b + 256 q], j = tid, 64 + tid, 192 - tid, 256 - tid (lane 0: 0, 64, 192, 128) - every
      // partner Z[2048 - k] of the lane's bins is in the lane's own registers (see SSR_W_FFT_TAIL_PAIRED).

      // ---- epilogue: four groups of four bins (partner values in, magnitudes out per group: few registers live at once)
      blk = blk0; ssr_launder(blk);
      float* ra0 = p.out_a ? p.out_a + (row0 + u) * OP : nullptr;   // wave-uniform row pointers
      float* rb0 = p.out_b ? p.out_b + (row0 + u) * OP : nullptr;
      SSR_WPHASE(blk, regs, {
        // UNCONDITIONAL (the last frame of a chunk re-requests a clamped, valid frame that nobody consumes): under a condition
        // the previous contents of the 64 + 32 registers would stay live through all three passes for the path not taken.
        // The two signals are requested at different times: 64 + 16 requests at once stop the wave at the 64th until the oldest
        // ones have returned, i.e. expose the latency they are here to hide.
        // All 128 data registers are live here, and a quarter of them is released per butterfly group - the first
        // signal is requested after group 0, the second after group 1
        SSR_SCHED_BARRIER();
        double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const int par = it & 1;
        const bool a_nz = L.nonzero(0, par), b_nz = L.nonzero(1, par);
        const bool both = a_nz && b_nz;                             // wave-uniform: the common case carries no selects
        // A silent target frame: every LSD term is log10(0 / e^2 + 1e-12)^2 = SSR_W_LSD_OF_ZERO exactly, as the reference and the
        // block engine have it.  It is added as that constant (wave-uniform, general path only) instead of 1,025 times the float32
        // logarithm sequence's value for 1e-12, whose one rounding error (about 1 ulp) nothing would average out.
        const int gmask = b_nz ? mask : (mask & ~SSR_M_LSD);
        const double lsd_silent = (want_lsd && !b_nz) ? SSR_W_LSD_OF_ZERO : 0.0;
        const bool store = MAG < 0 ? p.out_kind == SSR_OUT_MAG : MAG != 0;
        // the two magnitude rows as buffer views: scalar row base + one lane offset + an immediate per bin (a plain pointer
        // costs a 64-bit vector add per store)
        const SsrRwView<float> wa(ra0, store ? F : 0), wb(rb0, (store && rb0 != nullptr) ? F : 0);   // out_b == null: the target rows
        // are not written (ssr_pair_metrics_multi: they exist already) - the stores fall to the buffer range check
        // byte offset of bin j_b + 256 q in a magnitude row: lane part + immediate
        const int lane4 = 4 * tid, lane4_2 = 4 * (192 - tid), lane4_3 = 4 * ssr_wave_pj3(tid);
        auto bin_off = [&](int b, int q) -> int {
          return (b == 0 ? lane4 : b == 1 ? lane4 + 256 : b == 2 ? lane4_2 : lane4_3) + 1024 * q;
        };
        // Lane 0's butterflies 0 and 128 pair with THEMSELVES (q <-> 8 - q, bin 0 and the Nyquist bin with themselves; q <-> 7 - q):
        // its upper halves are rotated once into the registers the general rule (3 - b, 7 - q) reads.  Register 4 - the Nyquist bin
        // Z[1024], which pairs with itself - is taken right after group 0 (32 data registers are free by then), and only then
        // receives its rotated value.
        cx<T> rot4 = {(T)0, (T)0};
        if (tid == 0) {
          rot4 = R.v[28];
          const cx<T> t29 = R.v[29], t30 = R.v[30], t31 = R.v[31];
          R.v[31] = R.v[0]; R.v[30] = R.v[7]; R.v[29] = R.v[6]; R.v[28] = R.v[5];
          R.v[7] = t31; R.v[6] = t30; R.v[5] = t29;
        }
        constexpr int G = 2;                                        // bins in flight (the partners are in registers - there is no
                                                                    // LDS latency to cover)
        // The sixteen bins, two at a time.  FAST (a compile-time fact inside each copy of the loop): both frames hold signal and
        // the mask is the variant's full set - no zero forcing, no per-bin test of the mask, and the float32 arithmetic of a
        // bin pair runs as packed instructions (ssr_pair_bins2_fast).  The wave-uniform choice is made ONCE per frame, outside
        // the loop: taken per bin it split the epilogue into 48 basic blocks with two scalar branches each.
        constexpr int PF1 = SUMS ? 1 : 0;    // the butterfly group after which the first signal is requested (then the second)
        auto bins = [&](auto fast_tag) {
          constexpr bool FAST = decltype(fast_tag)::value;
          SSR_UNROLL for (int b = 0; b < 4; ++b) SSR_UNROLL for (int q0 = 0; q0 < 4; q0 += G) {
            cx<T> zn[G];
            SSR_UNROLL for (int q = 0; q < G; ++q) zn[q] = R.v[8 * (3 - b) + 7 - (q0 + q)];   // Z[2048 - k] out of butterfly 256 - j
            SSR_UNROLL for (int q = 0; q < G; q += 2) {
              const cx<T> zk0 = R.v[8 * b + q0 + q], zk1 = R.v[8 * b + q0 + q + 1];
              f2 e, t;
              if constexpr (FAST) {
                ssr_pair_bins2_fast<T, SUMS>(acc, zk0, zn[q], zk1, zn[q + 1], e, t);
              } else {
                float e0, t0, e1, t1;
                ssr_pair_bin<T, 0, true>(gmask, acc, zk0, zn[q], a_nz, b_nz, e0, t0);
                acc[0] += lsd_silent;
                ssr_pair_bin<T, 0, true>(gmask, acc, zk1, zn[q + 1], a_nz, b_nz, e1, t1);
                acc[0] += lsd_silent;
                e = f2_make(e0, e1); t = f2_make(t0, t1);
              }
              if (store) {
                wa.st_raw(bin_off(b, q0 + q), e.x);
                wa.st_raw(bin_off(b, q0 + q + 1), e.y);
                wb.st_raw(bin_off(b, q0 + q), t.x);
                wb.st_raw(bin_off(b, q0 + q + 1), t.y);
              }
            }
            if (b == 0 && q0 + G == 4) {
              if constexpr (STASH) {                                    // the Nyquist bin to the frame's owner, a silent frame's
                // part forced to zero (for this bin ar = 2 zq.x, ai = 0, br = 2 zq.y, bi = 0: what ssr_pair_bin's forcing gives); then
                // register 4's rotated value
                cx<T> zq = {ssr_wave_first(tid, R.v[4].x, nyq0.x), ssr_wave_first(tid, R.v[4].y, nyq0.y)};
                if (!a_nz) zq.x = (T)0;
                if (!b_nz) zq.y = (T)0;
                if (tid == (it & 63)) R.nyq = zq;
                if (tid == 0) R.v[4] = rot4;
              } else
              if (tid == 0) {                                           // the Nyquist bin, then register 4's rotated value
                const cx<T> zq = R.v[4];
                float e, t;
                double an[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                ssr_pair_bin<T, 0, true>(mask, an, zq, zq, a_nz, b_nz, e, t);
                if (want_lsd && t == 0.0f) an[0] = SSR_W_LSD_OF_ZERO;       // (the flush's rule: a target magnitude of exactly 0)
                for (int i = 0; i < 7; ++i) acc[i] += an[i];
                if (store) { wa.st_raw(4 * (N / 2), e); wb.st_raw(4 * (N / 2), t); }
                R.v[4] = rot4;
              }
            }
            if (b == PF1 && q0 + G == 4) {
              SSR_SCHED_BARRIER();
              ssr_wave_prefetch<T, 1>(p, R, tid, va, vb, u + S, n, n_frames);
              SSR_SCHED_BARRIER();
            }
            if (b == PF1 + 1 && q0 + G == 4) {
              SSR_SCHED_BARRIER();
              ssr_wave_prefetch<T, 2>(p, R, tid, va, vb, u + S, n, n_frames);
              SSR_SCHED_BARRIER();
            }
          }
        };
        constexpr int FULL = SUMS ? (SSR_M_LSD | SSR_M_LOG_SISPEC | SSR_M_SISPEC) : SSR_M_LSD;
        if (both && (mask & 7) == FULL) bins(SsrTrue{});
        else bins(SsrFalse{});
        if constexpr (STASH) { if (want_lsd) SSR_W_SUM(tid, acc[0], L.sc1, tid == (it & 63), R.lsd_frame, =); }
        else if (want_lsd) SSR_WAVE_SUM_STORE(tid, 64, acc[0], L.sc1);
        if constexpr (SUMS)
          for (int q = 0; q < 6; ++q) SSR_LDS_ACCUM(lsum + 64 * q + tid, acc[1 + q]);
      });
      if constexpr (STASH) { SSR_W_SUM_LAND(blk, regs, want_lsd, L.sc1, tid == (it & 63), R.lsd_frame, =); }
    }
    // ---- flush (STASH): lane l finishes frame it0 + l of the block - its Nyquist bin, its LSD, column 1024 of its two rows.  One view
    // over the block's rows with a per-lane row offset; lanes past the block's last frame are selected out - their zero stash is not a
    // zero term (a zero bin's LSD term is log10(1e-12)^2 = 144): they add 0.0 and store at offset -1, which the range check drops, as it
    // drops every target store when out_b is null.  (Byte offsets are 32-bit: 63 S rows of a row pitch far below 2^20 floats.)
    if constexpr (STASH) {
      const int nf = (ue - ub + S - 1) / S;                  // frames in the stash, 1 .. 64
      float* fa = p.out_a ? p.out_a + (row0 + ub) * OP : nullptr;
      float* fb = p.out_b ? p.out_b + (row0 + ub) * OP : nullptr;
      const int64_t span = (int64_t)(nf - 1) * S * OP + F;   // floats from the first row's start to the last row's end
      blk = blk0; ssr_launder(blk);
      SSR_WPHASE(blk, regs, {
        const bool store = MAG < 0 ? p.out_kind == SSR_OUT_MAG : MAG != 0;
        const SsrRwView<float> wa(fa, store ? span : 0), wb(fb, (store && fb != nullptr) ? span : 0);
        const bool mine = tid < nf;
        double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        float e, t;
        ssr_pair_bin<T, 0, true>(mask, acc, R.nyq, R.nyq, true, true, e, t);
        if (want_lsd && t == 0.0f) acc[0] = SSR_W_LSD_OF_ZERO;     // a silent target frame (its stash is zero): the exact term, see the epilogue
        const int off = mine ? 4 * (tid * S * (int)OP + N / 2) : -1;
        wa.st_raw(off, e); wb.st_raw(off, t);
        if constexpr (SUMS)
          for (int q = 0; q < 6; ++q) SSR_LDS_ACCUM(lsum + 64 * q + tid, mine ? acc[1 + q] : 0.0);
        // (the division stays: 1.0 / F is not exact)
        const double r = (want_lsd && mine) ? sqrt((R.lsd_frame + acc[0]) / (double)F) : 0.0;
        SSR_W_SUM(tid, r, L.sc1, tid == 0, R.lsd_total, +=);
        R.lsd_frame = 0.0; R.nyq = {(T)0, (T)0};
      });
      SSR_W_SUM_LAND(blk, regs, true, L.sc1, tid == 0, R.lsd_total, +=);
    }
    ub = ue;
  }

  if (part == nullptr) return;
  // ---- chunk tail: last frame's LSD and the wave-sums of the SISpec accumulators
  if constexpr (SUMS) {
    for (int q = 0; q < 6; ++q) {
      SSR_WPHASE(blk, regs, SSR_WAVE_SUM_STORE(tid, 64, lsum[64 * q + tid], L.sc1 + 1));
      SSR_WPHASE(blk, regs, if (tid == 0) part[1 + q] = L.sc1[1]);
    }
  } else {
    SSR_WPHASE(blk, regs, if (tid == 0) for (int q = 0; q < 6; ++q) part[1 + q] = 0.0);
  }
  SSR_WPHASE(blk, regs, if (tid == 0) {
    double lsd = R.lsd_total;
    if constexpr (!STASH) { if (want_lsd && u1 > u0) lsd += sqrt(L.sc1[0] / (double)F); }
    part[0] = lsd;
    part[7] = 0.0;
  });
}
