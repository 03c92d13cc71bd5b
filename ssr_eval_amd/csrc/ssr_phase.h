// Kernel bodies of the anti-wrapping phase distances of the bandwidth-extension literature (Ai & Ling 2023; AP-BWE, Lu et al.
// 2024), restated in DESIGN §17: instantaneous phase (IP), group delay (GD) and instantaneous angular frequency (IAF) of an
// estimate against its target, on float32 or float64 signals read in their own dtype.  Frames are centred with reflect padding,
// periodic Hann window, N = n_fft in {256 .. 2048}, hop H; all arithmetic is float64.  With C = Y conj(X) the cross-spectrum
// and a(z) = |atan2(Im z, Re z)| (0 at z = 0), the anti-wrapped differences of the papers are a(C[t][k]) (IP),
// a(C[t][k+1] conj(C[t][k])) (GD) and a(C[t+1][k] conj(C[t][k])) (IAF): differences of phases are arguments of products.
//
//   geometry   one workgroup: chunks of SSR_PHASE_FR frames per pair, their prefix sum over the pairs
//   dist       one workgroup of N / 8 threads per (pair, chunk): per frame the windowed target goes to the real part and the
//              windowed estimate to the imaginary part of ONE complex N-point transform (ssr_fft.h in LDS); X[k], Y[k] are split
//              from Z[k] and conj(Z[N - k]); a thread owns bins 4 tid .. 4 tid + 3 in every frame (bin N / 2: the last thread),
//              forms their C in registers - and that of bin 4 tid + 4, its GD neighbour, read from LDS - and keeps the previous
//              frame's for IAF; with IAF a chunk that does not start the signal transforms frame t0 - 1 first and scores it only as
//              the predecessor; a frame in which either signal is digitally silent gets C = 0, its exact value.  Three sums per
//              chunk: lane sums in frame order, wave reduction, the waves in order through LDS
//   finalize   one thread per pair: the chunk sums in chunk order over the exact cell counts; the NaN cases
//
// A transform holds one frame of one pair and the chunking of a pair depends on its own length only, so a pair has the same bits
// alone, in any batch and at any position; the three sums never mix, so a subset of `which` gives the bits of the full call.
// There are no atomics.  All bodies compile on the host too (SSR_HOST_EMU, tests/emu/phase_emu.cpp).
#pragma once
#include "ssr_pairs.h"
#include "ssr_fft.h"

#define SSR_PHASE_IP 1
#define SSR_PHASE_GD 2
#define SSR_PHASE_IAF 4
#define SSR_PHASE_FR 16                    // frames per chunk
#define SSR_PHASE_NT 256                   // threads of the geometry workgroup
#define SSR_PHASE_FIN_NT 64                // pairs per finalize workgroup
#define SSR_PHASE_LOGN_MIN 8
#define SSR_PHASE_LOGN_MAX 11

// T = 1 + n // H centred frames; none where the reflect padding of N / 2 samples is undefined (n <= N / 2)
SSR_HD int ssr_phase_frames(int n, int N, int H) { return n > N / 2 ? 1 + n / H : 0; }
SSR_HD int ssr_phase_chunks(int n, int N, int H) { return (ssr_phase_frames(n, N, H) + SSR_PHASE_FR - 1) / SSR_PHASE_FR; }
// log2 of n_fft, or -1 where n_fft is not 256, 512, 1024 or 2048
SSR_HD int ssr_phase_log2_nfft(int n_fft) {
  for (int g = SSR_PHASE_LOGN_MIN; g <= SSR_PHASE_LOGN_MAX; ++g)
    if (n_fft == (1 << g)) return g;
  return -1;
}

struct SsrPhaseParams {
  const void* tgt;              // targets, float32 or float64
  const int64_t* tgt_off;       // [n_tgt] device
  const void* est;              // estimates, float32 or float64
  const int64_t* est_off;       // [n_est] device
  const int32_t* tgt_len;       // [n_tgt] (workspace copy)
  const int32_t* tgt_index;     // [n_est] (workspace copy)
  int n_tgt, n_est;
  int which, N, H, k_lo, k_hi;  // scored bins k_lo .. k_hi of 0 .. N / 2
  const cx<double>* tw;         // [N] exp(-2 pi i k / N); the window is 0.5 - 0.5 Re tw
  int64_t* chunk_off;           // [n_est + 1] chunk prefix over pairs (the dist grid)
  double* part;                 // [chunk_off[n_est]][3] chunk sums: IP, GD, IAF
  double* out;                  // [n_est][popcount(which)]
};

// the anti-wrapping distance of the phase of z from 0: |arg z| in [0, pi]; 0 at z = 0 whatever the signs of its zeros
SSR_HD double ssr_phase_a(cx<double> z) { return (z.x == 0.0 && z.y == 0.0) ? 0.0 : fabs(atan2(z.y, z.x)); }
// u conj(v)
SSR_HD cx<double> ssr_phase_mulc(cx<double> u, cx<double> v) { return {u.x * v.x + u.y * v.y, u.y * v.x - u.x * v.y}; }

// ---- geometry: one workgroup of SSR_PHASE_NT threads.  LDS: NT int64.
template <typename BLK> SSR_BODY void ssr_phase_geometry_body(const SsrPhaseParams& p, BLK& blk, int64_t* sums) {
  const int NT = SSR_PHASE_NT, c = (p.n_est + NT - 1) / NT;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    int64_t a = 0;
    for (int e = tid * c; e < p.n_est && e < (tid + 1) * c; ++e) a += ssr_phase_chunks(p.tgt_len[p.tgt_index[e]], p.N, p.H);
    sums[tid] = a;
  });
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      int64_t a = 0;
      for (int t = 0; t < NT; ++t) { const int64_t v = sums[t]; sums[t] = a; a += v; }
    }
  });
  SSR_PHASE(blk, regs, {
    int64_t a = sums[tid];
    for (int e = tid * c; e < p.n_est && e < (tid + 1) * c; ++e) {
      p.chunk_off[e] = a;
      a += ssr_phase_chunks(p.tgt_len[p.tgt_index[e]], p.N, p.H);
    }
    if (tid == NT - 1) p.chunk_off[p.n_est] = a;
  });
}

// LDS of the dist body
template <int LOGN> struct SsrPhaseLds {
  double re[ssr_padded_len(1 << LOGN)], im[ssr_padded_len(1 << LOGN)];
  double ws[3][4];                          // per wave: the chunk's IP, GD, IAF sums
  int live[2][4];                           // per wave: the frame has a non-zero windowed sample of the target / of the estimate
};

struct SsrPhaseRegs {
  cx<double> v[8];
  double w[8];                              // the window at this thread's eight first-pass samples (the same in every frame)
  cx<double> c[5], pc[5];                   // C of bins 4 tid .. 4 tid + 4 in this frame and in the one before
  double s[3];                              // this thread's IP, GD, IAF sums over the chunk
};

// ---- dist: grid block g = (pair e, chunk c), N / 8 threads
template <typename TT, typename TE, int LOGN, typename BLK>
SSR_BODY void ssr_phase_dist_body(const SsrPhaseParams& p, BLK& blk, int64_t g, SsrPhaseLds<LOGN>& S) {
  using PL = SsrFftPlan<LOGN>;
  constexpr int N = PL::N, NT = PL::NT, NW = (NT + 63) / 64;
  const int e = ssr_prefix_find(p.chunk_off, p.n_est, g);
  const int ch = (int)(g - p.chunk_off[e]);
  const int ti = p.tgt_index[e];
  const int n = p.tgt_len[ti], H = p.H;
  const int T = ssr_phase_frames(n, N, H);
  const int t0 = ch * SSR_PHASE_FR, t1 = t0 + SSR_PHASE_FR < T ? t0 + SSR_PHASE_FR : T;
  const bool ip = (p.which & SSR_PHASE_IP) != 0, gd = (p.which & SSR_PHASE_GD) != 0, iaf = (p.which & SSR_PHASE_IAF) != 0;
  const int tb = (iaf && t0 > 0) ? t0 - 1 : t0;      // the warm-up frame: transformed, scored only as the IAF predecessor
  const int k_lo = p.k_lo, k_hi = p.k_hi;
  const TT* x = (const TT*)p.tgt + p.tgt_off[ti];
  const TE* y = (const TE*)p.est + p.est_off[e];
  const cx<double>* tw = p.tw;
  SSR_REGS(SsrPhaseRegs, regs, blk);
  SSR_PHASE(blk, regs, {
    SSR_UNROLL for (int r = 0; r < 8; ++r) R.w[r] = 0.5 - 0.5 * tw[ssr_fft_first_index<LOGN>(tid, r)].x;
    SSR_UNROLL for (int j = 0; j < 5; ++j) R.pc[j] = {0.0, 0.0};
    R.s[0] = R.s[1] = R.s[2] = 0.0;
  });
  for (int t = tb; t < t1; ++t) {
    const bool score = t >= t0, iaf_now = iaf && score && t > tb;
    ssr_launder(blk);     // (per-pass LDS addresses are recomputed where used, not hoisted across the frame loop)
    SSR_PHASE(blk, regs, {
      ssr_fft_load_packed_frame<LOGN>(tid, R.w, x, y, t, H, n, R.v);
      // a frame of digital silence has a zero spectrum; packed next to a loud frame the split would return the loud one's
      // rounding error for it instead, so such a frame is found here and its C set to zero below
      bool lx = false, ly = false;
      SSR_UNROLL for (int r = 0; r < 8; ++r) { lx = lx || R.v[r].x != 0.0; ly = ly || R.v[r].y != 0.0; }
      SSR_WAVE_ANY_STORE(tid, lx, S.live[0]);
      SSR_WAVE_ANY_STORE(tid, ly, S.live[1]);
      ssr_fft_compute<double, LOGN, 0>(tid, R.v, tw);
      ssr_fft_store<double, LOGN, 0>(tid, S.re, S.im, R.v);
    });
    ssr_fft_finish_natural<LOGN>(blk, regs, S.re, S.im, tw);
    SSR_PHASE(blk, regs, {
      // X[k] = (Z[k] + conj(Z[N - k])) / 2, Y[k] = (Z[k] - conj(Z[N - k])) / (2 i); at k = 0 and k = N / 2 the two are the real
      // and the imaginary part of Z[k] themselves and C is their real product
      int live_x = 0, live_y = 0;
      for (int q = 0; q < NW; ++q) { live_x |= S.live[0][q]; live_y |= S.live[1][q]; }
      const bool silent = !(live_x && live_y);
      SSR_UNROLL for (int j = 0; j < 5; ++j) {
        const int k = 4 * tid + j, kc = (N - k) & (N - 1);
        const double zr = S.re[ssr_pad(k)], zi = S.im[ssr_pad(k)];
        if (silent) {
          R.c[j] = {0.0, 0.0};
        } else if (k == kc) {
          R.c[j] = {zi * zr, 0.0};
        } else {
          const double cr = S.re[ssr_pad(kc)], ci = S.im[ssr_pad(kc)];
          const cx<double> X = {0.5 * (zr + cr), 0.5 * (zi - ci)}, Y = {0.5 * (zi + ci), 0.5 * (cr - zr)};
          R.c[j] = ssr_phase_mulc(Y, X);
        }
      }
      if (score) {
        SSR_UNROLL for (int j = 0; j < 5; ++j) {
          const int k = 4 * tid + j;
          const bool own = j < 4 || k == N / 2, in = own && k >= k_lo && k <= k_hi;
          if (ip && in) R.s[0] += ssr_phase_a(R.c[j]);
          if (j < 4) {
            if (gd && k >= k_lo && k < k_hi) R.s[1] += ssr_phase_a(ssr_phase_mulc(R.c[j + 1], R.c[j]));
          }
          if (iaf_now && in) R.s[2] += ssr_phase_a(ssr_phase_mulc(R.c[j], R.pc[j]));
        }
      }
      if (iaf) {
        SSR_UNROLL for (int j = 0; j < 5; ++j) R.pc[j] = R.c[j];
      }
    });
  }
  SSR_PHASE(blk, regs, {
    SSR_WAVE_SUM_STORE(tid, NT, R.s[0], S.ws[0]);
    SSR_WAVE_SUM_STORE(tid, NT, R.s[1], S.ws[1]);
    SSR_WAVE_SUM_STORE(tid, NT, R.s[2], S.ws[2]);
  });
  SSR_PHASE(blk, regs, {
    if (tid < 3) {
      double a = 0.0;
      for (int q = 0; q < NW; ++q) a += S.ws[tid][q];
      p.part[3 * g + tid] = a;
    }
  });
}

// ---- finalize: workgroup b scores pairs b NT .. b NT + NT - 1, one thread each
template <typename BLK> SSR_BODY void ssr_phase_finalize_body(const SsrPhaseParams& p, BLK& blk, int b) {
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    const int e = b * SSR_PHASE_FIN_NT + tid;
    if (e < p.n_est) {
      const int64_t T = ssr_phase_frames(p.tgt_len[p.tgt_index[e]], p.N, p.H), nb = p.k_hi - p.k_lo + 1;
      double s[3] = {0.0, 0.0, 0.0};
      for (int64_t g = p.chunk_off[e]; g < p.chunk_off[e + 1]; ++g) {
        s[0] += p.part[3 * g]; s[1] += p.part[3 * g + 1]; s[2] += p.part[3 * g + 2];
      }
      const int64_t cells[3] = {T * nb, T * (nb - 1), (T - 1) * nb};
      double* o = p.out + (int64_t)e * ssr_which_count(p.which);
      for (int m = 0; m < 3; ++m)
        if (p.which & (1 << m)) *o++ = (T > 0 && cells[m] > 0) ? s[m] / (double)cells[m] : (double)NAN;
    }
  });
}
