// Kernel bodies of the multi-resolution STFT distance of Parallel WaveGAN (Yamamoto et al. 2020), restated in DESIGN §18: per
// resolution (N, H, W) the spectral convergence sqrt(sum (m_x - m_y)^2 / sum m_x^2) and the mean |log m_x - log m_y| of an
// estimate against its target, m = sqrt(max(|.|^2, eps)); then their means over the resolutions.  float32 or float64 signals read
// in their own dtype; frames are centred with reflect padding, a periodic Hann window of W samples sits in the middle of the
// N-point frame (torch.stft's win_length placement), N = n_fft in {256 .. 2048}, hop H; all arithmetic is float64.
//
//   geometry   ssr_phase.h's: chunks of SSR_PHASE_FR frames per pair, their prefix sum over the pairs (once per resolution)
//   dist       one workgroup of N / 8 threads per (pair, chunk) of ONE resolution: the transform of ssr_phase_dist_body - the
//              windowed target in the real part, the windowed estimate in the imaginary part of one complex N-point transform in
//              LDS, X[k] and Y[k] split from Z[k] and conj(Z[N - k]) - with the window from a table and a magnitude epilogue: a
//              thread owns bins 4 tid .. 4 tid + 3 in every frame (bin N / 2: the last thread) and keeps three sums over the
//              chunk, sum (m_x - m_y)^2, sum m_x^2 and sum |log m_x - log m_y| = 0.5 |log(p_x / p_y)|.  Three per-wave votes on the
//              windowed samples make three exact statements exact: a digitally silent frame has |.|^2 = 0 (it clamps to eps, not
//              to the loud partner's rounding error), and a frame whose two windowed signals are the same has p_y = p_x.
//              Lane sums in frame order, wave reduction, the waves in order through LDS
//   finalize   one thread per pair: per resolution the chunk sums in chunk order, sc and mag over the exact cell count, then the
//              means over the resolutions in index order; NaN where a resolution has no frame
//
// No magnitude image exists outside registers.  A transform holds one frame of one pair and the chunking of a pair depends on its
// own length and the resolution only, so a pair has the same bits alone, in any batch and at any position, and a resolution's row
// does not depend on the other resolutions of the call.  There are no atomics.  All bodies compile on the host too (SSR_HOST_EMU,
// tests/emu/mrstft_emu.cpp).
#pragma once
#include "ssr_phase.h"

#define SSR_MRSTFT_MAX_RES 8

// the signals of a call (every resolution reads the same ones)
struct SsrMrstftSig {
  const void* tgt;              // targets, float32 or float64
  const int64_t* tgt_off;       // [n_tgt] device
  const void* est;              // estimates, float32 or float64
  const int64_t* est_off;       // [n_est] device
  const int32_t* tgt_len;       // [n_tgt] (workspace copy)
  const int32_t* tgt_index;     // [n_est] (workspace copy)
  int n_tgt, n_est;
};

// one resolution
struct SsrMrstftRes {
  int N, H, k_lo, k_hi;         // scored bins k_lo .. k_hi of 0 .. N / 2
  const cx<double>* tw;         // [N] exp(-2 pi i k / N)
  const double* win;            // [N] the Hann window of W samples, centred in the frame
  int64_t* chunk_off;           // [n_est + 1] chunk prefix over pairs (the dist grid)
  double* part;                 // [chunk_off[n_est]][3] chunk sums: (m_x - m_y)^2, m_x^2, |log m_x - log m_y|
};

struct SsrMrstftAll {
  int n_res;
  SsrMrstftRes res[SSR_MRSTFT_MAX_RES];
  double* out;                  // [n_est][n_res + 1][2]: (sc, mag) per resolution, then their means
};

// ---- geometry of one resolution: ssr_phase_geometry_body on this resolution's (N, H)
SSR_HD SsrPhaseParams ssr_mrstft_geometry_params(const SsrMrstftSig& p, const SsrMrstftRes& q) {
  SsrPhaseParams g{};
  g.tgt_len = p.tgt_len; g.tgt_index = p.tgt_index; g.n_tgt = p.n_tgt; g.n_est = p.n_est;
  g.N = q.N; g.H = q.H; g.chunk_off = q.chunk_off;
  return g;
}

// LDS of the dist body
template <int LOGN> struct SsrMrstftLds {
  double re[ssr_padded_len(1 << LOGN)], im[ssr_padded_len(1 << LOGN)];
  double ws[3][4];                          // per wave: the chunk's three sums
  int vote[3][4];                           // per wave: some windowed sample of the target / of the estimate is non-zero; some differs
};

struct SsrMrstftRegs {
  cx<double> v[8];
  double w[8];                              // the window at this thread's eight first-pass samples (the same in every frame)
  double s[3];                              // this thread's three sums over the chunk
};

// ---- dist: grid block g = (pair e, chunk c) of resolution q, N / 8 threads
template <typename TT, typename TE, int LOGN, typename BLK>
SSR_BODY void ssr_mrstft_dist_body(const SsrMrstftSig& p, const SsrMrstftRes& q, double eps, BLK& blk, int64_t g, SsrMrstftLds<LOGN>& S) {
  using PL = SsrFftPlan<LOGN>;
  constexpr int N = PL::N, NT = PL::NT, NW = (NT + 63) / 64;
  const int e = ssr_prefix_find(q.chunk_off, p.n_est, g);
  const int ch = (int)(g - q.chunk_off[e]);
  const int ti = p.tgt_index[e];
  const int n = p.tgt_len[ti], H = q.H;
  const int T = ssr_phase_frames(n, N, H);
  const int t0 = ch * SSR_PHASE_FR, t1 = t0 + SSR_PHASE_FR < T ? t0 + SSR_PHASE_FR : T;
  const int k_lo = q.k_lo, k_hi = q.k_hi;
  const TT* x = (const TT*)p.tgt + p.tgt_off[ti];
  const TE* y = (const TE*)p.est + p.est_off[e];
  const cx<double>* tw = q.tw;
  const double* win = q.win;
  SSR_REGS(SsrMrstftRegs, regs, blk);
  SSR_PHASE(blk, regs, {
    SSR_UNROLL for (int r = 0; r < 8; ++r) R.w[r] = win[ssr_fft_first_index<LOGN>(tid, r)];
    R.s[0] = R.s[1] = R.s[2] = 0.0;
  });
  for (int t = t0; t < t1; ++t) {
    ssr_launder(blk);     // (per-pass LDS addresses are recomputed where used, not hoisted across the frame loop)
    SSR_PHASE(blk, regs, {
      ssr_fft_load_packed_frame<LOGN>(tid, R.w, x, y, t, H, n, R.v);
      // what is exact about the two windowed frames and what the packed transform would round away: a silent frame has a zero
      // spectrum (next to a loud frame the split returns the loud one's rounding error for it), equal frames have equal spectra
      bool lx = false, ly = false, df = false;
      SSR_UNROLL for (int r = 0; r < 8; ++r) {
        lx = lx || R.v[r].x != 0.0; ly = ly || R.v[r].y != 0.0; df = df || R.v[r].x != R.v[r].y;
      }
      SSR_WAVE_ANY_STORE(tid, lx, S.vote[0]);
      SSR_WAVE_ANY_STORE(tid, ly, S.vote[1]);
      SSR_WAVE_ANY_STORE(tid, df, S.vote[2]);
      ssr_fft_compute<double, LOGN, 0>(tid, R.v, tw);
      ssr_fft_store<double, LOGN, 0>(tid, S.re, S.im, R.v);
    });
    ssr_fft_finish_natural<LOGN>(blk, regs, S.re, S.im, tw);
    SSR_PHASE(blk, regs, {
      // X[k] = (Z[k] + conj(Z[N - k])) / 2, Y[k] = (Z[k] - conj(Z[N - k])) / (2 i); at k = 0 and k = N / 2 the two are the real
      // and the imaginary part of Z[k] themselves
      int live_x = 0, live_y = 0, differ = 0;
      for (int w = 0; w < NW; ++w) { live_x |= S.vote[0][w]; live_y |= S.vote[1][w]; differ |= S.vote[2][w]; }
      SSR_UNROLL for (int j = 0; j < 5; ++j) {
        const int k = 4 * tid + j, kc = (N - k) & (N - 1);
        if ((j < 4 || k == N / 2) && k >= k_lo && k <= k_hi) {
          const double zr = S.re[ssr_pad(k)], zi = S.im[ssr_pad(k)];
          double px, py;
          if (k == kc) {
            px = zr * zr; py = zi * zi;
          } else {
            const double cr = S.re[ssr_pad(kc)], ci = S.im[ssr_pad(kc)];
            const double xr = 0.5 * (zr + cr), xi = 0.5 * (zi - ci), yr = 0.5 * (zi + ci), yi = 0.5 * (cr - zr);
            px = xr * xr + xi * xi; py = yr * yr + yi * yi;
          }
          if (!live_x) px = 0.0;
          if (!live_y) py = 0.0;
          if (!differ) py = px;
          px = px < eps ? eps : px;
          py = py < eps ? eps : py;
          // the two magnitudes literally: p_x + p_y - 2 sqrt(p_x p_y) would cancel where y is close to x
          const double mx = sqrt(px), my = sqrt(py), d = mx - my;
          R.s[0] += d * d;
          R.s[1] += mx * mx;
          R.s[2] += 0.5 * fabs(log(px / py));
        }
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
      for (int w = 0; w < NW; ++w) a += S.ws[tid][w];
      q.part[3 * g + tid] = a;
    }
  });
}

// ---- finalize: workgroup b scores pairs b NT .. b NT + NT - 1, one thread each
template <typename BLK> SSR_BODY void ssr_mrstft_finalize_body(const SsrMrstftSig& p, const SsrMrstftAll& a, BLK& blk, int b) {
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    const int e = b * SSR_PHASE_FIN_NT + tid;
    if (e < p.n_est) {
      const int n = p.tgt_len[p.tgt_index[e]];
      double* o = a.out + (int64_t)e * (a.n_res + 1) * 2;
      double sc_sum = 0.0, mag_sum = 0.0;
      SSR_UNROLL for (int r = 0; r < SSR_MRSTFT_MAX_RES; ++r) {      // (unrolled: the table is indexed statically)
        if (r < a.n_res) {
          const SsrMrstftRes& q = a.res[r];
          const int64_t T = ssr_phase_frames(n, q.N, q.H), cells = T * (q.k_hi - q.k_lo + 1);
          double s0 = 0.0, s1 = 0.0, s2 = 0.0;
          for (int64_t g = q.chunk_off[e]; g < q.chunk_off[e + 1]; ++g) {
            s0 += q.part[3 * g]; s1 += q.part[3 * g + 1]; s2 += q.part[3 * g + 2];
          }
          const double sc = T > 0 ? sqrt(s0 / s1) : (double)NAN, mag = T > 0 ? s2 / (double)cells : (double)NAN;
          o[2 * r] = sc; o[2 * r + 1] = mag;
          sc_sum += sc; mag_sum += mag;
        }
      }
      o[2 * a.n_res] = sc_sum / (double)a.n_res;
      o[2 * a.n_res + 1] = mag_sum / (double)a.n_res;
    }
  });
}

// ---- host table: torch.stft's window of win_length W in an N-point frame - the periodic Hann window 0.5 - 0.5 cos(2 pi i / W)
// at l + i, l = (N - W) / 2 rounded down, zero elsewhere (long double, rounded once)
static inline void ssr_mrstft_window_host(int N, int W, std::vector<double>& win) {
  const long double two_pi = 6.283185307179586476925286766559005768L;
  win.assign(N, 0.0);
  const int l = (N - W) / 2;
  for (int i = 0; i < W; ++i) win[l + i] = (double)(0.5L - 0.5L * cosl(two_pi * i / W));
}
