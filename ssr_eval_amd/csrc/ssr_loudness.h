// Kernel bodies of the loudness family (ITU-R BS.1770-4 integrated loudness with gating, EBU Tech 3341 momentary / short-term
// maxima, EBU Tech 3342 loudness range, sample peak and 4x oversampled peak), restated in DESIGN §21.  The first PER-SIGNAL family:
// a signal x of n samples at an integer rate fs, float32 or float64, mono (channel weight 1); all arithmetic is float64.
//
//   K-weighting  two biquads (shelf, high-pass) from the analog prototypes at fs (ssr_loud_tables_host), y = the cascade from the zero state
//   sub-blocks   h = (fs + 5) / 10 samples, S = n / h of them, E[s] = sum y^2 over sub-block s (samples past S h do not count)
//   blocks       momentary: 4 sub-blocks, z = (E[j] + .. + E[j + 3]) / (4 h), 0 <= j <= S - 4; short-term: 30, 0 <= j <= S - 30;
//                L(z) = -0.691 + 10 log10 z
//   lufs         over the momentary blocks with L > -70: G = L(mean z) - 10; lufs = L(mean z over L > -70 and L > G)
//   maxima       lufs_m_max / lufs_s_max: the largest L of the momentary / short-term blocks above -70
//   lra          over the short-term blocks with L > -70: G = L(mean z) - 20; v = the L > G sorted ascending (m of them);
//                lra = v[r(95)] - v[r(10)], r(p) = ((m - 1) p + 50) / 100
//   peaks        peak_db = 20 log10 max |x|; true_peak_db = 20 log10 max |u|, u = x oversampled 4x by the 81-tap Kaiser (beta 5) filter
//                of scipy.signal.resample_poly(x, 4, 1): u[4 q + r] = sum_d t[4 d + r] x[q + 10 - d], x zero outside [0, n)
//   NaN          an empty block set (S < 4, S < 30, nothing above -70); both peaks of an all-zero (or empty) signal
//
//   geometry   one workgroup: the prefix sums over the signals of their segments (S G) and of their peak tiles
//   filter     PARALLEL IN TIME as ssr_iir_pit.h: a sub-block is cut into G = 8 segments at floor(h g / G) (two lengths at most); one
//              lane per (signal, segment).  Sweep 1 filters the segment from the zero state and keeps the four end states; the scan
//              (one lane per signal, a sub-block's eight end states per load) hands the state on, z_in[k + 1] = M_k z_in[k] +
//              z_end[k] with M the 4 x 4 state map of the segment's length (of the shorter length, and one step more for the longer); sweep 2 filters again from z_in[k] and sums y^2 in
//              sample order.  The signal is read twice, y is never written.  A wave moves its lanes' 16-sample chunks together
//              through an LDS tile (ssr_pit_request / _take) so that global requests stay contiguous
//   peak       one workgroup per tile of 2048 samples: the tile and ten samples either side staged in LDS as float64, a thread
//              forms the four polyphase outputs of its samples (taps through scalar loads), max |x| and max |u| per tile.  max is
//              exactly associative: any reduction shape gives the same bits
//   gate       one workgroup per signal: E[s] = the eight segment sums in order (-> blocks_out), window sums of fixed shape, the
//              two gates, the maxima, the loudness-range ranks selected by counting, the tiles' peaks; writes the six values
//
// Every sum has a shape that depends on the signal's own length and the rate only: a signal gives the same bits alone, in any
// batch, at any position and in any run.  No atomics.  All bodies compile on the host too (SSR_HOST_EMU, tests/emu/loudness_emu.cpp).
#pragma once
#include <vector>
#include "ssr_pairs.h"
#include "ssr_iir_pit.h"

#define SSR_LOUD_G 8                       // segments per sub-block
#define SSR_LOUD_NT 256                    // threads of the geometry, peak and gate workgroups
#define SSR_LOUD_Q 24                      // short-term blocks per thread of the gate workgroup
#define SSR_LOUD_MAX_SUB (SSR_LOUD_NT * SSR_LOUD_Q)   // sub-blocks per signal: 6144 (10 min 14 s)
#define SSR_LOUD_TILE 2048                 // samples per peak tile
#define SSR_LOUD_HALF 10                   // input samples either side of an oversampled output
#define SSR_LOUD_TAPS 81
#define SSR_LOUD_MIN_RATE 8000
#define SSR_LOUD_MAX_RATE 192000
// the table of a rate (ssr_loud_tables_host): c[2][5] = b0 b1 b2 a1 a2 per stage, M of floor(h / G) steps, the taps
#define SSR_LOUD_TAB_M 10
#define SSR_LOUD_TAB_TAPS 26
#define SSR_LOUD_TAB_LEN 128
static_assert(SSR_LOUD_NT == SSR_PAIRS_NT, "the scan of the geometry workgroup is ssr_run_geometry_body's shape");
static_assert(SSR_LOUD_TAB_TAPS + SSR_LOUD_TAPS <= SSR_LOUD_TAB_LEN, "the table holds the taps");

SSR_HD int ssr_loud_sub_len(int rate) { return (rate + 5) / 10; }
SSR_HD int ssr_loud_sub_blocks(int n, int rate) { return n / ssr_loud_sub_len(rate); }
SSR_HD int64_t ssr_loud_segments(int n, int rate) { return (int64_t)ssr_loud_sub_blocks(n, rate) * SSR_LOUD_G; }
SSR_HD int64_t ssr_loud_tiles(int n) { return ((int64_t)n + SSR_LOUD_TILE - 1) / SSR_LOUD_TILE; }
SSR_HD int ssr_loud_seg_start(int h, int g) { return (int)(((int64_t)h * g) / SSR_LOUD_G); }

// ---- host: the table of a rate, float64 ---------------------------------------------------------------------------------------
// I0 by its power series (x <= 5: 30 terms reach 1e-17 of the sum)
inline double ssr_loud_i0(double x) {
  double s = 1.0, t = 1.0;
  for (int k = 1; k < 40; ++k) { t *= (x * x * 0.25) / ((double)k * (double)k); s += t; }
  return s;
}
inline void ssr_loud_step_host(double v, const double* c, double* z, double* out) {
  for (int s = 0; s < 2; ++s) {
    const double yo = c[5 * s] * v + z[2 * s];
    z[2 * s] = (c[5 * s + 1] * v - c[5 * s + 3] * yo) + z[2 * s + 1];
    z[2 * s + 1] = c[5 * s + 2] * v - c[5 * s + 4] * yo;
    v = yo;
  }
  if (out) *out = v;
}
inline void ssr_loud_tables_host(int rate, std::vector<double>& tab) {
  tab.assign(SSR_LOUD_TAB_LEN, 0.0);
  {   // stage 1: the shelf
    const double f0 = 1681.974450955533, Gdb = 3.999843853973347, Q = 0.7071752369554196;
    const double K = tan(M_PI * f0 / (double)rate), Vh = pow(10.0, Gdb / 20.0), Vb = pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    tab[0] = (Vh + Vb * K / Q + K * K) / a0; tab[1] = 2.0 * (K * K - Vh) / a0; tab[2] = (Vh - Vb * K / Q + K * K) / a0;
    tab[3] = 2.0 * (K * K - 1.0) / a0; tab[4] = (1.0 - K / Q + K * K) / a0;
  }
  {   // stage 2: the high-pass
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = tan(M_PI * f0 / (double)rate), d = 1.0 + K / Q + K * K;
    tab[5] = 1.0; tab[6] = -2.0; tab[7] = 1.0;
    tab[8] = 2.0 * (K * K - 1.0) / d; tab[9] = (1.0 - K / Q + K * K) / d;
  }
  // M[i][j]: state i after L steps from the unit state e_j without input, L = floor(h / G)
  const int L0 = ssr_loud_sub_len(rate) / SSR_LOUD_G;
  for (int j = 0; j < 4; ++j) {
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    z[j] = 1.0;
    for (int r = 0; r < L0; ++r) ssr_loud_step_host(0.0, tab.data(), z, nullptr);
    for (int i = 0; i < 4; ++i) tab[SSR_LOUD_TAB_M + 4 * i + j] = z[i];
  }
  // scipy.signal.resample_poly(x, 4, 1)'s filter: firwin(81, 1 / 4, window=("kaiser", 5.0)), unit sum, times 4
  double* t = tab.data() + SSR_LOUD_TAB_TAPS;
  const int half = (SSR_LOUD_TAPS - 1) / 2;
  double sum = 0.0;
  for (int k = 0; k < SSR_LOUD_TAPS; ++k) {
    const double m = (double)(k - half), a = M_PI * 0.25 * m, r = m / (double)half;
    const double sinc = k == half ? 1.0 : sin(a) / a;
    t[k] = 0.25 * sinc * (ssr_loud_i0(5.0 * sqrt(1.0 - r * r)) / ssr_loud_i0(5.0));
    sum += t[k];
  }
  for (int k = 0; k < SSR_LOUD_TAPS; ++k) t[k] = t[k] / sum * 4.0;
}

struct SsrLoudParams {
  const void* sig;              // signals, float32 or float64
  const int64_t* off;           // [n_sig] device: signal i starts at sig + off[i]
  const int32_t* len;           // [n_sig] (workspace copy)
  int n_sig, rate, h;           // h: samples per sub-block
  const double* tab;            // [SSR_LOUD_TAB_LEN] the rate's table
  int64_t* seg_pre;             // [n_sig + 1] segment prefix over signals (the filter grid)
  int64_t* tile_pre;            // [n_sig + 1] peak tile prefix over signals (the peak grid)
  double* zend;                 // [segments][4] end states of sweep 1
  double* zin;                  // [segments][4] start states of sweep 2
  double* part;                 // [segments] sum y^2 of a segment
  double* peak;                 // [tiles][2] max |x|, max |u| of a tile
  double* out;                  // [n_sig][6]: lufs, lra, lufs_m_max, lufs_s_max, peak_db, true_peak_db
  const int64_t* blocks_off;    // [n_sig] (workspace copy) or null
  double* blocks_out;           // E[s] of signal i at blocks_out + blocks_off[i], or null
};

// ---- geometry: one workgroup of SSR_LOUD_NT threads; thread t owns signals [t c, (t + 1) c).  LDS: 2 * NT int64.
template <typename BLK> SSR_BODY void ssr_loud_geometry_body(const SsrLoudParams& p, BLK& blk, int64_t* sums) {
  const int NT = SSR_LOUD_NT, c = (p.n_sig + NT - 1) / NT;
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    int64_t a = 0, b = 0;
    for (int i = tid * c; i < p.n_sig && i < (tid + 1) * c; ++i) { a += ssr_loud_segments(p.len[i], p.rate); b += ssr_loud_tiles(p.len[i]); }
    sums[tid] = a; sums[NT + tid] = b;
  });
  SSR_PHASE(blk, regs, {
    if (tid < 2) {
      int64_t a = 0;
      for (int t = 0; t < NT; ++t) { const int64_t v = sums[tid * NT + t]; sums[tid * NT + t] = a; a += v; }
    }
  });
  SSR_PHASE(blk, regs, {
    int64_t a = sums[tid], b = sums[NT + tid];
    for (int i = tid * c; i < p.n_sig && i < (tid + 1) * c; ++i) {
      p.seg_pre[i] = a; p.tile_pre[i] = b;
      a += ssr_loud_segments(p.len[i], p.rate); b += ssr_loud_tiles(p.len[i]);
    }
    if (tid == NT - 1) { p.seg_pre[p.n_sig] = a; p.tile_pre[p.n_sig] = b; }
  });
}

// ---- filter sweeps: lane = (signal, segment) by the segment prefix; 64 consecutive lanes to a one-wave workgroup.  SECOND = false:
// from the zero state, the end state only.  SECOND = true: from z_in, sum y^2 in sample order.  A lane past the grid stays, with
// an empty segment: the wave's staged loads need every lane.
template <typename X, bool SECOND> SSR_DEV void ssr_loud_filter_lane(const SsrLoudParams& p, int64_t lane, int64_t n_seg, SsrPitTile& t) {
  constexpr int CK = SSR_PIT_CK, G = SSR_LOUD_G;
  const bool live = lane < n_seg;
  const int h = p.h;
  int L = 0;
  const X* x = (const X*)p.sig;
  if (live) {
    const int i = ssr_prefix_find(p.seg_pre, p.n_sig, lane);
    const int64_t k = lane - p.seg_pre[i];
    const int s = (int)(k / G), g = (int)(k % G), n0 = ssr_loud_seg_start(h, g);
    L = ssr_loud_seg_start(h, g + 1) - n0;
    x += p.off[i] + (int64_t)s * h + n0;
  }
  const ssr_pit_row tab = ssr_pit_uniform(p.tab);
  double c[2][5], z[4];
  SSR_UNROLL for (int s = 0; s < 2; ++s) {
    SSR_UNROLL for (int j = 0; j < 5; ++j) c[s][j] = tab[5 * s + j];
  }
  SSR_UNROLL for (int j = 0; j < 4; ++j) z[j] = (SECOND && live) ? p.zin[lane * 4 + j] : 0.0;
  double acc = 0.0;
  const int n_ch = (h / G + 1 + CK - 1) / CK;       // chunks of the longer segment length (wave-uniform)
  SsrPitStage<X> st{};
  ssr_pit_request(CK <= L ? x : (const X*)nullptr, p.tab, t, st);
  for (int ch = 0; ch < n_ch; ++ch) {
    const int base = ch * CK;
    double b[CK];
    ssr_pit_take(st, t, b);
    const bool next_whole = ch + 1 < n_ch && base + 2 * CK <= L;
    ssr_pit_request(next_whole ? x + (base + CK) : (const X*)nullptr, p.tab, t, st);
    if (base + CK <= L) {
      SSR_UNROLL for (int i = 0; i < CK; ++i) {
        const double y = ssr_pit_step<2>(b[i], c, z);
        if (SECOND) acc += y * y;
      }
    } else if (base < L) {                          // the segment's last, partial chunk: sample by sample
      SSR_UNROLL for (int i = 0; i < CK; ++i) {
        if (base + i < L) {
          const double y = ssr_pit_step<2>((double)x[base + i], c, z);
          if (SECOND) acc += y * y;
        }
      }
    }
  }
  if (live) {
    if (SECOND) {
      p.part[lane] = acc;
    } else {
      SSR_UNROLL for (int j = 0; j < 4; ++j) p.zend[lane * 4 + j] = z[j];
    }
  }
}

// ---- scan: lane = signal.  z_in[0] = 0, z_in[k + 1] = M_k z_in[k] + z_end[k]; a sub-block's eight end states are loaded together,
// the next sub-block's ahead of the dependent chain.  Row sums: columns 0, 2 and 1, 3 in two partial sums (a fixed order).
SSR_DEV void ssr_loud_scan_signal(const SsrLoudParams& p, int i) {
  constexpr int G = SSR_LOUD_G;
  if (i >= p.n_sig) return;
  const int64_t k0 = p.seg_pre[i];
  const int S = (int)((p.seg_pre[i + 1] - k0) / G), h = p.h, L0 = h / G;
  const ssr_pit_row tab = ssr_pit_uniform(p.tab);
  double c[2][5], m[16], z[4] = {0.0, 0.0, 0.0, 0.0}, e[G * 4], en[G * 4];
  SSR_UNROLL for (int s = 0; s < 2; ++s) {
    SSR_UNROLL for (int j = 0; j < 5; ++j) c[s][j] = tab[5 * s + j];
  }
  SSR_UNROLL for (int j = 0; j < 16; ++j) m[j] = tab[SSR_LOUD_TAB_M + j];
  const double* zend = p.zend + k0 * 4;
  double* zin = p.zin + k0 * 4;
  if (S > 0) {
    SSR_UNROLL for (int j = 0; j < G * 4; ++j) e[j] = zend[j];
  }
  for (int s = 0; s < S; ++s) {
    const bool more = s + 1 < S;
    SSR_UNROLL for (int j = 0; j < G * 4; ++j) en[j] = more ? zend[(int64_t)(s + 1) * G * 4 + j] : 0.0;
    SSR_UNROLL for (int g = 0; g < G; ++g) {
      SSR_UNROLL for (int j = 0; j < 4; ++j) zin[((int64_t)s * G + g) * 4 + j] = z[j];
      double nz[4];
      SSR_UNROLL for (int r = 0; r < 4; ++r) nz[r] = (m[4 * r] * z[0] + m[4 * r + 2] * z[2]) + (m[4 * r + 1] * z[1] + m[4 * r + 3] * z[3]);
      // the longer of the two segment lengths: one more step without input (lane-uniform)
      if (ssr_loud_seg_start(h, g + 1) - ssr_loud_seg_start(h, g) > L0) ssr_pit_step<2>(0.0, c, nz);
      SSR_UNROLL for (int r = 0; r < 4; ++r) nz[r] += e[4 * g + r];
      SSR_UNROLL for (int r = 0; r < 4; ++r) z[r] = nz[r];
    }
    SSR_UNROLL for (int j = 0; j < G * 4; ++j) e[j] = en[j];
  }
}

// ---- peak: grid block g = (signal, tile of SSR_LOUD_TILE samples), SSR_LOUD_NT threads
struct SsrLoudPeakLds {
  double x[SSR_LOUD_TILE + 2 * SSR_LOUD_HALF];
  double m[2][SSR_LOUD_NT];
};
template <typename X, typename BLK> SSR_BODY void ssr_loud_peak_body(const SsrLoudParams& p, BLK& blk, int64_t g, SsrLoudPeakLds& S) {
  constexpr int NT = SSR_LOUD_NT, T = SSR_LOUD_TILE, HL = SSR_LOUD_HALF;
  const int i = ssr_prefix_find(p.tile_pre, p.n_sig, g);
  const int n = p.len[i];
  const int64_t q0 = (g - p.tile_pre[i]) * T;
  const X* x = (const X*)p.sig + p.off[i];
  const ssr_pit_row taps = ssr_pit_uniform(p.tab + SSR_LOUD_TAB_TAPS);
  SSR_REGS(int, regs, blk);
  SSR_PHASE(blk, regs, {
    for (int j = tid; j < T + 2 * HL; j += NT) {
      const int64_t pos = q0 - HL + j;
      S.x[j] = (pos >= 0 && pos < n) ? (double)x[pos] : 0.0;
    }
  });
  SSR_PHASE(blk, regs, {
    double mx = 0.0, mu = 0.0;
    for (int q = tid; q < T && q0 + q < n; q += NT) {
      // u[4 (q0 + q) + r] = sum_d taps[4 d + r] x[q0 + q + HL - d]: sample q0 + q + HL - d is S.x[q + 2 HL - d]
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      SSR_UNROLL for (int d = 0; d <= 2 * HL; ++d) {
        const double v = S.x[q + 2 * HL - d];
        a0 += taps[4 * d] * v;
        if (d < 2 * HL) { a1 += taps[4 * d + 1] * v; a2 += taps[4 * d + 2] * v; a3 += taps[4 * d + 3] * v; }
      }
      const double xv = fabs(S.x[q + HL]);
      mx = xv > mx ? xv : mx;
      a0 = fabs(a0); a1 = fabs(a1); a2 = fabs(a2); a3 = fabs(a3);
      a0 = a1 > a0 ? a1 : a0; a2 = a3 > a2 ? a3 : a2; a0 = a2 > a0 ? a2 : a0;
      mu = a0 > mu ? a0 : mu;
    }
    S.m[0][tid] = mx; S.m[1][tid] = mu;
  });
  SSR_PHASE(blk, regs, {
    if (tid < 2) {
      double a = 0.0;
      for (int t = 0; t < NT; ++t) a = S.m[tid][t] > a ? S.m[tid][t] : a;
      p.peak[g * 2 + tid] = a;
    }
  });
}

// ---- gate: workgroup i scores signal i, SSR_LOUD_NT threads
struct SsrLoudGateLds {
  double e[SSR_LOUD_MAX_SUB];               // E[s]; later the short-term loudness of the blocks inside both gates (NaN: outside)
  double sc[3][SSR_LOUD_NT], mid[3][16], res[3], rank[2];
};
struct SsrLoudGateRegs {
  double z[SSR_LOUD_Q];                     // this thread's short-term blocks j = tid + q NT: z, then L
  double a[3];
};
SSR_DEV double ssr_loud_lk(double z) { return -0.691 + 10.0 * log10(z); }
// block reduction of R.a[0 .. nv): entries below n_sum are sums (thread order in strides of 16, then the 16 in order), the others maxima -> S.res
template <typename BLK, typename REGS> SSR_BODY void ssr_loud_reduce(BLK& blk, REGS& regs, SsrLoudGateLds& S, int nv, int n_sum) {
  constexpr int NT = SSR_LOUD_NT;
  SSR_PHASE(blk, regs, { for (int q = 0; q < nv; ++q) S.sc[q][tid] = R.a[q]; });
  SSR_PHASE(blk, regs, {
    if (tid < 16 * nv) {
      const int q = tid >> 4, l = tid & 15;
      double a = S.sc[q][l];
      for (int t = l + 16; t < NT; t += 16) { const double v = S.sc[q][t]; a = q < n_sum ? a + v : (v > a ? v : a); }
      S.mid[q][l] = a;
    }
  });
  SSR_PHASE(blk, regs, {
    if (tid < nv) {
      double a = S.mid[tid][0];
      for (int l = 1; l < 16; ++l) { const double v = S.mid[tid][l]; a = tid < n_sum ? a + v : (v > a ? v : a); }
      S.res[tid] = a;
    }
  });
}
template <typename BLK> SSR_BODY void ssr_loud_gate_body(const SsrLoudParams& p, BLK& blk, int i, SsrLoudGateLds& S) {
  constexpr int NT = SSR_LOUD_NT, G = SSR_LOUD_G, Q = SSR_LOUD_Q;
  const int h = p.h, Sb = p.len[i] / h;
  const int nm = Sb >= 4 ? Sb - 3 : 0, ns = Sb >= 30 ? Sb - 29 : 0;
  const int64_t k0 = p.seg_pre[i], t0 = p.tile_pre[i], t1 = p.tile_pre[i + 1];
  const double dm = 4.0 * (double)h, ds = 30.0 * (double)h;
  double* out = p.out + (int64_t)i * 6;
  SSR_REGS(SsrLoudGateRegs, regs, blk);
  SSR_PHASE(blk, regs, {
    if (tid == 0) S.rank[0] = S.rank[1] = (double)NAN;
    for (int s = tid; s < Sb; s += NT) {
      const double* q = p.part + k0 + (int64_t)s * G;
      double a = q[0];
      SSR_UNROLL for (int g = 1; g < G; ++g) a += q[g];
      S.e[s] = a;
      if (p.blocks_out) p.blocks_out[p.blocks_off[i] + s] = a;
    }
  });
  // momentary blocks: the absolute gate, then the relative gate
  SSR_PHASE(blk, regs, {
    double sum = 0.0, cnt = 0.0, mx = -INFINITY;
    for (int j = tid; j < nm; j += NT) {
      const double z = ((S.e[j] + S.e[j + 1]) + (S.e[j + 2] + S.e[j + 3])) / dm, l = ssr_loud_lk(z);
      if (l > -70.0) { sum += z; cnt += 1.0; mx = l > mx ? l : mx; }
    }
    R.a[0] = sum; R.a[1] = cnt; R.a[2] = mx;
  });
  ssr_loud_reduce(blk, regs, S, 3, 2);
  SSR_PHASE(blk, regs, {
    const double cnt0 = S.res[1], gate = ssr_loud_lk(S.res[0] / cnt0) - 10.0;
    if (tid == 0) out[2] = cnt0 > 0.0 ? S.res[2] : (double)NAN;
    double sum = 0.0, cnt = 0.0;
    for (int j = tid; j < nm; j += NT) {
      const double z = ((S.e[j] + S.e[j + 1]) + (S.e[j + 2] + S.e[j + 3])) / dm, l = ssr_loud_lk(z);
      if (l > -70.0 && l > gate) { sum += z; cnt += 1.0; }
    }
    R.a[0] = sum; R.a[1] = cnt;
  });
  ssr_loud_reduce(blk, regs, S, 2, 2);
  SSR_PHASE(blk, regs, {
    if (tid == 0) out[0] = S.res[1] > 0.0 ? ssr_loud_lk(S.res[0] / S.res[1]) : (double)NAN;
  });
  // short-term blocks: thirty sub-blocks summed in order, kept in registers while E is still read
  SSR_PHASE(blk, regs, {
    double sum = 0.0, cnt = 0.0, mx = -INFINITY;
    SSR_UNROLL for (int q = 0; q < Q; ++q) {
      const int j = tid + q * NT;
      double l = (double)NAN;
      if (j < ns) {
        double a = S.e[j];
        for (int r = 1; r < 30; ++r) a += S.e[j + r];
        const double z = a / ds;
        l = ssr_loud_lk(z);
        if (l > -70.0) { sum += z; cnt += 1.0; mx = l > mx ? l : mx; } else { l = (double)NAN; }
      }
      R.z[q] = l;
    }
    R.a[0] = sum; R.a[1] = cnt; R.a[2] = mx;
  });
  ssr_loud_reduce(blk, regs, S, 3, 2);
  SSR_PHASE(blk, regs, {
    const double cnt0 = S.res[1], gate = ssr_loud_lk(S.res[0] / cnt0) - 20.0;
    if (tid == 0) out[3] = cnt0 > 0.0 ? S.res[2] : (double)NAN;
    double cnt = 0.0;
    SSR_UNROLL for (int q = 0; q < Q; ++q) {
      const int j = tid + q * NT;
      const bool in = R.z[q] > gate;                   // (NaN: outside the absolute gate, or no block)
      if (j < ns) S.e[j] = in ? R.z[q] : (double)NAN;
      cnt += in ? 1.0 : 0.0;
    }
    R.a[0] = cnt;
  });
  ssr_loud_reduce(blk, regs, S, 1, 1);
  // the two ranks by counting: the value with exactly r values before it (ties by position)
  SSR_PHASE(blk, regs, {
    const int m = (int)S.res[0];
    const int r_lo = ((m - 1) * 10 + 50) / 100, r_hi = ((m - 1) * 95 + 50) / 100;
    SSR_UNROLL for (int q = 0; q < Q; ++q) {
      const int j = tid + q * NT;
      if (j < ns && m > 0) {
        const double v = S.e[j];
        if (v == v) {
          int c = 0;
          for (int k = 0; k < ns; ++k) { const double w = S.e[k]; c += (w < v || (w == v && k < j)) ? 1 : 0; }
          if (c == r_lo) S.rank[0] = v;
          if (c == r_hi) S.rank[1] = v;
        }
      }
    }
    // the tiles' peaks
    double mx = 0.0, mu = 0.0;
    for (int64_t t = t0 + tid; t < t1; t += NT) { const double a = p.peak[2 * t], b = p.peak[2 * t + 1]; mx = a > mx ? a : mx; mu = b > mu ? b : mu; }
    R.a[0] = mx; R.a[1] = mu;
  });
  ssr_loud_reduce(blk, regs, S, 2, 0);
  SSR_PHASE(blk, regs, {
    if (tid == 0) {
      out[1] = S.rank[1] - S.rank[0];                 // (NaN where no short-term block is inside both gates)
      out[4] = S.res[0] > 0.0 ? 20.0 * log10(S.res[0]) : (double)NAN;
      out[5] = S.res[1] > 0.0 ? 20.0 * log10(S.res[1]) : (double)NAN;
    }
  });
}
