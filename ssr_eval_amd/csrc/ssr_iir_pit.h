// Kernel N1-fast: zero-phase IIR filtering PARALLEL IN TIME - the opt-in second arithmetic of sosfiltfilt (exact=False).
//
// The bit-exact kernel (ssr_iir.h) walks SciPy's recurrence, so a launch lasts as long as its longest utterance's chain of ~2 x len
// dependent steps whatever runs beside it.  The cascade of S second-order sections (direct form II transposed, states z in R^{2S},
// z[2s] / z[2s + 1] = the two delays of section s) is one LINEAR system: its response to (input, initial state) is the response
// to (input, 0) plus the response to (0, initial state).  So an utterance is cut into SEGMENTS of L = SSR_PIT_L samples that run
// side by side.  The cuts count from the first sample of the odd-extended signal, in both passes: what a signal is batched with
// does not change one bit of its result.
//
//   tables (per design, built on the device in the same call: 2S recurrences of L steps)
//       H[r][j]  output at step r of a segment from the unit initial state e_j and no input  (zero-input response)
//       M[i][j]  state i after L steps from e_j and no input
//   forward   local : one lane per (design, utterance, segment) runs the recurrence from the ZERO state over its L samples of the odd
//                     extension (formed in the signal's own arithmetic, as ssr_iir_ext does) -> zero-state output, end state
//             scan  : z_in[0] = zi * ext[0] (SciPy's steady-state initial condition, carried by the scan), z_in[k+1] = z_end[k] + M z_in[k]
//             correction: fwd[n] = zero-state[n] + sum_j H[n mod L][j] z_in[n / L][j], j ascending in two interleaved partial sums -
//                     FUSED into the backward passes' loads (the row of H is the same for every lane of a wave: scalar loads)
//   backward  the segments are the same sample ranges, walked downwards; the topmost (partial) one starts from SciPy's zi * fwd[-1]
//             sweep 1 : the recurrence from the zero state, END STATES only (nothing else is written)
//             scan    : z_in[K-2] = end state of the topmost segment (a true state), z_in[k-1] = z_end[k] + M z_in[k]
//             sweep 2 : the same loads again, the recurrence from z_in[k]: the result y = reverse(bwd)[edge : -edge] is written ONCE.
//                     (A correction pass over y as in the forward direction would read and rewrite the largest array of the call;
//                     the second sweep costs 5 S floating-point operations per sample and no memory traffic beyond the re-read.)
//
// All float64, no atomics, no order that depends on the launch geometry: two runs give the same bits.  NOT SciPy's bits: sums are
// re-associated across segments (and multiply-adds may be fused).  Contract: max|y - scipy| <= 1e-10 max|scipy| per signal (measured
// ~1e-12 over butter / cheby1 / ellip / bessel, orders 2-10, 1-12 kHz at 44.1 kHz; tests/test_iir_fast_host.py).
//
// Geometry.  The host knows the batch's total length, not the lengths (they live on the device), so segments are addressed by SLOT:
// item i's segment k is slot(i, k) = floor((off[i] + 2 emax i) / L) + i + k, emax = the call's largest edge - distinct for distinct
// (i, k) when the items do not overlap, below n_slots = (total + 2 emax n) / L + n + 1.  k_pit_map inverts it once per call; a local
// pass is one lane per (design, slot), 64 consecutive slots to a (one-wave) workgroup.  A lane filters 16-sample chunks of its own
// segment; the wave moves its 64 chunks between global memory and the lanes together, through an LDS tile, so that neighbouring
// lanes touch neighbouring 16-byte pieces of global memory although their segments lie 128 samples apart (ssr_pit_request / _take / _put).
#pragma once
#include "ssr_block.h"
#include "ssr_iir.h"

constexpr int SSR_PIT_L = 128;          // samples per segment
constexpr int SSR_PIT_CK = 16;          // samples per chunk of a lane (one 128-byte run of float64)
constexpr int SSR_PIT_MAXS = 8;         // sections
constexpr int SSR_PIT_ZS = 2 * SSR_PIT_MAXS;   // doubles per row of H / M and per slot of the state arrays' allocation
constexpr int SSR_PIT_MAXD = 48;        // designs per call
static_assert(SSR_PIT_L % SSR_PIT_CK == 0, "whole chunks per segment");

template <typename X> struct SsrPitParamsT {
  const X* x;                      // signals
  const int64_t* off;              // [n_items] element offset (also used for y)
  const int32_t* len;              // [n_items]
  int n_items, n_designs;
  const double* sos;               // [n_designs][8][6]
  const double* zi;                // [n_designs][8][2]
  double* y;                       // [n_designs][y_stride]
  int64_t y_stride;
  int emax, n_slots;
  // workspace
  int32_t* map;                    // [n_slots] item of a slot, -1: none
  double* H;                       // [n_designs][L][16]
  double* M;                       // [n_designs][16][16]
  double *zin_f, *zend, *zin_b;    // [n_designs] blocks of n_slots * 16 doubles; inside design d's block slot s is at s * 2 S_d
  double* fwd;                     // zero-state forward output: design d's item i at fwd_off[d] + off[i] + 2 edge[d] i
  int n_sections[SSR_PIT_MAXD], edge[SSR_PIT_MAXD];
  int64_t fwd_off[SSR_PIT_MAXD];
  int dsel[SSR_PIT_MAXD];          // the designs of ONE local launch: those of one section count (a kernel instance per count, so that a
                                   // one-section design does not run with the registers of an eight-section one)
};

// first slot of an item
SSR_DEV int ssr_pit_slot_base(int64_t off, int item, int emax) {
  return (int)((off + (int64_t)2 * emax * item) / SSR_PIT_L) + item;
}

// k_pit_map: the item whose segment a slot is (for the call's largest edge: a design with a smaller one leaves the last slots idle)
template <typename X> SSR_DEV void ssr_pit_map_slot(const SsrPitParamsT<X>& p, int slot) {
  if (slot >= p.n_slots) return;
  int lo = 0, hi = p.n_items - 1;                      // the last item whose first slot is <= slot
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (ssr_pit_slot_base(p.off[mid], mid, p.emax) <= slot) lo = mid; else hi = mid - 1;
  }
  const int k = slot - ssr_pit_slot_base(p.off[lo], lo, p.emax);
  const int ne = p.len[lo] + 2 * p.emax;
  p.map[slot] = (k >= 0 && (int64_t)k * SSR_PIT_L < ne) ? lo : -1;
}

// the segment of a (design, slot)
template <typename X> struct SsrPitSeg {
  const X* x;
  double* fwd;
  double* y;
  int len, ne, k, n0, n_seg;
  int64_t zoff;                    // of this slot in the state arrays
};
template <int S, typename X> SSR_DEV bool ssr_pit_seg(const SsrPitParamsT<X>& p, int d, int slot, SsrPitSeg<X>& q) {
  if (slot >= p.n_slots) return false;
  const int item = p.map[slot];
  if (item < 0) return false;
  const int64_t o = p.off[item];
  const int edge = p.edge[d];
  q.k = slot - ssr_pit_slot_base(o, item, p.emax);
  q.len = p.len[item];
  q.ne = q.len + 2 * edge;
  q.n0 = q.k * SSR_PIT_L;
  if (q.n0 >= q.ne) return false;
  q.n_seg = (q.ne + SSR_PIT_L - 1) / SSR_PIT_L;
  q.x = p.x + o;
  q.fwd = p.fwd + p.fwd_off[d] + o + (int64_t)2 * edge * item;
  q.y = p.y + (int64_t)d * p.y_stride + o;
  q.zoff = (int64_t)d * p.n_slots * SSR_PIT_ZS + (int64_t)slot * (2 * S);
  return true;
}

// A table row that every lane of a wave reads at the same address: a pointer into the CONSTANT address space, so that the loads
// are scalar (one request per wave, the row in scalar registers).  Through a plain pointer the compiler must assume that the
// kernel's own stores may hit the table and issues one vector load per lane.  (The tables are written by an earlier kernel of the call.)
#ifdef SSR_HOST_EMU
typedef const double* ssr_pit_row;
#else
typedef const double __attribute__((address_space(4)))* ssr_pit_row;
#endif
SSR_DEV ssr_pit_row ssr_pit_uniform(const double* p) { return (ssr_pit_row)p; }

// the sections' coefficients of a design (wave-uniform): c[s] = b0 b1 b2 a1 a2
template <int S> SSR_DEV void ssr_pit_coef(const double* sos, int d, double (&c)[S][5]) {
  SSR_UNROLL for (int s = 0; s < S; ++s) {
    const ssr_pit_row r = ssr_pit_uniform(sos + ((int64_t)d * SSR_PIT_MAXS + s) * 6);
    c[s][0] = r[0]; c[s][1] = r[1]; c[s][2] = r[2]; c[s][3] = r[4]; c[s][4] = r[5];
  }
}

// one sample through the S sections (the statements of ssr_iir_step; this arithmetic may fuse its multiply-adds)
template <int S> SSR_DEV double ssr_pit_step(double v, const double (&c)[S][5], double (&z)[2 * S]) {
  SSR_UNROLL for (int s = 0; s < S; ++s) {
    const double yo = c[s][0] * v + z[2 * s];
    z[2 * s] = (c[s][1] * v - c[s][3] * yo) + z[2 * s + 1];
    z[2 * s + 1] = c[s][2] * v - c[s][4] * yo;
    v = yo;
  }
  return v;
}

// sum_j h[j] z[j], j ascending, even and odd j in two partial sums (a fixed order)
template <int S> SSR_DEV double ssr_pit_dot(ssr_pit_row h, const double (&z)[2 * S]) {
  double a0 = 0.0, a1 = 0.0;
  SSR_UNROLL for (int s = 0; s < S; ++s) { a0 += h[2 * s] * z[2 * s]; a1 += h[2 * s + 1] * z[2 * s + 1]; }
  return a0 + a1;
}

// ---- a chunk (sixteen consecutive samples of a lane's own segment) through the wave's LDS tile -----------------------------------
// Neighbouring lanes' segments lie L samples apart: a lane that loaded its own chunk would make every 16-byte request of the wave
// touch 64 cache lines.  So the WAVE moves its 64 chunks together: a chunk is P = 16 sizeof(E) / 16 pieces of 16 bytes, and request j
// of P has lane l fetch piece l % P of the chunk of lane (64 / P) j + l / P - P neighbouring lanes cover one chunk's contiguous
// 64 or 128 bytes, a request 64 / P whole chunks.  The pieces wait in registers while the current chunk is filtered (the prefetch),
// then pass through the tile (row = owner lane, one piece of padding per row against bank conflicts) to their owners.  Stores go the
// other way.  Every lane of the wave takes part in every call, with `src` / `dst` = nullptr when its chunk is not a whole one inside
// the array (the loads then read `safe`, >= 16 readable bytes whose values nobody uses; the stores are skipped): such chunks go sample
// by sample in the bodies below.  The host statement is the lane's own copy.
#ifdef SSR_HOST_EMU
struct SsrPitTile {};
template <typename E> struct SsrPitStage { double b[SSR_PIT_CK]; };
template <typename E> SSR_DEV void ssr_pit_request(const E* src, const void*, SsrPitTile&, SsrPitStage<E>& st) {
  if (src) for (int j = 0; j < SSR_PIT_CK; ++j) st.b[j] = (double)src[j];
}
template <typename E> SSR_DEV void ssr_pit_take(const SsrPitStage<E>& st, SsrPitTile&, double (&b)[SSR_PIT_CK]) {
  for (int j = 0; j < SSR_PIT_CK; ++j) b[j] = st.b[j];
}
SSR_DEV void ssr_pit_put(double* dst, const double (&b)[SSR_PIT_CK], SsrPitTile&) {
  if (dst) for (int j = 0; j < SSR_PIT_CK; ++j) dst[j] = b[j];
}
#else
typedef unsigned int ssr_pit_q __attribute__((ext_vector_type(4)));                   // a piece (in LDS: 16-byte aligned)
typedef unsigned int ssr_pit_qu __attribute__((ext_vector_type(4), aligned(4)));      // in global memory: at the signals' own alignment
constexpr int SSR_PIT_ROWB = SSR_PIT_CK * 8 + 16;                                     // bytes per tile row of float64 chunks
constexpr int SSR_PIT_TILEB = 64 * SSR_PIT_ROWB;
struct SsrPitTile { char* lds; int lane; };
template <typename E> struct SsrPitStage { ssr_pit_q v[SSR_PIT_CK * sizeof(E) / 16]; };
SSR_DEV const char* ssr_pit_shfl_ptr(const void* p, int lane) {
  return reinterpret_cast<const char*>((uintptr_t)__shfl((unsigned long long)(uintptr_t)p, lane, 64));
}
template <typename E> SSR_DEV void ssr_pit_request(const E* src, const void* safe, SsrPitTile& t, SsrPitStage<E>& st) {
  constexpr int P = SSR_PIT_CK * sizeof(E) / 16;
  SSR_UNROLL for (int j = 0; j < P; ++j) {
    const char* o = ssr_pit_shfl_ptr(src, j * (64 / P) + t.lane / P);
    st.v[j] = *reinterpret_cast<const ssr_pit_qu*>(o ? o + (t.lane % P) * 16 : reinterpret_cast<const char*>(safe));
  }
}
template <typename E> SSR_DEV void ssr_pit_take(const SsrPitStage<E>& st, SsrPitTile& t, double (&b)[SSR_PIT_CK]) {
  constexpr int P = SSR_PIT_CK * sizeof(E) / 16, ROWB = SSR_PIT_CK * sizeof(E) + 16;
  __syncthreads();                                                   // (one wave: the tile's previous readers are done)
  SSR_UNROLL for (int j = 0; j < P; ++j)
    *reinterpret_cast<ssr_pit_q*>(t.lds + (j * (64 / P) + t.lane / P) * ROWB + (t.lane % P) * 16) = st.v[j];
  __syncthreads();
  SSR_UNROLL for (int j = 0; j < P; ++j) {
    const ssr_pit_q v = *reinterpret_cast<const ssr_pit_q*>(t.lds + t.lane * ROWB + j * 16);
    if constexpr (sizeof(E) == 4) {
      b[4 * j] = (double)__uint_as_float(v.x); b[4 * j + 1] = (double)__uint_as_float(v.y);
      b[4 * j + 2] = (double)__uint_as_float(v.z); b[4 * j + 3] = (double)__uint_as_float(v.w);
    } else {
      b[2 * j] = __hiloint2double((int)v.y, (int)v.x); b[2 * j + 1] = __hiloint2double((int)v.w, (int)v.z);
    }
  }
}
SSR_DEV void ssr_pit_put(double* dst, const double (&b)[SSR_PIT_CK], SsrPitTile& t) {
  constexpr int P = SSR_PIT_CK * 8 / 16;
  __syncthreads();
  SSR_UNROLL for (int j = 0; j < P; ++j) {
    ssr_pit_q v;
    v.x = (unsigned)__double2loint(b[2 * j]); v.y = (unsigned)__double2hiint(b[2 * j]);
    v.z = (unsigned)__double2loint(b[2 * j + 1]); v.w = (unsigned)__double2hiint(b[2 * j + 1]);
    *reinterpret_cast<ssr_pit_q*>(t.lds + t.lane * SSR_PIT_ROWB + j * 16) = v;
  }
  __syncthreads();
  SSR_UNROLL for (int j = 0; j < P; ++j) {
    const int owner = j * (64 / P) + t.lane / P;
    const ssr_pit_q v = *reinterpret_cast<const ssr_pit_q*>(t.lds + owner * SSR_PIT_ROWB + (t.lane % P) * 16);
    char* o = const_cast<char*>(ssr_pit_shfl_ptr(dst, owner));
    if (o) *reinterpret_cast<ssr_pit_qu*>(o + (t.lane % P) * 16) = v;
  }
}
#endif

// ---- tables: lane j < 2S of design d runs the recurrence from e_j without input -----------------------------------------------
template <int S, typename X> SSR_DEV void ssr_pit_tables(const SsrPitParamsT<X>& p, int d, int j) {
  if (j >= 2 * S) return;
  double c[S][5], z[2 * S];
  ssr_pit_coef<S>(p.sos, d, c);
  SSR_UNROLL for (int i = 0; i < 2 * S; ++i) z[i] = (i == j) ? 1.0 : 0.0;
  double* H = p.H + (int64_t)d * SSR_PIT_L * SSR_PIT_ZS;
  for (int r = 0; r < SSR_PIT_L; ++r) H[r * SSR_PIT_ZS + j] = ssr_pit_step<S>(0.0, c, z);
  double* M = p.M + (int64_t)d * SSR_PIT_ZS * SSR_PIT_ZS;
  SSR_UNROLL for (int i = 0; i < 2 * S; ++i) M[i * SSR_PIT_ZS + j] = z[i];
}

// ---- forward local pass ---------------------------------------------------------------------------------------------------------
// A lane whose slot holds no segment of this design stays, with an empty segment (ne = 0): the wave's staged accesses need every lane.
template <int S, typename X> SSR_DEV void ssr_pit_fwd_local(const SsrPitParamsT<X>& p, int d, int slot, SsrPitTile& t) {
  constexpr int L = SSR_PIT_L, CK = SSR_PIT_CK;
  SsrPitSeg<X> q;
  const bool live = ssr_pit_seg<S>(p, d, slot, q);
  if (!live) { q.len = 0; q.ne = 0; q.n0 = 0; q.k = 0; q.n_seg = 1; }
  const int edge = p.edge[d];
  double c[S][5], z[2 * S];
  ssr_pit_coef<S>(p.sos, d, c);
  SSR_UNROLL for (int i = 0; i < 2 * S; ++i) z[i] = 0.0;
  // a chunk inside the signal proper is loaded whole; one that touches the odd extension or the end goes sample by sample
  auto whole_at = [&](int base) -> bool { return base >= edge && base + CK <= edge + q.len; };
  SsrPitStage<X> st{};
  ssr_pit_request(whole_at(q.n0) ? q.x + (q.n0 - edge) : (const X*)nullptr, p.H, t, st);
  for (int ch = 0; ch < L / CK; ++ch) {
    const int base = q.n0 + ch * CK;
    double b[CK];
    ssr_pit_take(st, t, b);
    const bool next_whole = ch + 1 < L / CK && whole_at(base + CK);
    ssr_pit_request(next_whole ? q.x + (base + CK - edge) : (const X*)nullptr, p.H, t, st);
    const bool some = base < q.ne, full = base + CK <= q.ne;
    if (some) {
      if (!whole_at(base)) {
        SSR_UNROLL for (int i = 0; i < CK; ++i) b[i] = (base + i < q.ne) ? ssr_iir_ext(q.x, q.len, edge, base + i) : 0.0;
      }
      SSR_UNROLL for (int i = 0; i < CK; ++i) b[i] = ssr_pit_step<S>(b[i], c, z);
    }
    ssr_pit_put(full ? q.fwd + base : (double*)nullptr, b, t);
    if (some && !full) {
      SSR_UNROLL for (int i = 0; i < CK; ++i) if (base + i < q.ne) q.fwd[base + i] = b[i];
    }
  }
  if (live && q.n0 + L <= q.ne) {              // (a partial segment is an utterance's last: nobody takes over its state)
    SSR_UNROLL for (int i = 0; i < 2 * S; ++i) p.zend[q.zoff + i] = z[i];
  }
}

// ---- backward sweeps: positions n0 + L - 1 down to n0; the forward correction is applied to what is loaded ------------------
// WRITE = false: from the zero state, end state only.  WRITE = true: from the handed-off state, y written.
template <int S, bool WRITE, typename X> SSR_DEV void ssr_pit_bwd_local(const SsrPitParamsT<X>& p, int d, int slot, SsrPitTile& t) {
  constexpr int L = SSR_PIT_L, CK = SSR_PIT_CK;
  SsrPitSeg<X> q;
  const bool live = ssr_pit_seg<S>(p, d, slot, q);
  if (!live) { q.len = 0; q.ne = 0; q.n0 = 0; q.k = 0; q.n_seg = 1; }
  const int edge = p.edge[d];
  const bool top = q.k == q.n_seg - 1;        // holds the utterance's last sample: starts from zi * fwd[-1] at that sample
  double c[S][5], z[2 * S], zf[2 * S];
  ssr_pit_coef<S>(p.sos, d, c);
  SSR_UNROLL for (int i = 0; i < 2 * S; ++i) { zf[i] = 0.0; z[i] = 0.0; }
  if (live) {
    SSR_UNROLL for (int i = 0; i < 2 * S; ++i) {
      zf[i] = p.zin_f[q.zoff + i];
      if (WRITE && !top) z[i] = p.zin_b[q.zoff + i];
    }
  }
  const ssr_pit_row H = ssr_pit_uniform(p.H + (int64_t)d * L * SSR_PIT_ZS);
  const ssr_pit_row zi = ssr_pit_uniform(p.zi + (int64_t)d * SSR_PIT_ZS);
  // a chunk below the utterance's last sample is loaded whole; the one that holds it (or reaches past it) goes sample by sample
  auto whole_at = [&](int base) -> bool { return base + CK <= q.ne && !(top && base + CK == q.ne); };
  SsrPitStage<double> st{};
  ssr_pit_request(whole_at(q.n0 + L - CK) ? q.fwd + (q.n0 + L - CK) : (const double*)nullptr, p.H, t, st);
  for (int ch = 0; ch < L / CK; ++ch) {
    const int r0 = L - CK * (ch + 1);          // row of H of the chunk's lowest position (wave-uniform)
    const int base = q.n0 + r0;
    double b[CK];
    ssr_pit_take(st, t, b);
    const bool next_whole = r0 >= CK && whole_at(base - CK);
    ssr_pit_request(next_whole ? q.fwd + (base - CK) : (const double*)nullptr, p.H, t, st);
    const bool some = base < q.ne;
    if (some && whole_at(base)) {
      SSR_UNROLL for (int i = CK - 1; i >= 0; --i) {
        const double v = b[i] + ssr_pit_dot<S>(H + (r0 + i) * SSR_PIT_ZS, zf);
        b[i] = ssr_pit_step<S>(v, c, z);
      }
    } else if (some) {
      SSR_UNROLL for (int i = CK - 1; i >= 0; --i) {
        const int n = base + i;
        if (n < q.ne) {
          const double v = q.fwd[n] + ssr_pit_dot<S>(H + (r0 + i) * SSR_PIT_ZS, zf);
          if (n == q.ne - 1) {
            SSR_UNROLL for (int j = 0; j < 2 * S; ++j) z[j] = zi[j] * v;
          }
          b[i] = ssr_pit_step<S>(v, c, z);
        } else {
          b[i] = 0.0;
        }
      }
    }
    if constexpr (WRITE) {
      const int m0 = base - edge;               // y[m] = bwd at position m + edge
      const bool full = some && m0 >= 0 && m0 + CK <= q.len;
      ssr_pit_put(full ? q.y + m0 : (double*)nullptr, b, t);
      if (some && !full) {
        SSR_UNROLL for (int i = 0; i < CK; ++i) if (m0 + i >= 0 && m0 + i < q.len) q.y[m0 + i] = b[i];
      }
    }
  }
  if constexpr (!WRITE) {
    if (live) {
      SSR_UNROLL for (int i = 0; i < 2 * S; ++i) p.zend[q.zoff + i] = z[i];
    }
  }
}

// ---- hand-off scans: one (design, utterance) per 16-lane group, lane j = row j of M ----------------------------------------
// z_j <- e_j + sum_c M[j][c] z_c  (c ascending, two interleaved partial sums).  ONE statement for both builds: the device runs it
// with one row per lane (NL = 1: the arrays below have one element, the other rows' z come by shuffle inside the 16-lane group, and
// every lane of a group runs the same trip count); the host runs all 16 rows in one call (NL = 16: the arrays are indexed by row).
#ifdef SSR_HOST_EMU
constexpr int SSR_PIT_NL = 16;
#else
constexpr int SSR_PIT_NL = 1;
#endif
template <int NL> SSR_DEV double ssr_pit_row_z(const double (&z)[NL], int li, int c) {
#ifdef SSR_HOST_EMU
  (void)li;
  return z[c];
#else
  (void)c;
  return __shfl(z[li], c, 16);
#endif
}
template <int S, bool BACKWARD, typename X> SSR_DEV void ssr_pit_scan_item(const SsrPitParamsT<X>& p, int d, int item, int lane) {
  constexpr int L = SSR_PIT_L, R = 2 * S, NL = SSR_PIT_NL;
  const int edge = p.edge[d], len = p.len[item], ne = len + 2 * edge, K = (ne + L - 1) / L;
  const int64_t zb = (int64_t)d * p.n_slots * SSR_PIT_ZS + (int64_t)ssr_pit_slot_base(p.off[item], item, p.emax) * R;
  auto row_of = [&](int li) -> int { return NL == 1 ? lane : li; };             // lanes / rows >= R compute row 0 again and write nothing
  auto jr_of = [&](int li) -> int { return row_of(li) < R ? row_of(li) : 0; };
  double m[NL][R], z[NL], e[NL], nz[NL], en[NL];
  SSR_UNROLL for (int li = 0; li < NL; ++li) {
    SSR_UNROLL for (int c = 0; c < R; ++c) m[li][c] = p.M[((int64_t)d * SSR_PIT_ZS + jr_of(li)) * SSR_PIT_ZS + c];
  }
  const double* zend = p.zend + zb;
  // the next segment's end state is requested ahead of the dependent chain
  auto advance = [&](bool more, int64_t k_next) {
    SSR_UNROLL for (int li = 0; li < NL; ++li) {
      en[li] = more ? zend[k_next * R + jr_of(li)] : 0.0;
      double a0 = 0.0, a1 = 0.0;
      SSR_UNROLL for (int s = 0; s < S; ++s) {
        a0 += m[li][2 * s] * ssr_pit_row_z<NL>(z, li, 2 * s);
        a1 += m[li][2 * s + 1] * ssr_pit_row_z<NL>(z, li, 2 * s + 1);
      }
      nz[li] = e[li] + (a0 + a1);
    }
    SSR_UNROLL for (int li = 0; li < NL; ++li) { z[li] = nz[li]; e[li] = en[li]; }
  };
  if constexpr (!BACKWARD) {
    double* zin = p.zin_f + zb;
    const double x0 = ssr_iir_ext(p.x + p.off[item], len, edge, 0);
    SSR_UNROLL for (int li = 0; li < NL; ++li) {
      z[li] = p.zi[(int64_t)d * SSR_PIT_ZS + jr_of(li)] * x0;
      e[li] = K > 1 ? zend[jr_of(li)] : 0.0;
    }
    for (int k = 0; k < K; ++k) {
      SSR_UNROLL for (int li = 0; li < NL; ++li) if (row_of(li) < R) zin[(int64_t)k * R + row_of(li)] = z[li];
      if (k + 1 < K) advance(k + 2 < K, k + 1);
    }
  } else {
    double* zin = p.zin_b + zb;
    SSR_UNROLL for (int li = 0; li < NL; ++li) if (row_of(li) < R) zin[(int64_t)(K - 1) * R + row_of(li)] = 0.0;
    if (K < 2) return;
    SSR_UNROLL for (int li = 0; li < NL; ++li) {
      z[li] = zend[(int64_t)(K - 1) * R + jr_of(li)];
      e[li] = K > 2 ? zend[(int64_t)(K - 2) * R + jr_of(li)] : 0.0;
    }
    for (int k = K - 2; k >= 0; --k) {
      SSR_UNROLL for (int li = 0; li < NL; ++li) if (row_of(li) < R) zin[(int64_t)k * R + row_of(li)] = z[li];
      if (k > 0) advance(k > 1, k - 1);
    }
  }
}

// f.template operator()<S>() for the design's section count (wave-uniform)
#define SSR_PIT_DISPATCH(S_, CALL)                    \
  switch (S_) {                                       \
    case 1: { constexpr int S = 1; CALL; } break;     \
    case 2: { constexpr int S = 2; CALL; } break;     \
    case 3: { constexpr int S = 3; CALL; } break;     \
    case 4: { constexpr int S = 4; CALL; } break;     \
    case 5: { constexpr int S = 5; CALL; } break;     \
    case 6: { constexpr int S = 6; CALL; } break;     \
    case 7: { constexpr int S = 7; CALL; } break;     \
    default: { constexpr int S = 8; CALL; } break;    \
  }
