// Host emulation of the mel-distance kernel bodies (ssr_eval_amd/csrc/ssr_mel.h) for tests/test_mel_host.py: every kernel of
// ssr_pair_mel_metrics after the transform, run in launch order, one workgroup after another.  Test infrastructure; not part of
// the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libmel_emu.so mel_emu.cpp
#define SSR_HOST_EMU 1
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_mel.h"

struct FbStore {
  std::vector<int32_t> sched_bin, seg_first;
  std::vector<float> sched_w;
  std::vector<double> dct;
  SsrMelFb f;
  FbStore(const float* fb, int n_bins, int n_mels, int n_cep)
      : seg_first(n_mels + 1), dct((size_t)n_mels * (n_cep > 0 ? n_cep : 1)) {
    int nnz = 0;
    for (int m = 0; m < n_mels; ++m) {
      int lo = -1, hi = -1;
      for (int b = 0; b < n_bins; ++b)
        if (fb[(int64_t)b * n_mels + m] != 0.0f) { if (lo < 0) lo = b; hi = b + 1; }
      nnz += hi - lo;
    }
    const int steps = (nnz + SSR_MEL_NT - 1) / SSR_MEL_NT;
    sched_bin.assign((size_t)steps * SSR_MEL_NT, -1);
    sched_w.assign((size_t)steps * SSR_MEL_NT, -1.0f);
    f.fb = fb; f.sched_bin = sched_bin.data(); f.sched_w = sched_w.data(); f.seg_first = seg_first.data(); f.dct = dct.data();
    f.n_bins = n_bins; f.n_mels = n_mels; f.n_cep = n_cep; f.steps = steps;
    std::vector<int> lo(SSR_MEL_MAX), wd(SSR_MEL_MAX), start(SSR_MEL_MAX);
    SsrBlk blk{SSR_MEL_SCHED_NT};
    ssr_mel_schedule_body(f, blk, lo.data(), wd.data(), start.data());
  }
};

// est: n_keys planes of x_plane floats, item i from row row_off[i] (pitch floats per row); tgt: one plane.  out [n_items][n_keys][3]
extern "C" int mel_emu_metrics(const float* est, int64_t x_plane, const float* tgt, const int64_t* row_off, const int32_t* n_rows,
                               int n_items, int n_keys, int kg, int F, int pitch, const float* fb, int n_mels, int n_cep, int which,
                               double* out) {
  if (n_keys % kg) return -1;
  FbStore st(fb, F, n_mels, n_cep);
  int max_rows = 0;
  for (int i = 0; i < n_items; ++i) max_rows = n_rows[i] > max_rows ? n_rows[i] : max_rows;
  SsrMelParams p{};
  p.x = est; p.y = tgt; p.x_row = row_off; p.y_row = row_off; p.n_rows = n_rows; p.f = st.f; p.x_plane = x_plane;
  p.F = F; p.pitch = pitch; p.n_items = n_items; p.n_chunks = (max_rows + SSR_MEL_RUN - 1) / SSR_MEL_RUN; p.kg = kg; p.which = which;
  std::vector<double> part((size_t)n_keys * n_items * p.n_chunks * 3, -1.0);
  p.part = part.data();
  std::vector<float> buf(((F + 3) & ~3) + 4);
  std::vector<double> seg(SSR_MEL_SEGS), dl(SSR_MEL_MAX), cp(SSR_MEL_MAX), red(4), tot(3 * kg);
  SsrBlk blk{SSR_MEL_NT};
  const int64_t grid = (int64_t)(n_keys / kg) * n_items * p.n_chunks;
  for (int64_t g = 0; g < grid; ++g) {
    if (pitch % 4 == 0) ssr_mel_metrics_body<true>(p, blk, (int)(g % p.n_chunks), (int)(g / p.n_chunks), buf.data(), seg.data(), dl.data(), cp.data(), red.data(), tot.data());
    else ssr_mel_metrics_body<false>(p, blk, (int)(g % p.n_chunks), (int)(g / p.n_chunks), buf.data(), seg.data(), dl.data(), cp.data(), red.data(), tot.data());
  }
  SsrMelFinalizeParams fp{p.part, n_rows, p.n_chunks, n_items, n_keys, n_mels, which, out};
  for (int64_t i = 0; i < (int64_t)n_keys * n_items * 3; ++i) ssr_mel_finalize(fp, i);
  return 0;
}

// projection: images of n_rows[i] rows from row_off[i] (pitch F) -> out rows at the same offsets (pitch n_mels)
extern "C" int mel_emu_project(const float* sp, const int64_t* row_off, const int32_t* n_rows, int n_items, int F, const float* fb,
                               int n_mels, float* out) {
  FbStore st(fb, F, n_mels, 0);
  int max_rows = 0;
  for (int i = 0; i < n_items; ++i) max_rows = n_rows[i] > max_rows ? n_rows[i] : max_rows;
  SsrMelParams p{};
  p.x = sp; p.y = sp; p.x_row = row_off; p.y_row = row_off; p.n_rows = n_rows; p.f = st.f;
  p.F = F; p.pitch = F; p.n_items = n_items; p.n_chunks = (max_rows + SSR_MEL_RUN - 1) / SSR_MEL_RUN; p.kg = 1; p.mel = out;
  std::vector<float> buf(((F + 3) & ~3) + 4);
  std::vector<double> seg(SSR_MEL_SEGS);
  SsrBlk blk{SSR_MEL_NT};
  for (int64_t g = 0; g < (int64_t)n_items * p.n_chunks; ++g)
    ssr_mel_project_body<false>(p, blk, (int)(g % p.n_chunks), (int)(g / p.n_chunks), buf.data(), seg.data());
  return 0;
}

// the schedule of a table: steps, then every entry covered once (-1 in the output = untouched) -> sched_bin / sched_w / seg_first
extern "C" int mel_emu_schedule(const float* fb, int n_bins, int n_mels, int32_t* bin_out, float* w_out, int32_t* seg_first_out, int cap) {
  FbStore st(fb, n_bins, n_mels, 1);
  const int n = st.f.steps * SSR_MEL_NT;
  if (n > cap) return -1;
  for (int i = 0; i < n; ++i) { bin_out[i] = st.sched_bin[i]; w_out[i] = st.sched_w[i]; }
  for (int m = 0; m <= n_mels; ++m) seg_first_out[m] = st.seg_first[m];
  return st.f.steps;
}
