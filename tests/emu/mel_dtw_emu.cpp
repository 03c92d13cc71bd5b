// Host emulation of the DTW mel-cepstral distortion kernel bodies (ssr_eval_amd/csrc/ssr_mel_dtw.h) for tests/test_mel_dtw_host.py:
// the schedule, the cepstra of every plane and the warp of every (item, key), in launch order, one workgroup after another.  Test
// infrastructure; not part of the library.
// g++ -O2 -std=c++17 -shared -fPIC -o libmel_dtw_emu.so mel_dtw_emu.cpp
#define SSR_HOST_EMU 1
#include <vector>

#include "../../ssr_eval_amd/csrc/ssr_mel_dtw.h"

// cep: [n_keys + 1 planes][total rows][n_cep] (plane n_keys: the targets), item i from row row_off[i] -> out [n_items][n_keys][3]
static void run_dtw(const double* cep, int64_t c_plane, const int64_t* row_off, const int32_t* n_rows, int n_items, int n_keys, int n_cep,
                    int radius, double* out) {
  SsrMelDtwParams d{cep, row_off, n_rows, c_plane, 0, n_items, n_keys, n_cep, radius, out};
  std::vector<double> xd(SSR_MEL_NT);
  std::vector<int> xl(SSR_MEL_NT), xv(SSR_MEL_NT);
  SsrBlk blk{SSR_MEL_NT};
  for (int v = 0; v < n_keys * n_items; ++v) ssr_mel_dtw_body(d, blk, v, xd.data(), xl.data(), xv.data());
}

// the warp alone on injected cepstra
extern "C" int mel_dtw_emu_warp(const double* cep, int64_t total_rows, const int64_t* row_off, const int32_t* n_rows, int n_items, int n_keys,
                                int n_cep, int radius, double* out) {
  run_dtw(cep, total_rows * n_cep, row_off, n_rows, n_items, n_keys, n_cep, radius, out);
  return 0;
}

// the chain: est = n_keys planes of x_plane floats, item i from row row_off[i] (pitch floats per row); tgt: one plane.
// out [n_items][n_keys][3]; cep_out (optional): [n_keys + 1][total_rows][n_cep]
extern "C" int mel_dtw_emu_chain(const float* est, int64_t x_plane, const float* tgt, const int64_t* row_off, const int32_t* n_rows,
                                 int n_items, int n_keys, int64_t total_rows, int F, int pitch, const float* fb, int n_mels, int n_cep,
                                 int radius, double* out, double* cep_out) {
  std::vector<int32_t> sched_bin, seg_first(n_mels + 1);
  std::vector<float> sched_w;
  std::vector<double> dct((size_t)n_mels * n_cep);
  int nnz = 0;
  for (int m = 0; m < n_mels; ++m)
    for (int b = 0; b < F; ++b) nnz += fb[(int64_t)b * n_mels + m] != 0.0f;
  SsrMelCepParams c{};
  c.f.steps = (nnz + SSR_MEL_NT - 1) / SSR_MEL_NT;
  sched_bin.assign((size_t)c.f.steps * SSR_MEL_NT, -1);
  sched_w.assign((size_t)c.f.steps * SSR_MEL_NT, -1.0f);
  c.f.fb = fb; c.f.sched_bin = sched_bin.data(); c.f.sched_w = sched_w.data(); c.f.seg_first = seg_first.data(); c.f.dct = dct.data();
  c.f.n_bins = F; c.f.n_mels = n_mels; c.f.n_cep = n_cep;
  {
    std::vector<int> lo(SSR_MEL_MAX), wd(SSR_MEL_MAX), start(SSR_MEL_MAX);
    SsrBlk blk{SSR_MEL_SCHED_NT};
    ssr_mel_schedule_body(c.f, blk, lo.data(), wd.data(), start.data());
  }
  int max_rows = 0;
  for (int i = 0; i < n_items; ++i) max_rows = n_rows[i] > max_rows ? n_rows[i] : max_rows;
  std::vector<double> cep((size_t)(n_keys + 1) * total_rows * n_cep, -7.0);
  c.x = est; c.y = tgt; c.x_row = row_off; c.y_row = row_off; c.n_rows = n_rows; c.c_row = row_off;
  c.x_plane = x_plane; c.c_plane = total_rows * n_cep; c.c_stride = 0;
  c.F = F; c.pitch = pitch; c.n_items = n_items; c.n_chunks = (max_rows + SSR_MEL_RUN - 1) / SSR_MEL_RUN; c.n_keys = n_keys; c.cep = cep.data();
  std::vector<float> buf(((F + 3) & ~3) + 4);
  std::vector<double> seg(SSR_MEL_SEGS), dl(SSR_MEL_MAX), cp(SSR_MEL_MAX);
  SsrBlk blk{SSR_MEL_NT};
  const int64_t grid = (int64_t)(n_keys + 1) * n_items * c.n_chunks;
  for (int64_t g = 0; g < grid; ++g) {
    if (pitch % 4 == 0) ssr_mel_cepstra_body<true>(c, blk, (int)(g % c.n_chunks), (int)(g / c.n_chunks), buf.data(), seg.data(), dl.data(), cp.data());
    else ssr_mel_cepstra_body<false>(c, blk, (int)(g % c.n_chunks), (int)(g / c.n_chunks), buf.data(), seg.data(), dl.data(), cp.data());
  }
  if (cep_out)
    for (size_t i = 0; i < cep.size(); ++i) cep_out[i] = cep[i];
  run_dtw(cep.data(), c.c_plane, row_off, n_rows, n_items, n_keys, n_cep, radius, out);
  return 0;
}
