"""GPU tests (-m gpu) of k_stft_wave's frame loop after the fused windowed first pass (ssr_dft32_win) and the earlier table requests
(ssr_stft_wave.h), at the smallest batch that reaches every path of the loop.  One batch of seven pairs at 2048 / 512:

  1 sample; 700 samples (every frame reflected); 2048; 6,656 (14 frames); one pair of 1,030 frames; one whose estimate is all zeros;
  one with a silent stretch longer than a frame in the estimate and, elsewhere, in the target.

The long pair: the geometry of each batch is read back from the host functions that pick it (ssr_pair_units_per_chunk,
ssr_pair_interleave of ssr_host.h, called in the shipped library) and the test asserts that 1,030 frames lie in more than one chunk and
more than one interleave group under it.
The masks LSD, LSD | SSIM, LSD | SISpec | log-SISpec and all four run the four SUMS x MAG instantiations; SSIM only on the pairs of
seven frames or more.

Bars, float64 plans: magnitude rows within 2e-7 of the largest bin of the oracle's (tests/test_gpu_parity.py), LSD and SSIM within 1e-5
of the oracle (the same file), and LSD, SISpec and SSIM within 1e-7 of the block engine's - the four-waves-per-frame engine of
ssr_stft.h, the bar of tests/test_emu_kernels.py::test_wave_autonomous_engine_matches_oracle_and_block_engine; here both engines run
on the GPU.  The two SISpec values are held to the block engine only: on the 1,030-frame pair the oracle's own float32 sums are 3e-5
(log-SISpec) and 9e-6 (SISpec) away from both engines, which agree with each other to 1e-9 there in the host emulation.
log-SISpec, wave engine against block engine at 1e-7, is taken from the TRANSFORMS: float64 on the host from the magnitude rows each
engine writes for the same batch (test_log_sispec_of_the_rows_...), which is everything pass 0 and the window can influence.  The
value the wave kernel's own epilogue reports is 2e-7 ... 7e-6 away from the block engine's on this batch - its float32 logarithms are
packed v_log_f32 sequences of about 1 ulp, the block engine's are not; the epilogue is not part of this change and the parent commit's
library gives the same 7.24e-6 - and is held to the 1e-5 the GPU parity tests give that metric.
The 1-sample pair reflects into a constant frame: two bins carry the spectrum, the others are round-off, so its LSD and SISpec over all
bins are defined by round-off (tests/test_gpu_parity.py::test_short_signals_reflect_repeatedly_like_numpy_pad leaves such signals out of
the metrics for that reason; the block engine and the oracle differ by 10 % on it).  What is well defined is asserted: its magnitude
rows within 2e-7 of the largest bin of the oracle's, and the LSD over its two carrying bins, from those rows, within 1e-5 of the oracle's.
float32 plans are not the reference's arithmetic (eps = 1.2e-7; the transform alone is 3e-7 of the largest bin off); they keep the bars
the project holds them to: rows 3e-6 of the largest bin (tests/test_gpu_parity.py), metrics 5e-5
(tests/test_gpu_configs.py::test_float32_precision_plans_all_metrics)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_FFT, HOP, F = 2048, 512, 1025
LONG_FRAMES = 1030
BIG = [3, 4, 5, 6]                               # the pairs of seven frames or more


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from ssr_eval_amd import _lib
    _lib.load()


@pytest.fixture(scope="module")
def batch():
    """(estimates, targets, oracle metrics [7, 4] with NaN where SSIM has no image, oracle magnitude rows of every pair)."""
    from oracle import metrics as om
    from oracle import stft as ostft
    rng = np.random.default_rng(20480512)
    lens = [1, 700, 2048, 6656, (LONG_FRAMES - 1) * HOP + 17, 9 * HOP + 300, 7 * HOP + 3 * N_FFT]
    tgts = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    ests = [(0.8 * t + 0.02 * rng.standard_normal(len(t))).astype(np.float32) for t in tgts]
    ests[5][:] = 0.0
    n = lens[6]
    ests[6][n // 3: n // 3 + N_FFT + 2 * HOP] = 0.0
    tgts[6][n // 2: n // 2 + N_FFT + HOP + 5] = 0.0
    assert ostft.num_frames(lens[4], N_FFT, HOP) == LONG_FRAMES
    want = np.full((len(lens), 4), np.nan)
    for i, (e, t) in enumerate(zip(ests, tgts)):
        es, ts = om.wav_to_spectrogram(e, N_FFT, HOP), om.wav_to_spectrogram(t, N_FFT, HOP)
        want[i, :3] = [float(om.lsd(es, ts)), float(om.sispec(om.to_log(es), om.to_log(ts))), float(om.sispec(es, ts))]
        if i in BIG:
            want[i, 3] = float(om.ssim(es, ts))
    rows = {i: (ostft.stft_mag_TF(ests[i], N_FFT, HOP), ostft.stft_mag_TF(tgts[i], N_FFT, HOP)) for i in range(len(lens))}
    want.setflags(write=False)
    return ests, tgts, want, rows


@pytest.fixture(scope="module")
def block_engine(batch):
    """[7, 4] metrics of the block engine on the GPU: the same samples widened to float64 (exact) take ssr_pair_metrics_f64, whose
    transform is the four-waves-per-frame engine (ssr_stft_uses_wave_engine: float64 inputs never run k_stft_wave); SSIM only where it
    exists."""
    from ssr_eval_amd import backend as B
    ests, tgts, _want, _rows = batch
    plan = B.get_plan(N_FFT, HOP, "f64")
    e64, t64 = [e.astype(np.float64) for e in ests], [t.astype(np.float64) for t in tgts]
    out = np.full((len(ests), 4), np.nan)
    out[:, :3] = B.pair_metrics(plan, e64, t64, B.M_LSD | B.M_SISPEC | B.M_LOG_SISPEC)[:, :3]
    out[BIG] = B.pair_metrics(plan, [e64[i] for i in BIG], [t64[i] for i in BIG], B.M_ALL)
    out.setflags(write=False)
    return out


def geometry(plan, n_items, max_len):
    """(frames per chunk, chunks per interleave group) of the pair transform for a batch of float32 signals: what ssr_pair_geom asks
    the library's host functions (C++ linkage: ssr_host.h)."""
    import ctypes as C
    upc = getattr(plan.lib, "_Z24ssr_pair_units_per_chunkPK8ssr_planiib")
    ilv = getattr(plan.lib, "_Z19ssr_pair_interleavePK8ssr_planb")
    upc.restype, upc.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_bool]
    ilv.restype, ilv.argtypes = C.c_int, [C.c_void_p, C.c_bool]
    return int(upc(plan.handle, plan.frames(max_len), n_items, False)), int(ilv(plan.handle, False))


def assert_long_pair_spans_groups(plan, items, ests):
    u, S = geometry(plan, len(items), max(len(ests[i]) for i in items))
    print("    geometry read back: %d frames per chunk, %d chunks per interleave group" % (u, S))
    assert 4 in items and u >= 1 and S > 1
    assert LONG_FRAMES > u and LONG_FRAMES > u * S, (u, S)           # more than one chunk, more than one interleave group


def pair_rows(plan, ests, tgts, widen=False):
    """(rows of the estimates, rows of the targets): the magnitude images of the pair transform, through ssr_pair_lsd_bands with one key
    and one band - ssr_pair_images (ssr_pair_transform.h) leaves the estimates' plane, then the targets', at the head of its workspace,
    rows of ssr_mag_pitch(F) floats, item i from row frame_off[i]; no minimum number of frames.  float32 signals run
    k_stft_wave<T, false, true, true>; widen: the estimates as float64 (exact), which takes the block engine."""
    from ssr_eval_amd import _lib
    from ssr_eval_amd import backend as B
    n = len(tgts)
    with torch.cuda.device(plan.device):
        est = B.Ragged.from_list_keep64([e.astype(np.float64) for e in ests] if widen else ests, plan.device, allow_gaps=True)
        tgt = B.Ragged.from_list(tgts, plan.device, allow_gaps=True)
        r = B._Rows(plan, tgt.lens_host, tgt.device)
        ws_bytes = int(plan.lib.ssr_pair_lsd_bands_workspace_bytes(plan.handle, n, 1, tgt.max_len, r.total, 1))
        ws = B._workspace(ws_bytes, tgt.device)
        out = torch.empty((n, 1, 1), dtype=torch.float64, device=tgt.device)
        edges = B._host_i32(np.tile(np.array([0, F], np.int32), (n, 1)), plan.device)
        fn = plan.lib.ssr_pair_lsd_bands_est64 if widen else plan.lib.ssr_pair_lsd_bands
        _lib.check(fn(plan.handle, B._vp(est.data), B._vp(est.off), B._vp(tgt.data), B._vp(tgt.off), B._vp(tgt.len), B._vp(r.off), n, 1,
                      tgt.max_len, r.total, B._vp(edges), 1, B._vp(out), B._vp(ws), ws_bytes, B._stream()))
        torch.cuda.synchronize()
        pitch = (F + 3) & ~3
        plane = (r.total * pitch * 4 + 255) & ~255
        host = ws[:2 * plane].cpu().numpy()
    img = [host[k * plane:k * plane + r.total * pitch * 4].view(np.float32).reshape(r.total, pitch)[:, :F] for k in (0, 1)]
    return tuple([im[r.off_host[j]:r.off_host[j] + r.T[j]] for j in range(n)] for im in img)


def log_sispec64(e_rows, t_rows):
    """log-SISpec of two magnitude images, the oracle's formula in float64."""
    from oracle import metrics as om
    e, t = (torch.from_numpy(np.ascontiguousarray(x, np.float64))[None, None] for x in (e_rows, t_rows))
    return float(om.sispec(om.to_log(e), om.to_log(t)))


def _masks(B):
    """(mask, items, metric columns) of the four k_stft_wave<T, SUMS, true, MAG> instantiations"""
    every = list(range(7))
    return [(B.M_LSD, every, [0]),                                                   # SUMS = false, MAG = false
            (B.M_LSD | B.M_SSIM, BIG, [0, 3]),                                       # SUMS = false, MAG = true (bench.py's cfg-2)
            (B.M_LSD | B.M_SISPEC | B.M_LOG_SISPEC, every, [0, 1, 2]),               # SUMS = true, MAG = false
            (B.M_ALL, BIG, [0, 1, 2, 3])]                                            # SUMS = true, MAG = true


def _close(got, want, rtol, atol=0.0):
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print("    largest relative difference %.3e (bar %.1e)" % (float(err.max()), rtol))
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_metrics_of_every_instantiation_against_oracle_and_block_engine(batch, block_engine, prec):
    from ssr_eval_amd import backend as B
    ests, tgts, want, _rows = batch
    plan = B.get_plan(N_FFT, HOP, prec)
    for mask, items, cols in _masks(B):
        print("%s mask %d:" % (prec, mask))
        assert_long_pair_spans_groups(plan, items, ests)
        got = B.pair_metrics(plan, [ests[i] for i in items], [tgts[i] for i in items], mask)
        assert np.isfinite(got[:, cols]).all()
        keep = [j for j, i in enumerate(items) if i != 0]            # the 1-sample pair: test_one_sample_pair_..., see the module docstring
        items, got = [items[j] for j in keep], got[keep]
        ref_cols = [c for c in cols if c in (0, 3)]                  # LSD / SSIM against the oracle
        if prec == "f64":
            _close(got[:, ref_cols], want[items][:, ref_cols], 1e-5)
            tight = [c for c in cols if c != 1]                      # log-SISpec: see the module docstring
            _close(got[:, tight], block_engine[items][:, tight], 1e-7)
            if 1 in cols:
                _close(got[:, [1]], block_engine[items][:, [1]], 1e-5)
        else:
            _close(got[:, ref_cols], want[items][:, ref_cols], 5e-5, 5e-5)
            _close(got[:, cols], block_engine[items][:, cols], 5e-5, 5e-5)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_magnitude_rows_against_the_oracle(batch, prec):
    """The images k_stft_wave<T, *, true, true> leaves at the head of the workspace (ssr_pair_transform.h: the estimates' plane, then
    the targets', rows of ssr_mag_pitch(F) floats, item i from row frame_off[i]); exact zeros in silent frames and only there."""
    from ssr_eval_amd import backend as B
    ests, tgts, _want, rows = batch
    plan = B.get_plan(N_FFT, HOP, prec)
    bar = 2e-7 if prec == "f64" else 3e-6
    for mask in (B.M_LSD | B.M_SSIM, B.M_ALL):
        with torch.cuda.device(plan.device):
            b = B.PairBatch(plan, B.Ragged.from_list([ests[i] for i in BIG], plan.device), B.Ragged.from_list([tgts[i] for i in BIG], plan.device))
            b.run(mask)
            torch.cuda.synchronize()
            pitch = (F + 3) & ~3
            plane = (b.rows.total * pitch * 4 + 255) & ~255
            ws = b.ws.cpu().numpy()
        worst = 0.0
        for k, name in enumerate(("estimate", "target")):
            img = ws[k * plane:k * plane + b.rows.total * pitch * 4].view(np.float32).reshape(b.rows.total, pitch)[:, :F]
            for j, i in enumerate(BIG):
                m, ref = img[b.rows.off_host[j]:b.rows.off_host[j] + b.rows.T[j]], rows[i][k]
                assert m.shape == ref.shape, (name, i)
                if ref.max() > 0:
                    worst = max(worst, float(np.abs(m - ref).max() / ref.max()))
                assert np.abs(m - ref).max() <= bar * ref.max(), (name, i)
                assert ((m == 0) == (ref == 0)).all(), (name, i)
        print("%s mask %d: rows within %.3e of the largest bin (bar %.1e)" % (prec, mask, worst, bar))
    assert (rows[5][0] == 0).all() and (rows[6][0] == 0).all(axis=1).any() and (rows[6][1] == 0).all(axis=1).any()


@pytest.fixture(scope="module")
def transform_rows(batch):
    """{precision: (estimate rows, target rows)} of all seven pairs out of k_stft_wave, and the block engine's (float64 plan)."""
    from ssr_eval_amd import backend as B
    ests, tgts, _want, _rows = batch
    out = {prec: pair_rows(B.get_plan(N_FFT, HOP, prec), ests, tgts) for prec in ("f64", "f32")}
    out["block"] = pair_rows(B.get_plan(N_FFT, HOP, "f64"), ests, tgts, widen=True)
    return out


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_rows_of_every_pair_against_the_oracle(batch, transform_rows, prec):
    """All seven pairs, the 1-sample one among them, through the instantiation that writes rows without asking for seven frames."""
    from ssr_eval_amd import backend as B
    ests, _tgts, _want, rows = batch
    assert_long_pair_spans_groups(B.get_plan(N_FFT, HOP, prec), list(range(7)), ests)
    bar = 2e-7 if prec == "f64" else 3e-6
    worst = 0.0
    for k in (0, 1):
        for i in range(7):
            m, ref = transform_rows[prec][k][i], rows[i][k]
            assert m.shape == ref.shape, (k, i)
            if ref.max() > 0:
                worst = max(worst, float(np.abs(m - ref).max() / ref.max()))
            assert np.abs(m - ref).max() <= bar * ref.max(), (k, i)
            if i in BIG:
                assert ((m == 0) == (ref == 0)).all(), (k, i)
    print("%s: rows of all seven pairs within %.3e of the largest bin (bar %.1e)" % (prec, worst, bar))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_one_sample_pair_what_is_well_defined(batch, transform_rows, prec):
    """One sample reflects into a constant frame c: the windowed spectrum is c N / 4 in bin 0, c N / 8 in bin 1 and round-off elsewhere.
    The two carrying bins against the oracle's (the rows bar), the other bins below that bar of the largest, and the LSD over the two
    carrying bins - the oracle's formula on the kernel's rows - within 1e-5 of the same on the oracle's rows (float32 plan: 5e-5)."""
    from oracle import metrics as om
    _ests, _tgts, _want, rows = batch
    bar = 2e-7 if prec == "f64" else 3e-6
    got = [transform_rows[prec][k][0] for k in (0, 1)]
    ref = [rows[0][k] for k in (0, 1)]
    for g, r in zip(got, ref):
        assert g.shape == r.shape == (1, F) and r[0, 0] > 0 and r[0, 1] > 0
        assert np.abs(g[0, :2] - r[0, :2]).max() <= bar * r.max()
        assert g[0, 2:].max() <= bar * r.max() and r[0, 2:].max() <= bar * r.max()
    lsd2 = lambda e, t: float(om.lsd(torch.from_numpy(e[None, None, :, :2].copy()), torch.from_numpy(t[None, None, :, :2].copy())))
    a, b = lsd2(got[0], got[1]), lsd2(ref[0], ref[1])
    print("%s: LSD over the two carrying bins %.9g, oracle rows %.9g" % (prec, a, b))
    assert b > 0
    np.testing.assert_allclose(a, b, rtol=1e-5 if prec == "f64" else 5e-5)


def test_log_sispec_of_the_rows_wave_engine_against_block_engine(batch, transform_rows):
    """What the transform - pass 0 and its window included - contributes to log-SISpec, at the 1e-7 of the engine parity tests: the
    oracle's formula in float64 on the rows of k_stft_wave against the same on the block engine's rows, every pair but the 1-sample
    one (round-off, see the module docstring)."""
    worst = 0.0
    for i in range(1, 7):
        w = log_sispec64(transform_rows["f64"][0][i], transform_rows["f64"][1][i])
        b = log_sispec64(transform_rows["block"][0][i], transform_rows["block"][1][i])
        worst = max(worst, abs(w - b) / abs(b))
        np.testing.assert_allclose(w, b, rtol=1e-7, err_msg="pair %d" % i)
    print("log-SISpec from the rows, wave against block engine: largest relative difference %.3e (bar 1.0e-07)" % worst)
