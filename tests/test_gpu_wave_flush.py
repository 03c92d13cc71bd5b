"""GPU tests (-m gpu) of k_stft_wave's stash-and-flush epilogue (ssr_stft_wave.h, STASH): the Nyquist bin and the close of a frame's
LSD are kept with the frame's owner lane and finished by all lanes at once in a flush behind every 64 frames and in the chunk tail.
One batch of seven ragged pairs at 2048 / 512:

  1 sample; 2,047 samples; an all-zero estimate (9 frames); an all-zero target (9 frames); 140 frames; 14 frames; one with a silent
  stretch longer than a frame in the estimate and, elsewhere, in the target.

Every chunk of this batch is shorter than 64 frames (the geometry is read back from the library as tests/test_gpu_pass0.py does, and
asserted): each chunk ends in a flush of fewer than 64 frames.

A second batch reaches the flush in the MIDDLE of a chunk: the host picks ceil(longest item's frames x items / 16,384) frames per
chunk, at most 128 (tu_core.hip: ssr_units_per_chunk_for), so one pair of 2,100 frames beside 511 short pairs - a ragged batch of about
30 MB - runs at 66 frames per chunk and 8 chunks per interleave group: a full 64-lane flush with row offsets of 8 rows per lane, the
stash reset, and a second block of two frames.  The geometry is read back and asserted (more than 64).  The long pair's target is
silent across the frames a chunk's 64th and 65th frame fall on, its estimate across the last frames.  The 511 short pairs are one
seven-frame pair repeated: one oracle value, and 511 results that must be equal bit for bit.

Through ssr_pair_metrics (the four SUMS x MAG instantiations) and ssr_pair_metrics_multi with K = 3 keys (target rows written by the
first key only: the null target plane; an odd last key).  Bars, those of tests/test_gpu_pass0.py: rows within 2e-7 of the largest bin
of the oracle's (float32 plan 3e-6), exact zeros in silent frames and only there, LSD and SSIM within 1e-5 of the oracle (5e-5), SISpec
within 1e-7 and log-SISpec within 1e-5 of the block engine's on the GPU (5e-5); the multi call against the single calls of the same
keys under the contract of tests/test_gpu_configs.py::test_pair_metrics_multi_equals_k_calls_of_pair_metrics: key 0 bit for bit, keys 1
and 2 - two estimates per complex transform, another round-off than beside the target - at 1e-6 (float32 plans: their 5e-5).  The
1-sample pair's metrics are round-off (see that file): its rows are checked, its metrics only for being finite.
The all-zero target: every LSD term of that pair is log10(0 / e^2 + 1e-12) = -12.  The wave kernel's epilogue adds the terms of a silent
target frame as that exact constant (ssr_stft_wave.h: SSR_W_LSD_OF_ZERO); taken through its float32 logarithm sequence (about 1 ulp)
the pair's LSD was 12.00000127 against the block engine's and the oracle's 12.0 - one rounding error that nothing averages out, 1.06e-7
against the 1e-7 of the block-engine comparison.  The pair is in every comparison."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_FFT, HOP, F = 2048, 512, 1025
LONG_FRAMES = 140
BIG = [2, 3, 4, 5, 6]                            # the pairs of seven frames or more
ONE = 0                                          # the 1-sample pair


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from ssr_eval_amd import _lib
    _lib.load()


def _oracle(e, t, ssim):
    from oracle import metrics as om
    es, ts = om.wav_to_spectrogram(e, N_FFT, HOP), om.wav_to_spectrogram(t, N_FFT, HOP)
    return [float(om.lsd(es, ts)), float(om.sispec(om.to_log(es), om.to_log(ts))), float(om.sispec(es, ts)),
            float(om.ssim(es, ts)) if ssim else np.nan]


@pytest.fixture(scope="module")
def batch():
    """(three keys of estimates, targets, oracle metrics [7, 3, 4], oracle rows of key 0 and of the targets)"""
    from oracle import stft as ostft
    rng = np.random.default_rng(64)
    lens = [1, 2047, 9 * HOP + 300, 9 * HOP + 300, (LONG_FRAMES - 1) * HOP + 17, 6656, 7 * HOP + 3 * N_FFT]
    tgts = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    keys = [[(g * t + s * rng.standard_normal(len(t))).astype(np.float32) for t in tgts] for g, s in ((0.8, 0.02), (1.0, 0.05), (0.5, 0.01))]
    keys[0][2][:] = 0.0
    tgts[3][:] = 0.0
    n = lens[6]
    keys[0][6][n // 3: n // 3 + N_FFT + 2 * HOP] = 0.0
    tgts[6][n // 2: n // 2 + N_FFT + HOP + 5] = 0.0
    assert ostft.num_frames(lens[4], N_FFT, HOP) == LONG_FRAMES and ostft.num_frames(lens[1], N_FFT, HOP) == 4
    want = np.array([[_oracle(keys[k][i], tgts[i], i in BIG) for k in range(3)] for i in range(len(lens))])
    rows = [(ostft.stft_mag_TF(keys[0][i], N_FFT, HOP), ostft.stft_mag_TF(tgts[i], N_FFT, HOP)) for i in range(len(lens))]
    want.setflags(write=False)
    return keys, tgts, want, rows


@pytest.fixture(scope="module")
def block_engine(batch):
    """[7, 4] metrics of key 0 from the block engine on the GPU (float64 signals never run k_stft_wave)."""
    from ssr_eval_amd import backend as B
    keys, tgts, _want, _rows = batch
    plan = B.get_plan(N_FFT, HOP, "f64")
    e64, t64 = [e.astype(np.float64) for e in keys[0]], [t.astype(np.float64) for t in tgts]
    out = np.full((len(tgts), 4), np.nan)
    out[:, :3] = B.pair_metrics(plan, e64, t64, B.M_LSD | B.M_SISPEC | B.M_LOG_SISPEC)[:, :3]
    out[BIG] = B.pair_metrics(plan, [e64[i] for i in BIG], [t64[i] for i in BIG], B.M_ALL)
    out.setflags(write=False)
    return out


def _masks(B):
    every = list(range(7))
    return [(B.M_LSD, every, [0]), (B.M_LSD | B.M_SSIM, BIG, [0, 3]),
            (B.M_LSD | B.M_SISPEC | B.M_LOG_SISPEC, every, [0, 1, 2]), (B.M_ALL, BIG, [0, 1, 2, 3])]


def _close(what, got, want, rtol, atol=0.0):
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print("    %s: largest relative difference %.3e (bar %.1e)" % (what, float(err.max()) if err.size else 0.0, rtol))
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=what)


def _assert_short_chunks(plan, items, tgts):
    from test_gpu_pass0 import geometry
    u, S = geometry(plan, len(items), max(len(tgts[i]) for i in items))
    print("    geometry read back: %d frames per chunk, %d chunks per interleave group" % (u, S))
    assert 1 <= u < 64 and S > 1 and LONG_FRAMES > u * S           # flushes of fewer than 64 frames; the long pair spans groups


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_pair_metrics_of_every_instantiation(batch, block_engine, prec):
    """Measured on an MI355X, float64 plans: LSD / SSIM within 1.4e-7 of the oracle, LSD / SISpec / SSIM within 5.5e-8 and log-SISpec
    within 4.7e-6 of the block engine; float32 plans: 1.1e-6, 1.0e-6 and 4.3e-5 (bars 5e-5)."""
    from ssr_eval_amd import backend as B
    keys, tgts, want, _rows = batch
    plan = B.get_plan(N_FFT, HOP, prec)
    tol = (1e-5, 1e-7, 1e-5, 0.0) if prec == "f64" else (5e-5, 5e-5, 5e-5, 5e-5)
    failures = []                                 # every comparison of every mask is made and printed; then all of them must have held

    def close(*args):
        try:
            _close(*args)
        except AssertionError as e:
            failures.append(str(e))

    for mask, items, cols in _masks(B):
        print("%s mask %d:" % (prec, mask))
        _assert_short_chunks(plan, items, tgts)
        got = B.pair_metrics(plan, [keys[0][i] for i in items], [tgts[i] for i in items], mask)
        assert np.isfinite(got[:, cols]).all()
        keep = [j for j, i in enumerate(items) if i != ONE]
        it, got = [items[j] for j in keep], got[keep]
        ref_cols = [c for c in cols if c in (0, 3)]
        close("mask %d: LSD / SSIM against the oracle" % mask, got[:, ref_cols], want[it][:, 0][:, ref_cols], tol[0], tol[3])
        tight = [c for c in cols if c != 1]
        close("mask %d: LSD / SISpec / SSIM against the block engine" % mask, got[:, tight], block_engine[it][:, tight], tol[1], tol[3])
        if 1 in cols:
            close("mask %d: log-SISpec against the block engine" % mask, got[:, [1]], block_engine[it][:, [1]], tol[2], tol[3])
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_pair_metrics_multi_three_keys(batch, prec):
    """K = 3: the target rows are written with key 0 and not again (out_b == null for keys 1 and 2: the flush's target store must fall
    to the range check), the last key is an odd one.  Against the oracle, and against single calls per key."""
    from ssr_eval_amd import backend as B
    keys, tgts, want, _rows = batch
    plan = B.get_plan(N_FFT, HOP, prec)
    tol = 1e-5 if prec == "f64" else 5e-5
    atol = 0.0 if prec == "f64" else 5e-5
    for mask, items, cols in _masks(B):
        print("%s mask %d, three keys:" % (prec, mask))
        got = B.pair_metrics_multi(plan, [[key[i] for i in items] for key in keys], [tgts[i] for i in items], mask)
        assert got.shape == (len(items), 3, 4) and np.isfinite(got[:, :, cols]).all()
        keep = [j for j, i in enumerate(items) if i != ONE]
        it = [items[j] for j in keep]
        ref_cols = [c for c in cols if c in (0, 3)]
        _close("LSD / SSIM against the oracle", got[keep][:, :, ref_cols], want[it][:, :, ref_cols], tol, atol)
        for k in range(3):
            single = B.pair_metrics(plan, [keys[k][i] for i in items], [tgts[i] for i in items], mask)
            if k == 0:                            # transformed with the target, as the single call does: LSD / SISpec bit for bit
                lin = [c for c in cols if c != 3]
                np.testing.assert_array_equal(got[keep][:, 0][:, lin], single[keep][:, lin])
            # keys 1 and 2 share one complex transform: the contract of tests/test_gpu_configs.py::test_pair_metrics_multi_equals_k_calls_of_
            # pair_metrics (include/ssr_hip.h says why not bit for bit) - 1e-6 relative + 1e-6 (dB) on float64 plans; float32 plans: 5e-5
            rt, at = (1e-6, 1e-6) if prec == "f64" else (5e-5, 5e-5)
            _close("key %d against its single call" % k, got[keep][:, k][:, cols], single[keep][:, cols], rt, at)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_rows_with_their_nyquist_column(batch, prec):
    """All seven pairs' rows out of k_stft_wave<T, false, true, true>; column 1,024 - written by the flush - on its own as well."""
    from ssr_eval_amd import backend as B
    from test_gpu_pass0 import pair_rows
    keys, tgts, _want, rows = batch
    plan = B.get_plan(N_FFT, HOP, prec)
    _assert_short_chunks(plan, list(range(7)), tgts)
    got = pair_rows(plan, keys[0], tgts)
    bar = 2e-7 if prec == "f64" else 3e-6
    worst = worst_nyq = 0.0
    for k in (0, 1):
        for i in range(7):
            m, ref = got[k][i], rows[i][k]
            assert m.shape == ref.shape, (k, i)
            if ref.max() > 0:
                worst = max(worst, float(np.abs(m - ref).max() / ref.max()))
                worst_nyq = max(worst_nyq, float(np.abs(m[:, F - 1] - ref[:, F - 1]).max() / ref.max()))
            assert np.abs(m - ref).max() <= bar * ref.max(), (k, i)
            if i in BIG:
                assert ((m == 0) == (ref == 0)).all(), (k, i)
    print("%s: rows within %.3e of the largest bin, column 1024 within %.3e (bar %.1e)" % (prec, worst, worst_nyq, bar))
    assert (rows[2][0] == 0).all() and (rows[3][1] == 0).all()
    assert (rows[6][0] == 0).all(axis=1).any() and (rows[6][1] == 0).all(axis=1).any()
    assert (got[0][4][:, F - 1] > 0).all() and (got[1][4][:, F - 1] > 0).all()      # every frame's Nyquist value arrived


# ---- the flush in the middle of a chunk: more than 64 frames per chunk ------------------------------------------------------------
LONG2_FRAMES, N_SHORT = 2100, 511


@pytest.fixture(scope="module")
def long_batch():
    """(three keys of estimates, targets, oracle metrics of pairs 0 and 1 [2, 3, 4], oracle rows of pairs 0 and 1): pair 0 has 2,100
    frames, pairs 1 .. 511 are one seven-frame pair."""
    from oracle import stft as ostft
    rng = np.random.default_rng(6466)
    n_long, n_short = (LONG2_FRAMES - 1) * HOP + 33, 6 * HOP + 100
    t_long, t_short = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (n_long, n_short)]
    t_long[HOP * 500 - N_FFT // 2: HOP * 531 + N_FFT // 2] = 0.0       # frames 500 .. 531: frames 63 and 64 of the chunks of group 0
    gains = ((0.8, 0.02), (1.0, 0.05), (0.5, 0.01))
    e_long = [(g * t_long + s * rng.standard_normal(n_long)).astype(np.float32) for g, s in gains]
    e_short = [(g * t_short + s * rng.standard_normal(n_short)).astype(np.float32) for g, s in gains]
    e_long[0][HOP * 2090:] = 0.0                                       # the last frames of the item: silent estimate
    assert ostft.num_frames(n_long, N_FFT, HOP) == LONG2_FRAMES and ostft.num_frames(n_short, N_FFT, HOP) == 7
    tgts = [t_long] + [t_short] * N_SHORT
    keys = [[e_long[k]] + [e_short[k]] * N_SHORT for k in range(3)]
    want = np.array([[_oracle(keys[k][i], tgts[i], True) for k in range(3)] for i in (0, 1)])
    rows = [(ostft.stft_mag_TF(keys[0][i], N_FFT, HOP), ostft.stft_mag_TF(tgts[i], N_FFT, HOP)) for i in (0, 1)]
    want.setflags(write=False)
    return keys, tgts, want, rows


@pytest.fixture(scope="module")
def long_block_engine(long_batch):
    """[2, 4] metrics of key 0, pairs 0 and 1, from the block engine on the GPU"""
    from ssr_eval_amd import backend as B
    keys, tgts, _want, _rows = long_batch
    plan = B.get_plan(N_FFT, HOP, "f64")
    out = B.pair_metrics(plan, [keys[0][i].astype(np.float64) for i in (0, 1)], [tgts[i].astype(np.float64) for i in (0, 1)], B.M_ALL)
    out.setflags(write=False)
    return out


def _assert_long_chunks(plan, tgts):
    from test_gpu_pass0 import geometry
    u, S = geometry(plan, len(tgts), max(len(t) for t in tgts))
    print("    geometry read back: %d frames per chunk, %d chunks per interleave group" % (u, S))
    assert 64 < u <= 128 and S == 8 and LONG2_FRAMES > u * S           # a flush inside every full chunk, several interleave groups
    return u


LONG_MASKS = ((1, [0]), (1 | 8, [0, 3]), (1 | 2 | 4, [0, 1, 2]), (15, [0, 1, 2, 3]))      # LSD, + SSIM, + the SISpecs, all: the four instantiations


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_flush_inside_a_chunk_pair_metrics(long_batch, long_block_engine, prec):
    """The four instantiations at more than 64 frames per chunk, against the oracle and the block engine at the bars of
    test_pair_metrics_of_every_instantiation; the 511 copies of the short pair equal bit for bit."""
    from ssr_eval_amd import backend as B
    keys, tgts, want, _rows = long_batch
    plan = B.get_plan(N_FFT, HOP, prec)
    tol = (1e-5, 1e-7, 1e-5, 0.0) if prec == "f64" else (5e-5, 5e-5, 5e-5, 5e-5)
    _assert_long_chunks(plan, tgts)
    failures = []

    def close(*args):
        try:
            _close(*args)
        except AssertionError as e:
            failures.append(str(e))

    for mask, cols in LONG_MASKS:
        print("%s mask %d, more than 64 frames per chunk:" % (prec, mask))
        got = B.pair_metrics(plan, keys[0], tgts, mask)
        assert np.isfinite(got[:, cols]).all()
        assert (got[1:][:, cols] == got[1, cols]).all(), "copies of one pair differ"
        got = got[:2]
        ref_cols = [c for c in cols if c in (0, 3)]
        close("mask %d: LSD / SSIM against the oracle" % mask, got[:, ref_cols], want[:, 0][:, ref_cols], tol[0], tol[3])
        tight = [c for c in cols if c != 1]
        close("mask %d: LSD / SISpec / SSIM against the block engine" % mask, got[:, tight], long_block_engine[:, tight], tol[1], tol[3])
        if 1 in cols:
            close("mask %d: log-SISpec against the block engine" % mask, got[:, [1]], long_block_engine[:, [1]], tol[2], tol[3])
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_flush_inside_a_chunk_multi_three_keys(long_batch, prec):
    """ssr_pair_metrics_multi, K = 3, on the same batch: against the oracle and against the single calls (key 0 bit for bit)."""
    from ssr_eval_amd import backend as B
    keys, tgts, want, _rows = long_batch
    plan = B.get_plan(N_FFT, HOP, prec)
    tol, atol = (1e-5, 0.0) if prec == "f64" else (5e-5, 5e-5)
    rt, at = (1e-6, 1e-6) if prec == "f64" else (5e-5, 5e-5)
    for mask, cols in (LONG_MASKS[3], LONG_MASKS[0]):
        print("%s mask %d, three keys, more than 64 frames per chunk:" % (prec, mask))
        got = B.pair_metrics_multi(plan, keys, tgts, mask)
        assert got.shape == (len(tgts), 3, 4) and np.isfinite(got[:, :, cols]).all()
        assert (got[1:][:, :, cols] == got[1][:, cols]).all(), "copies of one pair differ"
        ref_cols = [c for c in cols if c in (0, 3)]
        _close("LSD / SSIM against the oracle", got[:2][:, :, ref_cols], want[:, :, ref_cols], tol, atol)
        for k in range(3):
            single = B.pair_metrics(plan, keys[k], tgts, mask)
            if k == 0:
                lin = [c for c in cols if c != 3]
                np.testing.assert_array_equal(got[:, 0][:, lin], single[:, lin])
            _close("key %d against its single call" % k, got[:, k][:, cols], single[:, cols], rt, at)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_flush_inside_a_chunk_rows(long_batch, prec):
    """The rows of the 2,100-frame pair and of the short pair's first and last copy, column 1,024 - stored by the flushes, 64 rows at a
    time, 8 rows apart - on its own as well; exact zeros in the silent frames and only there."""
    from ssr_eval_amd import backend as B
    from test_gpu_pass0 import pair_rows
    keys, tgts, _want, rows = long_batch
    plan = B.get_plan(N_FFT, HOP, prec)
    _assert_long_chunks(plan, tgts)
    got = pair_rows(plan, keys[0], tgts)
    bar = 2e-7 if prec == "f64" else 3e-6
    worst = worst_nyq = 0.0
    for k in (0, 1):
        for i, r in ((0, 0), (1, 1), (N_SHORT, 1)):
            m, ref = got[k][i], rows[r][k]
            assert m.shape == ref.shape, (k, i)
            worst = max(worst, float(np.abs(m - ref).max() / ref.max()))
            worst_nyq = max(worst_nyq, float(np.abs(m[:, F - 1] - ref[:, F - 1]).max() / ref.max()))
            assert np.abs(m - ref).max() <= bar * ref.max(), (k, i)
            assert ((m == 0) == (ref == 0)).all(), (k, i)
    print("%s: rows within %.3e of the largest bin, column 1024 within %.3e (bar %.1e)" % (prec, worst, worst_nyq, bar))
    silent_t, silent_e = (rows[0][1] == 0).all(axis=1), (rows[0][0] == 0).all(axis=1)
    assert silent_t[504] and silent_t[512] and silent_e[-1] and not silent_t[499] and not silent_e[0]
    assert (got[1][0][~silent_t, F - 1] > 0).all() and (got[0][0][~silent_e, F - 1] > 0).all()     # every frame's Nyquist value arrived
