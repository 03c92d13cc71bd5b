"""GPU tests (-m gpu) of the fused radix-8 passes of the wave engines (ssr_fft.h: ssr_bfly8_tw inside SSR_W_FFT_TAIL_X), at the
smallest inputs at which a pass can go wrong, for every kernel family that takes the shared 2048-point tail: k_stft_wave (2048 / 512;
the LSD + SSIM instance and the four-metric one), k_stft_r3_rot (2229 / 480), k_stft_rn_wave (1486 / 320, 743 / 160), the
float64-estimate and two-estimates-per-transform entry points, and the FFT low-pass at 2048 / 441 on the `segments` and `fused`
engines.  Four ragged items per case: one shorter than a frame (the reflection wraps), one of three hops plus a remainder, one with a
stretch of digital silence longer than a frame (exact-zero frames are forced), one of 9001 samples.

Tolerances are the ones the existing parity tests hold these entry points to:
  metrics against the oracle, 1e-5 relative        tests/test_gpu_parity.py::test_randomised_ragged_batches_against_oracle,
                                                   ::test_partially_silent_signals, ::test_short_signals_reflect_repeatedly_like_numpy_pad
  float64 estimates: LSD / SSIM 1e-6, SISpec 1e-5  tests/test_gpu_parity.py::test_pair_metrics_float64_estimate
  multi against K single calls: key 0 LSD / SISpec bit for bit, the rest rtol 1e-6 + atol 1e-6
                                                   tests/test_gpu_configs.py::test_pair_metrics_multi_equals_k_calls_of_pair_metrics,
                                                   ::test_pair_metrics_multi_est64_equals_k_calls_of_est64
  magnitudes 2e-7 of the largest bin               tests/test_gpu_parity.py::test_stft_magnitude_vs_oracle_ragged
  low-pass against the ideal float64 low-pass, 5e-8 absolute
                                                   tests/test_gpu_configs.py::test_lowpass_engines_fused_and_segments"""
import numpy as np
import pytest
import torch
from scipy import signal

pytestmark = pytest.mark.gpu

KEYS = ("lsd", "log_sispec", "sispec", "ssim")
SIZES = [(2048, 512), (2229, 480), (1486, 320), (743, 160)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from ssr_eval_amd import _lib
    _lib.load()


def _vec(d):
    return np.array([d[k] for k in KEYS])


def ragged_pairs(n_fft, hop, seed):
    """(estimates, targets): the four items of the module docstring; items 2 and 3 have at least seven frames (SSIM's minimum)."""
    rng = np.random.default_rng(seed)
    n_sil = 7 * hop + 3 * n_fft
    tgts = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (n_fft // 2 + 1, 3 * hop + 77, n_sil, 9001)]
    ests = [(0.8 * t + 0.02 * rng.standard_normal(len(t))).astype(np.float32) for t in tgts]
    ests[2][n_sil // 3: n_sil // 3 + n_fft + 2 * hop] = 0.0                 # whole silent frames in the estimate ...
    tgts[2][n_sil // 2: n_sil // 2 + n_fft + hop + 5] = 0.0                 # ... and, elsewhere, in the target
    return ests, tgts


_ORACLE = {}


def oracle_rows(n_fft, hop, ests, tgts, tag):
    """[n, 4] oracle metrics (SSIM NaN where the image has fewer than seven rows); computed once per input set."""
    key = (n_fft, hop, tag)
    if key not in _ORACLE:
        from oracle import metrics as om
        rows = []
        for e, t in zip(ests, tgts):
            es, ts = om.wav_to_spectrogram(e, n_fft, hop), om.wav_to_spectrogram(t, n_fft, hop)
            row = [float(om.lsd(es, ts)), float(om.sispec(om.to_log(es), om.to_log(ts))), float(om.sispec(es, ts)), np.nan]
            if es.shape[2] >= 7:
                row[3] = float(om.ssim(es, ts))
            rows.append(row)
        _ORACLE[key] = np.array(rows)
        _ORACLE[key].setflags(write=False)
    return _ORACLE[key]


@pytest.mark.parametrize("n_fft,hop", SIZES)
def test_pair_metrics_every_wave_family_against_the_oracle(n_fft, hop):
    from ssr_eval_amd import backend as B
    ests, tgts = ragged_pairs(n_fft, hop, n_fft)
    want = oracle_rows(n_fft, hop, ests, tgts, "f32")
    plan = B.get_plan(n_fft, hop, "f64")
    got3 = B.pair_metrics(plan, ests, tgts, B.M_LSD | B.M_SISPEC | B.M_LOG_SISPEC)           # the running-sums instance, no images
    np.testing.assert_allclose(got3[:, :3], want[:, :3], rtol=1e-5)
    full = B.pair_metrics(plan, ests[2:], tgts[2:], B.M_ALL)                                # the four-metric instance
    np.testing.assert_allclose(full, want[2:], rtol=1e-5)
    two = B.pair_metrics(plan, ests[2:], tgts[2:], B.M_LSD | B.M_SSIM)                      # the LSD + SSIM instance (bench.py's cfg-2)
    np.testing.assert_allclose(two[:, [0, 3]], want[2:][:, [0, 3]], rtol=1e-5)
    lsd = B.pair_metrics(plan, ests, tgts, B.M_LSD)                                         # LSD alone: no images, no sums
    np.testing.assert_allclose(lsd[:, 0], want[:, 0], rtol=1e-5)


@pytest.mark.parametrize("n_fft,hop", SIZES)
def test_multi_key_0_is_pair_metrics_bit_for_bit(n_fft, hop):
    from ssr_eval_amd import backend as B
    ests, tgts = ragged_pairs(n_fft, hop, n_fft)
    keys = [ests, [(0.5 * e).astype(np.float32) for e in ests], [(-e).astype(np.float32) for e in ests]]
    plan = B.get_plan(n_fft, hop, "f64")
    mask = B.M_LSD | B.M_SISPEC | B.M_LOG_SISPEC
    got = B.pair_metrics_multi(plan, keys, tgts, mask)
    for k, key in enumerate(keys):
        want = B.pair_metrics(plan, key, tgts, mask)
        if k == 0:
            np.testing.assert_array_equal(got[:, 0, :3], want[:, :3])
        np.testing.assert_allclose(got[:, k, :3], want[:, :3], rtol=1e-6, atol=1e-6)
    got = B.pair_metrics_multi(plan, [k[2:] for k in keys], tgts[2:], B.M_ALL)
    want = B.pair_metrics(plan, ests[2:], tgts[2:], B.M_ALL)
    np.testing.assert_array_equal(got[:, 0, :3], want[:, :3])
    np.testing.assert_allclose(got[:, 0], want, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("n_fft,hop", [(2048, 512), (2229, 480)])
def test_float64_estimate_and_two_estimate_entry_points(n_fft, hop):
    """Zero-phase IIR estimates stay float64 (stop band at the float64 round-off floor): ssr_pair_metrics_est64 against the oracle, and
    ssr_pair_metrics_multi_est64 (2229: two estimates per complex transform on the rotating engine) against single calls."""
    from ssr_eval_amd import backend as B
    from oracle import lowpass as olp
    _, tgts = ragged_pairs(n_fft, hop, n_fft + 1)
    designs = [olp.iir_sos(2000, 44100, 8, "cheby1"), olp.iir_sos(6000, 44100, 6, "butter"), olp.iir_sos(4000, 44100, 4, "bessel")]
    keys = [[signal.sosfiltfilt(sos, t) for t in tgts] for sos in designs]
    assert all(e.dtype == np.float64 for key in keys for e in key)
    plan = B.get_plan(n_fft, hop, "f64")
    want = oracle_rows(n_fft, hop, keys[0], tgts, "est64")
    got = B.pair_metrics(plan, keys[0][2:], tgts[2:], B.M_ALL)
    np.testing.assert_allclose(got[:, [0, 3]], want[2:][:, [0, 3]], rtol=1e-6)
    np.testing.assert_allclose(got[:, [1, 2]], want[2:][:, [1, 2]], rtol=1e-5)
    mask = B.M_LSD | B.M_SISPEC | B.M_LOG_SISPEC
    got3 = B.pair_metrics(plan, keys[0], tgts, mask)
    np.testing.assert_allclose(got3[:, 0], want[:, 0], rtol=1e-6)
    np.testing.assert_allclose(got3[:, 1:3], want[:, 1:3], rtol=1e-5)
    multi = B.pair_metrics_multi(plan, keys, tgts, mask)
    for k, key in enumerate(keys):
        single = B.pair_metrics(plan, key, tgts, mask)
        if k == 0:
            np.testing.assert_array_equal(multi[:, 0, :3], single[:, :3])
        np.testing.assert_allclose(multi[:, k, :3], single[:, :3], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("n_fft,hop", SIZES)
def test_magnitudes_against_the_oracle(n_fft, hop):
    from ssr_eval_amd import backend as B
    from oracle import stft as ostft
    _, tgts = ragged_pairs(n_fft, hop, n_fft)
    for x, m in zip(tgts, B.stft(B.get_plan(n_fft, hop, "f64"), tgts)):
        ref = ostft.stft_mag_TF(x, n_fft, hop)
        m = m.cpu().numpy()
        assert m.shape == ref.shape
        assert np.abs(m - ref).max() <= 2e-7 * ref.max()
        assert ((m == 0) == (ref == 0)).all()                                               # silent frames are exact zeros, only they


def test_fft_lowpass_segments_and_fused_and_exact_scaling():
    from ssr_eval_amd import backend as B
    from oracle import lowpass as olp
    hop = 441
    rng = np.random.default_rng(441)
    sigs = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in (1025 + 40, 3 * hop + 77, 7 * hop + 3 * 2048, 9001)]
    sigs[2][3000:3000 + 2048 + 2 * hop] = 0.0
    cuts = [300, 1025, 77, 512]
    want = [olp.stft_hard_lowpass(x, (c + 0.5) / 1025, n_fft=2048, hop=hop, arithmetic="ideal") for x, c in zip(sigs, cuts)]
    for engine in ("segments", "fused"):
        plan = B.Plan(2048, hop, "f64").set_lowpass_engine(engine)
        ys = [y.cpu().numpy() for y in B.fft_lowpass(plan, sigs, cuts)]
        for y, w in zip(ys, want):
            np.testing.assert_allclose(y, w, atol=5e-8)
        scaled = [y.cpu().numpy() for y in B.fft_lowpass(plan, [4.0 * x for x in sigs], cuts)]
        for y, s in zip(ys, scaled):
            np.testing.assert_array_equal(s, 4.0 * y)                                       # a power of two scales every bit pattern exactly
