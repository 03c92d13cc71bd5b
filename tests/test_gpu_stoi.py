"""GPU tests (-m gpu) of STOI / ESTOI: the resampling leg against scipy.signal.resample_poly with the Octave window (bits), the
ssr_stoi kernels through AudioMetrics against the float64 oracle (tests/stoi_oracle.py, 1e-7 absolute), the one-target /
K-estimate path against the plain batch (bits), determinism, and SSR_Eval_Helper(stoi=...)."""
import numpy as np
import pytest
import torch

import stoi_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-7


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"


def _pairs(rng, fs, lens):
    """Speech-like targets with silent stretches (the mask drops frames in the middle) and three kinds of estimate."""
    out = []
    for j, n in enumerate(lens):
        x = O.speech_like(rng, n, fs)
        kind = j % 3
        if kind == 0:
            y = x + 0.4 * np.abs(x).max() * rng.standard_normal(n)
        elif kind == 1:
            y = 0.3 * np.convolve(x, np.hanning(9) / 4, "same") + 0.02 * rng.standard_normal(n)
        else:
            y = np.roll(x, 37) * 1.5
        out.append((y, x))
    return out


@pytest.mark.parametrize("fs", [10000, 16000, 44100, 48000])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_stoi_and_estoi_match_the_oracle(fs, dtype):
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(fs + (dtype == np.float64))
    # ragged, not multiples of 128 at 10 kHz; the two shortest leave fewer than 30 frames
    lens = [int(fs * s) + d for s, d in ((2.0, 0), (1.3, 17), (3.1, 101), (0.35, 3), (0.2, 0), (1.77, 55))]
    pairs = [(y.astype(dtype), x.astype(dtype)) for y, x in _pairs(rng, fs, lens)]
    pairs.append((rng.standard_normal(lens[0]).astype(dtype), np.zeros(lens[0], dtype)))     # all-zero target
    am = AudioMetrics(fs)
    got = am.stoi_batch([y for y, _ in pairs], [x for _, x in pairs], extended="both")
    for (y, x), g in zip(pairs, got):
        want_s, want_e = O.stoi(x, y, fs), O.stoi(x, y, fs, extended=True)
        assert abs(g["stoi"] - want_s) < TOL, (len(x), g, want_s)
        assert abs(g["estoi"] - want_e) < TOL, (len(x), g, want_e)
    assert got[-1] == {"stoi": 0.0, "estoi": 0.0}
    assert got[4] == {"stoi": 1e-5, "estoi": 1e-5}
    # the single-pair API and the single measures
    y, x = pairs[0]
    assert am.stoi(y, x) == got[0]["stoi"] and am.stoi(y, x, extended=True) == got[0]["estoi"]
    assert am.stoi(y, x, extended="both") == got[0]


def test_sixty_second_utterance():
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(60)
    fs = 48000
    x = O.speech_like(rng, 60 * fs, fs, silences=((0.1, 0.12), (0.5, 0.55), (0.9, 0.93)))
    y = x + 0.2 * np.abs(x).max() * rng.standard_normal(x.shape)
    g = AudioMetrics(fs).stoi(y.astype(np.float32), x.astype(np.float32), extended="both")
    xf, yf = x.astype(np.float32), y.astype(np.float32)
    assert abs(g["stoi"] - O.stoi(xf, yf, fs)) < TOL
    assert abs(g["estoi"] - O.stoi(xf, yf, fs, extended=True)) < TOL


def test_truncation_to_the_common_length():
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(5)
    (y, x), = _pairs(rng, 16000, [40000])
    g = AudioMetrics(16000).stoi(y[:-40].astype(np.float32), x.astype(np.float32))
    m = len(y) - 40
    assert abs(g - O.stoi(x[:m].astype(np.float32), y[:m].astype(np.float32), 16000)) < TOL


@pytest.mark.parametrize("fs", [16000, 44100, 48000])
def test_resampling_leg_is_bit_identical_to_scipy(fs):
    from ssr_eval_amd import backend as B
    rng = np.random.default_rng(fs)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in (fs, fs // 3 + 7, 2 * fs + 1)]
    sigs.append(rng.standard_normal(fs // 2))                                   # float64
    r = B.resample_to_stoi_rate(sigs, fs)
    data = r.data.cpu().numpy()
    off = r.off.cpu().numpy()
    for s, o, n in zip(sigs, off, r.lens_host):
        want = O.resample_to_fs(s, fs)
        assert want.dtype == np.float64 and n == len(want)
        assert np.array_equal(data[o:o + n], want)


def test_multi_is_bit_identical_to_batch_and_runs_repeat():
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(11)
    fs, K = 48000, 4
    tg = [O.speech_like(rng, n, fs).astype(np.float32) for n in (96000, 70001, 15000, 150000)]
    ests = [[(t + (0.1 + 0.2 * k) * np.abs(t).max() * rng.standard_normal(len(t))).astype(np.float32 if k % 2 else np.float64)
             for t in tg] for k in range(K)]
    am = AudioMetrics(fs)
    multi = am.stoi_multi(ests, tg, extended="both")
    flat = am.stoi_batch([ests[k][i] for i in range(len(tg)) for k in range(K)], [tg[i] for i in range(len(tg)) for _ in range(K)],
                         extended="both")
    assert [d for row in multi for d in row] == flat
    again = am.stoi_multi(ests, tg, extended="both", deferred=True)()
    assert again == multi
    for i in range(len(tg)):
        for k in range(K):
            assert abs(multi[i][k]["estoi"] - O.stoi(tg[i], ests[k][i], fs, extended=True)) < TOL


def test_evaluate_with_stoi_from_wav_files(tmp_path, monkeypatch):
    """SSR_Eval_Helper(stoi="both").evaluate() on a small wav tree (identity testee, two FFT keys and four IIR keys, 44.1 kHz): the
    per-file values are AudioMetrics.stoi on the same estimates, the earlier metrics are those of a run without stoi, bit for bit,
    and with stoi=None the result is that run's."""
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee, AudioMetrics
    from ssr_eval_amd.io import write_wav, read_audio
    from ssr_eval_amd.lowpass import lowpass
    rng = np.random.default_rng(99)
    root = tmp_path / "vctk_test"
    counts = {"p360": 3, "p361": 2}
    for spk, c in counts.items():
        (root / spk).mkdir(parents=True)
        for i in range(c):
            x = 0.3 * O.speech_like(rng, int(rng.integers(50000, 90000)), 44100) / 3
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), x.astype(np.float32), 44100)
    monkeypatch.chdir(tmp_path)

    def run(stoi):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=44100, output_sr=44100, evaluation_sr=44100, test_data_root=str(root),
                            setting_fft={"cutoff_freq": [4000, 11025]},
                            setting_lowpass_filtering={"cutoff_freq": [6000], "filter_order": [4],
                                                       "filter": ["butter", "cheby", "ellip", "bessel"]}, stoi=stoi)
        return h.evaluate(save_json=False)
    plain, res = run(None), run("both")
    am = AudioMetrics(44100)
    fft = {"proc_fft_8000_44100": (4000, "stft_hard"), "proc_fft_22050_44100": (11025, "stft_hard")}
    iir = {"proc_%s_12000_4_44100" % t: (6000, f) for t, f in (("bw", "butter"), ("bessel", "bessel"), ("el", "ellip"), ("ch", "cheby1"))}
    n = 0
    for spk in counts:
        for fn in res[spk]:
            x, _ = read_audio(str(root / spk / fn))
            for key, (cut, kind) in {**fft, **iir}.items():
                got = res[spk][fn][key]
                assert list(got)[-2:] == ["stoi", "estoi"]
                assert {m: got[m] for m in plain[spk][fn][key]} == plain[spk][fn][key]
                est = lowpass(x, cut, 44100, order=1 if kind == "stft_hard" else 4, _type=kind)
                est = np.asarray(est, np.float64 if kind != "stft_hard" else np.float32)
                want = am.stoi(est, np.asarray(x, np.float32), extended="both")
                assert abs(got["stoi"] - want["stoi"]) < 1e-9 and abs(got["estoi"] - want["estoi"]) < 1e-9, (fn, key)
                assert abs(got["stoi"] - O.stoi(np.asarray(x, np.float32), est, 44100)) < TOL
                n += 1
    assert n == 5 * 6
    assert {"stoi", "estoi"} <= set(res["averaged"]["proc_fft_8000_44100"])
