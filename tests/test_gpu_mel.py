"""GPU tests (-m gpu) of the mel-spectrogram distances (mel_lsd, mel_l1, mcd): the HIP mel kernels (ssr_mel.h)
through AudioMetrics against the float64 oracle (tests/mel_oracle.py) at 1e-5 relative (1e-6 absolute near 0), float32 and
float64 estimates, ragged / short / 60 s signals, every filterbank option; mel_spectrogram against the reference's MelScale.forward
(tests/golden/reference_mel.npz) and the oracle; the multi path against the batch path; bits of a pair alone, in a batch and on a
second run; the image-level entry point; and SSR_Eval_Helper(mel=...)."""
import os

import numpy as np
import pytest
import torch

import mel_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = O.NAMES


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"


def _speechy(rng, n):
    return np.convolve(rng.standard_normal(n), np.hanning(15) / 4, "same")[:n].astype(np.float32)


def _close(got, want, what=""):
    for m in want:
        assert abs(got[m] - want[m]) <= 1e-5 * abs(want[m]) + 1e-6, (what, m, got[m], want[m])


def _fb(am, **mel):
    fb, n_cep = am.mel_filterbank(**mel)
    return fb.numpy(), n_cep


def _pairs(rng, fs, ed):
    out = []
    for n in (int(1.3 * fs) + 17, int(0.4 * fs), 300, 7, int(0.05 * fs) + 3):
        x = _speechy(rng, n)
        out.append((x, (x + 0.3 * np.std(x) * rng.standard_normal(n)).astype(ed)))
    x = _speechy(rng, fs // 2)
    out.append((x, x.astype(ed)))                                              # estimate = target
    out.append((x, (0.3 * x).astype(ed)))                                       # a global gain
    out.append((x, np.zeros(len(x), ed)))                                       # silence: every mel value at the clamp
    return out


@pytest.mark.parametrize("fs,n_fft,hop", [(16000, None, None), (24000, None, None), (44100, None, None), (48000, None, None),
                                          (48000, 2048, 512)])
@pytest.mark.parametrize("ed", [np.float32, np.float64])
def test_mel_distances_match_the_oracle(fs, n_fft, hop, ed):
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(fs + (ed == np.float64))
    am = AudioMetrics(fs, n_fft=n_fft, hop_length=hop)
    W, n_cep = _fb(am)
    pairs = _pairs(rng, fs, ed)
    got = am.mel_distance_batch([y for _, y in pairs], [x for x, _ in pairs])
    for j, ((x, y), g) in enumerate(zip(pairs, got)):
        assert list(g) == list(NAMES)
        _close(g, O.distances(y, x, fs, W, n_cep, am.n_fft, am.hop_length), (fs, j))
    # estimate = target: the two images come from one complex transform (float64 estimates: |.| rounded once from float64)
    assert got[5]["mel_l1"] < 1e-6 and got[5]["mcd"] < 1e-4
    # truncation to the common length, the single-pair API and subsets: the bits of the batch
    x, y = pairs[0]
    assert am.mel_distance(y, x) == got[0]
    assert am.mel_distance(y, x, ("mcd", "mel_lsd")) == {"mel_lsd": got[0]["mel_lsd"], "mcd": got[0]["mcd"]}
    _close(am.mel_distance(y[:-40], x), O.distances(y[:-40], x, fs, W, n_cep, am.n_fft, am.hop_length))


@pytest.mark.parametrize("opts", [dict(n_mels=80, norm="slaney", mel_scale="slaney"), dict(n_mels=100, mel_scale="slaney"),
                                  dict(n_mels=64, f_min=20.0, f_max=8000.0, n_cep=30), dict(n_mels=40, norm="slaney", n_cep=39),
                                  dict(n_mels=200, f_min=300.0, n_cep=1)])
def test_every_filterbank_option(opts):
    from ssr_eval_amd import AudioMetrics
    fs = 24000
    rng = np.random.default_rng(len(opts))
    am = AudioMetrics(fs)
    W, n_cep = _fb(am, **opts)
    pairs = _pairs(rng, fs, np.float32)[:4]
    got = am.mel_distance_batch([y for _, y in pairs], [x for x, _ in pairs], **opts)
    for (x, y), g in zip(pairs, got):
        _close(g, O.distances(y, x, fs, W, n_cep), opts)


def test_sixty_second_utterance():
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(60)
    fs = 48000
    x = _speechy(rng, 60 * fs)
    y = (x + 0.05 * rng.standard_normal(len(x))).astype(np.float32)
    am = AudioMetrics(fs)
    W, n_cep = _fb(am)
    _close(am.mel_distance(y, x), O.distances(y, x, fs, W, n_cep))


def test_mel_spectrogram_against_the_golden_forward_and_the_oracle():
    from ssr_eval_amd import AudioMetrics, backend as B
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_mel.npz"))
    for name, am, opts in (("nvsr_44100", AudioMetrics(44100), {}),
                           ("slaney_slaney_16000", AudioMetrics(16000, n_fft=742), dict(n_mels=80, norm="slaney", mel_scale="slaney"))):
        fb, _ = am.mel_filterbank(**opts)
        np.testing.assert_allclose(fb.numpy(), g["fb_" + name], rtol=0, atol=1e-7)     # (torch.exp of the host)
        F = fb.shape[0]
        rng = np.random.default_rng(int(g["fwd_seed_" + name]))
        x = np.abs(rng.standard_normal((60, F))) * np.exp(-np.arange(F) / (F / 4.0))[None, :]
        x = x.astype(np.float32)
        ref_fb = torch.from_numpy(np.ascontiguousarray(g["fb_" + name]))          # the reference's own table, as forward used it
        got = B.spectrogram_mel(torch.from_numpy(x)[None].cuda(), ref_fb)[0].cpu().numpy()
        np.testing.assert_allclose(got, g["fwd_" + name], rtol=1e-6, atol=0)
        np.testing.assert_allclose(got, O.mel(x, g["fb_" + name]), rtol=1e-7, atol=0)
        own = B.spectrogram_mel(torch.from_numpy(x)[None].cuda(), fb)[0].cpu().numpy()
        np.testing.assert_allclose(own, O.mel(x, fb.numpy()), rtol=1e-7, atol=0)
    am = AudioMetrics(44100)
    wav = _speechy(np.random.default_rng(3), 30000)
    ms = am.mel_spectrogram(wav)
    sp = am.wav_to_spectrogram(wav)[0, 0].numpy()
    assert ms.shape == (1, 1, sp.shape[0], 128) and ms.dtype == torch.float32 and ms.device.type == "cpu"
    np.testing.assert_allclose(ms[0, 0].numpy(), O.mel(sp, _fb(am)[0]), rtol=1e-6, atol=0)
    want = O.mel(O.magnitudes(wav, 44100), _fb(am)[0])
    np.testing.assert_allclose(ms[0, 0].numpy(), want, rtol=1e-5, atol=1e-6 * want.max())
    assert am.mel_spectrogram(wav, keep_on_device=True).is_cuda


def test_multi_against_batch_alone_and_repeat():
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(11)
    fs, K = 48000, 6
    tg = [_speechy(rng, n) for n in (96000, 70001, 15000, 150000, 480)]
    ests = [[(t + (0.05 + 0.2 * k) * rng.standard_normal(len(t))).astype(np.float32) for t in tg] for k in range(K)]
    ests[4] = [e.astype(np.float64) for e in ests[4]]                         # a float64 key next to the float32 ones
    am = AudioMetrics(fs)
    W, n_cep = _fb(am)
    multi = am.mel_distance_multi(ests, tg)
    again = am.mel_distance_multi(ests, tg, deferred=True)()
    assert again == multi
    chunked = am.mel_distance_multi(ests, tg, keys_per_chunk=2)                # other transform pairings: other image bits
    for i in range(len(tg)):
        for k in range(K):
            for name in NAMES:
                assert abs(chunked[i][k][name] - multi[i][k][name]) <= 1e-6 * abs(multi[i][k][name]) + 1e-9
    flat = am.mel_distance_batch([ests[k][i] for i in range(len(tg)) for k in range(K)], [tg[i] for i in range(len(tg)) for _ in range(K)])
    for i in range(len(tg)):
        for k in range(K):
            m, b = multi[i][k], flat[i * K + k]
            for name in NAMES:
                assert abs(m[name] - b[name]) <= 1e-6 * abs(b[name]) + 1e-9, (i, k, name, m[name], b[name])
            _close(m, O.distances(ests[k][i], tg[i], fs, W, n_cep), (i, k))
    for i in range(len(tg)):                                                  # a pair alone: its bits in the batch
        assert am.mel_distance(ests[1][i], tg[i]) == flat[i * K + 1]
    assert am.mel_distance_batch([ests[1][i] for i in range(len(tg))], tg) == [flat[i * K + 1] for i in range(len(tg))]


def test_image_level_entry_point():
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(5)
    am = AudioMetrics(16000)
    W, n_cep = _fb(am, n_mels=80)
    F = W.shape[0]
    T = 37
    tgt = np.abs(rng.standard_normal((2, 3, T, F))).astype(np.float32)
    est = (tgt * np.exp(0.3 * rng.standard_normal(tgt.shape))).astype(np.float32)
    est[1, 2] = tgt[1, 2]
    got = am.mel_distance_spectrogram(torch.from_numpy(est).cuda(), torch.from_numpy(tgt).cuda(), n_mels=80)
    assert list(got) == list(NAMES) and got["mcd"].shape == (2, 3) and got["mcd"].is_cuda
    for b in range(2):
        for c in range(3):
            want = O.distances_from_images(est[b, c], tgt[b, c], W, n_cep)
            _close({m: float(got[m][b, c]) for m in NAMES}, want, (b, c))
    assert float(got["mcd"][1, 2]) == 0.0
    only = am.mel_distance_spectrogram(torch.from_numpy(est), torch.from_numpy(tgt), "mel_l1", n_mels=80)
    assert list(only) == ["mel_l1"] and torch.equal(only["mel_l1"].cpu(), got["mel_l1"].cpu())


def test_evaluate_with_mel_from_wav_files(tmp_path, monkeypatch):
    """SSR_Eval_Helper(mel=...).evaluate() on a small wav tree (identity testee, two FFT keys and two IIR keys: float32 and float64
    estimates): the per-file values are AudioMetrics.mel_distance on the same estimates, the earlier metrics are those of a run
    without the option, bit for bit, mel=None is that run, and the keys come after the waveform metrics."""
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee, AudioMetrics
    from ssr_eval_amd.io import write_wav, read_audio
    from ssr_eval_amd.lowpass import lowpass
    rng = np.random.default_rng(99)
    root = tmp_path / "vctk_test"
    counts = {"p360": 3, "p361": 2}
    for spk, c in counts.items():
        (root / spk).mkdir(parents=True)
        for i in range(c):
            x = 0.1 * _speechy(rng, int(rng.integers(50000, 90000)))
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), x.astype(np.float32), 44100)
    monkeypatch.chdir(tmp_path)

    def run(**kw):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=44100, output_sr=44100, evaluation_sr=44100, test_data_root=str(root),
                            setting_fft={"cutoff_freq": [4000, 11025]},
                            setting_lowpass_filtering={"cutoff_freq": [6000], "filter_order": [4], "filter": ["butter", "cheby"]}, **kw)
        return h.evaluate(save_json=False)
    plain, res, off = run(), run(mel=True), run(mel=None)
    assert off == plain
    am = AudioMetrics(44100)
    keys = {"proc_fft_8000_44100": (4000, "stft_hard"), "proc_fft_22050_44100": (11025, "stft_hard"),
            "proc_bw_12000_4_44100": (6000, "butter"), "proc_ch_12000_4_44100": (6000, "cheby1")}
    n = 0
    for spk in counts:
        for fn in res[spk]:
            x, _ = read_audio(str(root / spk / fn))
            for key, (cut, kind) in keys.items():
                got = res[spk][fn][key]
                assert list(got)[-3:] == list(NAMES)
                assert {m: got[m] for m in plain[spk][fn][key]} == plain[spk][fn][key]
                est = lowpass(x, cut, 44100, order=1 if kind == "stft_hard" else 4, _type=kind)
                est = np.asarray(est, np.float64 if kind != "stft_hard" else np.float32)
                want = am.mel_distance(est, np.asarray(x, np.float32))
                for m in NAMES:
                    assert abs(got[m] - want[m]) <= 1e-6 * abs(want[m]) + 1e-9, (fn, key, m, got[m], want[m])
                n += 1
    assert n == 5 * 4
    assert set(NAMES) <= set(res["averaged"]["proc_fft_8000_44100"])
    full = run(mel={"n_mels": 80, "which": ("mcd",)}, waveform="snr")
    fn = next(iter(full["p360"]))
    assert list(full["p360"][fn]["proc_fft_8000_44100"]) == ["lsd", "log_sispec", "sispec", "ssim", "snr", "mcd"]
