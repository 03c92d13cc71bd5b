"""GPU tests (-m gpu) of the waveform metrics (SNR, SI-SDR, segmental SNR): ssr_wave_metrics through AudioMetrics against the
float64 oracle (tests/wave_oracle.py, 1e-8 dB absolute), on float32 / float64 targets and estimates in every combination, ragged
lengths and hard signals; waveform_multi against waveform_batch, a pair alone against the same pair in a batch and two runs
(bits); and SSR_Eval_Helper(waveform=...)."""
import numpy as np
import pytest
import torch

import wave_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-8
NAMES = ("snr", "si_sdr", "seg_snr")
DTYPES = [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)]


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"


def _check(got, x, y, fs):
    want = O.waveform(x, y, fs)
    for m in NAMES:
        if np.isnan(want[m]):
            assert np.isnan(got[m]), (m, len(x), got[m])
        else:
            assert abs(got[m] - want[m]) < TOL, (m, len(x), got[m], want[m])


def _speechy(rng, n):
    return np.convolve(rng.standard_normal(n), np.hanning(15) / 4, "same")[:n] if n else np.zeros(0)


def _hard_pairs(rng, fs, td, ed):
    """(target, estimate) pairs: ragged lengths (M = 0 and n = 0 among them) and the hard signals.  Targets hold float32 values in
    either dtype, so y = x is exact for every dtype combination."""
    L, R, _ = O.frame_geometry(fs, 0)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)      # noqa: E731
    out = []
    for n in (int(1.7 * fs) + 13, L + R - 1, L + R, 40 * R, 0, 5, int(0.9 * fs)):
        x = f32(_speechy(rng, n))
        out.append((x, x + 0.3 * np.std(x) * rng.standard_normal(n) if n else x))
    x = f32(_speechy(rng, fs))
    rms = np.sqrt(np.mean(x * x))
    out.append((x, x))                                                       # y = x
    out.append((x, x + 1e-5 * rms * rng.standard_normal(len(x))))            # about 100 dB: the cancellation case
    out.append((x, 0.6 * x - 0.2 + 0.05 * rng.standard_normal(len(x))))      # scaled, offset estimate
    d = f32(0.5 + 1e-3 * rng.standard_normal(fs // 2))                        # 0.5 DC on an rms-1e-3 signal
    out.append((d, d + 1e-4 * rng.standard_normal(len(d))))
    out.append((d, f32(0.5 + 1e-3 * rng.standard_normal(len(d)))))
    out.append((np.zeros(fs // 3), 0.1 * rng.standard_normal(fs // 3)))      # all-zero target
    out.append((np.zeros(fs // 3), np.zeros(fs // 3)))                        # both silent
    return [(np.asarray(x, td), np.asarray(y, ed)) for x, y in out]


@pytest.mark.parametrize("fs", [16000, 44100, 48000])
@pytest.mark.parametrize("dt", DTYPES)
def test_waveform_metrics_match_the_oracle(fs, dt):
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(fs + 2 * (dt[0] == np.float64) + (dt[1] == np.float64))
    pairs = _hard_pairs(rng, fs, *dt)
    am = AudioMetrics(fs)
    got = am.waveform_batch([y for _, y in pairs], [x for x, _ in pairs])
    for (x, y), g in zip(pairs, got):
        assert list(g) == list(NAMES)
        _check(g, x, y, fs)
    assert got[-1]["snr"] == 0.0 and got[-1]["si_sdr"] == 0.0
    assert all(np.isnan(v) for v in got[4].values())                        # n = 0
    assert np.isnan(got[1]["seg_snr"]) and got[2]["seg_snr"] == got[2]["seg_snr"]     # M = 0, M = 1
    assert all(np.isfinite(v) for v in got[7].values())                      # y = x
    # the single-pair API, the single measures and subsets: the same bits as in the batch
    y, x = pairs[0][1], pairs[0][0]
    assert am.waveform(y, x) == got[0]
    assert am.snr(y, x) == got[0]["snr"] and am.si_sdr(y, x) == got[0]["si_sdr"] and am.seg_snr(y, x) == got[0]["seg_snr"]
    assert am.waveform(y, x, ("seg_snr", "snr")) == {"snr": got[0]["snr"], "seg_snr": got[0]["seg_snr"]}


def test_mixed_dtypes_in_one_batch():
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(4)
    fs = 16000
    pairs = []
    for j, (td, ed) in enumerate(DTYPES * 2):
        x = np.asarray(_speechy(rng, 20000 + 997 * j), np.float32)
        pairs.append((x.astype(td), (x + 0.2 * rng.standard_normal(len(x))).astype(ed)))
    got = AudioMetrics(fs).waveform_batch([y for _, y in pairs], [x for x, _ in pairs])
    for (x, y), g in zip(pairs, got):
        _check(g, x, y, fs)


def test_sixty_second_utterance():
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(60)
    fs = 48000
    x = np.asarray(_speechy(rng, 60 * fs), np.float32)
    y = (x + 0.05 * rng.standard_normal(len(x))).astype(np.float32)
    _check(AudioMetrics(fs).waveform(y, x), x, y, fs)


def test_truncation_to_the_common_length():
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(5)
    x = np.asarray(_speechy(rng, 40000), np.float32)
    y = (x + 0.1 * rng.standard_normal(len(x))).astype(np.float32)[:-40]
    _check(AudioMetrics(16000).waveform(y, x), x[:-40], y, 16000)


def test_multi_batch_alone_and_repeat_are_bit_identical():
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(11)
    fs, K = 48000, 4
    tg = [np.asarray(_speechy(rng, n), np.float32) for n in (96000, 70001, 15000, 150000)]
    ests = [[(t + (0.05 + 0.2 * k) * rng.standard_normal(len(t))).astype(np.float32) for t in tg] for k in range(K)]
    am = AudioMetrics(fs)
    multi = am.waveform_multi(ests, tg)
    flat = am.waveform_batch([ests[k][i] for i in range(len(tg)) for k in range(K)], [tg[i] for i in range(len(tg)) for _ in range(K)])
    assert [d for row in multi for d in row] == flat
    assert am.waveform_multi(ests, tg, deferred=True)() == multi
    # resident device inputs: key-major slices of one buffer, read where they lie
    dev = torch.device("cuda", 0)
    buf = torch.from_numpy(np.concatenate([e for key in ests for e in key])).to(dev)
    tbuf = torch.from_numpy(np.concatenate(tg)).to(dev)
    lens = [len(t) for t in tg]
    offs = np.concatenate(([0], np.cumsum(lens)))
    dev_tg = [tbuf[offs[i]:offs[i + 1]] for i in range(len(tg))]
    dev_ests = [[buf[k * offs[-1] + offs[i]:k * offs[-1] + offs[i + 1]] for i in range(len(tg))] for k in range(K)]
    assert am.waveform_multi(dev_ests, dev_tg, resident=True) == multi
    for i in range(len(tg)):
        for k in range(K):
            assert am.waveform(ests[k][i], tg[i]) == multi[i][k]                    # alone
            _check(multi[i][k], tg[i], ests[k][i], fs)


def test_evaluate_with_waveform_from_wav_files(tmp_path, monkeypatch):
    """SSR_Eval_Helper(waveform=True).evaluate() on a small wav tree (identity testee, two FFT keys and four IIR keys: float32 and
    float64 estimates, 44.1 kHz): the per-file values are AudioMetrics.waveform on the same estimates, the earlier metrics are
    those of a run without the option, bit for bit, waveform=None is that run, and with lsd_split and stoi the metric order is
    the four, lsd_lf / lsd_hf, stoi / estoi, snr / si_sdr / seg_snr."""
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
                            setting_lowpass_filtering={"cutoff_freq": [6000], "filter_order": [4],
                                                       "filter": ["butter", "cheby", "ellip", "bessel"]}, **kw)
        return h.evaluate(save_json=False)
    plain, res, off = run(), run(waveform=True), run(waveform=None)
    assert off == plain
    am = AudioMetrics(44100)
    fft = {"proc_fft_8000_44100": (4000, "stft_hard"), "proc_fft_22050_44100": (11025, "stft_hard")}
    iir = {"proc_%s_12000_4_44100" % t: (6000, f) for t, f in (("bw", "butter"), ("bessel", "bessel"), ("el", "ellip"), ("ch", "cheby1"))}
    n = 0
    for spk in counts:
        for fn in res[spk]:
            x, _ = read_audio(str(root / spk / fn))
            for key, (cut, kind) in {**fft, **iir}.items():
                got = res[spk][fn][key]
                assert list(got)[-3:] == list(NAMES)
                assert {m: got[m] for m in plain[spk][fn][key]} == plain[spk][fn][key]
                est = lowpass(x, cut, 44100, order=1 if kind == "stft_hard" else 4, _type=kind)
                est = np.asarray(est, np.float64 if kind != "stft_hard" else np.float32)
                want = am.waveform(est, np.asarray(x, np.float32))
                for m in NAMES:
                    assert abs(got[m] - want[m]) < 1e-9, (fn, key, m, got[m], want[m])
                _check(got, np.asarray(x, np.float32), est, 44100)
                n += 1
    assert n == 5 * 6
    assert set(NAMES) <= set(res["averaged"]["proc_fft_8000_44100"])
    full = run(waveform=True, lsd_split=True, stoi="both")
    spk = "p360"
    fn = next(iter(full[spk]))
    assert list(full[spk][fn]["proc_fft_8000_44100"]) == ["lsd", "log_sispec", "sispec", "ssim", "lsd_lf", "lsd_hf", "stoi", "estoi",
                                                         "snr", "si_sdr", "seg_snr"]
    for m in NAMES:
        assert full[spk][fn]["proc_fft_8000_44100"][m] == res[spk][fn]["proc_fft_8000_44100"][m]
