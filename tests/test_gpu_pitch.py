"""GPU tests (-m gpu) of the pitch metrics: ssr_f0_track / ssr_f0_metrics through AudioMetrics against the float64 oracle
(tests/pitch_oracle.py) on the oracle's stable frames - the 16 kHz signals bit-identical to SciPy, identical tau* and voicing, f0 and
aperiodicity within 1e-9 relative, the five metrics within 1e-9 at 16, 44.1 and 48 kHz on float32 / float64 targets and estimates
in every combination; ragged lengths (n = 0, shorter than a hop, 60 s); an estimate low-passed at 4 kHz and scored at 48 kHz;
digital silence and an octave error; a pair alone and in a batch of 64 (bits), pitch_multi against pitch_batch, two runs; and
SSR_Eval_Helper(pitch=...)."""
import numpy as np
import pytest
import torch

import pitch_oracle as O

pytestmark = pytest.mark.gpu

REL = 1e-9
NAMES = O.NAMES
DTYPES = [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)]


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"


def harmonic(f0, fs, n, phase=0.0):
    """Six harmonics of f0 (Hz, a scalar or one value per sample) with falling amplitudes."""
    f = np.broadcast_to(np.asarray(f0, np.float64), (n,))
    ph = 2 * np.pi * np.cumsum(f) / fs + phase
    return 0.3 * sum((0.6 ** k) * np.sin((k + 1) * ph + k) for k in range(6))


def _voice(rng, fs, n):
    """A gliding, amplitude-modulated harmonic voice with a little noise and a pause in the middle."""
    x = harmonic(np.linspace(100, 260, n), fs, n) * (1 + 0.5 * np.sin(np.arange(n) * 6.0 / fs))
    x[n // 2:n // 2 + n // 8] = 0
    return x + 0.003 * rng.standard_normal(n)


def _lowpass(x, fs, cut):
    X = np.fft.rfft(x)
    X[np.fft.rfftfreq(len(x), 1.0 / fs) >= cut] = 0
    return np.fft.irfft(X, len(x))


def _check_metrics(got, x, y, fs, fmin=50.0, fmax=500.0):
    """False when the oracle calls the pair unstable (not compared)."""
    want, stable = O.pitch(np.asarray(x, np.float64), np.asarray(y, np.float64), fs, fmin, fmax)
    if not stable:
        return False
    for m in got:
        if np.isnan(want[m]):
            assert np.isnan(got[m]), (m, len(x), got[m])
        else:
            assert abs(got[m] - want[m]) <= REL * max(1.0, abs(want[m])), (m, len(x), got[m], want[m])
    return True


@pytest.mark.parametrize("fs", [8000, 16000, 22050, 44100, 48000])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_sixteen_khz_signals_are_bit_identical_to_scipy(fs, dt):
    from ssr_eval_amd import backend as B
    rng = np.random.default_rng(fs)
    sigs = [rng.standard_normal(n).astype(dt) for n in (fs, 1, 0, 12345)]
    r = B.resample_to_pitch_rate(sigs, fs)
    for got, x in zip(r.split() if r.packed else [r.data[int(o):int(o) + int(n)] for o, n in zip(r.off.cpu(), r.lens_host)], sigs):
        want = O.to_16k(x, fs)
        np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("fs", [16000, 44100, 48000])
def test_tracks_match_the_oracle(fs):
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(fs + 1)
    am = AudioMetrics(fs)
    for x, (fmin, fmax) in ((_voice(rng, fs, int(1.3 * fs)), (50.0, 500.0)), (harmonic(330.0, fs, fs // 2), (60.0, 1000.0)),
                            (harmonic(45.0, fs, fs // 2), (40.0, 400.0)), (rng.standard_normal(fs // 3), (50.0, 500.0))):
        x = x.astype(np.float32)
        got = am.f0(x, fmin, fmax)
        want = O.track(x, fs, fmin, fmax)
        st = want["stable"]
        assert st.mean() >= 0.99
        np.testing.assert_array_equal(got["voiced"][st], want["voiced"][st])
        np.testing.assert_array_equal(np.isnan(got["f0"]), np.isnan(want["f0"]))
        ok = st & ~np.isnan(want["f0"])
        np.testing.assert_allclose(got["f0"][ok], want["f0"][ok], rtol=REL, atol=0)
        np.testing.assert_allclose(got["aperiodicity"][st], want["aperiodicity"][st], rtol=REL, atol=0)


@pytest.mark.parametrize("fs", [16000, 44100, 48000])
@pytest.mark.parametrize("dt", DTYPES)
def test_metrics_match_the_oracle(fs, dt):
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(fs + 7 * DTYPES.index(dt))
    n = int(0.8 * fs)
    x = _voice(rng, fs, n)
    pairs = [(x, x), (x, _voice(rng, fs, n)), (x, harmonic(np.linspace(100, 260, n) * 1.1, fs, n)),
             (x, x + 0.02 * rng.standard_normal(n)), (harmonic(150.0, fs, n), harmonic(150.0, fs, n, 1.0))]
    tg = [np.asarray(t, np.float32).astype(dt[0]) for t, _ in pairs]
    es = [np.asarray(e, np.float32).astype(dt[1]) for _, e in pairs]
    got = AudioMetrics(fs).pitch_batch(es, tg)
    assert sum(_check_metrics(g, t, e, fs) for g, t, e in zip(got, tg, es)) >= len(pairs) - 1
    assert got[0]["f0_rmse"] == 0 and got[0]["gpe"] == 0 and got[0]["vde"] == 0 and got[0]["f0_corr"] == 1.0


def test_ragged_lengths_and_a_sixty_second_pair():
    from ssr_eval_amd import AudioMetrics
    fs = 16000
    rng = np.random.default_rng(3)
    am = AudioMetrics(fs)
    long_x = _voice(rng, fs, 60 * fs).astype(np.float32)
    long_y = (long_x + 0.01 * rng.standard_normal(len(long_x))).astype(np.float32)
    tg = [np.zeros(0, np.float32), harmonic(200.0, fs, 100).astype(np.float32), long_x, harmonic(120.0, fs, 5000).astype(np.float32)]
    es = [np.zeros(0, np.float32), harmonic(100.0, fs, 100).astype(np.float32), long_y, harmonic(125.0, fs, 5000).astype(np.float32)]
    got = am.pitch_batch(es, tg)
    assert all(np.isnan(v) for v in got[0].values())
    assert got[1]["vde"] == 0 and np.isnan(got[1]["f0_rmse"])          # one frame, half its window past the signal: unvoiced
    n_checked = sum(_check_metrics(g, t, e, fs) for g, t, e in zip(got, tg, es))
    assert n_checked >= 3
    tr = am.f0(np.zeros(0, np.float32))
    assert all(len(v) == 0 for v in tr.values())


def test_super_resolution_case_at_48k():
    """The estimate is the target low-passed at 4 kHz, scored at 48 kHz: its F0 track is the target's."""
    from ssr_eval_amd import AudioMetrics
    fs = 48000
    rng = np.random.default_rng(4)
    x = _voice(rng, fs, 2 * fs).astype(np.float32)
    y = _lowpass(x.astype(np.float64), fs, 4000.0).astype(np.float32)
    got = AudioMetrics(fs).pitch(y, x)
    assert _check_metrics(got, x, y, fs)
    assert got["gpe"] < 0.02 and got["f0_rmse"] < 10 and got["f0_corr"] > 0.99


def test_digital_silence_and_an_octave_error():
    from ssr_eval_amd import AudioMetrics
    fs = 44100
    am = AudioMetrics(fs)
    x = harmonic(220.0, fs, fs).astype(np.float32)
    z = np.zeros(fs, np.float32)
    tr = am.f0(z)
    assert not tr["voiced"].any() and np.isnan(tr["f0"]).all()
    sil = am.pitch(z, x)                                   # the estimate is silent: every voiced target frame is a V/UV error
    assert np.isnan(sil["f0_rmse"]) and np.isnan(sil["gpe"]) and sil["vde"] == sil["ffe"] > 0.9
    oct_ = am.pitch(harmonic(110.0, fs, fs).astype(np.float32), x)
    assert _check_metrics(oct_, x, harmonic(110.0, fs, fs).astype(np.float32), fs)
    assert oct_["gpe"] == 1.0 and abs(oct_["f0_rmse"] - 1200) < 25


def test_bits_alone_in_a_batch_multi_and_repeat():
    from ssr_eval_amd import AudioMetrics
    fs = 48000
    rng = np.random.default_rng(6)
    am = AudioMetrics(fs)
    n = fs // 2
    tg = [_voice(rng, fs, n + 37 * i).astype(np.float32) for i in range(16)]
    ests = [[(t + (0.01 + 0.02 * k) * rng.standard_normal(len(t))).astype(np.float32) for t in tg] for k in range(4)]
    flat_e = [ests[k][i] for i in range(16) for k in range(4)]
    flat_t = [tg[i] for i in range(16) for _ in range(4)]
    batch = am.pitch_batch(flat_e, flat_t)                 # 64 pairs
    assert len(batch) == 64
    multi = am.pitch_multi(ests, tg)
    for i in range(16):
        for k in range(4):
            a, b = multi[i][k], batch[4 * i + k]
            assert all(a[m] == b[m] or (np.isnan(a[m]) and np.isnan(b[m])) for m in NAMES), (i, k)
    for j in (0, 21, 63):
        alone = am.pitch(flat_e[j], flat_t[j])
        assert all(alone[m] == batch[j][m] or (np.isnan(alone[m]) and np.isnan(batch[j][m])) for m in NAMES), j
    again = am.pitch_batch(flat_e, flat_t)
    np.testing.assert_array_equal(np.array([[r[m] for m in NAMES] for r in again]), np.array([[r[m] for m in NAMES] for r in batch]))
    sub = am.pitch_batch(flat_e[:5], flat_t[:5], which=("ffe", "f0_rmse"))
    assert [list(s) for s in sub] == [["f0_rmse", "ffe"]] * 5
    assert all(s["ffe"] == b["ffe"] and s["f0_rmse"] == b["f0_rmse"] for s, b in zip(sub, batch))
    dev_t = [torch.from_numpy(t).cuda() for t in flat_t[:8]]           # device tensors give the same bits
    dev_e = [torch.from_numpy(e).cuda() for e in flat_e[:8]]
    on_dev = am.pitch_batch(dev_e, dev_t, resident=True)
    assert all(on_dev[j][m] == batch[j][m] or np.isnan(batch[j][m]) for j in range(8) for m in NAMES)


def test_evaluate_with_pitch_from_wav_files(tmp_path, monkeypatch):
    """SSR_Eval_Helper(pitch=True).evaluate() on a small wav tree (identity testee, two FFT keys and two IIR keys: float32 and
    float64 estimates, 44.1 kHz): the per-file values are AudioMetrics.pitch on the same estimates, the earlier metrics are those of a
    run without the option, bit for bit, pitch=None is that run, and the pitch metrics come last in the metric order.  With all six
    optional families on, the keys of a result come in the order the families run and the pitch values are the pitch=True run's bits."""
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee, AudioMetrics
    from ssr_eval_amd.io import write_wav, read_audio
    from ssr_eval_amd.lowpass import lowpass
    rng = np.random.default_rng(99)
    fs = 44100
    root = tmp_path / "vctk_test"
    counts = {"p360": 2, "p361": 1}
    for spk, c in counts.items():
        (root / spk).mkdir(parents=True)
        for i in range(c):
            x = _voice(rng, fs, int(rng.integers(30000, 50000)))
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), x.astype(np.float32), fs)
    monkeypatch.chdir(tmp_path)

    def run(**kw):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=fs, output_sr=fs, evaluation_sr=fs, test_data_root=str(root),
                            setting_fft={"cutoff_freq": [4000, 11025]},
                            setting_lowpass_filtering={"cutoff_freq": [6000], "filter_order": [4], "filter": ["butter", "cheby"]}, **kw)
        return h.evaluate(save_json=False)
    plain, res, off = run(), run(pitch=True), run(pitch=None)
    assert off == plain
    am = AudioMetrics(fs)
    keys = {"proc_fft_8000_44100": (4000, "stft_hard"), "proc_fft_22050_44100": (11025, "stft_hard"),
            "proc_bw_12000_4_44100": (6000, "butter"), "proc_ch_12000_4_44100": (6000, "cheby1")}
    n = 0
    for spk in counts:
        for fn in res[spk]:
            x, _ = read_audio(str(root / spk / fn))
            for key, (cut, kind) in keys.items():
                got = res[spk][fn][key]
                assert list(got)[-5:] == list(NAMES)
                assert {m: got[m] for m in plain[spk][fn][key]} == plain[spk][fn][key]
                est = lowpass(x, cut, fs, order=1 if kind == "stft_hard" else 4, _type=kind)
                est = np.asarray(est, np.float64 if kind != "stft_hard" else np.float32)
                want = am.pitch(est, np.asarray(x, np.float32))
                for m in NAMES:
                    assert abs(got[m] - want[m]) < 1e-9 or (np.isnan(got[m]) and np.isnan(want[m])), (fn, key, m, got[m], want[m])
                n += 1
    assert n == 3 * 4
    assert set(NAMES) <= set(res["averaged"]["proc_fft_8000_44100"])
    sub = run(pitch={"which": ("vde", "f0_rmse"), "fmin": 60.0}, waveform=("snr",))
    fn = next(iter(sub["p360"]))
    assert list(sub["p360"][fn]["proc_fft_8000_44100"])[-3:] == ["snr", "f0_rmse", "vde"]
    # every optional family at once: the result keys in the order the families run, the pitch values those of the pitch=True run
    full = run(lsd_split=True, stoi="both", waveform=True, mel=True, quality=True, pitch=True)
    order = ["lsd", "log_sispec", "sispec", "ssim", "lsd_lf", "lsd_hf", "stoi", "estoi", "snr", "si_sdr", "seg_snr", "mel_lsd", "mel_l1",
             "mcd", "llr", "cep_dist", "wss", "fwseg_snr", "f0_rmse", "f0_corr", "gpe", "vde", "ffe"]
    for spk in counts:
        for fn in res[spk]:
            for key in keys:
                got = full[spk][fn][key]
                assert list(got) == order
                assert np.array([got[m] for m in NAMES]).tobytes() == np.array([res[spk][fn][key][m] for m in NAMES]).tobytes()
