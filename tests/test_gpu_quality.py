"""GPU tests (-m gpu) of the objective quality measures (LLR, LPC cepstral distance, WSS, fwSNRseg): ssr_quality_metrics through
AudioMetrics against the float64 oracle (tests/quality_oracle.py, 1e-5 absolute), on float32 / float64 targets and estimates in
every combination, speech-like and noise signals, an estimate low-passed at 4 kHz and scored at 48 kHz, ragged lengths (M = 0 and
n = 0 among them), a 60 s pair and a target with digital silence; the y == x identities; quality_multi against quality_batch, a
pair alone against the same pair in a batch of 64 (bits); `which` subsets and `lpc_order`; and SSR_Eval_Helper(quality=...)."""
import numpy as np
import pytest
import torch

import quality_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5
NAMES = O.NAMES
DTYPES = [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)]


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"


def _check(got, x, y, fs, lpc_order=None):
    want = O.quality(x, y, fs, lpc_order)
    for m in NAMES:
        if np.isnan(want[m]):
            assert np.isnan(got[m]), (m, len(x), got[m])
        else:
            assert abs(got[m] - want[m]) < TOL, (m, len(x), got[m], want[m])


def _speechy(rng, n, fs):
    """Noise through a few resonances (a vowel-like spectral envelope) with a syllable-rate amplitude: no digital silence."""
    if n == 0:
        return np.zeros(0)
    e = rng.standard_normal(n + 400)
    y = np.zeros_like(e)
    for f0, r in ((500.0, 0.97), (1500.0, 0.95), (2500.0, 0.93)):
        a1, a2 = 2 * r * np.cos(2 * np.pi * f0 / fs), -r * r
        z = np.zeros_like(e)
        for i in range(2, len(e)):
            z[i] = e[i] + a1 * z[i - 1] + a2 * z[i - 2]
        y += z / np.std(z)
    y = y[400:]
    return 0.1 * y * (1.2 + np.sin(2 * np.pi * 4.0 * np.arange(n) / fs))


def _lowpass(x, fs, cut):
    X = np.fft.rfft(x)
    X[np.fft.rfftfreq(len(x), 1.0 / fs) >= cut] = 0
    return np.fft.irfft(X, len(x))


def _pairs(rng, fs, td, ed):
    """(target, estimate) pairs; targets hold float32 values in either dtype."""
    L, R, _ = O.frame_geometry(fs, 0)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)      # noqa: E731
    out = []
    x = f32(_speechy(rng, int(0.6 * fs) + 17, fs))
    out.append((x, x + 0.02 * rng.standard_normal(len(x))))                 # speech + mild noise
    out.append((x, 0.7 * x + 0.002 * rng.standard_normal(len(x))))          # scaled
    out.append((x, _lowpass(x, fs, 4000.0)))                                # the SR case: low-passed at 4 kHz
    nz = f32(0.1 * rng.standard_normal(int(0.4 * fs)))
    out.append((nz, nz + 0.05 * rng.standard_normal(len(nz))))              # noise
    z = f32(_speechy(rng, int(0.5 * fs), fs))
    z[len(z) // 4:len(z) // 2] = 0.0                                         # digital silence in the target
    out.append((z, z + 0.01 * rng.standard_normal(len(z))))
    for n in (L + R - 1, L + R, L + 3 * R, 0, 7):                           # M = 0, M = 1, M = 3, n = 0, n < L
        x = f32(_speechy(rng, n, fs))
        out.append((x, x + 0.05 * rng.standard_normal(n)))
    return [(np.asarray(x, td), np.asarray(y, ed)) for x, y in out]


@pytest.mark.parametrize("fs", [16000, 44100, 48000])
@pytest.mark.parametrize("dt", DTYPES)
def test_quality_matches_the_oracle(fs, dt):
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(fs + 2 * (dt[0] == np.float64) + (dt[1] == np.float64))
    pairs = _pairs(rng, fs, *dt)
    am = AudioMetrics(fs)
    got = am.quality_batch([y for _, y in pairs], [x for x, _ in pairs])
    for (x, y), g in zip(pairs, got):
        assert list(g) == list(NAMES)
        _check(g, x, y, fs)
    for i in (5, 8, 9):                                                      # M = 0, n = 0, n < L
        assert all(np.isnan(v) for v in got[i].values()), i
    assert all(np.isfinite(v) for v in got[6].values())                      # M = 1
    # the single-pair API and the single measures: the same bits as in the batch
    y, x = pairs[0][1], pairs[0][0]
    assert am.quality(y, x) == got[0]
    assert am.llr(y, x) == got[0]["llr"] and am.cep_dist(y, x) == got[0]["cep_dist"]
    assert am.wss(y, x) == got[0]["wss"] and am.fwseg_snr(y, x) == got[0]["fwseg_snr"]


@pytest.mark.parametrize("fs", [16000, 48000])
def test_identical_signals_give_the_exact_identities(fs):
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(7)
    sigs = [np.asarray(_speechy(rng, fs, fs), np.float32), np.asarray(0.1 * rng.standard_normal(fs // 2), np.float32),
            np.asarray(_speechy(rng, fs // 3, fs), np.float64)]
    got = AudioMetrics(fs).quality_batch([s.copy() for s in sigs], sigs)
    for g in got:
        assert g == {"llr": 0.0, "cep_dist": 0.0, "wss": 0.0, "fwseg_snr": 35.0}, g


def test_sixty_second_pair():
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(60)
    fs = 48000
    x = np.asarray(np.tile(_speechy(rng, 5 * fs, fs), 12) + 1e-3 * rng.standard_normal(60 * fs), np.float32)
    y = (x + 0.01 * rng.standard_normal(len(x))).astype(np.float32)
    _check(AudioMetrics(fs).quality(y, x), x, y, fs)


def test_multi_batch_alone_and_repeat_are_bit_identical():
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(11)
    fs, K = 48000, 4
    tg = [np.asarray(_speechy(rng, n, fs), np.float32) for n in (30000, 24001, 1900, 41000)]
    ests = [[(t + (0.01 + 0.05 * k) * rng.standard_normal(len(t))).astype(np.float32) for t in tg] for k in range(K)]
    am = AudioMetrics(fs)
    multi = am.quality_multi(ests, tg)
    flat = am.quality_batch([ests[k][i] for i in range(len(tg)) for k in range(K)], [tg[i] for i in range(len(tg)) for _ in range(K)])
    assert [d for row in multi for d in row] == flat
    assert am.quality_multi(ests, tg, deferred=True)() == multi
    # resident device inputs: key-major slices of one buffer, read where they lie
    dev = torch.device("cuda", 0)
    buf = torch.from_numpy(np.concatenate([e for key in ests for e in key])).to(dev)
    tbuf = torch.from_numpy(np.concatenate(tg)).to(dev)
    offs = np.concatenate(([0], np.cumsum([len(t) for t in tg])))
    dev_tg = [tbuf[offs[i]:offs[i + 1]] for i in range(len(tg))]
    dev_ests = [[buf[k * offs[-1] + offs[i]:k * offs[-1] + offs[i + 1]] for i in range(len(tg))] for k in range(K)]
    assert am.quality_multi(dev_ests, dev_tg, resident=True) == multi
    for i in range(len(tg)):
        for k in range(K):
            assert am.quality(ests[k][i], tg[i]) == multi[i][k]                   # alone
            _check(multi[i][k], tg[i], ests[k][i], fs)


def test_a_pair_alone_and_in_a_batch_of_64():
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(64)
    fs = 16000
    tg = [np.asarray(_speechy(rng, int(rng.integers(3000, 12000)), fs), np.float32) for _ in range(64)]
    es = [(t + 0.03 * rng.standard_normal(len(t))).astype(np.float32) for t in tg]
    am = AudioMetrics(fs)
    batch = am.quality_batch(es, tg)
    for i in (0, 17, 63):
        assert am.quality(es[i], tg[i]) == batch[i]


def test_which_subsets_and_lpc_order():
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(12)
    fs = 44100
    x = np.asarray(_speechy(rng, fs // 2, fs), np.float32)
    ys = [(x + 0.02 * rng.standard_normal(len(x))).astype(np.float32), _lowpass(x, fs, 4000.0).astype(np.float32)]
    am = AudioMetrics(fs)
    full = am.quality_batch(ys, [x, x])
    for which in ("llr", "cep_dist", "wss", "fwseg_snr", ("wss", "llr"), ("cep_dist", "fwseg_snr"), ("llr", "cep_dist", "wss")):
        sub = am.quality_batch(ys, [x, x], which)
        names = (which,) if isinstance(which, str) else which
        for f, s in zip(full, sub):
            assert list(s) == [m for m in NAMES if m in names]
            assert s == {m: f[m] for m in s}
    got = am.quality_batch(ys, [x, x], lpc_order=12)
    for g, y in zip(got, ys):
        _check(g, x, y, fs, lpc_order=12)
    assert got[0]["llr"] != full[0]["llr"] and got[0]["wss"] == full[0]["wss"]
    with pytest.raises(ValueError):
        am.quality(ys[0], x, lpc_order=33)


def test_evaluate_with_quality_from_wav_files(tmp_path, monkeypatch):
    """SSR_Eval_Helper(quality=True).evaluate() on a small wav tree (identity testee, two FFT keys and two IIR keys: float32 and
    float64 estimates, 44.1 kHz): the per-file values are AudioMetrics.quality on the same estimates, the earlier metrics are those of
    a run without the option, bit for bit, quality=None is that run, and the measures come last in the metric order."""
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
            x = _speechy(rng, int(rng.integers(30000, 50000)), fs)
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), x.astype(np.float32), fs)
    monkeypatch.chdir(tmp_path)

    def run(**kw):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=fs, output_sr=fs, evaluation_sr=fs, test_data_root=str(root),
                            setting_fft={"cutoff_freq": [4000, 11025]},
                            setting_lowpass_filtering={"cutoff_freq": [6000], "filter_order": [4], "filter": ["butter", "cheby"]}, **kw)
        return h.evaluate(save_json=False)
    plain, res, off = run(), run(quality=True), run(quality=None)
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
                assert list(got)[-4:] == list(NAMES)
                assert {m: got[m] for m in plain[spk][fn][key]} == plain[spk][fn][key]
                est = lowpass(x, cut, fs, order=1 if kind == "stft_hard" else 4, _type=kind)
                est = np.asarray(est, np.float64 if kind != "stft_hard" else np.float32)
                want = am.quality(est, np.asarray(x, np.float32))
                for m in NAMES:
                    assert abs(got[m] - want[m]) < 1e-9, (fn, key, m, got[m], want[m])
                n += 1
    assert n == 3 * 4
    assert set(NAMES) <= set(res["averaged"]["proc_fft_8000_44100"])
    sub = run(quality={"which": ("wss", "llr"), "lpc_order": 12}, waveform=("snr",))
    fn = next(iter(sub["p360"]))
    assert list(sub["p360"][fn]["proc_fft_8000_44100"])[-3:] == ["snr", "llr", "wss"]
