"""GPU tests (-m gpu) of the DTW-aligned mel-cepstral distortion (mcd_dtw, dtw_dev, dtw_len): k_mel_cepstra and
k_mel_dtw through AudioMetrics against the float64 oracle (tests/mel_dtw_oracle.py) - the value at the mel family's 1e-5 relative
(1e-6 absolute near 0), the path integers exactly on pairs whose path the oracle finds stable under 1e-4 relative perturbations of
every local cost (all pairs here are) - float32 and float64 estimates, ragged batches down to one frame, every radius class;
radius 0 against mcd; monotonicity in the radius bit for bit; the image-level entry point; multi against batch, a pair alone and a
second run bit for bit; a 16 s signal; the 48 kHz default front end; and SSR_Eval_Helper(mel_dtw=...)."""
import numpy as np
import pytest
import torch

import mel_dtw_oracle as DO
import mel_oracle as MO

pytestmark = pytest.mark.gpu

FS, N_FFT, HOP, N_MELS = 16000, 512, 128, 40
MEL = dict(n_mels=N_MELS)
RADII = (0, 1, 5, 16, 31)
# (samples, shift, noise) of the ragged batch: 1.0 s, 0.4 s, then T = 3, 1 and 2 frames.  Their paths are stable at every radius
# (a band of one frame forces a pair that lags by more than a frame through the target's silent stretch, where every route ties and
# only the tie rule decides: such pairs are not accepted at R = 1) ...
RAGGED = ((16000, 100, 0.0), (6400, 100, 0.003), (300, 100, 0.0), (7, 0, 0.003), (129, 100, 0.003))
# ... and one that lags by more than two frames, whose path is compared from R = 5 on
LAGGING = (16000, 300, 0.003)


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"


def make_pair(n, shift, noise, ed=np.float32, rate=FS):
    """(estimate, target): the harmonic test signal and its shifted, noisy copy."""
    x = DO.harmonic(n, rate)
    return DO.shifted(x, shift, noise).astype(ed), x.astype(np.float32)


def metrics(rate=FS, n_fft=N_FFT, hop=HOP):
    from ssr_eval_amd import AudioMetrics
    return AudioMetrics(rate, n_fft=n_fft, hop_length=hop)


def oracle_cepstra(am, est, tgt, **mel):
    fb, n_cep = am.mel_filterbank(**mel)
    m = min(len(est), len(tgt))
    return tuple(DO.cepstra(MO.magnitudes(w[:m], am.rate, am.n_fft, am.hop_length), fb.numpy(), n_cep) for w in (est, tgt))


def check(got, cE, cG, R, what, path=True):
    """got against the oracle: the value at the mel family's bar; the path integers exactly (the pair's path must be stable)."""
    want = DO.dtw(cE, cG, R)
    print(what, "R", R, "got", got, "want", {k: want[k] for k in DO.NAMES})
    assert list(got) == list(DO.NAMES)
    assert abs(got["mcd_dtw"] - want["mcd_dtw"]) <= 1e-5 * abs(want["mcd_dtw"]) + 1e-6, (what, R, got, want)
    if path:
        assert DO.path_is_stable(cE, cG, R, rel=1e-4), (what, R)
        assert got["dtw_len"] == want["dtw_len"] and got["dtw_dev"] == want["dtw_dev"], (what, R, got, want)


_ORACLE = {}


def ragged(ed):
    """The ragged batch and its oracle cepstra (computed once per estimate dtype)."""
    if ed not in _ORACLE:
        am = metrics()
        pairs = [make_pair(n, sh, nz, ed) for n, sh, nz in RAGGED + (LAGGING,)]
        _ORACLE[ed] = (pairs, [oracle_cepstra(am, e, t, **MEL) for e, t in pairs])
    return _ORACLE[ed]


@pytest.mark.parametrize("ed", [np.float32, np.float64])
def test_against_the_oracle(ed):
    am = metrics()
    pairs, ceps = ragged(ed)
    for R in RADII:
        got = am.mel_dtw_batch([e for e, _ in pairs], [t for _, t in pairs], R, **MEL)
        for j, (g, (cE, cG)) in enumerate(zip(got, ceps)):
            check(g, cE, cG, R, (ed.__name__, j), path=j < len(RAGGED) or R >= 5)
    assert [len(c[0]) for c in ceps] == [126, 51, 3, 1, 2, 126]
    # the single-pair call and truncation to the common length
    e, t = pairs[0]
    assert am.mel_dtw(e, t, 16, **MEL) == am.mel_dtw_batch([e], [t], 16, **MEL)[0]
    cE, cG = oracle_cepstra(am, e[:-40], t, **MEL)
    check(am.mel_dtw(e[:-40], t, 5, **MEL), cE, cG, 5, "truncated", path=False)


def test_radius_zero_is_mcd():
    am = metrics()
    pairs, ceps = ragged(np.float32)
    pairs = pairs + [make_pair(16000, 700, 0.003)]
    got = am.mel_dtw_batch([e for e, _ in pairs], [t for _, t in pairs], 0, **MEL)
    mcd = am.mel_distance_batch([e for e, _ in pairs], [t for _, t in pairs], "mcd", **MEL)
    n = 0
    for g, m, (e, _) in zip(got, mcd, pairs):
        print(g, m)
        T = 1 + len(e) // HOP
        assert g["dtw_dev"] == 0.0 and g["dtw_len"] == T
        if m["mcd"] > 0.1:
            assert abs(g["mcd_dtw"] - m["mcd"]) <= 1e-9 * m["mcd"]
            n += 1
    assert n >= 4


def test_monotone_in_the_radius_bit_for_bit():
    am = metrics()
    pairs = [make_pair(n, sh, nz) for n, sh, nz in RAGGED + (LAGGING, (16000, 700, 0.0), (9000, 256, 0.003))]
    v = [np.array([g["mcd_dtw"] for g in am.mel_dtw_batch([e for e, _ in pairs], [t for _, t in pairs], R, **MEL)]) for R in RADII]
    for a, b in zip(v, v[1:]):
        assert (b <= a).all(), (a, b)
    assert (v[-1] < v[0]).sum() >= 4          # and the warp does find something on the shifted pairs


def image_pair():
    """Hand-made [T, F] images: a smooth spectral envelope that moves over time, the estimate two frames late, with a run of
    identical all-zero rows in both."""
    T, F = 45, N_FFT // 2 + 1
    f = np.arange(F)[None, :]
    t = np.arange(T + 2)[:, None]
    S = np.exp(-((f - 40.0 - 3.0 * t) / 25.0) ** 2) + 0.3 * np.exp(-((f - 200.0 + 2.0 * t) / 40.0) ** 2) + 1e-3
    S = S * (1.0 + 0.2 * np.sin(0.7 * t))
    tgt, est = S[2:].copy(), 1.1 * S[:-2]
    tgt[14:23] = 0.0
    est[16:25] = 0.0
    return est.astype(np.float32), tgt.astype(np.float32)


def test_image_level_entry_point():
    am = metrics()
    fb, n_cep = am.mel_filterbank(**MEL)
    est, tgt = image_pair()
    cE, cG = DO.cepstra(est, fb.numpy(), n_cep), DO.cepstra(tgt, fb.numpy(), n_cep)
    E = torch.from_numpy(np.stack([est, tgt]).reshape(2, 1, *est.shape)).cuda()
    G = torch.from_numpy(np.stack([tgt, tgt]).reshape(2, 1, *tgt.shape)).cuda()
    for R in (0, 3, 31):
        got = am.mel_dtw_spectrogram(E, G, R, **MEL)
        assert list(got) == list(DO.NAMES) and got["mcd_dtw"].shape == (2, 1) and got["mcd_dtw"].is_cuda
        check({m: float(got[m][0, 0]) for m in DO.NAMES}, cE, cG, R, "images")
        check({m: float(got[m][1, 0]) for m in DO.NAMES}, cG, cG, R, "images, estimate = target")
        assert float(got["mcd_dtw"][1, 0]) == 0.0 and float(got["dtw_dev"][1, 0]) == 0.0
    assert DO.dtw(cE, cG, 3)["dtw_dev"] > 1.5          # the two-frame lag is found through the zero rows


@pytest.mark.parametrize("K", [4, 5])
def test_multi_equals_batch_bit_for_bit(K):
    am = metrics()
    tg = [DO.harmonic(n).astype(np.float32) for n in (16000, 6400, 300, 9000)]
    ests = [[DO.shifted(t.astype(np.float64), min(60 * k, len(t) // 2), 0.001 * k, seed=k).astype(np.float32) for t in tg] for k in range(K)]
    multi = am.mel_dtw_multi(ests, tg, 16, **MEL)
    flat = am.mel_dtw_batch([ests[k][i] for i in range(len(tg)) for k in range(K)], [tg[i] for i in range(len(tg)) for _ in range(K)], 16, **MEL)
    assert [multi[i][k] for i in range(len(tg)) for k in range(K)] == flat
    assert am.mel_dtw_multi(ests, tg, 16, deferred=True, **MEL)() == multi          # a second run
    for i in range(len(tg)):                                                        # a pair alone: its bits in the batch
        assert am.mel_dtw(ests[K - 1][i], tg[i], 16, **MEL) == multi[i][K - 1]
    short = am.mel_dtw_multi(ests, tg, 16, lengths=False, **MEL)
    assert list(short[0][0]) == ["mcd_dtw", "dtw_dev"] and short[1][2]["mcd_dtw"] == multi[1][2]["mcd_dtw"]


def test_sixteen_second_signal():
    am = metrics()
    e, t = make_pair(16 * FS, 300, 0.003)
    cE, cG = oracle_cepstra(am, e, t, **MEL)
    assert len(cE) == 2001
    check(am.mel_dtw(e, t, 16, **MEL), cE, cG, 16, "16 s")


def test_default_front_end_at_48_khz():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(48000)
    e, t = make_pair(24000, 900, 0.0, rate=48000)
    cE, cG = oracle_cepstra(am, e, t)
    for R in (16, 31):
        check(am.mel_dtw(e, t, R), cE, cG, R, "48 kHz")
    assert am.mel_dtw(e, t) == am.mel_dtw(e, t, 16)


def test_evaluate_with_mel_dtw_from_wav_files(tmp_path, monkeypatch):
    """SSR_Eval_Helper(mel_dtw=True).evaluate() on a four-file wav tree (identity testee, two FFT keys): every key carries mcd_dtw
    and dtw_dev (no dtw_len) after the mel keys, the per-file values are AudioMetrics.mel_dtw on the same estimates, `averaged` is
    their mean, the earlier metrics are those of a run without the option bit for bit, and mel_dtw=None is that run."""
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee, AudioMetrics
    from ssr_eval_amd.io import write_wav, read_audio
    from ssr_eval_amd.lowpass import lowpass
    rng = np.random.default_rng(16)
    root = tmp_path / "vctk_test"
    counts = {"p360": 2, "p361": 2}
    for spk, c in counts.items():
        (root / spk).mkdir(parents=True)
        for i in range(c):
            x = DO.harmonic(int(rng.integers(30000, 50000)), 44100, seed=i)
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), x.astype(np.float32), 44100)
    monkeypatch.chdir(tmp_path)

    def run(**kw):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=44100, output_sr=44100, evaluation_sr=44100, test_data_root=str(root),
                            setting_fft={"cutoff_freq": [4000, 11025]}, **kw)
        return h.evaluate(save_json=False)
    plain, res, off = run(), run(mel_dtw=True), run(mel_dtw=None)
    assert off == plain
    assert run(mel=None) == plain
    am = AudioMetrics(44100)
    keys = {"proc_fft_8000_44100": 4000, "proc_fft_22050_44100": 11025}
    per_key = {k: [] for k in keys}
    for spk in counts:
        for fn in res[spk]:
            x, _ = read_audio(str(root / spk / fn))
            for key, cut in keys.items():
                got = res[spk][fn][key]
                assert list(got)[-2:] == ["mcd_dtw", "dtw_dev"] and "dtw_len" not in got
                assert {m: got[m] for m in plain[spk][fn][key]} == plain[spk][fn][key]
                est = np.asarray(lowpass(x, cut, 44100, order=1, _type="stft_hard"), np.float32)
                want = am.mel_dtw(est, np.asarray(x, np.float32))
                for m in ("mcd_dtw", "dtw_dev"):
                    assert abs(got[m] - want[m]) <= 1e-6 * abs(want[m]) + 1e-9, (fn, key, m, got[m], want[m])
                per_key[key].append(got)
    for key, rows in per_key.items():
        assert len(rows) == 4
        for m in ("mcd_dtw", "dtw_dev"):
            assert res["averaged"][key][m] == pytest.approx(np.mean([r[m] for r in rows]), rel=1e-12, abs=1e-15)
        assert "dtw_len" not in res["averaged"][key]
    full = run(mel={"n_mels": 80, "which": ("mcd",)}, mel_dtw={"radius": 4, "n_mels": 80}, waveform="snr")
    fn = next(iter(full["p360"]))
    assert list(full["p360"][fn]["proc_fft_8000_44100"]) == ["lsd", "log_sispec", "sispec", "ssim", "snr", "mcd", "mcd_dtw", "dtw_dev"]
