"""GPU tests (-m gpu) of the band-split LSD (LSD-LF / LSD-HF): the HIP band reduction (ssr_lsd_bands.h) through the C ABI, the
waveform-level calls and SSR_Eval_Helper(lsd_split=...), against the oracle's LSD (oracle/metrics.py, pinned to the reference)
applied to the band's columns of oracle spectrograms."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("lsd", "log_sispec", "sispec", "ssim")
CUTOFFS_HZ = [1000, 2000, 4000, 6000, 8000, 12000, 16000]


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"


def band_lsd(es, ts, a, b):
    """The reference's AudioMetrics.lsd on the columns [a, b) of two [1, 1, T, F] oracle spectrograms."""
    from oracle import metrics as om
    return float(om.lsd(es[..., a:b].clone(), ts[..., a:b].clone()))


def oracle_split(est, tgt, rate, cutoff_hz):
    from oracle import metrics as om
    n_fft, hop = om.stft_params(rate)
    m = min(est.shape[0], tgt.shape[0])
    es, ts = om.wav_to_spectrogram(est[:m], n_fft, hop), om.wav_to_spectrogram(tgt[:m], n_fft, hop)
    F = n_fft // 2 + 1
    c = int(F * (cutoff_hz / (rate / 2)))
    return band_lsd(es, ts, 0, c), band_lsd(es, ts, c, F)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


def _images(rng, n, T, F):
    x = np.abs(rng.standard_normal((n, T, F))).astype(np.float32)
    x[:, :, ::7] *= 1e-3                              # some bins far below their neighbours
    return x


@pytest.mark.parametrize("F", [1025, 1115, 513, 372])
def test_image_level_ragged_rows_shared_targets_against_sliced_oracle(F):
    """ssr_spectrogram_lsd_bands on ragged images (T = 5 .. 140), two estimates per target, 1 to 8 bands per image including
    single-bin bands and [0, F)."""
    from ssr_eval_amd import _lib
    from ssr_eval_amd.backend import _vp
    rng = np.random.default_rng(F)
    T = [140, 5, 77, 33, 96, 12]
    n_img = 2 * len(T)                                 # image 2 i and 2 i + 1 share target i
    tgt_off = np.concatenate(([0], np.cumsum(T)[:-1])).astype(np.int64)
    tgt = np.concatenate([_images(rng, 1, t, F)[0] for t in T])
    est_rows = [t for t in T for _ in range(2)]
    est_off = np.concatenate(([0], np.cumsum(est_rows)[:-1])).astype(np.int64)
    est = np.concatenate([_images(rng, 1, t, F)[0] for t in est_rows])
    for nb in (1, 2, 3, 8):
        edges = []
        for v in range(n_img):
            if nb == 1:
                e = [0, F] if v % 2 == 0 else [F // 3, F // 3 + 1]                  # the whole band / one bin
            else:
                inner = np.sort(rng.choice(np.arange(4, F - 1), nb - 1, replace=False))     # inside (3, F - 1): both layouts
                e = [0] + inner.tolist() + [F] if v % 2 == 0 else [3] + inner.tolist() + [F - 1]
                if v == 1:
                    e = list(range(5, 5 + nb + 1))                                     # every band one bin wide
            edges.append(e)
        edges = np.array(edges, dtype=np.int32)
        lib = _lib.load()
        d = lambda a: torch.from_numpy(a).cuda()                                       # noqa: E731
        x, y, xo, yo = d(est), d(tgt), d(est_off), d(np.repeat(tgt_off, 2))
        rows = d(np.array(est_rows, dtype=np.int32))
        out = torch.empty((n_img, nb), dtype=torch.float64, device="cuda")
        ws_bytes = lib.ssr_spectrogram_lsd_bands_workspace_bytes(n_img, max(T), nb)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        _lib.check(lib.ssr_spectrogram_lsd_bands(_vp(x), _vp(xo), _vp(y), _vp(yo), _vp(rows), n_img, max(T), F,
                                                 edges.ctypes.data_as(C.c_void_p), nb, _vp(out), _vp(ws), ws_bytes, None))
        got = out.cpu().numpy()
        for v in range(n_img):
            i, t = v // 2, est_rows[v]
            es = torch.from_numpy(est[est_off[v]:est_off[v] + t])[None, None]
            ts = torch.from_numpy(tgt[tgt_off[i]:tgt_off[i] + t])[None, None]
            for j in range(nb):
                want = band_lsd(es, ts, edges[v, j], edges[v, j + 1])
                assert _rel(got[v, j], want) < 1e-5, (F, nb, v, j, got[v, j], want)


def test_tensor_api_lsd_bands():
    """AudioMetrics.lsd_bands on [B, C, T, F] tensors: one edge list for every image, or one per image; [0, F) is lsd()."""
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(7)
    am = AudioMetrics(44100)
    e, t = torch.from_numpy(_images(rng, 6, 50, 1025).reshape(2, 3, 50, 1025)), torch.from_numpy(_images(rng, 6, 50, 1025).reshape(2, 3, 50, 1025))
    got = am.lsd_bands(e, t, [0, 100, 101, 557, 1025]).numpy()
    assert got.shape == (2, 3, 4)
    for b in range(2):
        for c in range(3):
            for j, (lo, hi) in enumerate([(0, 100), (100, 101), (101, 557), (557, 1025)]):
                assert _rel(got[b, c, j], band_lsd(e[b:b + 1, c:c + 1], t[b:b + 1, c:c + 1], lo, hi)) < 1e-5
    full = am.lsd_bands(e, t, [0, 1025]).numpy()[..., 0]
    np.testing.assert_allclose(full, am.lsd(e, t).numpy()[..., 0, 0], rtol=1e-5)
    per = np.broadcast_to(np.array([0, 512, 1025]), (2, 3, 3)).copy()
    per[1, 2] = [10, 20, 30]
    got = am.lsd_bands(e.cuda(), t.cuda(), per)
    assert got.is_cuda
    assert _rel(got[1, 2, 1].item(), band_lsd(e[1:2, 2:3], t[1:2, 2:3], 20, 30)) < 1e-5


@pytest.mark.parametrize("name", ["noise48k", "noise44k", "noise16k", "speech48k_fftlp6k", "speech44k_fftlp4k_ragged", "speech24k_scaled"])
def test_full_band_through_the_waveform_path_is_the_lsd(golden, name):
    """Bands [0, F) (a split at or above Nyquist: lsd_lf is the whole band, lsd_hf NaN) against ssr_pair_metrics' lsd (<= 1e-6) and
    against the reference's golden LSD (1e-5)."""
    from ssr_eval_amd import AudioMetrics
    rate = int(golden["ev_%s_rate" % name])
    am = AudioMetrics(rate)
    est, tgt = golden["ev_%s_est" % name], golden["ev_%s_tgt" % name]
    got = am.lsd_split(est, tgt, rate)
    assert np.isnan(got["lsd_hf"])
    assert _rel(got["lsd_lf"], am.evaluation(est, tgt)["lsd"]) <= 1e-6
    assert _rel(got["lsd_lf"], float(golden["ev_%s_out" % name][0])) < 1e-5


@pytest.mark.parametrize("rate", [48000, 44100, 16000])
def test_waveform_level_float32_keys_against_oracle(rate):
    """K = 7 FFT-low-passed float32 estimates per target, each split at its own cutoff (lsd_split_multi), and one key."""
    from ssr_eval_amd import AudioMetrics
    from ssr_eval_amd.lowpass import stft_hard_lowpass_multi
    rng = np.random.default_rng(rate)
    n = 3
    tgts = [(0.1 * rng.standard_normal(int(rng.integers(rate // 2, rate)))).astype(np.float32) for _ in range(n)]
    cuts = [c for c in CUTOFFS_HZ if c < rate // 2]
    ys = stft_hard_lowpass_multi(tgts, [c / (rate / 2) for c in cuts])
    ests = [[np.asarray(y, dtype=np.float32) + (1e-3 * rng.standard_normal(y.shape[0])).astype(np.float32) for y in key] for key in ys]
    am = AudioMetrics(rate)
    got = am.lsd_split_multi(ests, tgts, cuts)
    for i in range(n):
        for k, c in enumerate(cuts):
            lf, hf = oracle_split(ests[k][i], tgts[i], rate, c)
            assert _rel(got[i][k]["lsd_lf"], lf) < 1e-5 and _rel(got[i][k]["lsd_hf"], hf) < 1e-5, (i, k)
    one = am.lsd_split_multi([ests[2]], tgts, [cuts[2]])
    for i in range(n):
        lf, hf = oracle_split(ests[2][i], tgts[i], rate, cuts[2])
        assert _rel(one[i][0]["lsd_lf"], lf) < 1e-5 and _rel(one[i][0]["lsd_hf"], hf) < 1e-5
    single = am.lsd_split(ests[1][0], tgts[0], cuts[1])
    assert _rel(single["lsd_lf"], got[0][1]["lsd_lf"]) < 1e-6 and _rel(single["lsd_hf"], got[0][1]["lsd_hf"]) < 1e-6


@pytest.mark.parametrize("rate", [48000, 44100])
def test_waveform_level_36_float64_iir_keys_against_oracle(rate):
    """K = 36 float64 IIR keys (lowpass_iir_multi: four designs x three cutoffs x three orders), split at their cutoffs."""
    from ssr_eval_amd import AudioMetrics
    from ssr_eval_amd.lowpass import lowpass_iir_multi
    rng = np.random.default_rng(36 + rate)
    n = 2
    tgts = [(0.1 * rng.standard_normal(int(rng.integers(rate // 2, rate)))).astype(np.float32) for _ in range(n)]
    specs = [(c, o, f) for f in ("butter", "cheby1", "ellip", "bessel") for c in (2000, 4000, 8000) for o in (2, 4, 8)]
    ys = lowpass_iir_multi(tgts, specs, rate)
    ests = [[np.asarray(y) for y in key] for key in ys]
    assert all(e.dtype == np.float64 for key in ests for e in key)
    am = AudioMetrics(rate)
    got = am.lsd_split_multi(ests, tgts, [s[0] for s in specs])
    for i in range(n):
        for k, (c, _, _) in enumerate(specs):
            lf, hf = oracle_split(ests[k][i], tgts[i], rate, c)
            assert _rel(got[i][k]["lsd_lf"], lf) < 1e-5 and _rel(got[i][k]["lsd_hf"], hf) < 1e-5, (i, k)


@pytest.mark.parametrize("est64,n_fft,hop", [
    pytest.param(False, 2229, 480, id="False"), pytest.param(True, 2229, 480, id="True"),
    pytest.param(False, 4096, 1024, id="False-4096x1024"), pytest.param(True, 4096, 1024, id="True-4096x1024")])
def test_chunked_keys_equal_one_launch(est64, n_fft, hop):
    """backend.pair_lsd_bands in chunks of keys equals the unchunked call (to the float32 rounding of a magnitude taken with a
    different transform partner: <= 1e-6 relative).  2229: the keys go two per complex transform; 4096 (a block engine): every key
    goes with the target, whose rows land in the scratch plane from key 1 on."""
    from ssr_eval_amd import backend as B
    rng = np.random.default_rng(11)
    n, K, rate = 3, 12, 48000
    plan = B.get_plan(n_fft, hop)
    tgts = [(0.1 * rng.standard_normal(20000 + 999 * i)).astype(np.float32) for i in range(n)]
    dt = np.float64 if est64 else np.float32
    ests = [[(t + 0.02 * rng.standard_normal(t.shape[0])).astype(dt) for t in tgts] for _ in range(K)]
    F = plan.n_bins
    edges = [[[0, 50 + 40 * k, 600, F] for _ in range(n)] for k in range(K)]
    whole = B.pair_lsd_bands(plan, ests, tgts, edges)
    for kc in (1, 5, 6):
        part = B.pair_lsd_bands(plan, ests, tgts, edges, keys_per_chunk=kc)
        np.testing.assert_allclose(part, whole, rtol=1e-6)
    from oracle import metrics as om
    es, ts = om.wav_to_spectrogram(ests[7][1], n_fft, hop), om.wav_to_spectrogram(tgts[1], n_fft, hop)
    assert _rel(whole[1, 7, 1], band_lsd(es, ts, 50 + 40 * 7, 600)) < 1e-5


def test_low_passed_estimate_keeps_its_low_band():
    """An FFT-low-passed estimate at its own cutoff: the low band is intact, the high band is what was removed."""
    from ssr_eval_amd import AudioMetrics
    from ssr_eval_amd.lowpass import lowpass
    rng = np.random.default_rng(3)
    tgt = (0.1 * rng.standard_normal(44100)).astype(np.float32)
    est = np.asarray(lowpass(tgt, 4000, 44100, order=1, _type="stft_hard"), dtype=np.float32)
    d = AudioMetrics(44100).lsd_split(est, tgt, 4000)
    assert d["lsd_lf"] < 0.05 * d["lsd_hf"], d
    assert d["lsd_hf"] > 1.0


def test_evaluate_with_lsd_split_from_wav_files(tmp_path, monkeypatch):
    """SSR_Eval_Helper(lsd_split=True).evaluate() on a small wav tree (identity testee, two FFT keys, 44.1 kHz throughout): the per-file
    values are direct lsd_split calls on the same estimates, each_speaker / averaged are the mean of speaker means, and the four
    reference metrics are those of a run without lsd_split, bit for bit."""
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee, AudioMetrics
    from ssr_eval_amd.io import write_wav, read_audio
    from ssr_eval_amd.lowpass import lowpass
    from oracle import aggregate as oagg
    rng = np.random.default_rng(4242)
    root = tmp_path / "vctk_test"
    counts = {"p360": 3, "p361": 2}
    for spk, c in counts.items():
        (root / spk).mkdir(parents=True)
        for i in range(c):
            n = int(rng.integers(30000, 60000))
            t = np.arange(n) / 44100.0
            x = 0.2 * np.sin(2 * np.pi * (180 + 50 * i) * t) + 0.05 * rng.standard_normal(n)
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), x.astype(np.float32), 44100)
    monkeypatch.chdir(tmp_path)

    def run(split):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=44100, output_sr=44100, evaluation_sr=44100, test_data_root=str(root),
                            setting_fft={"cutoff_freq": [4000, 11025]}, lsd_split=split)
        return h.evaluate(save_json=False)
    plain, res = run(None), run(True)
    keys = {"proc_fft_8000_44100": 4000, "proc_fft_22050_44100": 11025}
    am = AudioMetrics(44100)
    expect = {}
    for spk in counts:
        expect[spk] = {}
        for fn in res[spk]:
            x, _ = read_audio(str(root / spk / fn))
            expect[spk][fn] = {}
            for key, cut in keys.items():
                got = res[spk][fn][key]
                assert list(got)[:6] == ["lsd", "log_sispec", "sispec", "ssim", "lsd_lf", "lsd_hf"]
                assert {m: got[m] for m in KEYS} == plain[spk][fn][key]
                est = np.asarray(lowpass(x, cut, 44100, order=1, _type="stft_hard"), dtype=np.float32)
                want = am.lsd_split(est, np.asarray(x, np.float32), cut)
                for m in ("lsd_lf", "lsd_hf"):
                    assert _rel(got[m], want[m]) < 1e-6, (fn, key, m)
                expect[spk][fn][key] = {m: got[m] for m in ("lsd_lf", "lsd_hf")}
    for key in keys:
        assert {m: res["averaged"][key][m] for m in KEYS} == plain["averaged"][key]
        for spk in counts:
            assert {m: res["each_speaker"][spk][key][m] for m in KEYS} == plain["each_speaker"][spk][key]
    each, avg = oagg.aggregate(expect)
    for key in keys:
        for m in ("lsd_lf", "lsd_hf"):
            assert _rel(res["averaged"][key][m], avg[key][m]) < 1e-12
            for spk in counts:
                assert _rel(res["each_speaker"][spk][key][m], each[spk][key][m]) < 1e-12
