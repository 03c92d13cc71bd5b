"""GPU tests (-m gpu) of the multi-resolution STFT distance (ssr_mrstft_metrics): ragged batches against the
float64 oracle (tests/mrstft_oracle.py) within 1e-9 (absolute + relative) - the bound and the argument of
tests/test_mrstft_host.py, on the same kind of signals -, the chunk edges and shortest lengths, the exact and NaN cases,
bit-identity of a pair alone / inside a batch / on a repeated call / through the multi path, a 60 s pair, and
SSR_Eval_Helper(mrstft=...) with the bootstrap on a small wav tree."""
import numpy as np
import pytest
import torch

import mrstft_oracle as O

pytestmark = pytest.mark.gpu

NAMES = ("mrstft_sc", "mrstft_mag", "mrstft")
TOL = 1e-9
DEFAULT = O.DEFAULT_RESOLUTIONS


def _noise(rng, n, dtype=np.float32, sigma=0.1):
    return (sigma * rng.standard_normal(n)).astype(np.float32).astype(dtype)


def _near(rng, x, level=0.03, sigma=0.1, dtype=None):
    return (x + level * _noise(rng, len(x), x.dtype, sigma)).astype(x.dtype if dtype is None else dtype)


def _close(got, want):
    return (np.isnan(got) and np.isnan(want)) or abs(got - want) <= TOL + TOL * abs(want)


def _check(got, ests, tgts, resolutions=DEFAULT, bands=None, eps=O.EPS):
    """per_resolution dict rows against the oracle: within TOL, NaN where it has NaN -> the worst absolute difference."""
    worst = 0.0
    for e, (d, y, x) in enumerate(zip(got, ests, tgts)):
        want, rows = O.mrstft(x, y, resolutions, bands, eps)
        assert list(d)[:3] == list(NAMES)
        pairs = [(d[m], want[m], m) for m in NAMES]
        assert [(r["n_fft"], r["hop"], r["win"]) for r in d["resolutions"]] == [tuple(r) for r in resolutions]
        for r, (g, w) in enumerate(zip(d["resolutions"], rows)):
            pairs += [(g["sc"], w[0], "sc%d" % r), (g["mag"], w[1], "mag%d" % r)]
        for g, w, m in pairs:
            print("pair %d n=%d %s: got %.17g want %.17g diff %.3g" % (e, len(x), m, g, w, abs(g - w)))
            assert _close(g, w), (e, m, g, w)
            if not np.isnan(w):
                worst = max(worst, abs(g - w))
    return worst


@pytest.mark.parametrize("rate,resolutions,band", [(16000, None, None), (48000, None, None), (48000, None, (4000.0, 12000.0)),
                                                   (16000, ((256, 64, 256), (512, 171, 301)), (0, 300))])
def test_ragged_batch_against_the_oracle(rate, resolutions, band):
    """12 pairs of 0.1 .. 1.0 s, float32 and float64 on either side, some targets shared; estimates near their target and
    independent ones: every value within 1e-9."""
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(rate + (0 if band is None else 1) + (0 if resolutions is None else 2))
    am = AudioMetrics(rate)
    lens = [int(rate * s) for s in (0.1, 0.13, 0.25, 0.3377, 0.5, 0.61, 0.77, 1.0)]
    tgts, ests = [], []
    for i, n in enumerate(lens):
        x = _noise(rng, n, np.float64 if i % 4 == 3 else np.float32)
        for _ in range(2 if i < 4 else 1):                                 # the short targets carry two estimates each
            tgts.append(x)
            dt = np.float64 if len(ests) % 3 == 2 else np.float32
            ests.append(_near(rng, x, dtype=dt) if len(ests) % 2 else _noise(rng, n, dt))
    assert len(ests) == 12
    got = am.mrstft_batch(ests, tgts, resolutions, band, per_resolution=True)
    res = DEFAULT if resolutions is None else resolutions
    print("worst", _check(got, ests, tgts, res, am._mrstft_bins(rate, res, band)))
    assert all(np.isfinite(d["mrstft"]) for d in got)


@pytest.mark.parametrize("n_fft", O.N_FFTS)
def test_chunk_edges_and_shortest_lengths(n_fft):
    """T = 1 and 2 (hop = n_fft), T = 16, 17 and 33 (hop = n_fft / 4: the chunk edges), a hop that does not divide n_fft, the
    shortest valid length and n = n_fft / 2 (NaN), at win = n_fft, an even and an odd win < n_fft - through the backend call,
    float32 targets with float64 estimates."""
    from ssr_eval_amd import backend as B
    rng = np.random.default_rng(n_fft)
    for hop, frames in ((n_fft, (1, 2)), (n_fft // 4, (16, 17, 33)), (n_fft // 3 + 1, (17,))):
        res = ((n_fft, hop, n_fft), (n_fft, hop, n_fft // 2 + 88), (n_fft, hop, n_fft // 2 + 89))
        lens = [max((T - 1) * hop + 1, n_fft // 2 + 1) for T in frames] + [n_fft // 2 + 1, n_fft // 2]
        assert [O.num_frames(n, n_fft, hop) for n in lens[:-2]] == list(frames)
        tgts = [_noise(rng, n) for n in lens]
        ests = [_near(rng, t, dtype=np.float64) for t in tgts]
        full = B.mrstft_metrics(tgts, ests, list(range(len(lens))), res)
        assert full.shape == (len(lens), 4, 2) and np.isnan(full[-1]).all() and np.isfinite(full[:-1]).all()
        for e in range(len(lens)):
            want, rows = O.mrstft(tgts[e], ests[e], res)
            for r, w in enumerate(rows + [(want["mrstft_sc"], want["mrstft_mag"])]):
                print(n_fft, hop, lens[e], r, full[e, r], w)
                assert _close(full[e, r, 0], w[0]) and _close(full[e, r, 1], w[1]), (hop, e, r, full[e, r], w)
        # a resolution's row does not depend on the other resolutions of the call
        alone = B.mrstft_metrics(tgts, ests, list(range(len(lens))), res[1:2])
        assert alone[:, 0].tobytes() == np.ascontiguousarray(full[:, 1]).tobytes()


def test_exact_and_nan_cases():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(16000)
    rng = np.random.default_rng(4)
    zero = {m: 0.0 for m in NAMES}
    z0 = np.zeros(0, np.float32)
    assert all(np.isnan(v) for v in am.mrstft(z0, z0).values())                                        # n = 0
    x = _noise(rng, 8000)
    for y in (x, x.copy(), x.astype(np.float64)):                                                      # y == x: exactly 0 / 0
        d = am.mrstft(y, x, DEFAULT + ((256, 64, 256), (512, 50, 241)), per_resolution=True)
        assert {m: d[m] for m in NAMES} == zero and all(r["sc"] == 0.0 and r["mag"] == 0.0 for r in d["resolutions"]), d
    s = np.zeros(4000, np.float32)
    assert am.mrstft(s, s) == zero                                                                     # both silent
    # n = N / 2 of one resolution: NaN there and in the means, the other rows finite
    d = am.mrstft(_near(rng, x[:1024]), x[:1024], per_resolution=True)
    assert all(np.isnan(d[m]) for m in NAMES) and np.isnan(d["resolutions"][1]["sc"]) and np.isnan(d["resolutions"][1]["mag"])
    assert all(np.isfinite(d["resolutions"][r][k]) for r in (0, 2) for k in ("sc", "mag"))
    # silent estimate against a loud target and the reverse; a silent stretch inside both, and inside the estimate only
    y = _noise(rng, 8000)
    y[3000:3000 + 2 * 2048 + 5] = 0.0
    x2, y2 = x.copy(), _near(rng, x)
    x2[1000:6500] = 0.0
    y2[1000:6500] = 0.0
    sz = np.zeros(8000, np.float32)
    ests, tgts = [sz, x, y, y2], [x, sz, x, x2]
    _check(am.mrstft_batch(ests, tgts, per_resolution=True), ests, tgts)
    # the vote: a silent signal against a loud one (sigma = 100: bins of about 1.4e3 at N = 512, the packed transform's rounding
    # error squared about 1e-25) at eps = 1e-36 - the split alone would hand the silent side that rounding error and clamp nothing;
    # with the vote it is eps exactly, as the oracle's zero spectrum; then a silent stretch inside a loud pair
    res, lx, lz = ((512, 128, 512),), 1e3 * _noise(rng, 8000, np.float64), np.zeros(8000, np.float64)
    assert (3e-16 * np.max(O.magnitudes(lx, *res[0], eps=1e-36))) ** 2 > 1e6 * 1e-36
    lx2, ly2 = lx.copy(), 1e3 * _noise(rng, 8000, np.float64)
    ly2[1500:1500 + 3 * 512] = 0.0
    lx2[4000:4000 + 2 * 512] = 0.0
    ve, vt = [lz, lx, lx.astype(np.float32), ly2], [lx, lz, lz, lx2]
    _check(am.mrstft_batch(ve, vt, res, eps=1e-36, per_resolution=True), ve, vt, res, eps=1e-36)
    _check(am.mrstft_batch(ests, tgts, eps=1e-3, per_resolution=True), ests, tgts, eps=1e-3)


def _bits(d):
    return np.array([d[m] for m in NAMES] + [v for r in d["resolutions"] for v in (r["sc"], r["mag"])]).tobytes()


def test_a_pair_has_the_same_bits_alone_in_a_batch_and_again():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(48000)
    rng = np.random.default_rng(8)
    lens = [int(n) for n in rng.integers(1100, 9000, 48)]
    tgts = [_noise(rng, n) for n in lens]
    ests = [_near(rng, t, 0.3) for t in tgts]
    batch = am.mrstft_batch(ests, tgts, per_resolution=True)
    again = am.mrstft_batch(ests, tgts, per_resolution=True)
    assert [_bits(d) for d in batch] == [_bits(d) for d in again]
    for i in (0, 17, 47):
        assert _bits(am.mrstft(ests[i], tgts[i], per_resolution=True)) == _bits(batch[i]), i
    dev = am.mrstft_batch([torch.from_numpy(e).cuda() for e in ests[:8]], [torch.from_numpy(t).cuda() for t in tgts[:8]],
                          per_resolution=True, resident=True)                                          # device tensors: the same bits
    assert [_bits(d) for d in dev] == [_bits(d) for d in batch[:8]]
    plain = am.mrstft_batch(ests[:4], tgts[:4])
    assert [list(d) for d in plain] == [list(NAMES)] * 4
    assert all(p[m] == b[m] for p, b in zip(plain, batch) for m in NAMES)
    assert all(d["mrstft"] == d["mrstft_sc"] + d["mrstft_mag"] for d in batch)


def test_multi_is_single_calls():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(16000)
    rng = np.random.default_rng(9)
    lens = (3000, 5000, 1777, 16000)
    tgts = [_noise(rng, n) for n in lens]
    by_key = [[_near(rng, t, 0.1 * (k + 1)) for t in tgts] for k in range(3)]
    multi = am.mrstft_multi(by_key, tgts, per_resolution=True)
    assert len(multi) == 4 and all(len(row) == 3 for row in multi)
    for i in range(4):
        for k in range(3):
            assert _bits(multi[i][k]) == _bits(am.mrstft(by_key[k][i], tgts[i], per_resolution=True)), (i, k)


def test_a_minute_at_48_khz():
    """One 60 s pair: 24,001 / 12,001 / 57,601 frames in 1,501 / 751 / 3,601 chunks, the chunk sums added in chunk order."""
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(10)
    n = 60 * 48000
    x = _noise(rng, n)
    y = _near(rng, x, 0.2)
    got = AudioMetrics(48000).mrstft(y, x, per_resolution=True)
    _check([got], [y], [x])


def test_evaluate_with_mrstft_and_bootstrap_from_wav_files(tmp_path, monkeypatch):
    """SSR_Eval_Helper(mrstft=True, bootstrap=200).evaluate() on a small wav tree (identity testee, two FFT keys, 44.1 kHz): every
    key carries the three values of AudioMetrics.mrstft on the same estimate - and the oracle's within 1e-9 -, last in the metric
    order, after the phase keys; the confidence block has the three columns; the other metrics are those of a run without the
    option, bit for bit; mrstft=None is that run."""
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee, AudioMetrics
    from ssr_eval_amd.io import write_wav, read_audio
    from ssr_eval_amd.lowpass import lowpass
    rng = np.random.default_rng(11)
    fs = 44100
    root = tmp_path / "vctk_test"
    counts = {"p360": 3, "p361": 2}
    for spk, c in counts.items():
        (root / spk).mkdir(parents=True)
        for i in range(c):
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), _noise(rng, int(rng.integers(20000, 40000))), fs)
    monkeypatch.chdir(tmp_path)

    def run(**kw):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=fs, output_sr=fs, evaluation_sr=fs, test_data_root=str(root),
                            setting_fft={"cutoff_freq": [4000, 11025]}, **kw)
        return h.evaluate(save_json=False)
    plain, off, res = run(), run(mrstft=None), run(mrstft=True, bootstrap=200, phase="phase_ip")
    assert off == plain and not any("mrstft" in m for m in plain["averaged"]["proc_fft_8000_44100"])
    am = AudioMetrics(fs)
    keys = {"proc_fft_8000_44100": 4000, "proc_fft_22050_44100": 11025}
    n = 0
    for spk in counts:
        for fn in res[spk]:
            x, _ = read_audio(str(root / spk / fn))
            x = np.asarray(x, np.float32)
            for key, cut in keys.items():
                got = res[spk][fn][key]
                assert list(got)[-4:] == ["phase_ip"] + list(NAMES)
                assert {m: got[m] for m in plain[spk][fn][key]} == plain[spk][fn][key]
                est = np.asarray(lowpass(x, cut, fs, order=1, _type="stft_hard"), np.float32)
                want, oracle = am.mrstft(est, x), O.mrstft(x, est)[0]
                for m in NAMES:
                    print(fn, key, m, got[m], want[m], oracle[m])
                    assert got[m] == want[m], (fn, key, m, got[m], want[m])
                    assert _close(got[m], oracle[m]), (fn, key, m, got[m], oracle[m])
                n += 1
    assert n == 5 * 2
    for key in keys:
        assert list(res["averaged"][key])[-3:] == list(NAMES)
        conf = res["confidence"]["averaged"][key]
        assert list(conf) == list(res["averaged"][key])
        for m in NAMES:
            assert set(conf[m]) == {"se", "lo", "hi"} and 0 <= conf[m]["lo"] <= conf[m]["hi"] and conf[m]["se"] >= 0
    sub = run(mrstft={"resolutions": ((512, 128, 512),), "band": (0, 4000), "eps": 1e-5}, waveform=("snr",))
    fn = next(iter(sub["p360"]))
    got = sub["p360"][fn]["proc_fft_8000_44100"]
    assert list(got)[-4:] == ["snr"] + list(NAMES)
    x = np.asarray(read_audio(str(root / "p360" / fn))[0], np.float32)
    est = np.asarray(lowpass(x, 4000, fs, order=1, _type="stft_hard"), np.float32)
    want = O.mrstft(x, est, ((512, 128, 512),), [am._phase_bins(fs, 512, (0, 4000))], 1e-5)[0]
    assert all(_close(got[m], want[m]) for m in NAMES), (got, want)
