"""GPU tests (-m gpu) of the anti-wrapping phase distances (ssr_phase_metrics): ragged batches against the
float64 oracle (tests/phase_oracle.py) within 1e-9 rad - the bound of tests/test_phase_host.py, under the same conditioning
assertion -, the NaN cases, bit-identity of a pair alone / inside a batch / on a repeated call / through the multi path, a 60 s
pair, and SSR_Eval_Helper(phase=...) with the bootstrap and compare_results on a small wav tree."""
import numpy as np
import pytest
import torch

import phase_oracle as O

pytestmark = pytest.mark.gpu

NAMES = O.NAMES
TOL = 1e-9
R_MIN = 1e-6
FR = 16                                   # frames per chunk (SSR_PHASE_FR)


def _noise(rng, n, dtype=np.float32):
    return rng.standard_normal(n).astype(np.float32).astype(dtype)


def _check(got, ests, tgts, n_fft, hop, bins=None):
    """Dict rows against the oracle: within TOL, NaN where it has NaN; every scored cell at r >= R_MIN -> the worst difference."""
    worst = 0.0
    for e, (d, y, x) in enumerate(zip(got, ests, tgts)):
        want = O.phase_distance(x, y, n_fft, hop, bins)
        assert min(O.conditioning(x, y, n_fft, hop, bins)) >= R_MIN, e
        assert list(d) == list(NAMES)
        for m in NAMES:
            print("pair %d n=%d %s: got %.17g want %.17g diff %.3g" % (e, len(x), m, d[m], want[m], abs(d[m] - want[m])))
            if np.isnan(want[m]):
                assert np.isnan(d[m]), (e, m, d[m])
            else:
                worst = max(worst, abs(d[m] - want[m]))
                assert abs(d[m] - want[m]) <= TOL, (e, m, d[m], want[m])
    return worst


@pytest.mark.parametrize("rate,n_fft,hop,band", [(16000, 256, None, None), (16000, 512, 512, (1000.0, 5000.0)), (16000, 1024, 342, None),
                                                 (48000, 1024, None, None), (48000, 2048, None, (0, 0)),
                                                 (48000, 2048, 2048, (24000, 24000))])
def test_ragged_batch_against_the_oracle(rate, n_fft, hop, band):
    """12 pairs of 0.1 .. 1.0 s, float32 and float64 on either side, some targets shared: every value within 1e-9 rad."""
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(rate + n_fft)
    am = AudioMetrics(rate)
    lens = [int(rate * s) for s in (0.1, 0.13, 0.25, 0.3377, 0.5, 0.61, 0.77, 1.0)]
    tgts, ests = [], []
    for i, n in enumerate(lens):
        x = _noise(rng, n, np.float64 if i % 4 == 3 else np.float32)
        for _ in range(2 if i < 4 else 1):                                 # the short targets carry two estimates each
            tgts.append(x)
            ests.append(_noise(rng, n, np.float64 if len(ests) % 3 == 2 else np.float32))
    assert len(ests) == 12
    got = am.phase_distance_batch(ests, tgts, "all", n_fft, hop, band)
    h = n_fft // 4 if hop is None else hop
    bins = am._phase_bins(rate, n_fft, band)
    _check(got, ests, tgts, n_fft, h, bins)
    if bins is not None and bins[0] == bins[1]:
        assert all(np.isnan(d["phase_gd"]) and not np.isnan(d["phase_ip"]) for d in got)


@pytest.mark.parametrize("n_fft", O.N_FFTS)
def test_chunk_edges_and_shortest_lengths(n_fft):
    """T = 1 and 2 (hop = n_fft), T = FR, FR + 1 and 2 FR + 1 (hop = n_fft / 4: IAF across a chunk boundary and the warm-up frame),
    the shortest valid length - through the backend call, float32 targets with float64 estimates; `which` subsets give the bits of
    the full call."""
    from ssr_eval_amd import backend as B
    rng = np.random.default_rng(n_fft)
    for hop, frames in ((n_fft, (1, 2)), (n_fft // 4, (FR, FR + 1, 2 * FR + 1))):
        lens = [max((T - 1) * hop + 1, n_fft // 2 + 1) for T in frames] + [n_fft // 2 + 1]
        assert [O.num_frames(n, n_fft, hop) for n in lens[:-1]] == list(frames)
        tgts = [_noise(rng, n) for n in lens]
        ests = [_noise(rng, n, np.float64) for n in lens]
        full = B.phase_metrics(tgts, ests, list(range(len(lens))), n_fft, hop)
        _check([dict(zip(NAMES, row)) for row in full], ests, tgts, n_fft, hop)
        for which in (1, 3, 4, 6):
            sub = B.phase_metrics(tgts, ests, list(range(len(lens))), n_fft, hop, which=which)
            cols = [j for j in range(3) if which & (1 << j)]
            assert sub.tobytes() == np.ascontiguousarray(full[:, cols]).tobytes(), which


def test_nan_cases_and_silence():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(16000)
    rng = np.random.default_rng(4)
    z = np.zeros(0, np.float32)
    assert all(np.isnan(v) for v in am.phase_distance(z, z).values())                                  # n = 0
    for n in (1, 511, 512):                                                                            # n <= N / 2
        assert all(np.isnan(v) for v in am.phase_distance(_noise(rng, n), _noise(rng, n)).values()), n
    one = am.phase_distance(_noise(rng, 513), _noise(rng, 513), hop=1024)                              # T = 1
    assert np.isnan(one["phase_iaf"]) and 0 <= one["phase_ip"] <= np.pi and 0 <= one["phase_gd"] <= np.pi
    single = am.phase_distance(_noise(rng, 4000), _noise(rng, 4000), band=(2000, 2010))                # a single-bin band
    assert am._phase_bins(16000, 1024, (2000, 2010)) == (128, 128)
    assert np.isnan(single["phase_gd"]) and 0 <= single["phase_ip"] <= np.pi and 0 <= single["phase_iaf"] <= np.pi
    assert am.phase_distance(_noise(rng, 4000), _noise(rng, 4000), which="phase_gd", band=(2000, 2010)).keys() == {"phase_gd"}
    # the zero rule: silence against silence scores 0 and is counted; a silent stretch of the estimate only scores 0 on its frames
    s = np.zeros(4000, np.float32)
    assert am.phase_distance(s, s) == {m: 0.0 for m in NAMES}
    x, y = _noise(rng, 8000), _noise(rng, 8000)
    y[3000:3000 + 2 * 1024 + 5] = 0.0
    x2, y2 = x.copy(), y.copy()
    x2[1000:2500] = 0.0
    y2[1000:2500] = 0.0
    _check(am.phase_distance_batch([y, y2], [x, x2], n_fft=256, hop=64), [y, y2], [x, x2], 256, 64)
    # y = x and y = -x
    same, neg = am.phase_distance(x, x), am.phase_distance(-x, x)
    assert all(same[m] <= 1e-12 for m in NAMES)
    assert abs(neg["phase_ip"] - np.pi) <= 1e-12 and neg["phase_gd"] <= 1e-12 and neg["phase_iaf"] <= 1e-12


def _bits(d):
    return np.array([d[m] for m in NAMES]).tobytes()


def test_a_pair_has_the_same_bits_alone_in_a_batch_and_again():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(48000)
    rng = np.random.default_rng(8)
    lens = [int(n) for n in rng.integers(600, 9000, 64)]
    tgts = [_noise(rng, n) for n in lens]
    ests = [_noise(rng, n) for n in lens]
    batch = am.phase_distance_batch(ests, tgts, n_fft=512)
    again = am.phase_distance_batch(ests, tgts, n_fft=512)
    assert [_bits(d) for d in batch] == [_bits(d) for d in again]
    for i in (0, 17, 40, 63):
        assert _bits(am.phase_distance(ests[i], tgts[i], n_fft=512)) == _bits(batch[i]), i
    dev = am.phase_distance_batch([torch.from_numpy(e).cuda() for e in ests[:8]], [torch.from_numpy(t).cuda() for t in tgts[:8]],
                                  n_fft=512, resident=True)                                             # device tensors: the same bits
    assert [_bits(d) for d in dev] == [_bits(d) for d in batch[:8]]


def test_multi_is_three_single_calls():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(16000)
    rng = np.random.default_rng(9)
    lens = (3000, 5000, 777, 16000)
    tgts = [_noise(rng, n) for n in lens]
    by_key = [[_noise(rng, n) for n in lens] for _ in range(3)]
    multi = am.phase_distance_multi(by_key, tgts, hop=200)
    assert len(multi) == 4 and all(len(row) == 3 for row in multi)
    for i in range(4):
        for k in range(3):
            assert _bits(multi[i][k]) == _bits(am.phase_distance(by_key[k][i], tgts[i], hop=200)), (i, k)
    sub = am.phase_distance_multi(by_key, tgts, ("phase_iaf", "phase_ip"), hop=200)
    assert all(list(sub[i][k]) == ["phase_ip", "phase_iaf"] and sub[i][k]["phase_iaf"] == multi[i][k]["phase_iaf"] and
               sub[i][k]["phase_ip"] == multi[i][k]["phase_ip"] for i in range(4) for k in range(3))


def test_a_minute_at_48_khz():
    """One 60 s pair: 5,626 frames in 352 chunks, the chunk sums added in chunk order."""
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(10)
    n = 60 * 48000
    x, y = _noise(rng, n), _noise(rng, n)
    got = AudioMetrics(48000).phase_distance(y, x, hop=512)
    _check([got], [y], [x], 1024, 512)


def test_evaluate_with_phase_and_bootstrap_from_wav_files(tmp_path, monkeypatch):
    """SSR_Eval_Helper(phase=True, bootstrap=200).evaluate() on a small wav tree (identity testee, two FFT keys, 44.1 kHz): every key
    carries the three phase values of AudioMetrics.phase_distance on the same estimate, last in the metric order; the confidence
    block has the three columns and so has compare_results() of two such runs; the other metrics are those of a run without the
    option, bit for bit; phase=None is that run."""
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee, AudioMetrics, compare_results
    from ssr_eval_amd.io import write_wav, read_audio
    from ssr_eval_amd.lowpass import lowpass
    rng = np.random.default_rng(11)
    fs = 44100
    root = tmp_path / "vctk_test"
    counts = {"p360": 3, "p361": 2}
    for spk, c in counts.items():
        (root / spk).mkdir(parents=True)
        for i in range(c):
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), 0.1 * _noise(rng, int(rng.integers(20000, 40000))), fs)
    monkeypatch.chdir(tmp_path)

    def run(**kw):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=fs, output_sr=fs, evaluation_sr=fs, test_data_root=str(root),
                            setting_fft={"cutoff_freq": [4000, 11025]}, **kw)
        return h.evaluate(save_json=False)
    plain, off, res = run(), run(phase=None), run(phase=True, bootstrap=200)
    assert off == plain and not any("phase" in m for m in plain["averaged"]["proc_fft_8000_44100"])
    am = AudioMetrics(fs)
    keys = {"proc_fft_8000_44100": 4000, "proc_fft_22050_44100": 11025}
    n = 0
    for spk in counts:
        for fn in res[spk]:
            x, _ = read_audio(str(root / spk / fn))
            for key, cut in keys.items():
                got = res[spk][fn][key]
                assert list(got)[-3:] == list(NAMES)
                assert {m: got[m] for m in plain[spk][fn][key]} == plain[spk][fn][key]
                assert "phase_ip" not in plain[spk][fn][key]
                est = np.asarray(lowpass(x, cut, fs, order=1, _type="stft_hard"), np.float32)
                want = am.phase_distance(est, np.asarray(x, np.float32))
                for m in NAMES:
                    print(fn, key, m, got[m], want[m])
                    assert got[m] == want[m], (fn, key, m, got[m], want[m])
                n += 1
    assert n == 5 * 2
    for key in keys:
        assert list(res["averaged"][key])[-3:] == list(NAMES)
        conf = res["confidence"]["averaged"][key]
        assert list(conf) == list(res["averaged"][key])
        for m in NAMES:
            assert set(conf[m]) == {"se", "lo", "hi"} and 0 <= conf[m]["lo"] <= conf[m]["hi"] <= np.pi and conf[m]["se"] >= 0
    # compare_results pairs the phase columns like any other: against a run with 512-point frames the three differ, the rest do not
    res2 = run(phase={"n_fft": 512})
    cmp_ = compare_results(res, res2, n_boot=200, seed=1)
    assert sorted(cmp_) == sorted(keys)
    for key in keys:
        assert list(cmp_[key]) == list(res["averaged"][key]) and list(cmp_[key])[-3:] == list(NAMES)
        for m, v in cmp_[key].items():
            print(key, m, v)
            assert sorted(v) == ["diff", "hi", "lo", "p", "se"]
            assert abs(v["diff"] - (res["averaged"][key][m] - res2["averaged"][key][m])) <= 1e-12, (key, m)
            if m in NAMES:
                assert v["diff"] != 0 and v["se"] > 0 and v["lo"] <= v["hi"] and 0 < v["p"] <= 1, (key, m)
            else:
                assert v == {"diff": 0.0, "se": 0.0, "lo": 0.0, "hi": 0.0, "p": 1.0}, (key, m)
    sub = run(phase={"which": ("phase_iaf",), "n_fft": 512, "band": (0, 4000)}, waveform=("snr",))
    fn = next(iter(sub["p360"]))
    assert list(sub["p360"][fn]["proc_fft_8000_44100"])[-2:] == ["snr", "phase_iaf"]
