"""GPU tests (-m gpu) of the filter-invariant SDR (ssr_bss_sdr): the input list and the geometry shapes of
tests/test_bss_host.py through the C ABI against the float64 oracle (tests/bss_oracle.py) at the same bars - sdr within 1e-6 dB,
sdr_lag equal, the filter within 1e-10 of max|c| on the white target -, a 64-pair ragged batch, the exact facts, the multi path
against single calls bit for bit, a 60 s pair, and SSR_Eval_Helper(bss_sdr=True) with the bootstrap on a small wav tree.  (Guard
bands and poison on every device buffer of the call: tests/test_gpu_memory_discipline.py.)

The worst sdr difference seen on the GPU is 5.8e-10 dB."""
import numpy as np
import pytest
import torch

import bss_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("sdr", "sdr_lag")
TOL_DB = 1e-6
TILE = 16384


def check_rows(out, tgts, ests, idx, taps, what=""):
    """every row against the oracle: sdr within TOL_DB (NaN where it has NaN), sdr_lag equal -> the worst sdr difference"""
    worst = 0.0
    for e, (y, i) in enumerate(zip(ests, idx)):
        sdr, lag, _ = O.bss_sdr(tgts[i], y, taps)
        print(what, "pair", e, "n", len(y), "taps", taps, "got", out[e], "want", sdr, lag,
              "diff %.3g" % (0.0 if np.isnan(sdr) else abs(out[e][0] - sdr)))
        if np.isnan(sdr):
            assert np.isnan(out[e]).all(), (what, e, out[e])
            continue
        assert abs(out[e][0] - sdr) < TOL_DB, (what, e, out[e][0], sdr)
        assert out[e][1] == lag, (what, e, out[e][1], lag)
        worst = max(worst, abs(out[e][0] - sdr))
    return worst


@pytest.mark.parametrize("dt", [(np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64), (np.float64, np.float64)],
                         ids=["f32-f32", "f64-f32", "f32-f64", "f64-f64"])
def test_input_list_against_the_oracle(dt):
    """White, low-passed and brickwalled noise, a sine and a constant; 20 dB and 100 dB of noise and a delay of 37 samples at gain
    0.7: three estimates per target next to each other, 512 taps, through backend.bss_sdr (the C ABI's call shape)."""
    from ssr_eval_amd import backend as B
    names = list(O.targets())
    tg = [x.astype(dt[0]) for x in O.targets().values()]
    ests, idx = [], []
    for i, x in enumerate(tg):
        for y in O.estimates(x.astype(np.float64)).values():
            ests.append(y.astype(dt[1]))
            idx.append(i)
    out, filt = B.bss_sdr(tg, ests, idx, 512, return_filter=True)
    assert out.shape == (15, 2) and filt.shape == (15, 512)
    print("worst sdr difference", check_rows(out, tg, ests, idx, 512, "inputs"))
    assert [out[3 * i + 2, 1] for i, m in enumerate(names) if m != "sine"] == [37.0] * 4
    for e in range(3):                                                                         # the white target: condition about 2
        c = O.bss_sdr(tg[0], ests[e], 512)[2]
        assert np.max(np.abs(filt[e] - c)) <= 1e-10 * np.max(np.abs(c)), e
    assert B.bss_sdr(tg, ests, idx, 512).tobytes() == out.tobytes()                            # filt = NULL: the same bits


@pytest.mark.parametrize("L", [1, 2, 64, 511, 512])
def test_geometry_shapes(L):
    """n in {0, 1, 5, L - 1, L, L + 1, one tile - 1, one tile + 1, 4099} in one call, three estimates sharing the 4099 target in a
    run next to the singletons; a pair alone and at another position has the bits it has in the batch."""
    from ssr_eval_amd import backend as B
    rng = np.random.default_rng(100 + L)
    lens = [0, 1, 5, max(L - 1, 0), L, L + 1, TILE - 1, TILE + 1, 4099]
    tg = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    ests, idx = [], []
    for i, x in enumerate(tg):
        for k in range(3 if lens[i] == 4099 else 1):
            d = min(k + 1, len(x))
            ests.append(0.7 * np.concatenate([np.zeros(d), x[:len(x) - d].astype(np.float64)]) + 0.01 * (k + 1) * rng.standard_normal(len(x)))
            idx.append(i)
    out, filt = B.bss_sdr(tg, ests, idx, L, return_filter=True)
    check_rows(out, tg, ests, idx, L, "shapes")
    assert np.isnan(out[0]).all() and np.all(filt[0] == 0.0)
    for e in (2, 7, len(ests) - 2):
        alone, fa = B.bss_sdr([tg[idx[e]]], [ests[e]], [0], L, return_filter=True)
        assert alone.tobytes() == out[e:e + 1].tobytes() and fa.tobytes() == filt[e:e + 1].tobytes(), e
    order = list(range(len(ests)))[::-1]
    back = B.bss_sdr(tg, [ests[e] for e in order], [idx[e] for e in order], L)
    assert back[::-1].tobytes() == out.tobytes()


def test_ragged_batch_of_64_pairs():
    """64 pairs of 1 .. 3 tiles, float32 and float64 on either side, every fourth target carrying two estimates, 128 taps, through
    AudioMetrics.bss_sdr_batch (one call per dtype group); the same bits on a repeated call and from device tensors."""
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(48000)
    rng = np.random.default_rng(21)
    tgts, ests = [], []
    while len(ests) < 64:
        n = int(rng.integers(1, 3 * TILE + 1))
        x = (0.1 * rng.standard_normal(n)).astype(np.float64 if len(tgts) % 5 == 4 else np.float32)
        for _ in range(2 if len(ests) % 4 == 0 and len(ests) < 63 else 1):
            d = int(rng.integers(0, 100))
            y = 0.8 * np.concatenate([np.zeros(min(d, n)), x[:max(n - d, 0)]]) + 0.02 * rng.standard_normal(n)
            tgts.append(x)
            ests.append(y.astype(np.float64 if len(ests) % 3 == 2 else np.float32))
    assert len(ests) == 64 and max(len(e) for e in ests) > 2 * TILE
    got = am.bss_sdr_batch(ests, tgts, taps=128)
    assert [list(d) for d in got] == [list(NAMES)] * 64
    rows = [[d["sdr"], d["sdr_lag"]] for d in got]
    print("worst sdr difference", check_rows(rows, tgts, ests, list(range(64)), 128, "ragged"))
    assert am.bss_sdr_batch(ests, tgts, taps=128) == got
    dev = am.bss_sdr_batch([torch.from_numpy(e).to(DEV) for e in ests[:8]], [torch.from_numpy(t).to(DEV) for t in tgts[:8]], taps=128,
                           resident=True)
    assert dev == got[:8]
    for i in (0, 31, 63):
        assert am.bss_sdr(ests[i], tgts[i], taps=128) == got[i], i


def test_exact_facts():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(48000)
    rng = np.random.default_rng(7)
    x = (0.1 * rng.standard_normal(4099)).astype(np.float32)
    for y in (x, x.copy(), x.astype(np.float64)):                    # y == x: the EPS ceiling, lag 0, the filter a unit impulse
        d = am.bss_sdr(y, x, return_filter=True)
        sxx = float(np.sum(x.astype(np.float64) ** 2))
        assert abs(d["sdr"] - 10.0 * np.log10((sxx + O.EPS) / O.EPS)) < TOL_DB and d["sdr_lag"] == 0.0, d
        assert d["filter"].shape == (512,) and d["filter"][0] == 1.0 and np.all(d["filter"][1:] == 0.0)
    for L in (2, 64, 512):                                           # an exact FIR image of the target
        xf, yf, h = O.exact_fir_pair(L)
        d = am.bss_sdr(yf, xf, taps=L, return_filter=True)
        print("exact FIR", L, d["sdr"], d["sdr_lag"], np.max(np.abs(d["filter"] - h)))
        assert d["sdr"] >= 120.0, (L, d["sdr"])
        if L in (2, 64):
            assert np.max(np.abs(d["filter"] - h)) <= 1e-10, L
    # n = 0 and an all-zero target: NaN in both columns, the neighbours untouched
    tg = [x, np.zeros(0, np.float32), x[:700], np.zeros(900, np.float32), x[:300]]
    ests = [t + np.float32(0.01) for t in tg]
    got = am.bss_sdr_batch(ests, tg, taps=64, return_filter=True)
    for e in (1, 3):
        assert np.isnan(got[e]["sdr"]) and np.isnan(got[e]["sdr_lag"]) and np.all(got[e]["filter"] == 0.0)
    for e in (0, 2, 4):
        alone = am.bss_sdr(ests[e], tg[e], taps=64, return_filter=True)
        assert alone["sdr"] == got[e]["sdr"] and alone["sdr_lag"] == got[e]["sdr_lag"] and np.array_equal(alone["filter"], got[e]["filter"])
    check_rows([[d["sdr"], d["sdr_lag"]] for d in got], tg, ests, list(range(5)), 64, "nan neighbours")
    # nested tap counts on one pair: more taps never score lower
    xl = O.targets(n=6000)["lowpass"]
    yl = O.estimates(xl)["20dB"] + 0.3 * np.concatenate([np.zeros(11), xl[:-11]])
    prev = -np.inf
    for L in (1, 2, 8, 16, 64, 512):
        sdr = am.bss_sdr(yl, xl, taps=L)["sdr"]
        assert sdr >= prev - 1e-9, (L, sdr, prev)
        prev = sdr


def test_multi_is_three_batch_calls():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(16000)
    rng = np.random.default_rng(9)
    lens = (3000, 5000, 1777, TILE + 5)
    tgts = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    by_key = [[(t + 0.1 * (k + 1) * 0.1 * rng.standard_normal(len(t))).astype(np.float32) for t in tgts] for k in range(3)]
    multi = am.bss_sdr_multi(by_key, tgts, taps=64, return_filter=True)
    assert len(multi) == 4 and all(len(row) == 3 for row in multi)
    for k in range(3):
        single = am.bss_sdr_batch(by_key[k], tgts, taps=64, return_filter=True)
        for i in range(4):
            a, b = multi[i][k], single[i]
            assert list(a) == ["sdr", "sdr_lag", "filter"]
            assert np.array([a["sdr"], a["sdr_lag"]]).tobytes() == np.array([b["sdr"], b["sdr_lag"]]).tobytes(), (i, k)
            assert a["filter"].tobytes() == b["filter"].tobytes(), (i, k)
    deferred = am.bss_sdr_multi(by_key, tgts, taps=64, deferred=True)
    assert [[d["sdr"] for d in row] for row in deferred()] == [[d["sdr"] for d in row] for row in multi]


def test_a_minute_at_48_khz():
    """One 60 s pair: 176 tiles, the tile partials added in tile order; the estimate 240 samples late."""
    from ssr_eval_amd import AudioMetrics
    rng = np.random.default_rng(10)
    n = 60 * 48000
    x = (0.1 * rng.standard_normal(n)).astype(np.float32)
    y = (0.9 * np.concatenate([np.zeros(240, np.float32), x[:-240]]) + 0.01 * rng.standard_normal(n)).astype(np.float32)
    d = AudioMetrics(48000).bss_sdr(y, x)
    worst = check_rows([[d["sdr"], d["sdr_lag"]]], [x], [y], [0], 512, "minute")
    print("worst", worst)
    assert d["sdr_lag"] == 240.0


def test_evaluate_with_bss_sdr_and_bootstrap_from_wav_files(tmp_path, monkeypatch):
    """SSR_Eval_Helper(bss_sdr=True, bootstrap=200).evaluate() on a small wav tree (identity testee, two FFT keys, 44.1 kHz): every
    key carries sdr and sdr_lag of AudioMetrics.bss_sdr on the same estimate - and the oracle's within 1e-6 dB -, last in the metric
    order; the confidence block has the two columns and so has compare_results() of two such runs; the other metrics are those of a run without the option, bit for bit;
    bss_sdr=None is that run."""
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
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))),
                      (0.1 * rng.standard_normal(int(rng.integers(20000, 40000)))).astype(np.float32), fs)
    monkeypatch.chdir(tmp_path)

    def run(**kw):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=fs, output_sr=fs, evaluation_sr=fs, test_data_root=str(root),
                            setting_fft={"cutoff_freq": [4000, 11025]}, **kw)
        return h.evaluate(save_json=False)
    plain, off, res = run(), run(bss_sdr=None), run(bss_sdr=True, bootstrap=200, mrstft=True)
    assert off == plain and not any(m in NAMES for m in plain["averaged"]["proc_fft_8000_44100"])
    am = AudioMetrics(fs)
    keys = {"proc_fft_8000_44100": 4000, "proc_fft_22050_44100": 11025}
    n = 0
    for spk in counts:
        for fn in res[spk]:
            x = np.asarray(read_audio(str(root / spk / fn))[0], np.float32)
            for key, cut in keys.items():
                got = res[spk][fn][key]
                assert list(got)[-3:] == ["mrstft"] + list(NAMES)
                assert {m: got[m] for m in plain[spk][fn][key]} == plain[spk][fn][key]
                est = np.asarray(lowpass(x, cut, fs, order=1, _type="stft_hard"), np.float32)
                want, (sdr, lag, _) = am.bss_sdr(est, x), O.bss_sdr(x, est)
                print(fn, key, got["sdr"], got["sdr_lag"], want, sdr, lag)
                assert got["sdr"] == want["sdr"] and got["sdr_lag"] == want["sdr_lag"]
                assert abs(got["sdr"] - sdr) < TOL_DB and got["sdr_lag"] == lag
                n += 1
    assert n == 5 * 2
    for key in keys:
        assert list(res["averaged"][key])[-2:] == list(NAMES)
        conf = res["confidence"]["averaged"][key]
        assert list(conf) == list(res["averaged"][key])
        for m in NAMES:
            assert set(conf[m]) == {"se", "lo", "hi"} and conf[m]["lo"] <= conf[m]["hi"] and conf[m]["se"] >= 0
    # compare_results pairs the two columns like any other: against a run with 8 taps sdr differs (fewer taps never score higher),
    # sdr_lag and the rest do not
    res2 = run(bss_sdr={"taps": 8}, mrstft=True)
    cmp_ = compare_results(res, res2, n_boot=200, seed=1)
    assert sorted(cmp_) == sorted(keys)
    for key in keys:
        assert list(cmp_[key]) == list(res["averaged"][key]) and list(cmp_[key])[-2:] == list(NAMES)
        for m, v in cmp_[key].items():
            print(key, m, v)
            assert sorted(v) == ["diff", "hi", "lo", "p", "se"]
            assert abs(v["diff"] - (res["averaged"][key][m] - res2["averaged"][key][m])) <= 1e-12, (key, m)
            if m == "sdr":
                assert v["diff"] > 0 and v["se"] > 0 and 0 < v["lo"] <= v["hi"] and 0 < v["p"] <= 1, (key, v)
            else:
                assert v == {"diff": 0.0, "se": 0.0, "lo": 0.0, "hi": 0.0, "p": 1.0}, (key, m)
    sub = run(bss_sdr={"taps": 32}, waveform=("snr",))
    fn = next(iter(sub["p360"]))
    got = sub["p360"][fn]["proc_fft_8000_44100"]
    assert list(got)[-3:] == ["snr"] + list(NAMES)
    x = np.asarray(read_audio(str(root / "p360" / fn))[0], np.float32)
    est = np.asarray(lowpass(x, 4000, fs, order=1, _type="stft_hard"), np.float32)
    sdr, lag, _ = O.bss_sdr(x, est, 32)
    assert abs(got["sdr"] - sdr) < TOL_DB and got["sdr_lag"] == lag
