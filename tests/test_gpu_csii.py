"""GPU tests (-m gpu) of the coherence speech intelligibility index (ssr_csii): the geometry batch, the
transform sizes and the rates of tests/test_csii_host.py on the device, against the float64 oracle (tests/csii_oracle.py) with the
same bars - the CSII values within 1e-7, i3 within 3e-7, segment counts equal, under the same level-margin assertion - and the same
bit-for-bit properties; AudioMetrics.csii / _batch / _multi on host arrays and device tensors; every device buffer of ssr_csii
between guard bands, on poisoned inputs, and the one-byte-less workspace; SSR_Eval_Helper(csii=...) on a small wav tree."""
import numpy as np
import pytest
import torch

import coherence_oracle as CO
import csii_oracle as O
import guarded as G
from test_csii_host import DTYPES, DTYPE_IDS, GEOMETRY_SPLITS, _geometry_batch, split_bands

pytestmark = pytest.mark.gpu

DEV = "cuda"
FR = O.FR


def B():
    from ssr_eval_amd import backend
    return backend


def run(tgts, ests, idx, fs, n_fft, hop, band=None, splits=None, with_bands=True):
    """-> (out [n_est, 13], T [n_est, 4, n_bands] or None), as run_emu of the host file"""
    return B().csii_metrics(tgts, ests, idx, fs, n_fft, hop, band, split_bands(fs, n_fft, band, splits, len(ests)), return_bands=with_bands)


@pytest.mark.parametrize("dt", DTYPES, ids=DTYPE_IDS)
def test_geometry_shapes_and_bit_level_properties(dt):
    """The host file's ragged batch at N = 256, hop 64: K = 0, 1 (NaN), 2, 31, 32, 33 (three estimates of one target), 65.  A pair
    alone and at another position gives the bits it gives in the batch, a gain of 0.5 changes no bit, bands_out = NULL changes no
    bit of out, a repeated call repeats the bits."""
    fs, N, H, tg, ests, idx = _geometry_batch(dt)
    splits = GEOMETRY_SPLITS                                              # (two of them above the last centre: the empty _hf)
    out, T = run(tg, ests, idx, fs, N, H, splits=splits)
    worst = O.check_rows(out, tg, ests, idx, fs, N, H, None, splits, T, what="shapes")
    print("worst CSII %.3g, i3 %.3g, band value %.3g" % tuple(worst))
    assert np.isnan(out[:2, :9]).all() and out[:, 9].tolist() == [0, 1, 2, FR - 1, FR, FR + 1, FR + 1, FR + 1, 2 * FR + 1]
    assert np.isnan(out[[6, 8], 5:9]).all() and np.isfinite(out[[6, 8], 0]).all() and np.isfinite(out[[5, 7], 5]).all()
    none, _ = run(tg, ests, idx, fs, N, H)
    assert none[:, :5].tobytes() == out[:, :5].tobytes() and np.isnan(none[:, 5:9]).all()       # the split moves no bit of the others
    again, Ta = run(tg, ests, idx, fs, N, H, splits=splits)
    assert again.tobytes() == out.tobytes() and Ta.tobytes() == T.tobytes()
    for e in (2, 5, 6, len(ests) - 1):
        alone, T1 = run([tg[idx[e]]], [ests[e]], [0], fs, N, H, splits=[splits[e]])
        assert alone.tobytes() == out[e:e + 1].tobytes() and T1.tobytes() == T[e:e + 1].tobytes(), e
    order = list(range(len(ests)))[::-1]
    back, Tb = run(tg, [ests[e] for e in order], [idx[e] for e in order], fs, N, H, splits=[splits[e] for e in order])
    assert back[::-1].tobytes() == out.tobytes() and Tb[::-1].tobytes() == T.tobytes()
    half, Th = run(tg, [(0.5 * e.astype(np.float64)).astype(dt[1]) for e in ests], idx, fs, N, H, splits=splits)
    assert half.tobytes() == out.tobytes() and Th.tobytes() == T.tobytes()
    assert run(tg, ests, idx, fs, N, H, splits=splits, with_bands=False)[0].tobytes() == out.tobytes()


@pytest.mark.parametrize("fs,n_fft,hop,K", [(48000, 2048, 1024, 3), (44100, 1024, 341, FR + 1), (16000, 512, 512, 4), (16000, 256, 1, FR + 2),
                                            (8000, 512, 77, 2 * FR + 1)])
def test_other_transform_sizes_rates_and_hops(fs, n_fft, hop, K):
    n = CO.len_for_segments(K, n_fft, hop, min(3, hop - 1))
    x = O.speech_like(n, fs, 70 + n_fft // 256 + hop)
    tg = [x.astype(np.float32), x[:n_fft - 1].astype(np.float32)]
    ests = [O.noisy(x, 6.0, 3), O.distorted(x)[:n_fft - 1]]
    out, T = run(tg, ests, [0, 1], fs, n_fft, hop, splits=[1500.0, 1500.0])
    worst = O.check_rows(out, tg, ests, [0, 1], fs, n_fft, hop, None, [1500.0, 1500.0], T, what="sizes")
    print("worst CSII %.3g, i3 %.3g, band value %.3g" % tuple(worst))
    assert np.isnan(out[1, :9]).all() and np.isfinite(out[0, 0]) and out[:, 9].tolist() == [K, 0]


def test_exact_facts_silence_and_the_empty_batch():
    fs, N, H, n = 16000, 512, 256, 12000
    x = O.speech_like(n, fs, 90)
    xf, z = x.astype(np.float32), np.zeros(n, np.float32)
    out, T = run([xf], [xf, xf.astype(np.float32) * 0.5], [0, 0], fs, N, H, splits=[2000.0, 2000.0])
    assert np.all(out[:, 9:] >= 2) and np.all(out[:, :4] == 1.0) and np.all(out[:, 5:9] == 1.0) and np.all(T == 1.0), out
    out, T = run([z], [xf], [0], fs, N, H, splits=[2000.0])
    assert np.isnan(out[0, :9]).all() and np.isnan(T).all() and out[0, 9:].tolist() == [CO.segments(n, N, H), 0, 0, 0]
    out, T = run([xf], [z], [0], fs, N, H, splits=[2000.0])
    assert np.all(out[0, :4] == 0.0) and np.all(T == 0.0)
    x2, y = x.copy(), O.noisy(x, 8.0, 91)
    y2 = y.copy()
    x2[3000:3000 + 3 * N] = 0.0
    y2[7000:7000 + 2 * N + 17] = 0.0
    tg, es, idx = [x2, x], [y, y2, y], [0, 1, 1]
    out, T = run(tg, es, idx, fs, N, H, splits=[2000.0] * 3)
    O.check_rows(out, tg, es, idx, fs, N, H, None, [2000.0] * 3, T, what="silent stretches")
    noise = O.noisy(x, 0.0, 5)
    out, _ = run([x], [noise], [0], fs, 256, 128)
    O.check_rows(out, [x], [noise], [0], fs, 256, 128, what="white noise at 0 dB")
    assert 1.0 > out[0, 3] > out[0, 2] > out[0, 1] > 0.0
    out, T = run([x], [], [], fs, N, H)
    assert out.shape == (0, 13) and T.shape == (0, 4, 20)


def test_audio_metrics_single_batch_multi_and_resident_inputs():
    """AudioMetrics(16000): the dict of csii() is the oracle's; _batch and _multi give the bits of the single call, per-pair and
    per-key split frequencies included; device tensors give the bits of host arrays."""
    from ssr_eval_amd import AudioMetrics
    fs = 16000
    am = AudioMetrics(fs)
    xs = [O.speech_like(n, fs, 20 + i) for i, n in enumerate((9000, 12000, 10007))]
    tgts = [x.astype(np.float32) for x in xs]
    ests = [O.noisy(x, 4.0 + i, 30 + i).astype(np.float32 if i != 1 else np.float64) for i, x in enumerate(xs)]
    d = am.csii(ests[0], tgts[0], split_hz=3000, return_bands=True, return_counts=True)
    assert list(d) == ["csii", "csii_low", "csii_mid", "csii_high", "i3", "csii_hf", "csii_mid_hf", "band_values", "centre_hz", "n_segments",
                       "n_low", "n_mid", "n_high"]
    want, cnt, T = O.csii(tgts[0], ests[0], fs, split_hz=3000)
    assert O.level_margin(tgts[0], 256, 128) >= O.LEVEL_MARGIN
    for k, c in zip(list(d)[:7], (0, 1, 2, 3, 4, 5, 7)):
        assert abs(d[k] - want[c]) <= (O.TOL_I3 if k == "i3" else O.TOL), (k, d[k], want[c])
    assert [d["n_segments"], d["n_low"], d["n_mid"], d["n_high"]] == list(cnt) and np.max(np.abs(d["band_values"] - T)) <= O.TOL
    assert list(am.csii(ests[0], tgts[0], names=("i3", "csii"))) == ["csii", "i3"]
    bits = lambda q: np.array([v for k, v in q.items()]).tobytes()      # noqa: E731
    splits = [4000, None, 2500.5]
    batch = am.csii_batch(ests, tgts, split_hz=splits)
    for i in range(3):
        assert bits(am.csii(ests[i], tgts[i], split_hz=splits[i])) == bits(batch[i]), i
    assert np.isnan(batch[1]["csii_hf"]) and np.isfinite(batch[0]["csii_hf"])
    by_key = [ests, [e[::-1].copy() for e in ests]]
    multi = am.csii_multi(by_key, tgts, split_hz=[3000, None])
    for i in range(3):
        assert bits(multi[i][0]) == bits(am.csii(by_key[0][i], tgts[i], split_hz=3000)), i
        assert bits(multi[i][1]) == bits(am.csii(by_key[1][i], tgts[i])), i
    dev = am.csii_batch([torch.from_numpy(e).to(DEV) for e in ests], [torch.from_numpy(t).to(DEV) for t in tgts], split_hz=splits, resident=True)
    assert [bits(q) for q in dev] == [bits(q) for q in batch]


# ---- where the kernels touch memory ---------------------------------------------------------------------------------------------
def _csii_inputs(dtype):
    lens = [1, 255, 256, CO.len_for_segments(2, 256, 64), CO.len_for_segments(FR + 1, 256, 64, 7)]
    xs = [O.speech_like(n, 16000, 600 + i) + 1e-3 for i, n in enumerate(lens)]
    tgt = [x.astype(dtype) for x in xs]
    idx = list(range(len(lens))) + [len(lens) - 1]                        # two estimates of the last target
    est = [O.noisy(xs[i], 5.0, 610 + k).astype(dtype) for k, i in enumerate(idx)]
    return tgt, est, idx


@pytest.mark.parametrize("placement", ["odd", "quad"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("with_bands", [True, False], ids=["bands_out", "null"])
def test_guard_bands_and_poison(monkeypatch, dtype, placement, with_bands):
    """ssr_csii on separate device tensors, then on views into NaN-filled arenas with `out`, `bands_out` and the workspace between
    0xFF guard bands and 0xFF inside: the same bits, no guard damaged, no arena written, the signals read where they lie, and the
    `all` column finite where K >= 2 (a read outside an item or of an unwritten workspace byte would be NaN)."""
    bk = B()
    gaps = {"odd": G.GAPS_ODD, "quad": G.GAPS_QUAD}[placement]
    tgt, est, idx = _csii_inputs(dtype)

    def call(put):
        return bk.csii_metrics(put(tgt), put(est), idx, 16000, 256, 64, None, [10] * len(est), return_bands=with_bands)
    plain = G.bits([a for a in call(lambda arrays: [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]) if a is not None])
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        got = call(lambda arrays: g.arena(arrays, gaps, torch.from_numpy(np.asarray(arrays[0])).dtype, DEV)[0])
        assert len(g.blocks) >= (3 if with_bands else 2)                   # out, bands_out and the workspace
        assert g.arenas and g.read_in_place()
        g.check()
        got = G.bits([a for a in got if a is not None])
    G.assert_same_bits(plain, got, "csii")
    rows = np.frombuffer(got[0][2], np.float64).reshape(got[0][0])
    assert np.isnan(rows[:3, :9]).all() and np.isfinite(rows[3:, 0]).all() and np.isfinite(rows[:, 9:]).all(), rows
    assert np.isfinite(rows[4:, :9]).all(), rows


def test_one_byte_less_than_reported_is_refused(monkeypatch):
    """With ssr_csii_workspace_bytes reporting one byte less than it should the call is SSR_ERR_WORKSPACE and nothing is enqueued:
    `out`, `bands_out` and the workspace still hold only 0xFF."""
    bk = B()
    lib = bk._lib.load()
    real = lib.ssr_csii_workspace_bytes
    asked = []

    def one_less(*a):
        n = int(real(*a))
        assert n > 0
        asked.append(n)
        return n - 1
    tgt, est, idx = _csii_inputs(np.float32)
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        m.setattr(lib, "ssr_csii_workspace_bytes", one_less)
        with pytest.raises(bk.SsrHipError, match=r"libssrhip error -4\b"):
            bk.csii_metrics(g.arena(tgt, G.GAPS_ODD, torch.float32, DEV)[0], g.arena(est, G.GAPS_ODD, torch.float32, DEV)[0], idx, 16000, 256,
                            64, return_bands=True)
        assert asked
        g.check()
        assert g.untouched_payloads(("backend.py:put", "backend.py:_uniform_images")) == []


# ---- SSR_Eval_Helper(csii=...) ----------------------------------------------------------------------------------------------------
FS = 16000
LENGTHS = {"p360": (8000, 8411), "p361": (9001, 9600), "p362": (8200, 9100), "p363": (8800, 9300)}
KEYS = ("csii", "csii_mid", "i3", "csii_hf")


def _bits(v):
    return np.float64(v).tobytes()                                        # NaN equals NaN


def _write_tree(root):
    """Four speakers x two files of the synthetic voiced signal."""
    from ssr_eval_amd.io import write_wav
    for s, (spk, lens) in enumerate(LENGTHS.items()):
        (root / spk).mkdir(parents=True)
        for i, n in enumerate(lens):
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), O.speech_like(n, FS, 700 + 10 * s + i).astype(np.float32), FS)


def test_evaluate_with_csii_on_the_eight_file_tree(tmp_path):
    """evaluate() on the eight-file 16 kHz tree with two FFT keys: the four keys sit behind full_key_order()'s; the values are
    AudioMetrics.csii_multi's on the same arrays; with the option off the result is what it is without the keyword."""
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee, AudioMetrics
    from ssr_eval_amd.eval import every_key_order, full_key_order
    from ssr_eval_amd.io import read_audio
    from ssr_eval_amd.lowpass import lowpass
    root = tmp_path / "vctk_test"
    _write_tree(root)
    cutoffs = [2000, 3000]

    def go(**kw):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=FS, output_sr=FS, evaluation_sr=FS, test_data_root=str(root),
                            setting_fft={"cutoff_freq": list(cutoffs)}, **kw)
        return h.evaluate(save_json=False)
    none, off, on, both = go(), go(csii=None), go(csii=True), go(csii=True, auditory=True, loudness=True)
    assert off == none
    keys = ["proc_fft_%d_%d" % (2 * c, FS) for c in cutoffs]
    order = every_key_order()
    assert order[:len(full_key_order())] == full_key_order() and order[-4:] == KEYS
    am = AudioMetrics(FS)
    seen = 0
    for spk in LENGTHS:
        for fn, by_key in on[spk].items():
            assert list(by_key) == keys
            x = np.asarray(read_audio(str(root / spk / fn))[0], np.float32)
            ests = [np.asarray(lowpass(x, cut, FS, order=1, _type="stft_hard"), np.float32) for cut in cutoffs]
            want = am.csii_multi([[e] for e in ests], [x], split_hz=[float(c) for c in cutoffs], names=KEYS)[0]
            for k, (key, cut) in enumerate(zip(keys, cutoffs)):
                d, b = by_key[key], both[spk][fn][key]
                assert list(d) == list(order[:4]) + list(KEYS), (spk, fn, key, list(d))
                assert list(b) == [m for m in order if m in b] and list(b)[-4:] == list(KEYS) and list(b)[-6:-4] == ["nsim", "nsim_hf"]
                assert [_bits(d[m]) for m in KEYS] == [_bits(want[k][m]) for m in KEYS] == [_bits(b[m]) for m in KEYS], (spk, fn, key, d, want[k])
                assert [_bits(d[m]) for m in order[:4]] == [_bits(none[spk][fn][key][m]) for m in order[:4]]
                assert all(np.isfinite(d[m]) for m in KEYS) and 0.0 <= d["csii_hf"] < d["csii"] <= 1.0, (spk, fn, key, d)
                seen += 1
    assert seen == 8 * len(cutoffs)
    for key in keys:
        assert list(on["averaged"][key]) == list(order[:4]) + list(KEYS)
