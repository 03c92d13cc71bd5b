"""GPU tests (-m gpu) of the magnitude-squared coherence family (ssr_coherence): the input list and the geometry
cases of tests/test_coherence_host.py on the device, against the float64 oracle (tests/coherence_oracle.py) with the same tolerances
- msc and the per-bin coherence within 1e-9, coh_sdr within 1e-6 dB, coh_bins equal, under the same conditioning assertions - and
the same bit-for-bit properties; AudioMetrics.coherence / _batch / _multi; every device buffer of ssr_coherence between guard
bands, on poisoned inputs, and the one-byte-less workspace; SSR_Eval_Helper(coherence=...) on a small wav tree."""
import numpy as np
import pytest
import torch

import coherence_oracle as O
import guarded as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
FR = O.FR
DTYPES = [(np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64), (np.float64, np.float64)]
DTYPE_IDS = ["f32-f32", "f64-f32", "f32-f64", "f64-f64"]


def B():
    from ssr_eval_amd import backend
    return backend


def run(tgts, ests, idx, n_fft, hop, bands, thr=0.5, spectrum=True):
    """-> (out [n_est, n_bands, 3], g2 [n_est, n_fft / 2 + 1] or None), as run_emu of the host file"""
    got = B().coherence_metrics(tgts, ests, idx, n_fft, hop, O.band_table(bands, len(ests)), thr, return_spectrum=spectrum)
    return got if spectrum else (got, None)


@pytest.mark.parametrize("case", range(len(O.CASES)))
def test_input_list_against_the_oracle(case):
    n, N, H = O.CASES[case]
    x, y = O.input_pair(n, 100 + case)
    bands = O.input_bands(N)
    margin, rx, ry = O.conditioning(x, y, N, H)
    assert margin >= O.THR_MARGIN and rx >= O.R_MIN and ry >= O.R_MIN
    for dt in (np.float64, np.float32):
        tg, es = [x.astype(dt)], [y.astype(dt)]
        out, g2 = run(tg, es, [0], N, H, bands)
        worst = O.check_rows(out, g2, tg, es, [0], N, H, bands, what="inputs")
        print("n %d N %d H %d %s: worst msc %.3g, per bin %.3g, coh_sdr %.3g dB" % ((n, N, H, np.dtype(dt).name) + tuple(worst)))
        assert 3.0 < out[0, 0, 1] < 6.0 and -14.0 < out[0, 2, 1] < -5.0 and out[0, 1, 1] > 12.0
        assert out[0, 1, 0] > 0.9 and out[0, 2, 0] < 0.3


@pytest.mark.parametrize("dt", DTYPES, ids=DTYPE_IDS)
def test_geometry_shapes_and_bit_level_properties(dt):
    """The host file's batch at N = 256, hop 64: K = 0 and K = 1 (NaN), K = 2, the chunk length, the chunk length plus one, three
    chunks; three estimates sharing one target in a run, then one with its own; the input bands, the empty band, bin 0 alone and
    bin N / 2 alone.  A pair alone and at another position gives the bits it gives in the batch, a band's row does not depend on
    the other bands, msc_out = NULL changes no bit of out, a repeated call repeats the bits."""
    N, H = 256, 64
    lens = [255, 256, O.len_for_segments(2, N, H), O.len_for_segments(FR, N, H, 5), O.len_for_segments(FR + 1, N, H),
            O.len_for_segments(2 * FR + 1, N, H, 63)]
    pairs = [O.input_pair(n, 200 + i) for i, n in enumerate(lens)]
    tg = [x.astype(dt[0]) for x, _ in pairs]
    ests, idx = [], []
    for i, (x, y) in enumerate(pairs):
        for k in range(3 if i == 4 else 1):
            ests.append((y + 0.1 * k * np.random.default_rng(300 + k).standard_normal(len(y))).astype(dt[1]))
            idx.append(i)
    bands = O.input_bands(N) + [(5, 4), (0, 0), (N // 2, N // 2)]
    out, g2 = run(tg, ests, idx, N, H, bands)
    worst = O.check_rows(out, g2, tg, ests, idx, N, H, bands, what="shapes")
    print("worst msc %.3g, per bin %.3g, coh_sdr %.3g dB" % tuple(worst))
    assert np.isnan(out[:2]).all() and np.isnan(g2[:2]).all() and np.isfinite(out[2:, [0, 1, 2, 3, 5, 6]]).all()
    assert np.isnan(out[:, 4]).all()
    assert out[3, 5, 0] == g2[3, 0] and out[3, 6, 0] == g2[3, N // 2]
    again, ga = run(tg, ests, idx, N, H, bands)
    assert again.tobytes() == out.tobytes() and ga.tobytes() == g2.tobytes()
    for e in (2, 3, 5, len(ests) - 1):
        alone, g1 = run([tg[idx[e]]], [ests[e]], [0], N, H, bands)
        assert alone.tobytes() == out[e:e + 1].tobytes() and g1.tobytes() == g2[e:e + 1].tobytes(), e
    order = list(range(len(ests)))[::-1]
    back, gb = run(tg, [ests[e] for e in order], [idx[e] for e in order], N, H, bands)
    assert back[::-1].tobytes() == out.tobytes() and gb[::-1].tobytes() == g2.tobytes()
    for b in (0, 2, 3, 6):
        sub, _ = run(tg, ests, idx, N, H, [bands[b]])
        assert sub[:, 0].tobytes() == np.ascontiguousarray(out[:, b]).tobytes(), b
    swapped, _ = run(tg, ests, idx, N, H, bands[::-1])
    assert np.ascontiguousarray(swapped[:, ::-1]).tobytes() == out.tobytes()
    assert run(tg, ests, idx, N, H, bands, spectrum=False)[0].tobytes() == out.tobytes()
    per_est = [[(0, N // 2), (10 + 7 * e, N // 2)] for e in range(len(ests))]
    po, _ = run(tg, ests, idx, N, H, per_est)
    O.check_rows(po, None, tg, ests, idx, N, H, per_est, what="per-estimate bands")
    assert np.ascontiguousarray(po[:, 0]).tobytes() == np.ascontiguousarray(out[:, 0]).tobytes()


@pytest.mark.parametrize("n_fft,hop,K", [(2048, 1024, 3), (1024, 341, FR + 1), (512, 512, 4), (256, 1, FR), (2048, 2048, 2)])
def test_other_transform_sizes(n_fft, hop, K):
    n = O.len_for_segments(K, n_fft, hop, min(3, hop - 1))
    x, y = O.input_pair(n, 400 + n_fft + hop)
    tg = [x.astype(np.float32), x[:n_fft - 1].astype(np.float32)]
    ests = [y, y[:n_fft - 1]]
    bands = O.input_bands(n_fft) + [(n_fft // 2, n_fft // 2)]
    out, g2 = run(tg, ests, [0, 1], n_fft, hop, bands, thr=0.25)
    worst = O.check_rows(out, g2, tg, ests, [0, 1], n_fft, hop, bands, thr=0.25, what="sizes")
    print("worst msc %.3g, per bin %.3g, coh_sdr %.3g dB" % tuple(worst))
    assert np.isnan(out[1]).all() and np.isfinite(out[0]).all()


def test_exact_facts_and_the_empty_batch():
    N, H, n = 512, 128, 6000
    x, y = O.input_pair(n, 7)
    xf = x.astype(np.float32)
    bands = [(0, N // 2), (40, 200), (N // 2, N // 2)]
    for same in (xf, xf.astype(np.float64)):
        out, g2 = run([xf], [same], [0], N, H, bands)
        print("y == x", out[0])
        assert (out[0, :, 0] >= 1 - 1e-12).all() and (out[0, :, 1] >= 120.0).all() and out[0, :, 2].tolist() == [257.0, 161.0, 1.0]
    z = np.zeros(n, np.float32)
    for tg, es in (([xf], [z]), ([z], [xf]), ([z], [z])):
        out, g2 = run(tg, es, [0], N, H, bands)
        assert np.all(out[0, :, 0] == 0.0) and np.all(out[0, :, 2] == 0.0) and np.all(g2 == 0.0), out
    x2, y2, y3 = x.copy(), y.copy(), y.copy()
    x2[700:700 + 3 * N] = 0.0
    y2[700:700 + 3 * N] = 0.0
    y3[2500:2500 + 2 * N + 17] = 0.0
    tg, es, idx = [x2, x], [y2, y3, y2], [0, 1, 1]
    out, g2 = run(tg, es, idx, N, H, bands)
    O.check_rows(out, g2, tg, es, idx, N, H, bands, what="silent stretches")
    ref = O.gamma2(x, y, N, H)[0]
    for thr in (0.05, 0.95, 1.0):
        assert np.min(np.abs(ref - thr)) > 1e-6 and run([x], [y], [0], N, H, [(0, N // 2)], thr=thr)[0][0, 0, 2] == np.sum(ref >= thr), thr
    out, g2 = run([x], [], [], N, H, np.zeros((0, 1, 2), np.int32))
    assert out.shape == (0, 1, 3) and g2.shape == (0, N // 2 + 1)


def test_audio_metrics_single_batch_multi_and_resident_inputs():
    """AudioMetrics(16000): the dict of coherence() is the oracle's on the band's bins; _batch and _multi give the bits of the single
    call, per-pair and per-key split frequencies included; device tensors give the bits of host arrays."""
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(16000)
    pairs = [O.input_pair(n, 500 + i) for i, n in enumerate((3000, 5000, 4099))]
    tgts = [x.astype(np.float32) for x, _ in pairs]
    ests = [y.astype(np.float32 if i != 1 else np.float64) for i, (_, y) in enumerate(pairs)]
    N, H = 512, 256
    d = am.coherence(ests[0], tgts[0], n_fft=N, band=(500, 7000), split_hz=4000, threshold=0.4, return_spectrum=True)
    assert list(d) == ["msc", "coh_sdr", "coh_bw", "msc_hf", "coh_sdr_hf", "msc_spectrum"]
    lo, hi = am._phase_bins(16000, N, (500, 7000))
    want, wg = O.coherence(tgts[0], ests[0], N, H, [(lo, hi), (128, hi)], 0.4)
    assert (lo, hi) == (16, 224) and abs(d["msc"] - want[0, 0]) <= O.TOL and abs(d["coh_sdr"] - want[0, 1]) <= O.TOL_DB
    assert d["coh_bw"] == want[0, 2] * 16000 / N and abs(d["msc_hf"] - want[1, 0]) <= O.TOL and abs(d["coh_sdr_hf"] - want[1, 1]) <= O.TOL_DB
    assert d["msc_hf"] < d["msc"] and np.max(np.abs(d["msc_spectrum"] - wg)) <= O.TOL
    assert list(am.coherence(ests[0], tgts[0])) == ["msc", "coh_sdr", "coh_bw"]
    bits = lambda q: np.array([v for k, v in q.items() if k != "msc_spectrum"]).tobytes()      # noqa: E731
    splits = [4000, None, 2500.5]
    batch = am.coherence_batch(ests, tgts, n_fft=N, split_hz=splits)
    for i in range(3):
        one = am.coherence(ests[i], tgts[i], n_fft=N, split_hz=splits[i])
        if splits[i] is None:
            assert np.isnan(batch[i]["msc_hf"]) and np.isnan(batch[i]["coh_sdr_hf"]) and bits(one) == bits({k: batch[i][k] for k in one})
        else:
            assert bits(one) == bits(batch[i]), i
    by_key = [ests, [e[::-1].copy() for e in ests]]
    multi = am.coherence_multi(by_key, tgts, n_fft=N, split_hz=[3000, None])
    for i in range(3):
        assert bits(multi[i][0]) == bits(am.coherence(by_key[0][i], tgts[i], n_fft=N, split_hz=3000)), i
        assert np.isnan(multi[i][1]["msc_hf"]) and multi[i][1]["msc"] == am.coherence(by_key[1][i], tgts[i], n_fft=N)["msc"], i
    dev = am.coherence_batch([torch.from_numpy(e).to(DEV) for e in ests], [torch.from_numpy(t).to(DEV) for t in tgts], n_fft=N,
                             split_hz=splits, resident=True)
    assert [bits(q) for q in dev] == [bits(q) for q in batch]


# ---- where the kernels touch memory ---------------------------------------------------------------------------------------------
def _coh_inputs(dtype):
    lens = [1, 255, 256, O.len_for_segments(2, 256, 64), O.len_for_segments(FR + 1, 256, 64, 7)]
    pairs = [O.input_pair(n, 600 + i) for i, n in enumerate(lens)]
    tgt = [x.astype(dtype) for x, _ in pairs]
    idx = list(range(len(lens))) + [len(lens) - 1]                        # two estimates of the last target
    est = [pairs[i][1].astype(dtype) for i in idx]
    return tgt, est, idx


@pytest.mark.parametrize("placement", ["odd", "quad"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("with_spectrum", [True, False], ids=["msc_out", "null"])
def test_guard_bands_and_poison(monkeypatch, dtype, placement, with_spectrum):
    """ssr_coherence on separate device tensors, then on views into NaN-filled arenas with `out`, `msc_out` and the workspace between
    0xFF guard bands and 0xFF inside: the same bits, no guard damaged, no arena written, the signals read where they lie, and
    everything finite where K >= 2 (a read outside an item or of an unwritten workspace byte would be NaN)."""
    bk = B()
    gaps = {"odd": G.GAPS_ODD, "quad": G.GAPS_QUAD}[placement]
    tgt, est, idx = _coh_inputs(dtype)
    bands = [(0, 128), (64, 128), (128, 128)]

    def call(put):
        return bk.coherence_metrics(put(tgt), put(est), idx, 256, 64, bands, return_spectrum=with_spectrum)
    plain = G.bits(call(lambda arrays: [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]))
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        got = call(lambda arrays: g.arena(arrays, gaps, torch.from_numpy(np.asarray(arrays[0])).dtype, DEV)[0])
        assert len(g.blocks) >= (3 if with_spectrum else 2)                # out, msc_out and the workspace
        assert g.arenas and g.read_in_place()
        g.check()
        got = G.bits(got)
    G.assert_same_bits(plain, got, "coherence")
    arrays = [np.frombuffer(b, np.dtype(d)).reshape(s) for s, d, b in got]
    for a in arrays:
        assert np.isnan(a[:3]).all() and np.isfinite(a[3:]).all(), a


def test_one_byte_less_than_reported_is_refused(monkeypatch):
    """With ssr_coherence_workspace_bytes reporting one byte less than it should the call is SSR_ERR_WORKSPACE and nothing is
    enqueued: `out`, `msc_out` and the workspace still hold only 0xFF."""
    bk = B()
    lib = bk._lib.load()
    real = lib.ssr_coherence_workspace_bytes
    asked = []

    def one_less(*a):
        n = int(real(*a))
        assert n > 0
        asked.append(n)
        return n - 1
    tgt, est, idx = _coh_inputs(np.float32)
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        m.setattr(lib, "ssr_coherence_workspace_bytes", one_less)
        with pytest.raises(bk.SsrHipError, match=r"libssrhip error -4\b"):
            bk.coherence_metrics(g.arena(tgt, G.GAPS_ODD, torch.float32, DEV)[0], g.arena(est, G.GAPS_ODD, torch.float32, DEV)[0], idx, 256,
                                 64, [(0, 128)], return_spectrum=True)
        assert asked
        g.check()
        assert g.untouched_payloads(("backend.py:put", "backend.py:_uniform_images")) == []


# ---- SSR_Eval_Helper(coherence=...) ----------------------------------------------------------------------------------------------
FS = 16000
LENGTHS = {"p360": (8000, 8411), "p361": (9001, 9600)}
OTHERS = dict(lsd_split=True, stoi="both", waveform=True, mel=True, mel_dtw=True, quality=True, pitch=True, phase=True, mrstft=True,
              bss_sdr=True)
COH = ("msc", "coh_sdr", "coh_bw", "msc_hf", "coh_sdr_hf")


def _bits(v):
    return np.float64(v).tobytes()                                        # NaN equals NaN


def _write_tree(root):
    """Two speakers x two files: a 220 Hz tone with two harmonics plus noise (the tree of tests/test_gpu_all_families.py)."""
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(12)
    for spk, lens in LENGTHS.items():
        (root / spk).mkdir(parents=True)
        for i, n in enumerate(lens):
            t = np.arange(n) / FS
            x = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.1 * np.sin(2 * np.pi * 440 * t) + 0.05 * np.sin(2 * np.pi * 1760 * t)
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), (x + 0.02 * rng.standard_normal(n)).astype(np.float32), FS)


@pytest.mark.parametrize("cutoffs", [[2000, 3000], [2000]], ids=["K2-multi", "K1-batch"])
def test_evaluate_with_coherence_alone_and_with_every_other_option(tmp_path, cutoffs):
    """evaluate() on the four-file 16 kHz tree through the multi path (K = 2) and the flat path (K = 1): the five keys are bit-equal
    with `coherence=True` alone and with the ten other options on; the other 33 values are bit-equal to a run without the option;
    keys are listed in all_key_order(); the identity testee returns the low-passed input, so the coherence above the key's cutoff
    is below the band's; a fixed `split` moves the two _hf values only."""
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee, AudioMetrics
    from ssr_eval_amd.eval import all_key_order, result_key_order
    from ssr_eval_amd.io import read_audio
    from ssr_eval_amd.lowpass import lowpass
    root = tmp_path / "vctk_test"
    _write_tree(root)

    def go(**kw):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=FS, output_sr=FS, evaluation_sr=FS, test_data_root=str(root),
                            setting_fft={"cutoff_freq": list(cutoffs)}, **kw)
        return h.evaluate(save_json=False)
    alone, everything, others, none = go(coherence=True), go(coherence=True, **OTHERS), go(**OTHERS), go()
    fixed = go(coherence={"split": 1000, "n_fft": 1024})
    assert go(coherence=None) == none
    keys = ["proc_fft_%d_%d" % (2 * c, FS) for c in cutoffs]
    order = all_key_order()
    assert order[:33] == result_key_order() and order[33:] == COH
    am = AudioMetrics(FS)
    seen = 0
    for spk in LENGTHS:
        for fn, by_key in everything[spk].items():
            assert list(by_key) == keys
            x, _ = read_audio(str(root / spk / fn))
            for key, cut in zip(keys, cutoffs):
                d, a, o = by_key[key], alone[spk][fn][key], others[spk][fn][key]
                assert list(d) == list(order) and len(d) == 38, (spk, fn, key, list(d))
                assert list(a) == list(order[:4]) + list(COH) and list(o) == list(order[:33])
                assert list(none[spk][fn][key]) == list(order[:4])
                for m in COH:
                    print(spk, fn, key, m, d[m])
                    assert _bits(d[m]) == _bits(a[m]), (spk, fn, key, m, d[m], a[m])
                for m in order[:33]:
                    assert _bits(d[m]) == _bits(o[m]), (spk, fn, key, m, d[m], o[m])
                for m in order[:4]:
                    assert _bits(a[m]) == _bits(none[spk][fn][key][m]), (spk, fn, key, m)
                assert all(np.isfinite(d[m]) for m in COH) and 0.0 <= d["msc_hf"] < d["msc"] <= 1.0, (spk, fn, key, d)
                est = np.asarray(lowpass(x, cut, FS, order=1, _type="stft_hard"), np.float32)
                want = am.coherence(est, np.asarray(x, np.float32), split_hz=cut)
                assert [_bits(d[m]) for m in COH] == [_bits(want[m]) for m in COH], (spk, fn, key, d, want)
                f = fixed[spk][fn][key]
                assert [_bits(f[m]) for m in COH[:3]] == [_bits(d[m]) for m in COH[:3]]
                assert _bits(f["msc_hf"]) == _bits(am.coherence(est, np.asarray(x, np.float32), split_hz=1000)["msc_hf"])
                seen += 1
    assert seen == 4 * len(cutoffs)
    for key in keys:
        assert list(everything["averaged"][key]) == list(order)
        for spk in LENGTHS:
            assert list(everything["each_speaker"][spk][key]) == list(order)
