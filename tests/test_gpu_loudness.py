"""GPU tests (-m gpu) of the loudness family (ssr_loudness): the input list and the geometry cases of
tests/test_loudness_host.py on the device, against the float64 oracle (tests/loudness_oracle.py) with the same bars - E[s] within
1e-10 of the signal's largest sub-block energy, the four loudness values within 1e-6 LU, true_peak_db within 1e-9 dB, peak_db
within 1e-12 dB, under the same conditioning assertions - and the same bit-for-bit properties; AudioMetrics.loudness / _batch /
_multi; every device buffer of ssr_loudness between guard bands, on poisoned inputs, and the one-byte-less workspace;
SSR_Eval_Helper(loudness=True) on a small wav tree.
Worst differences seen on an MI355X: see DESIGN.md section 21."""
import numpy as np
import pytest
import torch

import guarded as G
import loudness_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"


def B():
    from ssr_eval_amd import backend
    return backend


def run(sigs, fs, blocks=True):
    """-> (out [n, 6], [E of each signal] or None), as run_emu of the host file"""
    got = B().loudness_metrics(sigs, fs, return_blocks=blocks)
    return got if blocks else (got, None)


@pytest.mark.parametrize("fs", O.RATES)
def test_input_list_against_the_oracle(fs):
    names = ("levels", "silence", "sine")
    x = {"levels": O.piecewise_noise(fs), "silence": O.noise_with_silence(fs), "sine": O.quarter_rate_sine(fs)}
    c = O.conditioning(x["levels"], fs)
    assert c[0] >= 1 and c[1] >= 1 and c[4] >= O.GATE_MARGIN and c[5] >= O.RANK_MARGIN, c
    O.assert_conditioned(x["silence"], fs, "silence")
    for dt in (np.float64, np.float32):
        sigs = [x[k].astype(dt) for k in names]
        out, E = run(sigs, fs)
        for k, s, o, e in zip(names, sigs, out, E):
            worst = O.check(o, e, s, fs, k)
            print(fs, k, np.dtype(dt).name, "worst E %.3g, loudness %.3g LU, true peak %.3g dB, peak %.3g dB" % worst)
    assert abs(out[2, 4] + 3.0103) < 1e-3 and abs(out[2, 5]) < 0.2


@pytest.mark.parametrize("fs,dt", [(44100, np.float32), (44100, np.float64), (8000, np.float32), (48000, np.float64)],
                         ids=["44k1-f32", "44k1-f64", "8k-f32", "48k-f64"])
def test_geometry_shapes_and_bit_level_properties(fs, dt):
    """The host file's batch (S = 0, 3, 4, 5, 29, 30, 31, n no multiple of h, n = 0, 1, 80, all-zero signals, a zero stretch) against
    the oracle; a signal alone and at another position gives the bits it gives in the batch, blocks_out = NULL changes no bit of
    out, a repeated call repeats the bits."""
    sigs = O.geometry_signals(fs, dt)
    out, E = run(sigs, fs)
    for i, s in enumerate(sigs):
        worst = O.check(out[i], E[i], s, fs, "signal %d (n = %d)" % (i, len(s)))
    print("last signal: worst E %.3g, loudness %.3g LU, true peak %.3g dB, peak %.3g dB" % worst)
    assert np.isnan(out[[0, 1], :4]).all() and np.isnan(out[7]).all() and np.isnan(out[10]).all() and np.isnan(out[11]).all()
    assert np.isfinite(out[2, [0, 2, 4, 5]]).all() and np.isnan(out[[2, 3, 4]][:, [1, 3]]).all() and np.isfinite(out[[5, 6, 12]]).all()
    again, Ea = run(sigs, fs)
    assert again.tobytes() == out.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(Ea, E))
    for i in (2, 6, 9, 12):
        alone, E1 = run([sigs[i]], fs)
        assert alone.tobytes() == out[i:i + 1].tobytes() and E1[0].tobytes() == E[i].tobytes(), i
    back, Eb = run(sigs[::-1], fs)
    assert back[::-1].tobytes() == out.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(Eb[::-1], E))
    assert run(sigs, fs, blocks=False)[0].tobytes() == out.tobytes()


def test_exact_facts_ten_minutes_and_the_empty_batch():
    """Scaling by a power of two: the bar of the host file (four roundings of values below 128).  All-zero input: NaN everywhere.
    6000 sub-blocks (10 minutes at 8 kHz) against the oracle; 6145 are refused; an empty batch is an empty result."""
    fs = 22050
    x = O.piecewise_noise(fs) * 0.5
    bar = 4 * np.spacing(128.0)
    base, Eb = run([x], fs)
    for k in (-3, 1, 4):
        got, E = run([x * 2.0 ** k], fs)
        shift = 20.0 * np.log10(2.0) * k
        d = got[0] - base[0] - np.array([shift, 0.0, shift, shift, shift, shift])
        print(k, d)
        assert np.max(np.abs(d)) <= bar and np.array_equal(E[0], Eb[0] * 4.0 ** k)
    z, Ez = run([np.zeros(3 * fs + 5, np.float32)], fs)
    assert np.isnan(z).all() and not np.any(Ez[0]) and len(Ez[0]) == 30
    rng = np.random.default_rng(3)
    long = (0.05 * rng.standard_normal(800 * 6000 + 17)).astype(np.float32)
    long[800 * 2000:800 * 2500] *= 0.01
    got, E = run([long], 8000)
    print("10 minutes at 8 kHz: worst", O.check(got[0], E[0], long, 8000, "10 minutes"))
    with pytest.raises(ValueError):
        run([np.zeros(800 * 6145, np.float32)], 8000)
    out, E = run([], fs)
    assert out.shape == (0, 6) and E == []


def test_audio_metrics_single_batch_multi_and_resident_inputs(monkeypatch):
    """AudioMetrics(16000): loudness() is the oracle's row; float32 and float64 signals mixed in one list give the bits of the single
    calls; lufs_diff of y == x is exactly 0; a target shared by several estimates is measured once; device tensors give the bits
    of host arrays."""
    from ssr_eval_amd import AudioMetrics
    fs = 16000
    am = AudioMetrics(fs)
    rng = np.random.default_rng(21)
    tgts = [(0.1 * rng.standard_normal(n)).astype(dt) for n, dt in ((52000, np.float32), (49001, np.float64), (7000, np.float32))]
    ests = [(0.5 * t + 0.01 * rng.standard_normal(len(t))).astype(dt) for t, dt in zip(tgts, (np.float64, np.float32, np.float32))]
    d = am.loudness(ests[0], tgts[0], return_blocks=True)
    assert list(d) == list(O.NAMES) + ["lufs_diff", "lra_diff", "true_peak_diff", "blocks", "target_blocks"]
    O.check([d[k] for k in O.NAMES], d["blocks"], ests[0], fs, "estimate")
    t = am.loudness(tgts[0], return_blocks=True)
    assert list(t) == list(O.NAMES) + ["blocks"] and t["blocks"].tobytes() == d["target_blocks"].tobytes()
    O.check([t[k] for k in O.NAMES], t["blocks"], tgts[0], fs, "target")
    assert d["lufs_diff"] == d["lufs"] - t["lufs"] and d["lra_diff"] == d["lra"] - t["lra"] and d["true_peak_diff"] == d["true_peak_db"] - t["true_peak_db"]
    # half the target plus white noise of a tenth of its level: 10 log10(0.25 + 0.01) = -5.85 LU (both are white: the weighting cancels)
    assert abs(d["lufs_diff"] + 5.85) < 0.05
    same = am.loudness(tgts[0], tgts[0].copy())
    assert same["lufs_diff"] == 0.0 and same["lra_diff"] == 0.0 and same["true_peak_diff"] == 0.0
    short = am.loudness(ests[2], tgts[2])                                             # 0.44 s: S = 4, no short-term block
    assert np.isfinite(short["lufs"]) and np.isnan(short["lra"]) and np.isnan(short["lra_diff"]) and np.isfinite(short["lufs_diff"])
    bits = lambda q: np.array([q[k] for k in O.NAMES + ("lufs_diff", "lra_diff", "true_peak_diff")]).tobytes()      # noqa: E731
    batch = am.loudness_batch(ests, tgts)
    for i in range(3):
        assert bits(batch[i]) == bits(am.loudness(ests[i], tgts[i])), i
    assert am.loudness_batch(ests, tgts, names=("lufs", "true_peak_diff"))[1] == {"lufs": batch[1]["lufs"], "true_peak_diff": batch[1]["true_peak_diff"]}
    # K = 2 estimates per target: the target is measured once
    bk = B()
    measured = []
    real = bk.loudness_metrics
    monkeypatch.setattr(bk, "loudness_metrics", lambda sigs, *a, **kw: (measured.append(len(list(sigs))), real(sigs, *a, **kw))[1])
    by_key = [[ests[1], ests[2]], [ests[1][::-1].copy(), ests[2][::-1].copy()]]
    multi = am.loudness_multi(by_key, tgts[1:])
    assert sum(measured) == 4 + 2                                                      # four estimates, two targets
    monkeypatch.undo()
    for i in range(2):
        for k in range(2):
            assert bits(multi[i][k]) == bits(am.loudness(by_key[k][i], tgts[1 + i])), (i, k)
    dev = am.loudness_batch([torch.from_numpy(e).to(DEV) for e in ests], [torch.from_numpy(t).to(DEV) for t in tgts], resident=True)
    assert [bits(q) for q in dev] == [bits(q) for q in batch]


# ---- where the kernels touch memory ---------------------------------------------------------------------------------------------
def _inputs(dtype, fs=8000):
    return [s for s in O.geometry_signals(fs, dtype, seed=31) if len(s)]             # (an arena view needs a sample)


@pytest.mark.parametrize("placement", ["odd", "quad"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("with_blocks", [True, False], ids=["blocks_out", "null"])
def test_guard_bands_and_poison(monkeypatch, dtype, placement, with_blocks):
    """ssr_loudness on separate device tensors, then on views into a NaN-filled arena with `out`, `blocks_out` and the workspace
    between 0xFF guard bands and 0xFF inside: the same bits, no guard damaged, no arena written, the signals read where they lie,
    and NaN only where the oracle's rules put it (a read outside a signal or of an unwritten workspace byte would be NaN)."""
    bk = B()
    fs = 8000
    gaps = {"odd": G.GAPS_ODD, "quad": G.GAPS_QUAD}[placement]
    sigs = _inputs(dtype, fs)

    def call(put):
        return bk.loudness_metrics(put(sigs), fs, return_blocks=with_blocks)
    plain = call(lambda arrays: [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays])
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        got = call(lambda arrays: g.arena(arrays, gaps, torch.from_numpy(np.asarray(arrays[0])).dtype, DEV)[0])
        assert len(g.blocks) >= (3 if with_blocks else 2)                  # out, blocks_out and the workspace
        assert g.arenas and g.read_in_place()
        g.check()
    rows = got[0] if with_blocks else got
    G.assert_same_bits(plain[0] if with_blocks else plain, rows, "loudness")
    if with_blocks:
        G.assert_same_bits(list(plain[1]), list(got[1]), "blocks")
        assert all(np.isfinite(e).all() for e in got[1])
    want = np.array([O.row(s, fs) for s in sigs])
    assert np.array_equal(np.isnan(rows), np.isnan(want)), (rows, want)


def test_one_byte_less_than_reported_is_refused(monkeypatch):
    """With ssr_loudness_workspace_bytes reporting one byte less than it should the call is SSR_ERR_WORKSPACE and nothing is
    enqueued: `out`, `blocks_out` and the workspace still hold only 0xFF."""
    bk = B()
    lib = bk._lib.load()
    real = lib.ssr_loudness_workspace_bytes
    asked = []

    def one_less(*a):
        n = int(real(*a))
        assert n > 0
        asked.append(n)
        return n - 1
    sigs = _inputs(np.float32)
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        m.setattr(lib, "ssr_loudness_workspace_bytes", one_less)
        with pytest.raises(bk.SsrHipError, match=r"libssrhip error -4\b"):
            bk.loudness_metrics(g.arena(sigs, G.GAPS_ODD, torch.float32, DEV)[0], 8000, return_blocks=True)
        assert asked
        g.check()
        assert g.untouched_payloads(("backend.py:put", "backend.py:_uniform_images")) == []


# ---- SSR_Eval_Helper(loudness=True) ----------------------------------------------------------------------------------------------
FS = 16000
LENGTHS = {"p360": (8000, 8411), "p361": (9001, 9600)}
OTHERS = dict(lsd_split=True, stoi="both", waveform=True, mel=True, mel_dtw=True, quality=True, pitch=True, phase=True, mrstft=True,
              bss_sdr=True, coherence=True)
LOUD = ("lufs", "lufs_diff", "true_peak_db", "true_peak_diff")


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
def test_evaluate_with_loudness_alone_and_with_every_other_option(tmp_path, cutoffs):
    """evaluate() on the four-file 16 kHz tree through the multi path (K = 2) and the flat path (K = 1): the four keys are bit-equal
    with `loudness=True` alone and with the eleven other options on; the other values are bit-equal to a run without the option;
    keys are listed in full_key_order(); the values are AudioMetrics.loudness's on the same arrays; with the option off the
    result is what it is without the argument, key for key."""
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee, AudioMetrics
    from ssr_eval_amd.eval import all_key_order, full_key_order
    from ssr_eval_amd.io import read_audio
    from ssr_eval_amd.lowpass import lowpass
    root = tmp_path / "vctk_test"
    _write_tree(root)

    def go(**kw):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=FS, output_sr=FS, evaluation_sr=FS, test_data_root=str(root),
                            setting_fft={"cutoff_freq": list(cutoffs)}, **kw)
        return h.evaluate(save_json=False)
    alone, everything, others, none = go(loudness=True), go(loudness=True, **OTHERS), go(**OTHERS), go()
    assert go(loudness=None) == none
    keys = ["proc_fft_%d_%d" % (2 * c, FS) for c in cutoffs]
    order, before = full_key_order(), all_key_order()
    at = order.index("lufs")
    assert order[:len(before)] == before and order[at:at + 4] == LOUD
    am = AudioMetrics(FS)
    seen = 0
    for spk in LENGTHS:
        for fn, by_key in everything[spk].items():
            assert list(by_key) == keys
            x, _ = read_audio(str(root / spk / fn))
            for key, cut in zip(keys, cutoffs):
                d, a, o = by_key[key], alone[spk][fn][key], others[spk][fn][key]
                assert list(d) == [k for k in order if k in d] and set(d) == set(before) | set(LOUD), (spk, fn, key, list(d))
                assert list(a) == list(order[:4]) + list(LOUD) and list(o) == list(before)
                assert list(none[spk][fn][key]) == list(order[:4])
                for m in LOUD:
                    print(spk, fn, key, m, d[m])
                    assert _bits(d[m]) == _bits(a[m]), (spk, fn, key, m, d[m], a[m])
                for m in before:
                    assert _bits(d[m]) == _bits(o[m]), (spk, fn, key, m, d[m], o[m])
                for m in order[:4]:
                    assert _bits(a[m]) == _bits(none[spk][fn][key][m]), (spk, fn, key, m)
                assert all(np.isfinite(d[m]) for m in LOUD) and -30.0 < d["lufs"] < -5.0 and d["lufs_diff"] < 0.0, (spk, fn, key, d)
                est = np.asarray(lowpass(x, cut, FS, order=1, _type="stft_hard"), np.float32)
                want = am.loudness(est, np.asarray(x, np.float32))
                assert [_bits(d[m]) for m in LOUD] == [_bits(want[m]) for m in LOUD], (spk, fn, key, d, want)
                seen += 1
    assert seen == 4 * len(cutoffs)
    for key in keys:
        assert list(everything["averaged"][key]) == [k for k in order if k in everything["averaged"][key]]
        assert list(alone["averaged"][key]) == list(order[:4]) + list(LOUD)
        for spk in LENGTHS:
            assert list(alone["each_speaker"][spk][key]) == list(order[:4]) + list(LOUD)
