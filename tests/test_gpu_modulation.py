"""GPU tests (-m gpu) of the modulation family (ssr_modulation): the geometry batches, the dtype batches and the
silence / gain cases of tests/test_modulation_host.py on the device, against the float64 oracle (tests/modulation_oracle.py) with the
same bars - Ebar within 1e-9 of the signal's largest cell, srmr within 1e-9 max(1, |srmr|), c90 and K* equal, mod_dist* within 1e-6
dB, srmr_diff within 2e-9 max(1, |srmr|), under the same conditioning assertions - and the same bit-for-bit properties;
AudioMetrics.srmr / modulation / _batch / _multi on host arrays and device tensors; a batch split under the workspace cap; every
device buffer of ssr_modulation between guard bands, on poisoned inputs, and the one-byte-less workspace;
SSR_Eval_Helper(modulation=True) on a small wav tree with an mp3 key.
Worst differences seen on an MI355X: Ebar 9.1e-13 of the largest cell, srmr 2.0e-13, mod_dist* 2.6e-13 dB, srmr_diff 1.2e-12; on the
emulated bodies 7.7e-13, 2.4e-13, 3.1e-13 dB and 6.2e-13."""
import math
import shutil

import numpy as np
import pytest
import torch

import auditory_oracle as A
import guarded as G
import modulation_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
FS = 16000
SHAPES, SHAPE_IDS, same_bits, sub_case = O.SHAPES, O.SHAPE_IDS, O.same_bits, O.sub_case
TILE = 32                                     # SSR_MOD_TILE: the envelope rows of k_mod_bank's staging tile


def B():
    from ssr_eval_amd import backend
    return backend


def run(c, spec=True, put=None):
    """ssr_modulation on Case c through backend.modulation_metrics -> (signal_out, pair_out, spectrum_out or None); put: how the two
    signal lists reach the call (default: the host arrays).  The oracle's designs are the call's own within 1e-14."""
    fc, coef, mod, S, ktab = B().modulation_design(c.fs, c.hop, c.n_bands, None, c.kstar)
    assert np.max(np.abs(coef - c.coef)) <= 1e-14 and np.max(np.abs(mod - c.mod)) <= 1e-15 and S == c.S and np.array_equal(ktab, c.ktab)
    tgts, ests = (c.tgts, c.ests) if put is None else put(c.tgts, c.ests)
    return B().modulation_metrics(tgts, ests, c.index, c.fs, c.n_bands, None, B().MODULATION_ENV_RATE, c.range_db, c.kstar, c.splits, spec, c.hop)


@pytest.mark.parametrize("fs,n_bands,env_rate", SHAPES, ids=SHAPE_IDS)
def test_geometry_shapes_and_bit_level_properties(fs, n_bands, env_rate):
    """The host file's geometry batch against the oracle; a repeated call repeats the bits; a pair alone gives the bits it gives in
    the batch, so does the reversed batch, the targets alone (n_est = 0) give their bits, and spectrum_out = NULL changes no bit."""
    c = O.geometry_case(fs, n_bands, env_rate, tile=TILE)
    got = run(c)
    print(fs, n_bands, env_rate, "hop_e %d S %d: worst Ebar %.3g, srmr %.3g, mod_dist %.3g dB, srmr_diff %.3g" % ((c.hop, c.S) + c.check(*got, name="geometry")))
    sig, pair, sx = got
    n_t = len(c.tgts)
    assert np.isnan(sig[0]).all() and np.isnan(sx[0]).all() and np.isfinite(sig[1:n_t]).all() and np.isnan(pair[0]).all()
    assert np.isfinite(pair[1:, :2]).all() and [[j for j in range(4) if math.isnan(pair[e, j])] for e in (1, 2, 3, 4)] == [[3], [2], [], [2, 3]]
    assert same_bits(run(c), got)
    for e in (1, 2, 3, 5):
        one = run(sub_case(c, [c.index[e]], [e]))
        assert one[1].tobytes() == pair[e:e + 1].tobytes() and same_bits([one[0], one[2]], [sig[[c.index[e], n_t + e]], sx[[c.index[e], n_t + e]]]), e
    back = run(sub_case(c, list(range(n_t))[::-1], list(range(len(c.ests)))[::-1]))
    assert back[1][::-1].tobytes() == pair.tobytes()
    assert same_bits([back[0][:n_t][::-1], back[0][n_t:][::-1], back[2][:n_t][::-1]], [sig[:n_t], sig[n_t:], sx[:n_t]])
    alone = run(sub_case(c, list(range(n_t)), []))
    assert alone[1].shape == (0, 4) and same_bits([alone[0], alone[2]], [sig[:n_t], sx[:n_t]])
    off = run(c, spec=False)
    assert off[2] is None and same_bits(off[:2], got[:2])


@pytest.mark.parametrize("tdt,edt", [(np.float32, np.float64), (np.float32, np.float32), (np.float64, np.float64)], ids=["f32-f64", "f32", "f64"])
def test_dtypes_range_and_constant_kstar(tdt, edt):
    """The short geometry batch at 8 kHz in the other dtype combinations; range_db away from its default; kstar as a constant; and an
    empty batch is an empty result."""
    c = O.geometry_case(8000, 32, short=True, tdt=tdt, edt=edt)
    base = run(c)
    print(np.dtype(tdt).name, np.dtype(edt).name, "worst Ebar %.3g, srmr %.3g, mod_dist %.3g dB, srmr_diff %.3g" % c.check(*base, name="dtypes"))
    for rdb, ks in ((35.5, None), (60.0, 6)):
        v = sub_case(c, list(range(len(c.tgts))), list(range(len(c.ests))))
        v.range_db, v.kstar, v.ktab = rdb, ks, O.kstar_table(c.fc, ks)
        got = run(v)
        v.check(*got, name="range %s kstar %s" % (rdb, ks))
        assert got[2].tobytes() == base[2].tobytes() and (ks is None or (np.all(got[0][1:len(c.tgts), 1] == 6) and not np.array_equal(got[0], base[0])))
    sig, pair, sx = run(O.Case([], [], [], 8000, 5))
    assert sig.shape == (0, 4) and pair.shape == (0, 4) and sx.shape == (0, 32, 8)


def test_silence_identity_and_gain():
    """The host file's case: a silent target and a silent estimate (NaN for the pair), a level factor that overflows (NaN, no
    infinity), estimate = target (0 exactly), gains of a power of two (the bits of srmr) and of 0.3 (1e-12)."""
    hop = O.hop_e(FS)
    x = O.voiced(6000, FS, 5)
    y = O.reverberated(x, FS, 6, 0.2)
    z = np.zeros(6000)
    c = O.Case([x, z, 0.25 * x, 0.3 * x, 1e10 * x], [z, x.copy(), y, 0.5 * y, y, 1e-148 * y, 0.3 * y, 3e38 * y], [0, 0, 0, 0, 1, 4, 0, 0], FS, hop,
               splits=[9] * 8)
    sig, pair, sx = run(c)
    print("worst Ebar %.3g, srmr %.3g, mod_dist %.3g dB, srmr_diff %.3g" % c.check(sig, pair, sx, name="silence"))
    n_t = 5
    assert np.isnan(sig[1, :3]).all() and sig[1, 3] == 0.0 and not np.any(sx[1]) and np.isnan(sig[n_t, :3]).all() and sig[n_t, 3] == 0.0
    assert np.isnan(pair[0]).all() and np.isnan(pair[4]).all() and np.isnan(pair[5]).all() and np.isfinite(sig[n_t + 5]).all()
    assert not np.isinf(sig).any() and not np.isinf(pair).any() and not np.isinf(sx).any()
    assert pair[1, 0] == 0.0 and pair[1, 1] == 0.0 and pair[1, 2] == 0.0 and pair[1, 3] == 0.0
    assert sig[2, :3].tobytes() == sig[0, :3].tobytes() and sig[n_t + 3, :3].tobytes() == sig[n_t + 2, :3].tobytes() and pair[3].tobytes() == pair[2].tobytes()
    for a, b in ((sig[3], sig[0]), (sig[4], sig[0]), (sig[n_t + 6], sig[n_t + 2]), (sig[n_t + 7], sig[n_t + 2])):
        assert abs(a[0] / b[0] - 1.0) <= 1e-12 and a[1:3].tobytes() == b[1:3].tobytes()
    assert np.max(np.abs(pair[6] - pair[2])) <= 1e-9 and np.max(np.abs(pair[7] - pair[2])) <= 1e-9 and pair[2, 1] > 1.0


def _signals():
    tgts = [O.voiced(7000, FS, 50).astype(np.float32), O.voiced(6100, FS, 51), O.voiced(5000, FS, 52).astype(np.float32)]
    ests = [O.reverberated(tgts[0].astype(np.float64), FS, 53, 0.2), (tgts[1] + A.noise(6100, 54, 0.02)).astype(np.float32),
            (0.5 * tgts[2] + A.noise(5000, 55, 0.001)).astype(np.float32)]
    return tgts, ests


def test_audio_metrics_single_batch_multi_and_resident_inputs():
    """AudioMetrics(16000): srmr() and modulation() are the oracle's values; float32 and float64 signals mixed in one list give the
    bits of the single calls; K = 2 estimates per target with a split per key; device tensors give the bits of host arrays."""
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(FS)
    hop = O.hop_e(FS)
    fc, _ = A.design(FS, 32)
    tgts, ests = _signals()
    at, ae = O.analyses_of([np.asarray(tgts[0], np.float64), ests[0]], FS, hop, 32)
    O.assert_conditioned(at, "target")
    O.assert_conditioned(ae, "estimate", at)
    alone = am.srmr(tgts[0], return_spectrum=True)
    assert list(alone) == ["srmr", "kstar", "c90", "mod_spectrum", "centre_hz", "mod_hz"] and np.max(np.abs(alone["centre_hz"] - fc)) <= 1e-9
    assert abs(alone["srmr"] - at["srmr"]) <= O.TOL_SRMR * max(1.0, at["srmr"]) and (alone["kstar"], alone["c90"]) == (at["kstar"], at["c90"])
    assert np.max(np.abs(alone["mod_spectrum"] - at["E"])) <= O.TOL_E * np.max(at["E"]) and np.allclose(alone["mod_hz"], O.mod_centres())
    assert am.srmr(tgts[0]) == {k: alone[k] for k in ("srmr", "kstar", "c90")}
    short = am.srmr(tgts[0][:407 * hop])
    assert math.isnan(short["srmr"]) and (short["kstar"], short["c90"]) == (-1, -1)
    d = am.modulation(ests[0], tgts[0], split_hz=2000.0, return_spectrum=True)
    want, _ = O.pair_of(at, ae, O.split_band(fc, 2000.0))
    assert list(d)[:5] == ["srmr", "srmr_diff", "mod_dist", "mod_dist_hf", "mod_dist_lf"] and list(d)[5:] == ["mod_spectrum", "target_mod_spectrum", "centre_hz", "mod_hz"]
    print("modulation()", {k: d[k] for k in list(d)[:5]}, "oracle", ae["srmr"], want)
    assert abs(d["srmr"] - ae["srmr"]) <= O.TOL_SRMR * max(1.0, ae["srmr"]) and abs(d["srmr_diff"] - want[0]) <= O.TOL_DIFF * max(1.0, min(at["srmr"], ae["srmr"]))
    assert max(abs(d[k] - w) for k, w in zip(("mod_dist", "mod_dist_hf", "mod_dist_lf"), want[1:])) <= O.TOL_DIST
    assert d["target_mod_spectrum"].tobytes() == alone["mod_spectrum"].tobytes() and d["mod_spectrum"].shape == (32, 8)
    plain = am.modulation(ests[0], tgts[0])
    assert plain["mod_dist"] == d["mod_dist"] and math.isnan(plain["mod_dist_hf"]) and math.isnan(plain["mod_dist_lf"]) and len(plain) == 5
    same = am.modulation(tgts[1], tgts[1].copy(), split_hz=1000.0)
    assert same["srmr_diff"] == 0.0 and same["mod_dist"] == 0.0 and same["mod_dist_hf"] == 0.0 and same["mod_dist_lf"] == 0.0
    assert am.modulation(0.25 * ests[0], tgts[0])["mod_dist"] == d["mod_dist"]
    bits = lambda q: np.array([q[k] for k in ("srmr", "srmr_diff", "mod_dist", "mod_dist_hf", "mod_dist_lf") if k in q]).tobytes()      # noqa: E731
    batch = am.modulation_batch(ests, tgts, split_hz=[4000.0, None, 1000.0])
    for i, s in enumerate((4000.0, None, 1000.0)):
        assert bits(batch[i]) == bits(am.modulation(ests[i], tgts[i], split_hz=s)), i
    assert math.isnan(batch[1]["mod_dist_hf"]) and np.isfinite(batch[1]["mod_dist"])
    assert am.modulation_batch(ests, tgts, names=("mod_dist",))[1] == {"mod_dist": batch[1]["mod_dist"]}
    by_key = [[ests[1], ests[2]], [ests[1][::-1].copy(), ests[2][::-1].copy()]]
    multi = am.modulation_multi(by_key, tgts[1:], split_hz=[2000.0, 3000.0])
    for i in range(2):
        for k in range(2):
            assert bits(multi[i][k]) == bits(am.modulation(by_key[k][i], tgts[1 + i], split_hz=(2000.0, 3000.0)[k])), (i, k)
    dev = am.modulation_batch([torch.from_numpy(np.ascontiguousarray(e)).to(DEV) for e in ests], [torch.from_numpy(a).to(DEV) for a in tgts],
                              split_hz=[4000.0, None, 1000.0], resident=True)
    assert [bits(q) for q in dev] == [bits(q) for q in batch]
    other = am.modulation(ests[0], tgts[0], env_rate=3200, kstar=6, n_bands=24, range_db=40.0)
    assert np.isfinite(other["srmr"]) and other["srmr"] != d["srmr"]


def test_a_batch_over_the_workspace_cap_is_split_and_keeps_its_bits(monkeypatch):
    """Six targets with their estimates interleaved: under a cap that holds two signals the call becomes several ssr_modulation calls
    of whole targets, and no bit changes."""
    bk = B()
    lib = bk._lib.load()
    tgts = [O.voiced(5000 + 301 * i, FS, 70 + i) for i in range(6)]
    index = [5, 0, 3, 3, 1, 0, 4, 3]
    ests = [0.5 * tgts[t] + A.noise(len(tgts[t]), 80 + e, 0.01) for e, t in enumerate(index)]
    args = (tgts, ests, index, FS, 32, None, 1600, 60.0, None, [e % 5 - 1 for e in range(8)], True)
    whole = bk.modulation_metrics(*args)
    real, calls = lib.ssr_modulation, []

    def counted(*a):
        calls.append((a[4], a[9]))
        return real(*a)
    with monkeypatch.context() as m:
        m.setattr(lib, "ssr_modulation", counted)
        m.setattr(bk, "MODULATION_WORKSPACE_CAP", 600000)
        split = bk.modulation_metrics(*args)
    assert len(calls) >= 3 and sum(c[0] for c in calls) == 6 and sum(c[1] for c in calls) == 8
    assert same_bits(split, whole) and np.isfinite(whole[0]).all() and np.isfinite(whole[1][:, :2]).all()


# ---- where the kernels touch memory ---------------------------------------------------------------------------------------------
def _case(tdt, edt, n_bands=32):
    return O.geometry_case(8000, n_bands, short=True, tdt=tdt, edt=edt)


@pytest.mark.parametrize("placement", ["odd", "quad"])
@pytest.mark.parametrize("tdt,edt", [(np.float32, np.float32), (np.float64, np.float32), (np.float64, np.float64)], ids=["f32", "f64-f32", "f64"])
@pytest.mark.parametrize("with_opt", [True, False], ids=["spectrum_out", "null"])
@pytest.mark.parametrize("n_bands", [32, 40])
def test_guard_bands_and_poison(monkeypatch, tdt, edt, placement, with_opt, n_bands):
    """ssr_modulation on separate device tensors, then on views into NaN-filled arenas with signal_out, pair_out, spectrum_out and the
    workspace between 0xFF guard bands and 0xFF inside: the same bits, no guard damaged, no arena written, the signals read where
    they lie, and NaN only where the oracle's rules put it (a read outside a signal or of an unwritten workspace byte would be NaN)."""
    gaps = {"odd": G.GAPS_ODD, "quad": G.GAPS_QUAD}[placement]
    c = _case(tdt, edt, n_bands)
    to_dev = lambda arrays: [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]      # noqa: E731
    plain = run(c, with_opt, lambda t, e: (to_dev(t), to_dev(e)))
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        got = run(c, with_opt, lambda t, e: (g.arena(t, gaps, torch.from_numpy(t[0]).dtype, DEV)[0], g.arena(e, gaps, torch.from_numpy(e[0]).dtype, DEV)[0]))
        assert len(g.blocks) >= (4 if with_opt else 3)                     # signal_out, pair_out, spectrum_out and the workspace
        assert len(g.arenas) == 2 and g.read_in_place()
        g.check()
    G.assert_same_bits([p for p in plain if p is not None], [p for p in got if p is not None], "modulation")
    c.check(*got, name="guarded")
    # the targets alone: est, est_off, tgt_index, split_band and pair_out are NULL
    solo = sub_case(c, list(range(len(c.tgts))), [])
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        alone = run(solo, with_opt, lambda t, e: (g.arena(t, gaps, torch.from_numpy(t[0]).dtype, DEV)[0], []))
        assert g.arenas and g.read_in_place()
        g.check()
    assert alone[0].tobytes() == got[0][:len(c.tgts)].tobytes()


def test_one_byte_less_than_reported_is_refused(monkeypatch):
    """With ssr_modulation_workspace_bytes reporting one byte less than it should the call is SSR_ERR_WORKSPACE and nothing is
    enqueued: the outputs and the workspace still hold only 0xFF."""
    bk = B()
    lib = bk._lib.load()
    real = lib.ssr_modulation_workspace_bytes
    asked = []

    def one_less(*a):
        n = int(real(*a))
        assert n > 0
        asked.append(n)
        return n - 1
    c = _case(np.float32, np.float32)
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        m.setattr(lib, "ssr_modulation_workspace_bytes", one_less)
        with pytest.raises(bk.SsrHipError, match=r"libssrhip error -4\b"):
            run(c, True, lambda t, e: (g.arena(t, G.GAPS_ODD, torch.float32, DEV)[0], g.arena(e, G.GAPS_ODD, torch.float32, DEV)[0]))
        assert asked
        g.check()
        assert g.untouched_payloads(("backend.py:put", "backend.py:_uniform_images")) == []


# ---- SSR_Eval_Helper(modulation=True) --------------------------------------------------------------------------------------------
LENGTHS = {"p360": (8000, 8411), "p361": (9001, 9600)}
MOD = ("srmr", "srmr_diff", "mod_dist", "mod_dist_hf")


def _write_tree(root):
    """Two speakers x two files: a 220 Hz tone with harmonics under a 5 Hz level movement, plus noise"""
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(12)
    for spk, lens in LENGTHS.items():
        (root / spk).mkdir(parents=True)
        for i, n in enumerate(lens):
            t = np.arange(n) / FS
            x = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.1 * np.sin(2 * np.pi * 440 * t) + 0.05 * np.sin(2 * np.pi * 1760 * t) + 0.03 * np.sin(2 * np.pi * 3520 * t)
            x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 5.0 * t + i))
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), (x + 0.02 * rng.standard_normal(n)).astype(np.float32), FS)


def test_evaluate_with_modulation(tmp_path, monkeypatch):
    """evaluate() on a four-file 16 kHz tree with an mp3 key (the codec replaced by a copy at 0.8 of the level) and two FFT keys: the
    four keys appear for every degradation key in full_key_order() order, in front of the auditory family's; the values are the
    oracle's on the very arrays the helper scored; mod_dist_hf is NaN for the mp3 key, which has no cutoff; and with the option off
    the result is what it is without the argument."""
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee, AudioMetrics
    from ssr_eval_amd.eval import all_key_order, full_key_order
    from ssr_eval_amd.io import read_audio, write_wav
    root = tmp_path / "vctk_test"
    _write_tree(root)
    cutoffs = [2000, 3000]

    def fake_sox(self, args):
        if "-C" in args:                                           # encode: source -> "<key>.mp3"
            y, sr = read_audio(args[0])
            write_wav(args[3] + ".wav", (0.8 * y).astype(np.float32), sr)
            shutil.move(args[3] + ".wav", args[3])
        else:                                                      # decode: "<key>.mp3" -> temp
            shutil.copy(args[0], args[1])
    monkeypatch.setattr(SSR_Eval_Helper, "_run_sox", fake_sox)
    scored = []
    real = AudioMetrics.modulation_multi

    def recording(self, by_key, targets, *a, **kw):
        host = lambda w: w.detach().cpu().numpy().copy() if isinstance(w, torch.Tensor) else np.array(w)      # noqa: E731
        scored.append(([[host(w) for w in ws] for ws in by_key], [host(w) for w in targets], a))
        return real(self, by_key, targets, *a, **kw)
    monkeypatch.setattr(AudioMetrics, "modulation_multi", recording)

    def go(**kw):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=FS, output_sr=FS, evaluation_sr=FS, test_data_root=str(root),
                            setting_fft={"cutoff_freq": list(cutoffs)}, setting_mp3_compression={"low_kbps": [32]}, **kw)
        return h.evaluate(save_json=False)
    on = go(modulation=True)
    kept = list(scored)
    both, none = go(modulation=True, auditory=True), go()
    assert go(modulation=None) == none
    keys = ["proc_mp3_32_%d" % FS] + ["proc_fft_%d_%d" % (2 * c, FS) for c in cutoffs]
    order, before = full_key_order(), all_key_order()
    assert order[:len(before)] == before and order[-6:] == MOD + ("nsim", "nsim_hf") and order.index("srmr") > order.index("ltas_dist")
    # the oracle on what the helper scored: by_key[k][i] against targets[i], key k split at its own cutoff
    hop = O.hop_e(FS)
    fc, _ = A.design(FS, 32)
    want, n_files = {}, 0
    as_key = lambda w: np.asarray(w, np.float32).tobytes()      # noqa: E731
    for by_key, tgts, a in kept:
        assert a[0] == [None, 2000, 3000] and len(by_key) == 3
        an_t = O.analyses_of([np.asarray(t, np.float64) for t in tgts], FS, hop, 32)
        for k in range(3):
            an_e = O.analyses_of([np.asarray(e, np.float64) for e in by_key[k]], FS, hop, 32)
            for i in range(len(tgts)):
                O.assert_conditioned(an_t[i], "target")
                O.assert_conditioned(an_e[i], "estimate", an_t[i])
                want[(as_key(tgts[i]), k)] = (an_t[i], an_e[i], O.pair_of(an_t[i], an_e[i], O.split_band(fc, a[0][k]))[0])
        n_files += len(tgts)
    assert n_files == 4
    for spk in LENGTHS:
        for fn in sorted(on[spk]):
            assert list(on[spk][fn]) == keys
            x, _ = read_audio(str(root / spk / fn))
            for k, key in enumerate(keys):
                d, b = on[spk][fn][key], both[spk][fn][key]
                at, ae, pw = want[(as_key(x), k)]
                assert list(d) == list(order[:4]) + list(MOD) and list(b) == list(order[:4]) + list(MOD) + ["nsim", "nsim_hf"]
                assert list(none[spk][fn][key]) == list(order[:4])
                print(spk, fn, key, {m: d[m] for m in MOD}, "oracle", ae["srmr"], pw)
                assert abs(d["srmr"] - ae["srmr"]) <= O.TOL_SRMR * max(1.0, ae["srmr"])
                assert abs(d["srmr_diff"] - pw[0]) <= O.TOL_DIFF * max(1.0, min(at["srmr"], ae["srmr"])) and abs(d["mod_dist"] - pw[1]) <= O.TOL_DIST
                if k == 0:
                    assert math.isnan(d["mod_dist_hf"]) and math.isnan(pw[2]) and d["mod_dist"] < 0.5      # (a copy at another level, 16-bit)
                else:
                    assert abs(d["mod_dist_hf"] - pw[2]) <= O.TOL_DIST and d["mod_dist_hf"] > d["mod_dist"] > 0.0
                for m in MOD:
                    assert np.float64(d[m]).tobytes() == np.float64(b[m]).tobytes(), (spk, fn, key, m)
                for m in order[:4]:
                    assert np.float64(d[m]).tobytes() == np.float64(none[spk][fn][key][m]).tobytes(), (spk, fn, key, m)
    for key in keys:
        assert list(on["averaged"][key]) == list(order[:4]) + list(MOD)
        for spk in LENGTHS:
            assert list(on["each_speaker"][spk][key]) == list(order[:4]) + list(MOD)
