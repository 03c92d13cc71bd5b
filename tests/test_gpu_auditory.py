"""GPU tests (-m gpu) of the auditory family (ssr_auditory): the geometry batches and the ragged batch of
tests/test_auditory_host.py on the device, against the float64 oracle (tests/auditory_oracle.py) with the same bars - P within 1e-9
of the target's largest cell (10^(D / 10) of the dB images' unclamped cells against the oracle's P: only the images leave the
library), the NSIM values within 1e-9, the dB images within 1e-6 dB, under the same conditioning assertions - and the same bit-for-bit properties;
AudioMetrics.nsim / _batch / _multi / gammatone_spectrogram on host arrays and device tensors; every device buffer of ssr_auditory
between guard bands, on poisoned inputs, and the one-byte-less workspace; SSR_Eval_Helper(auditory=True) on a small wav tree.
Worst differences seen on an MI355X: P 1.2e-14 of the target's largest cell, NSIM values 1.1e-14, dB images 2.5e-12 dB; on the
emulated bodies 1.2e-14, 1.1e-14 and 2.5e-12 dB
(DESIGN.md section 23)."""
import math

import numpy as np
import pytest
import torch

import auditory_oracle as O
import guarded as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
FS = 16000


def B():
    from ssr_eval_amd import backend
    return backend


def run(c, bands=True, images=True, put=None):
    """ssr_auditory on Case c through backend.auditory_metrics -> (pair_out, band_out or None, the dB images per signal or None);
    put: how the two signal lists reach the call (default: the host arrays).  The oracle scores with the coefficients the call
    used (backend.gammatone_design's: the oracle's own within 1e-14)."""
    fc, coef = B().gammatone_design(c.fs, len(c.coef))
    assert np.max(np.abs(coef - c.coef)) <= 1e-14
    c.coef = coef
    tgts, ests = (c.tgts, c.ests) if put is None else put(c.tgts, c.ests)
    return B().auditory_metrics(tgts, ests, c.index, c.fs, len(coef), None, c.range_db, c.match, c.splits, bands, images, c.hop)


def same_bits(a, b):
    return all((x is None and y is None) or np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("fs,hop,n_bands,ks", [(16000, 160, 32, (8, 9, 64)), (16000, 8, 3, (8, 9, 64, 512, 513)), (16000, 8, 32, (8, 9, 16, 64, 65, 128)),
                                               (16000, 8, 64, (8, 9, 32, 33, 64)), (16000, 100, 3, (8, 9, 64)), (48000, 480, 32, (8, 9)),
                                               (16000, 513, 64, (8, 9))],
                         ids=["hop160-32", "hop8-3", "hop8-32", "hop8-64", "hop100-3-4tiles", "48k-hop480-32-2tiles", "hop513-64-2tiles"])
def test_geometry_shapes_and_bit_level_properties(fs, hop, n_bands, ks):
    """The host file's geometry batch against the oracle in two dtype combinations; a repeated call repeats the bits; a pair alone
    gives the bits it gives in the batch, so does the reversed batch, and band_out = image_out = NULL changes no bit of pair_out."""
    c = O.geometry_case(fs, hop, n_bands, ks)
    got = run(c)
    worst = c.check(*got, name="hop %d C %d" % (hop, n_bands))
    print(hop, n_bands, "worst P %.3g, NSIM %.3g, dB image %.3g" % worst)
    pair, bd, img = got
    n_t = len(c.tgts)
    assert np.isnan(pair[:3]).all() and np.isfinite(pair[3, 0]) and [len(i) for i in img[:4]] == [0, 1, 2, 3]
    assert np.isfinite(pair[4:, 0]).all() and not np.isinf(pair).any() and np.isnan(bd[:, [0, -1]]).all() and np.isfinite(bd[3:, 1:-1]).all()
    again = run(c)
    assert again[0].tobytes() == pair.tobytes() and again[1].tobytes() == bd.tobytes() and same_bits(again[2], img)
    f64 = O.geometry_case(fs, hop, n_bands, ks[:2], tdt=np.float32, edt=np.float64)
    print("f32 / f64: worst P %.3g, NSIM %.3g, dB image %.3g" % f64.check(*run(f64), name="f32/f64"))
    for e in (3, 5, n_t - 1, n_t, n_t + 1):
        one = run(O.Case([c.tgts[c.index[e]]], [c.ests[e]], [0], c.coef, hop, splits=[c.splits[e]], edt=np.float32, fs=fs))
        assert one[0].tobytes() == pair[e:e + 1].tobytes() and one[1].tobytes() == bd[e:e + 1].tobytes(), e
        assert same_bits(one[2], [img[c.index[e]], img[n_t + e]]), e
    back = run(O.Case(c.tgts[::-1], c.ests[::-1], [n_t - 1 - t for t in c.index[::-1]], c.coef, hop, splits=c.splits[::-1], edt=np.float32, fs=fs))
    assert back[0][::-1].tobytes() == pair.tobytes() and back[1][::-1].tobytes() == bd.tobytes() and same_bits(back[2][::-1], img[n_t:] + img[:n_t])
    off = run(c, bands=False, images=False)
    assert off[0].tobytes() == pair.tobytes() and off[1] is None and off[2] is None
    alone = run(O.Case(c.tgts, [], [], c.coef, hop, fs=fs))                       # n_est = 0: the targets' images
    assert alone[0].shape == (0, 3) and same_bits(alone[2], img[:n_t])


@pytest.mark.parametrize("tdt,edt", [(np.float64, np.float64), (np.float32, np.float32)], ids=["f64", "f32"])
def test_ragged_batch_and_three_estimates_per_target(tdt, edt):
    """The host file's ragged batch: six signals of 0.5 s or less, K = 3 estimates on the first at three different splits; with and
    without level matching; range_db away from its default; and an empty batch is an empty result."""
    fc, coef = O.design(FS, 32)
    lens = (8000, 6123, 4801, 3000, 1777, 640)
    tgts = [O.harmonic(n, FS, 10 + i) if i % 2 == 0 else O.noise(n, 10 + i) for i, n in enumerate(lens)]
    ests = [O.lowpassed(tgts[0], 0.25), tgts[0] + O.noise(lens[0], 30, 0.02), O.noise(lens[0], 31)] + \
        [0.7 * t + O.noise(len(t), 40 + i, 0.01) for i, t in enumerate(tgts[1:])]
    index = [0, 0, 0, 1, 2, 3, 4, 5]
    splits = [-1, 31, O.split_band(fc, 2000.0), 5, 1, 30, -1, 17]
    power = None
    for match, rdb in ((True, 60.0), (False, 60.0), (True, 35.5)):
        c = O.Case(tgts, ests, index, coef, 160, range_db=rdb, match=match, splits=splits, tdt=tdt, edt=edt, power=power)
        got = run(c)
        print(np.dtype(tdt).name, match, rdb, "worst P %.3g, NSIM %.3g, dB image %.3g" % c.check(*got, name="ragged"), got[0][:3, 0])
        pair, power = got[0], c.power
        assert np.isnan(pair[0, 1:]).all() and np.isnan(pair[1, 1]) and np.isfinite(pair[1, 2]) and np.isfinite(pair[2]).all()
    pair, bd, img = run(O.Case([], [], [], coef, 160))
    assert pair.shape == (0, 3) and bd.shape == (0, 32) and img == []


def test_silence_identity_and_gain():
    fc, coef = O.design(FS, 32)
    x = O.harmonic(3000, FS, 5)
    y = O.lowpassed(x, 0.3)
    z = np.zeros(3000)
    # (1e-160 y: its image is denormal and the level factor overflows - the pair's NaN rule, no infinity)
    c = O.Case([x, z], [z, x.copy(), y, 0.5 * y, y, 1e-160 * y], [0, 0, 0, 0, 1, 0], coef, 160, splits=[9] * 6)
    pair, bd, img = run(c)
    c.check(pair, bd, img, name="silence")
    assert np.isnan(pair[5]).all() and np.isnan(bd[5]).all() and np.isnan(img[2 + 5]).all() and not any(np.isinf(i).any() for i in img)
    assert np.isfinite(pair[0]).all() and pair[0, 0] < 0.5 and np.max(np.abs(pair[1] - 1.0)) <= 1e-12 and np.max(np.abs(bd[1, 1:-1] - 1.0)) <= 1e-12
    assert pair[2].tobytes() == pair[3].tobytes() and np.isnan(pair[4]).all() and np.isnan(bd[4]).all()
    assert np.isnan(img[1]).all() and np.isnan(img[2 + 4]).all() and not np.isinf(pair).any()


def test_audio_metrics_single_batch_multi_and_resident_inputs():
    """AudioMetrics(16000): nsim() is the oracle's values; float32 and float64 signals mixed in one list give the bits of the single
    calls; K = 2 estimates per target with a split per key; device tensors give the bits of host arrays; the spectrogram of a signal
    is the target image of a pair."""
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(FS)
    fc, coef = B().gammatone_design(FS)
    tgts = [O.harmonic(5000, FS, 50).astype(np.float32), O.noise(4100, 51), O.harmonic(3000, FS, 52).astype(np.float32)]
    ests = [O.lowpassed(tgts[0].astype(np.float64), 0.25), (tgts[1] + O.noise(4100, 54, 0.02)).astype(np.float32),
            (0.5 * tgts[2] + O.noise(3000, 55, 0.001)).astype(np.float32)]
    d = am.nsim(ests[0], tgts[0], split_hz=2000.0, return_bands=True)
    assert list(d) == ["nsim", "nsim_hf", "nsim_lf", "fvnsim", "centre_hz"] and np.array_equal(d["centre_hz"], fc)
    want = O.analyse(np.asarray(tgts[0], np.float64), ests[0], coef, 160, split=O.split_band(fc, 2000.0))
    O.assert_conditioned(np.asarray(tgts[0], np.float64), ests[0], coef, 160, d=want)
    worst = max(abs(d[k] - w) for k, w in zip(("nsim", "nsim_hf", "nsim_lf"), want["pair"]))
    worst = max(worst, float(np.nanmax(np.abs(d["fvnsim"] - want["bands"]))))
    print("worst NSIM difference", worst, {k: d[k] for k in ("nsim", "nsim_hf", "nsim_lf")})
    assert worst <= O.TOL_NSIM and d["nsim_hf"] < d["nsim_lf"] < 1.0 and np.isnan(d["fvnsim"][[0, -1]]).all()
    plain = am.nsim(ests[0], tgts[0])
    assert plain["nsim"] == d["nsim"] and math.isnan(plain["nsim_hf"]) and math.isnan(plain["nsim_lf"]) and list(plain) == ["nsim", "nsim_hf", "nsim_lf"]
    assert all(abs(v - 1.0) <= 1e-12 for v in am.nsim(tgts[1], tgts[1].copy(), split_hz=1000.0).values())
    short = am.nsim(tgts[0][:639], tgts[0][:639], split_hz=1000.0)
    assert all(math.isnan(v) for v in short.values())
    assert am.nsim(0.25 * ests[0], tgts[0])["nsim"] == d["nsim"] and am.nsim(0.25 * ests[0], tgts[0], match_level=False)["nsim"] != d["nsim"]
    bits = lambda q: np.array([q[k] for k in ("nsim", "nsim_hf", "nsim_lf") if k in q]).tobytes()      # noqa: E731
    batch = am.nsim_batch(ests, tgts, split_hz=[4000.0, None, 1000.0])
    for i, s in enumerate((4000.0, None, 1000.0)):
        assert bits(batch[i]) == bits(am.nsim(ests[i], tgts[i], split_hz=s)), i
    assert math.isnan(batch[1]["nsim_hf"]) and np.isfinite(batch[1]["nsim"])
    assert am.nsim_batch(ests, tgts, names=("nsim",))[1] == {"nsim": batch[1]["nsim"]}
    by_key = [[ests[1], ests[2]], [ests[1][::-1].copy(), ests[2][::-1].copy()]]
    multi = am.nsim_multi(by_key, tgts[1:], split_hz=[2000.0, 3000.0])
    for i in range(2):
        for k in range(2):
            assert bits(multi[i][k]) == bits(am.nsim(by_key[k][i], tgts[1 + i], split_hz=(2000.0, 3000.0)[k])), (i, k)
    dev = am.nsim_batch([torch.from_numpy(np.ascontiguousarray(e)).to(DEV) for e in ests], [torch.from_numpy(a).to(DEV) for a in tgts],
                        split_hz=[4000.0, None, 1000.0], resident=True)
    assert [bits(q) for q in dev] == [bits(q) for q in batch]
    img, hz = am.gammatone_spectrogram(tgts[0])
    assert img.shape == (O.rows(5000, 160), 32) and np.array_equal(hz, fc)
    assert np.max(np.abs(img - want["Dr"])) <= 1e-6 and abs(np.max(img) - np.min(img)) <= 60.0 + 1e-9


# ---- where the kernels touch memory ---------------------------------------------------------------------------------------------
SHAPES = {"hop8-32": (8, 32, (8, 9, 64, 65)), "hop100-3-4tiles": (100, 3, (8, 9, 64))}      # (hop, bands, ks); 3 bands: tiles of 32 samples


def _case(tdt, edt, shape="hop8-32"):
    hop, n_bands, ks = SHAPES[shape]
    c = O.geometry_case(FS, hop, n_bands, ks, tdt=tdt, edt=edt)
    c.power = None
    return c


@pytest.mark.parametrize("placement", ["odd", "quad"])
@pytest.mark.parametrize("tdt,edt", [(np.float32, np.float32), (np.float64, np.float32), (np.float64, np.float64)], ids=["f32", "f64-f32", "f64"])
@pytest.mark.parametrize("with_opt", [True, False], ids=["band_image_out", "null"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_guard_bands_and_poison(monkeypatch, tdt, edt, placement, with_opt, shape):
    """ssr_auditory on separate device tensors, then on views into NaN-filled arenas with pair_out, band_out, image_out and the
    workspace between 0xFF guard bands and 0xFF inside: the same bits, no guard damaged, no arena written, the signals read where
    they lie, and NaN only where the oracle's rules put it (a read outside a signal or of an unwritten workspace byte would be NaN)."""
    gaps = {"odd": G.GAPS_ODD, "quad": G.GAPS_QUAD}[placement]
    c = _case(tdt, edt, shape)
    to_dev = lambda arrays: [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]      # noqa: E731
    plain = run(c, with_opt, with_opt, lambda t, e: (to_dev(t), to_dev(e)))
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        got = run(c, with_opt, with_opt,
                  lambda t, e: (g.arena(t, gaps, torch.from_numpy(t[0]).dtype, DEV)[0], g.arena(e, gaps, torch.from_numpy(e[0]).dtype, DEV)[0]))
        assert len(g.blocks) >= (4 if with_opt else 2)                     # pair_out, band_out, image_out and the workspace
        assert len(g.arenas) == 2 and g.read_in_place()
        g.check()
    G.assert_same_bits([plain[0]] + ([plain[1]] + list(plain[2]) if with_opt else []), [got[0]] + ([got[1]] + list(got[2]) if with_opt else []), "auditory")
    if with_opt:
        c.check(*got, name="guarded")
    # the targets alone: est, est_off, tgt_index, split_band and pair_out are NULL
    solo = O.Case(c.tgts, [], [], c.coef, c.hop, tdt=tdt)
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        alone = run(solo, False, True, lambda t, e: (g.arena(t, gaps, torch.from_numpy(t[0]).dtype, DEV)[0], []))
        assert g.arenas and g.read_in_place()
        g.check()
    if with_opt:
        assert same_bits(alone[2], got[2][:len(c.tgts)])


def test_one_byte_less_than_reported_is_refused(monkeypatch):
    """With ssr_auditory_workspace_bytes reporting one byte less than it should the call is SSR_ERR_WORKSPACE and nothing is
    enqueued: the outputs and the workspace still hold only 0xFF."""
    bk = B()
    lib = bk._lib.load()
    real = lib.ssr_auditory_workspace_bytes
    asked = []

    def one_less(*a):
        n = int(real(*a))
        assert n > 0
        asked.append(n)
        return n - 1
    c = _case(np.float32, np.float32)
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        m.setattr(lib, "ssr_auditory_workspace_bytes", one_less)
        with pytest.raises(bk.SsrHipError, match=r"libssrhip error -4\b"):
            run(c, True, True, lambda t, e: (g.arena(t, G.GAPS_ODD, torch.float32, DEV)[0], g.arena(e, G.GAPS_ODD, torch.float32, DEV)[0]))
        assert asked
        g.check()
        assert g.untouched_payloads(("backend.py:put", "backend.py:_uniform_images")) == []


# ---- SSR_Eval_Helper(auditory=True) ----------------------------------------------------------------------------------------------
LENGTHS = {"p360": (8000, 8411, 9100, 12000), "p361": (9001, 9600, 8192, 10001)}
AUD = ("nsim", "nsim_hf")


def _bits(v):
    return np.float64(v).tobytes()                                        # NaN equals NaN


def _write_tree(root):
    """Two speakers x four files: a 220 Hz tone with two harmonics plus noise (the tree of tests/test_gpu_spectrum.py, eight files)."""
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(12)
    for spk, lens in LENGTHS.items():
        (root / spk).mkdir(parents=True)
        for i, n in enumerate(lens):
            t = np.arange(n) / FS
            x = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.1 * np.sin(2 * np.pi * 440 * t) + 0.05 * np.sin(2 * np.pi * 1760 * t)
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), (x + 0.02 * rng.standard_normal(n)).astype(np.float32), FS)


def test_evaluate_with_auditory(tmp_path):
    """evaluate() on the eight-file 16 kHz tree with two FFT keys: the two keys appear in full_key_order() order behind the other
    families', the values are AudioMetrics.nsim_multi's on the same arrays, and with the option off the result is what it is
    without the argument, key for key."""
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee, AudioMetrics
    from ssr_eval_amd.eval import all_key_order, full_key_order
    from ssr_eval_amd.io import read_audio
    from ssr_eval_amd.lowpass import lowpass
    root = tmp_path / "vctk_test"
    _write_tree(root)
    cutoffs = [2000, 3000]

    def go(**kw):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=FS, output_sr=FS, evaluation_sr=FS, test_data_root=str(root),
                            setting_fft={"cutoff_freq": list(cutoffs)}, **kw)
        return h.evaluate(save_json=False)
    on, both, bw, none = go(auditory=True), go(auditory=True, bandwidth=True), go(bandwidth=True), go()
    assert go(auditory=None) == none
    keys = ["proc_fft_%d_%d" % (2 * c, FS) for c in cutoffs]
    order, before = full_key_order(), all_key_order()
    assert order[:len(before)] == before and order[-2:] == AUD and order.index("nsim") > order.index("ltas_dist")
    am = AudioMetrics(FS)
    files, tgts, by_key = [], [], [[], []]
    for spk in LENGTHS:
        for fn in sorted(on[spk]):
            x, _ = read_audio(str(root / spk / fn))
            files.append((spk, fn))
            tgts.append(np.asarray(x, np.float32))
            for k, cut in enumerate(cutoffs):
                by_key[k].append(np.asarray(lowpass(x, cut, FS, order=1, _type="stft_hard"), np.float32))
    want = am.nsim_multi(by_key, tgts, split_hz=[float(c) for c in cutoffs], names=AUD)
    assert len(files) == 8
    for i, (spk, fn) in enumerate(files):
        assert list(on[spk][fn]) == keys
        for k, key in enumerate(keys):
            d, b = on[spk][fn][key], both[spk][fn][key]
            assert list(d) == list(order[:4]) + list(AUD) and list(b) == [m for m in order if m in b] and list(b)[-2:] == list(AUD)
            assert list(none[spk][fn][key]) == list(order[:4])
            for m in AUD:
                print(spk, fn, key, m, d[m])
                assert _bits(d[m]) == _bits(b[m]) == _bits(want[i][k][m]), (spk, fn, key, m, d[m], b[m], want[i][k][m])
            for m in order[:4]:
                assert _bits(d[m]) == _bits(none[spk][fn][key][m]), (spk, fn, key, m)
            for m in bw[spk][fn][key]:
                assert _bits(b[m]) == _bits(bw[spk][fn][key][m]), (spk, fn, key, m)
            assert all(np.isfinite(d[m]) for m in AUD) and d["nsim_hf"] < d["nsim"] < 1.0, (spk, fn, key, d)
    for key in keys:
        assert list(on["averaged"][key]) == list(order[:4]) + list(AUD)
        for spk in LENGTHS:
            assert list(on["each_speaker"][spk][key]) == list(order[:4]) + list(AUD)
