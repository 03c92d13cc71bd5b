"""GPU tests (-m gpu) of the spectrum family (ssr_spectrum): the input list and the geometry cases of
tests/test_spectrum_host.py on the device, against the float64 oracle (tests/spectrum_oracle.py) with the same bars - P within 1e-9
of the signal's largest bin, rolloff and edge bins equal to the oracle's, the centroid within 1e-9 fs, every dB value within 1e-6 dB,
under the same conditioning assertions - and the same bit-for-bit properties; AudioMetrics.bandwidth / _batch / _multi on host arrays
and device tensors; every device buffer of ssr_spectrum between guard bands, on poisoned inputs, and the one-byte-less workspace;
SSR_Eval_Helper(bandwidth=True) on a small wav tree.
Worst differences seen on an MI355X: spectrum 1.7e-15 of the largest bin, centroid 2.3e-13 bins, dB values 7.4e-12 dB (DESIGN.md
section 22)."""
import math

import numpy as np
import pytest
import torch

import guarded as G
import spectrum_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"


def B():
    from ssr_eval_amd import backend
    return backend


def run(c, ltas=True, put=None):
    """ssr_spectrum on Case c -> (sig_out, pair_out, ltas_out or None, None), as run() of the host file; put: how the two signal
    lists reach the call (default: the host arrays)."""
    tgts, ests = (c.tgts, c.ests) if put is None else put(c.tgts, c.ests)
    got = B().spectrum_metrics(tgts, ests, c.index, c.N, c.H, (c.lo, c.hi), c.rho, c.drop, c.bands, c.splits, return_ltas=ltas)
    return got[0], got[1], (got[2] if ltas else None), None


@pytest.mark.parametrize("fs,N,H", O.CASES)
def test_input_list_against_the_oracle(fs, N, H):
    """The host file's list: white, low-passed and coloured noise as targets, K = 1 and K = 3 estimates per target, the four dtype
    combinations, the default third-octave table, a split per pair."""
    n = N + 70 * H + 13
    tgts = [O.make(k, n, 20 + j) for j, k in enumerate(("white", "lowpassed", "coloured"))]
    ests = [O.make("lowpassed", n, 30), O.make("coloured", n, 31), O.make("white", n, 32), O.make("lowpassed", n, 33), 0.5 * tgts[0]]
    index = [0, 1, 2, 0, 0]
    splits = [O.split_bin(fs, N, fs / 8), O.split_bin(fs, N, fs / 4), -1, N // 2, N // 2 + 1]
    bands = O.third_octave_bands(fs, N)
    for tdt, edt in ((np.float64, np.float64), (np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64)):
        c = O.Case(tgts, ests, index, N, H, bands=bands, splits=splits, tdt=tdt, edt=edt)
        got = run(c)
        worst = c.check(got, "%s/%s" % (np.dtype(tdt).name, np.dtype(edt).name))
        print(fs, N, H, np.dtype(tdt).name, np.dtype(edt).name, "worst spectrum %.3g, centroid %.3g bins, dB %.3g" % worst)
        pair = got[1]
        assert np.isnan(pair[2, [0, 1, 5]]).all() and np.isnan(pair[4, [0, 1, 5]]).all() and np.isfinite(pair[3]).all()
        if tdt == edt:                                            # 0.5 x target: every difference is exactly zero
            assert np.array_equal(pair[4, [2, 3, 4, 6, 7]], np.zeros(5))


@pytest.mark.parametrize("N,H", [(256, 256), (256, 128), (256, 1), (512, 200), (1024, 512), (2048, 1024)],
                         ids=["256-hopN", "256-half", "256-hop1", "512", "1024", "2048"])
def test_geometry_shapes_and_bit_level_properties(N, H):
    """The host file's batch (K = 0, 1, 2, 3, 31, 32, 33, 64, 65 segments, digital silence from an odd and from an even segment on,
    an all-zero and an empty signal; K = 1 and K = 3 estimates per target) against the oracle; a repeated call repeats the bits; a
    signal alone (n_est = 0) and a pair alone give the bits they give in the batch, so does the reversed batch, and ltas_out = NULL
    changes no bit of the other outputs."""
    splits = [N // 4, -1, N // 8, N // 2, 3, N // 4, N // 4, N // 4, N // 4]
    c = O.geometry_case(N, H, splits=splits, bands=[(2, 9), (10, 40), (41, N // 2)])
    got = run(c)
    worst = c.check(got, "N %d hop %d" % (N, H))
    print(N, H, "worst spectrum %.3g, centroid %.3g bins, dB %.3g" % worst)
    sig, pair, lt, _ = got
    n_t = len(c.tgts)
    assert np.isnan(sig[0]).all() and np.isnan(lt[0]).all() and np.isnan(sig[[11, 12]]).all() and np.isfinite(sig[1:11]).all()
    assert not np.any(lt[11]) and np.isnan(lt[12]).all() and np.isnan(pair[[6, 7, 8]]).all() and not np.isinf(pair).any()
    again = run(c)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:3], got[:3]))
    for i in (1, 4, 8, 10):
        alone = run(O.Case([c.tgts[i]], [], [], N, H, bands=c.bands))
        assert alone[0].tobytes() == sig[i:i + 1].tobytes() and alone[2].tobytes() == lt[i:i + 1].tobytes() and alone[1].shape == (0, 8), i
    for e in (0, 2, 5):
        one = run(O.Case([c.tgts[c.index[e]]], [c.ests[e]], [0], N, H, bands=c.bands, splits=[splits[e]], edt=np.float32))
        assert one[1].tobytes() == pair[e:e + 1].tobytes() and one[0][1].tobytes() == sig[n_t + e].tobytes(), e
    order = list(range(n_t))[::-1]
    back = run(O.Case([c.tgts[i] for i in order], c.ests[::-1], [n_t - 1 - t for t in c.index[::-1]], N, H, bands=c.bands, splits=splits[::-1],
                      edt=np.float32))
    assert back[0][:n_t][::-1].tobytes() == sig[:n_t].tobytes() and back[0][n_t:][::-1].tobytes() == sig[n_t:].tobytes()
    assert back[1][::-1].tobytes() == pair.tobytes() and back[2][n_t:][::-1].tobytes() == lt[n_t:].tobytes()
    off = run(c, ltas=False)
    assert off[0].tobytes() == sig.tobytes() and off[1].tobytes() == pair.tobytes()


def test_bands_band_tables_sine_and_the_empty_batch():
    """band with lo > 0 and hi < N / 2, the empty band, 1 and 40 analysis bands, rolloff and drop_db away from their defaults; the
    bin-centred sine and the silent estimate by their exact rules; an empty batch is an empty result."""
    N, H = 256, 128
    n = N + 50 * H
    tgts, ests = [O.white(n, 40), O.coloured(n, 41)], [O.lowpassed(n, 42, 0.6, -60.0), O.white(n, 43), O.coloured(n, 44, 0.5)]
    index, splits = [0, 0, 1], [50, 20, 127]
    forty = [(4 + 3 * i, 6 + 3 * i) for i in range(40)]
    for lo, hi, bands, rho, drop in ((0, N // 2, forty, 0.97, 60.0), (4, 123, forty, 0.5, 20.0), (10, 100, [(10, 100)], 0.999, 3.0),
                                     (17, 17, [(17, 17)], 0.97, 60.0)):
        c = O.Case(tgts, ests, index, N, H, lo=lo, hi=hi, rho=rho, drop=drop, bands=bands, splits=splits)
        worst = c.check(run(c), "band %d..%d" % (lo, hi))
        print(lo, hi, len(bands), "worst spectrum %.3g, centroid %.3g bins, dB %.3g" % worst)
    sig, pair, lt, _ = run(O.Case(tgts, ests, index, N, H, lo=9, hi=8, splits=splits))
    assert np.isnan(sig).all() and np.isnan(pair).all() and np.isfinite(lt).all()
    N, H, k0 = 512, 256, 40
    s = O.sine(N + 20 * H, N, k0)
    sig, pair, lt, _ = run(O.Case([s], [s.copy(), 0.5 * s, np.zeros(len(s))], [0, 0, 0], N, H, bands=[(30, 50), (200, 256)], splits=[200, 200, 200]))
    floor = 10.0 * math.log10(O.EPS)
    assert sig[0, 0] == k0 + 1 and abs(pair[0, 0] - floor) <= 1e-9 and abs(pair[0, 1] - floor) <= 1e-9
    assert np.array_equal(pair[:2, 2:], np.zeros((2, 6))) and np.isnan(pair[2, [0, 2, 3, 4, 5, 6, 7]]).all() and pair[2, 1] == pair[0, 1]
    assert np.isnan(sig[3]).all() and not np.isinf(pair).any()
    sig, pair, lt, _ = run(O.Case([], [], [], N, H))
    assert sig.shape == (0, 3) and pair.shape == (0, 8) and lt.shape == (0, N // 2 + 1)


def test_audio_metrics_single_batch_multi_and_resident_inputs():
    """AudioMetrics(16000): bandwidth() is the oracle's values in Hz; signals alone, with and without a split; float32 and float64
    signals mixed in one list give the bits of the single calls; the differences of y == x are exactly 0; K = 2 estimates per target
    with a split per key; device tensors give the bits of host arrays."""
    from ssr_eval_amd import AudioMetrics
    fs, N, H = 16000, 2048, 1024
    am = AudioMetrics(fs)
    hz = fs / N
    tgts = [O.white(52000, 50).astype(np.float32), O.coloured(49001, 51), O.white(30000, 52).astype(np.float32)]
    ests = [O.lowpassed(52000, 53, 0.5, -70.0), O.lowpassed(49001, 54, 0.25, -70.0).astype(np.float32), O.coloured(30000, 55).astype(np.float32)]
    bands = O.third_octave_bands(fs, N)
    d = am.bandwidth(ests[0], tgts[0], split_hz=5000.0, return_ltas=True)
    names = ("bw_hz", "edge_hz", "centroid_hz", "hf_db", "bw_diff", "edge_diff", "centroid_diff", "hf_diff", "ltas_dist", "ltas_max")
    assert list(d) == list(names) + ["ltas", "target_ltas"]
    dy, dx = (O.analyse(np.asarray(s, np.float64), N, H, bands=bands) for s in (ests[0], tgts[0]))
    O.assert_conditioned(np.asarray(ests[0], np.float64), N, H, bands=bands)
    want = O.pair_row(dy, dx, O.split_bin(fs, N, 5000.0), 0, N // 2)
    assert d["bw_hz"] == dy["roll"] * hz and d["edge_hz"] == dy["edge"] * hz and abs(d["centroid_hz"] - dy["centroid"] * hz) <= 1e-9 * fs
    assert d["bw_diff"] == want[2] * hz and d["edge_diff"] == want[3] * hz and abs(d["centroid_diff"] - want[4] * hz) <= 1e-9 * fs
    worst = max(abs(d[k] - w) for k, w in (("hf_db", want[0]), ("hf_diff", want[5]), ("ltas_dist", want[6]), ("ltas_max", want[7])))
    print("worst dB difference", worst, d)
    assert worst <= O.TOL_DB and 3500.0 < d["bw_hz"] < 4500.0 and d["hf_diff"] < -15.0
    assert np.max(np.abs(d["ltas"] * dy["K"] - dy["cp"])) <= 1e-9 * np.max(dy["cp"])
    t = am.bandwidth(tgts[0], split_hz=5000.0, return_ltas=True)
    assert list(t) == list(names[:4]) + ["ltas"] and t["ltas"].tobytes() == d["target_ltas"].tobytes()
    assert abs(t["hf_db"] - want[1]) <= O.TOL_DB and d["hf_diff"] == d["hf_db"] - t["hf_db"] and d["bw_diff"] == d["bw_hz"] - t["bw_hz"]
    plain = am.bandwidth(tgts[0])
    assert math.isnan(plain["hf_db"]) and all(plain[k] == t[k] for k in names[:3])
    same = am.bandwidth(tgts[1], tgts[1].copy(), split_hz=2000.0)
    assert all(same[k] == 0.0 for k in names[4:])
    short = am.bandwidth(tgts[0][:2047], tgts[0][:2047])
    assert all(math.isnan(short[k]) for k in names)
    bits = lambda q: np.array([q[k] for k in names if k in q]).tobytes()      # noqa: E731
    batch = am.bandwidth_batch(ests, tgts, split_hz=[4000.0, None, 1000.0])
    for i, s in enumerate((4000.0, None, 1000.0)):
        assert bits(batch[i]) == bits(am.bandwidth(ests[i], tgts[i], split_hz=s)), i
    assert math.isnan(batch[1]["hf_diff"]) and np.isfinite(batch[1]["ltas_dist"])
    assert am.bandwidth_batch(ests, tgts, names=("bw_hz", "ltas_dist"))[1] == {"bw_hz": batch[1]["bw_hz"], "ltas_dist": batch[1]["ltas_dist"]}
    alone = am.bandwidth_batch(ests + tgts)
    assert [bits(q)[:24] for q in alone[:3]] == [bits(q)[:24] for q in batch]
    by_key = [[ests[1], ests[2]], [ests[1][::-1].copy(), ests[2][::-1].copy()]]
    multi = am.bandwidth_multi(by_key, tgts[1:], split_hz=[2000.0, 3000.0])
    for i in range(2):
        for k in range(2):
            assert bits(multi[i][k]) == bits(am.bandwidth(by_key[k][i], tgts[1 + i], split_hz=(2000.0, 3000.0)[k])), (i, k)
    dev = am.bandwidth_batch([torch.from_numpy(np.ascontiguousarray(e)).to(DEV) for e in ests], [torch.from_numpy(a).to(DEV) for a in tgts],
                             split_hz=[4000.0, None, 1000.0], resident=True)
    assert [bits(q) for q in dev] == [bits(q) for q in batch]


# ---- where the kernels touch memory ---------------------------------------------------------------------------------------------
def _case(tdt, edt, N=256, H=128):
    c = O.geometry_case(N, H, tdt=tdt, edt=edt, splits=[N // 4, -1, N // 8, N // 2, 3, N // 4, N // 4, N // 4, N // 4],
                        bands=[(2, 9), (10, 40), (41, N // 2)])
    keep = [e for e, t in enumerate(c.index) if len(c.tgts[t])]                       # (an arena view needs a sample)
    tgts = [t for t in c.tgts if len(t)]
    remap = {id(t): i for i, t in enumerate(tgts)}
    return O.Case(tgts, [c.ests[e] for e in keep], [remap[id(c.tgts[c.index[e]])] for e in keep], N, H, bands=c.bands,
                  splits=[c.splits[e] for e in keep], tdt=tdt, edt=edt)


@pytest.mark.parametrize("placement", ["odd", "quad"])
@pytest.mark.parametrize("tdt,edt", [(np.float32, np.float32), (np.float64, np.float32), (np.float64, np.float64)], ids=["f32", "f64-f32", "f64"])
@pytest.mark.parametrize("with_ltas", [True, False], ids=["ltas_out", "null"])
def test_guard_bands_and_poison(monkeypatch, tdt, edt, placement, with_ltas):
    """ssr_spectrum on separate device tensors, then on views into NaN-filled arenas with sig_out, pair_out, ltas_out and the
    workspace between 0xFF guard bands and 0xFF inside: the same bits, no guard damaged, no arena written, the signals read where
    they lie, and NaN only where the oracle's rules put it (a read outside a signal or of an unwritten workspace byte would be NaN)."""
    gaps = {"odd": G.GAPS_ODD, "quad": G.GAPS_QUAD}[placement]
    c = _case(tdt, edt)
    to_dev = lambda arrays: [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]      # noqa: E731
    plain = run(c, with_ltas, lambda t, e: (to_dev(t), to_dev(e)))
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        got = run(c, with_ltas, lambda t, e: (g.arena(t, gaps, torch.from_numpy(t[0]).dtype, DEV)[0], g.arena(e, gaps, torch.from_numpy(e[0]).dtype, DEV)[0]))
        assert len(g.blocks) >= (4 if with_ltas else 3)                    # sig_out, pair_out, ltas_out and the workspace
        assert len(g.arenas) == 2 and g.read_in_place()
        g.check()
    G.assert_same_bits(list(plain[:3 if with_ltas else 2]), list(got[:3 if with_ltas else 2]), "spectrum")
    c.check(got, "guarded")
    # signals alone: est, est_off, tgt_index, split and pair_out are NULL
    solo = O.Case(c.tgts, [], [], c.N, c.H, bands=c.bands, tdt=tdt)
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        alone = run(solo, with_ltas, lambda t, e: (g.arena(t, gaps, torch.from_numpy(t[0]).dtype, DEV)[0], []))
        assert g.arenas and g.read_in_place()
        g.check()
    assert alone[0].tobytes() == got[0][:len(c.tgts)].tobytes()


def test_one_byte_less_than_reported_is_refused(monkeypatch):
    """With ssr_spectrum_workspace_bytes reporting one byte less than it should the call is SSR_ERR_WORKSPACE and nothing is
    enqueued: the outputs and the workspace still hold only 0xFF."""
    bk = B()
    lib = bk._lib.load()
    real = lib.ssr_spectrum_workspace_bytes
    asked = []

    def one_less(*a):
        n = int(real(*a))
        assert n > 0
        asked.append(n)
        return n - 1
    c = _case(np.float32, np.float32)
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        m.setattr(lib, "ssr_spectrum_workspace_bytes", one_less)
        with pytest.raises(bk.SsrHipError, match=r"libssrhip error -4\b"):
            run(c, True, lambda t, e: (g.arena(t, G.GAPS_ODD, torch.float32, DEV)[0], g.arena(e, G.GAPS_ODD, torch.float32, DEV)[0]))
        assert asked
        g.check()
        assert g.untouched_payloads(("backend.py:put", "backend.py:_uniform_images")) == []


# ---- SSR_Eval_Helper(bandwidth=True) ---------------------------------------------------------------------------------------------
FS = 16000
LENGTHS = {"p360": (8000, 8411, 9100, 12000), "p361": (9001, 9600, 8192, 10001)}
BW = ("bw_hz", "bw_diff", "hf_diff", "ltas_dist")


def _bits(v):
    return np.float64(v).tobytes()                                        # NaN equals NaN


def _write_tree(root):
    """Two speakers x four files: a 220 Hz tone with two harmonics plus noise (the tree of tests/test_gpu_loudness.py, eight files)."""
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(12)
    for spk, lens in LENGTHS.items():
        (root / spk).mkdir(parents=True)
        for i, n in enumerate(lens):
            t = np.arange(n) / FS
            x = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.1 * np.sin(2 * np.pi * 440 * t) + 0.05 * np.sin(2 * np.pi * 1760 * t)
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), (x + 0.02 * rng.standard_normal(n)).astype(np.float32), FS)


def test_evaluate_with_bandwidth(tmp_path):
    """evaluate() on the eight-file 16 kHz tree with two FFT keys: the four keys appear in full_key_order() order behind the other
    families', the values are AudioMetrics.bandwidth_multi's on the same arrays, and with the option off the result is what it is
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
    on, both, loud, none = go(bandwidth=True), go(bandwidth=True, loudness=True), go(loudness=True), go()
    assert go(bandwidth=None) == none
    keys = ["proc_fft_%d_%d" % (2 * c, FS) for c in cutoffs]
    order, before = full_key_order(), all_key_order()
    at = order.index("bw_hz")
    assert order[:len(before)] == before and order[at:at + 4] == BW and at > order.index("true_peak_diff")
    am = AudioMetrics(FS)
    files, tgts, by_key = [], [], [[], []]
    for spk in LENGTHS:
        for fn in sorted(on[spk]):
            x, _ = read_audio(str(root / spk / fn))
            files.append((spk, fn))
            tgts.append(np.asarray(x, np.float32))
            for k, cut in enumerate(cutoffs):
                by_key[k].append(np.asarray(lowpass(x, cut, FS, order=1, _type="stft_hard"), np.float32))
    want = am.bandwidth_multi(by_key, tgts, split_hz=[float(c) for c in cutoffs], names=BW)
    assert len(files) == 8
    for i, (spk, fn) in enumerate(files):
        assert list(on[spk][fn]) == keys
        for k, key in enumerate(keys):
            d, b = on[spk][fn][key], both[spk][fn][key]
            assert list(d) == list(order[:4]) + list(BW) and list(b) == [m for m in order if m in b] and list(b)[-4:] == list(BW)
            assert list(none[spk][fn][key]) == list(order[:4])
            for m in BW:
                print(spk, fn, key, m, d[m])
                assert _bits(d[m]) == _bits(b[m]) == _bits(want[i][k][m]), (spk, fn, key, m, d[m], b[m], want[i][k][m])
            for m in order[:4]:
                assert _bits(d[m]) == _bits(none[spk][fn][key][m]), (spk, fn, key, m)
            for m in loud[spk][fn][key]:
                assert _bits(b[m]) == _bits(loud[spk][fn][key][m]), (spk, fn, key, m)
            assert all(np.isfinite(d[m]) for m in BW) and d["bw_diff"] < 0.0 and d["hf_diff"] < -10.0 and d["ltas_dist"] > 1.0, (spk, fn, key, d)
    for key in keys:
        assert list(on["averaged"][key]) == list(order[:4]) + list(BW)
        for spk in LENGTHS:
            assert list(on["each_speaker"][spk][key]) == list(order[:4]) + list(BW)
