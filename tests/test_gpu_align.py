"""GPU tests (-m gpu) of the delay stage (backend.align, AudioMetrics.align*, SSR_Eval_Helper(align=...)) against
the NumPy float64 oracle (tests/align_oracle.py).

Bars (set by the issue; the reasons are its own): c within 1e-10 sqrt(Ex Ey) of the oracle - n 2^-53 sum|x y| with Cauchy-Schwarz at
n <= 2^20, the sizes here sit 25x inside; d* and edge equal wherever the oracle's peak leads its runner-up by more than 2e-10 sqrt(Ex
Ey) - twice the bar on c -, and the inputs (align_oracle.geometry_batch: a faint independent noise on every estimate) make that hold
for every pair, which is asserted; frac within 1e-8 wherever the oracle's denominator is at least 1e-3 c[d*], which every non-edge pair
is asserted to meet; corr within 1e-10; the integer-mode output bit-identical to NumPy slicing; the fractional-mode output within
1e-12 max|y| (float64) or one float32 ulp of max|y| (float32) of the oracle's filter at the frac the kernel reported."""
import functools

import numpy as np
import pytest
import torch

import align_oracle as O
import guarded as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


def B():
    from ssr_eval_amd import backend
    return backend


def host(shifted):
    return [z.cpu().numpy() for z in shifted]


def check_pair(x, y, L, row, z, c, subsample, ref):
    """One pair against the oracle dict `ref` at the bars above; -> (d* was compared, the parabola was compared)."""
    s = ref["scale"]
    assert np.max(np.abs(c - ref["c"])) <= 1e-10 * s, ("c", np.max(np.abs(c - ref["c"])), s)
    if not (ref["degenerate"] or ref["margin"] > 2e-10 * s):
        return False, False
    assert (row[0], row[3]) == (ref["delay"], ref["edge"]), (row, ref["delay"], ref["edge"])
    if ref["degenerate"]:
        assert np.isnan(row[2]) and row[1] == 0.0 and z.dtype == y.dtype and z.tobytes() == y.tobytes()
        return True, False
    assert abs(row[2] - ref["corr"]) <= 1e-10
    parabola = False
    if not ref["edge"]:
        assert abs(ref["den"]) >= 1e-3 * ref["c"][ref["delay"] + L], "the input does not qualify for the parabola's bar"
        assert abs(row[1] - ref["frac"]) <= 1e-8, (row[1], ref["frac"])
        parabola = True
    else:
        assert row[1] == 0.0
    if not subsample or row[1] == 0.0:
        assert z.dtype == y.dtype and z.tobytes() == O.shift(y, ref["delay"]).tobytes()
    else:
        zo = O.shift(y, ref["delay"], row[1])
        peak = float(np.max(np.abs(y)))
        bar = 1e-12 * peak if y.dtype == np.float64 else float(np.spacing(np.float32(peak)))
        assert z.dtype == y.dtype and np.max(np.abs(z.astype(np.float64) - zo.astype(np.float64))) <= bar
    return True, parabola


@functools.lru_cache(maxsize=None)
def geometry(L, kind):
    """The batch of one lag count and dtype combination and its oracle dicts, made once."""
    tdt, edt = {"f32": (np.float32, np.float32), "f64": (np.float64, np.float64)}[kind]
    tgts, ests, idx = O.geometry_batch(L, tdt, edt)
    return tgts, ests, idx, [O.estimate(tgts[i], e, L) for e, i in zip(ests, idx)]


@pytest.mark.parametrize("kind", ["f32", "f64"])
@pytest.mark.parametrize("L", O.LAGS)
def test_geometry_batches_match_the_oracle(L, kind):
    """Per lag count (around a lane's 8 lags and a block's 2048) one ragged batch: targets of 1, 7, L - 1, L + 1, 16383, 16384, 16385
    and 40000 samples, two estimates each (the second longer or shorter than its target) with true delays 0, +-1, +-37, +-(L - 1),
    +-L and L + 5 in turn, in integer and in fractional mode."""
    tgts, ests, idx, refs = geometry(L, kind)
    assert len(set(idx)) == len(tgts) and all(idx.count(i) == 2 for i in set(idx))
    for sub in (False, True):
        rows, shifted, c = B().align(tgts, ests, idx, max_lag=L, subsample=sub, return_corr=True)
        assert rows.shape == (len(ests), 4) and c.shape == (len(ests), 2 * L + 1) and len(shifted) == len(ests)
        got = [check_pair(tgts[idx[e]], ests[e], L, rows[e], z, c[e], sub, refs[e]) for e, z in enumerate(host(shifted))]
        assert all(g[0] for g in got)                                       # no pair is exempt
        assert sum(g[1] for g in got) == sum(1 for r in refs if not r["edge"] and not r["degenerate"]) > 0
        assert {int(r[3]) for r in rows} == {0, 1}


def test_mixed_dtype_lists_and_three_estimates_of_one_target():
    """float32 and float64 side by side on both sides: targets are widened, every estimate comes back in its own dtype; three
    estimates with different delays name one target."""
    L = 300
    x = O.lowpassed(O.TILE + 77, 1)
    tgts = [x.astype(np.float32), O.noise(5000, 2)]
    ests = [O.delayed(x, 5).astype(np.float32), O.delayed(x, -200, O.TILE + 500), O.delayed(x, 299, O.TILE).astype(np.float32),
            O.delayed(tgts[1], -41, 4000).astype(np.float32), O.delayed(tgts[1], 40, 6000)]
    idx = [0, 0, 0, 1, 1]
    for sub in (False, True):
        rows, shifted, c = B().align(tgts, ests, idx, L, sub, return_corr=True)
        assert list(rows[:, 0]) == [5, -200, 299, -41, 40]
        for e, z in enumerate(host(shifted)):
            x64 = tgts[idx[e]].astype(np.float64)
            assert all(check_pair(x64, ests[e], L, rows[e], z, c[e], sub, O.estimate(x64, ests[e], L))[:1])
    # return_corr changes no bit, and deferred results are the immediate ones
    r0, s0, none = B().align(tgts, ests, idx, L, True)
    assert none is None and r0.tobytes() == rows.tobytes() and G.bits(s0) == G.bits(shifted)
    r1, s1, c1 = B().align(tgts, ests, idx, L, True, return_corr=True, deferred=True)
    assert r1().tobytes() == rows.tobytes() and c1().tobytes() == c.tobytes() and G.bits(s1) == G.bits(shifted)
    r2, s2, _ = B().align(tgts, ests, idx, L, shift=False)
    assert s2 is None and r2.tobytes() == rows.tobytes()
    r3, s3, _ = B().align(tgts, [], [], L)
    assert r3.shape == (0, 4) and s3 == []


def test_silence_empty_and_negated_pairs():
    """Digital silence or no sample on either side, and y = -x inside the span where x's autocorrelation is positive: delay 0, frac
    0, edge 0, NaN corr, the estimate unchanged bit for bit."""
    x = O.lowpassed(3000, 9).astype(np.float32)
    zero = np.zeros(3000, np.float32)
    tgts, ests, idx = [x, zero, x[:0]], [zero, x, -x, x, x[:0]], [0, 1, 0, 2, 0]
    for sub in (False, True):
        rows, shifted, c = B().align(tgts, ests, idx, 4, sub, return_corr=True)
        for e, z in enumerate(host(shifted)):
            ref = O.estimate(tgts[idx[e]], ests[e], 4)
            assert ref["degenerate"]
            assert check_pair(tgts[idx[e]], ests[e], 4, rows[e], z, c[e], sub, ref)[0]
            assert rows[e][0] == 0 and rows[e][1] == 0 and np.isnan(rows[e][2]) and rows[e][3] == 0
    # all of a call's estimates empty: nothing to shift
    rows, shifted, _ = B().align([x], [x[:0], x[:0]], [0, 0], 8)
    assert np.isnan(rows[:, 2]).all() and [len(z) for z in shifted] == [0, 0]


def big_batch():
    """2 * 256 + 3 pairs: lengths in a cycle of period 7 from 1 sample to a tile and 5, runs of 1 to 3 estimates per target, delays in
    a cycle of period 11, every third estimate longer than its target."""
    lens = (1, 300, 777, 2048, 2049, 5000, O.TILE + 5)
    delays = (0, 1, -1, 7, -8, 37, -37, 63, -64, 64, 70)
    tgts, ests, idx = [], [], []
    while len(ests) < 515:
        t = len(tgts)
        x = O.lowpassed(lens[t % 7], 1000 + t).astype(np.float32)
        tgts.append(x)
        for _ in range(1 + t % 3):
            e = len(ests)
            if e < 515:
                m = len(x) + (9 if e % 3 == 0 else 0)
                ests.append((O.delayed(x.astype(np.float64), delays[e % 11], m) + 1e-3 * O.noise(m, 5000 + e)).astype(np.float32))
                idx.append(t)
    return tgts, ests, idx


@pytest.mark.parametrize("sub", [False, True], ids=["integer", "fractional"])
def test_a_pair_alone_is_its_row_in_a_batch_of_515(sub):
    tgts, ests, idx = big_batch()
    assert len(ests) == 2 * 256 + 3
    rows, shifted, c = B().align(tgts, ests, idx, 64, sub, return_corr=True)
    shifted = host(shifted)
    again = B().align(tgts, ests, idx, 64, sub, return_corr=True)
    assert again[0].tobytes() == rows.tobytes() and again[2].tobytes() == c.tobytes() and G.bits(again[1]) == G.bits(shifted)
    for e in (0, 1, 255, 256, 257, 300, 513, 514):
        r1, s1, c1 = B().align([tgts[idx[e]]], [ests[e]], [0], 64, sub, return_corr=True)
        assert r1[0].tobytes() == rows[e].tobytes() and c1[0].tobytes() == c[e].tobytes(), e
        assert s1[0].cpu().numpy().tobytes() == shifted[e].tobytes(), e
        ref = O.estimate(tgts[idx[e]], ests[e], 64)
        check_pair(tgts[idx[e]], ests[e], 64, rows[e], shifted[e], c[e], sub, ref)


# ---- guard bands and poison ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gaps", [G.GAPS_ODD, G.GAPS_QUAD], ids=["odd", "quad"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_guard_bands_and_poison(monkeypatch, dtype, gaps):
    """ssr_align on separate device tensors, then on views into NaN-filled arenas with rows, c, the shifted signals and the workspace
    (exactly ssr_align_workspace_bytes) between 0xFF guard bands and 0xFF inside: the same bits, no guard damaged, no arena written,
    every output finite (corr apart: NaN for the silent pair, and for a pair whose delay lies outside a search of one lag)."""
    bk = B()
    x = [O.lowpassed(n, 40 + n).astype(dtype) for n in (1, 2, 700, O.TILE + 3)]
    idx = [0, 1, 2, 3, 3, 2]
    ds = [0, 1, -37, 64, -65, 5]
    est = [O.delayed(x[i], d, len(x[i]) + k).astype(dtype) for k, (i, d) in enumerate(zip(idx, ds))]
    est[5] = np.zeros_like(est[5])                                            # silence: NaN corr, the estimate unchanged
    for L, sub in ((64, False), (64, True), (2049, True), (1, False)):
        def call(put):
            return bk.align(put(x), put(est), idx, L, sub, return_corr=True)
        plain = G.bits(call(lambda arrays: [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]))
        torch.cuda.synchronize()
        with monkeypatch.context() as m:
            g = G.Guarded().route(m)
            got = call(lambda arrays: g.arena(arrays, gaps, torch.from_numpy(arrays[0]).dtype, DEV)[0])
            assert len(g.blocks) >= 4                                         # rows, c, the shifted signals, the workspace
            assert len(g.arenas) == 2 and g.read_in_place()
            g.check()
            got = G.bits(got)
        G.assert_same_bits(plain, got, ("align", L, sub))
        arrays = [np.frombuffer(b, np.dtype(d)).reshape(s) for s, d, b in got]
        rows = arrays[0]
        assert np.isfinite(np.delete(rows, 2, axis=1)).all() and np.isnan(rows[5, 2]) and np.isfinite(rows[:2, 2]).all()
        assert all(np.isfinite(a).all() for a in arrays[1:])


# ---- AudioMetrics -------------------------------------------------------------------------------------------------------------------
def test_audio_metrics_align_delay_batch_and_multi():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(16000)
    x = O.lowpassed(9000, 3).astype(np.float32)
    y = O.delayed(x, 37)
    z, d = am.align(y, x)
    assert list(d) == ["delay", "delay_frac", "align_corr", "align_edge"] and d["delay"] == 37.0 and d["align_edge"] == 0.0 and d["align_corr"] > 0.99
    assert isinstance(z, np.ndarray) and z.dtype == np.float32 and z.tobytes() == O.shift(y, 37).tobytes()
    assert am.delay(y, x) == d and am.delay(y, x, max_lag=37)["align_edge"] == 1.0
    late = O.delayed(x, -20).astype(np.float64)
    aligned, dicts = am.align_batch([y, late], [x, x], max_lag=64)
    assert [q["delay"] for q in dicts] == [37.0, -20.0] and aligned[1].dtype == np.float64 and aligned[0].tobytes() == z.tobytes()
    by_key, rows = am.align_multi([[y, late.astype(np.float32)], [late.astype(np.float32), y]], [x, x], max_lag=64, resident=True, deferred=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for k in by_key for t in k)
    assert [[q["delay"] for q in r] for r in rows()] == [[37.0, -20.0], [-20.0, 37.0]]
    assert by_key[0][0].cpu().numpy().tobytes() == z.tobytes() and by_key[1][1].cpu().numpy().tobytes() == z.tobytes()


def test_subsample_takes_out_a_fractional_delay():
    """37 samples and a two-tap FIR (0.6, 0.4), 0.4 of a sample more: the delay found lies inside (37, 38) and si_sdr after the
    fractional shift exceeds the whole-sample shift's.  A direction check, not a bar: the parabola is a biased estimate."""
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(16000)
    x = O.lowpassed(20000, 77, width=17)
    y = np.convolve(O.delayed(x, 37), [0.6, 0.4])[:20000]
    z_int, d_int = am.align(y, x, max_lag=128)
    z_sub, d_sub = am.align(y, x, max_lag=128, subsample=True)
    assert d_int == d_sub and d_int["delay"] == 37.0 and 0.0 < d_int["delay_frac"] < 0.5
    s_int, s_sub = am.si_sdr(z_int, x), am.si_sdr(z_sub, x)
    print("si_sdr after the whole-sample shift %.2f dB, after the fractional shift %.2f dB, delay %.4f" % (s_int, s_sub, 37 + d_sub["delay_frac"]))
    assert s_sub > s_int


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
FS = 16000
REFERENCE = ("lsd", "log_sispec", "sispec", "ssim")
LENGTHS = {"p360": (8000, 8411, 9001), "p361": (9600, 10240, 11111), "p362": (12800, 14399)}
SETTINGS = lambda: dict(setting_fft={"cutoff_freq": [2000, 3000]},      # noqa: E731
                        setting_lowpass_filtering={"cutoff_freq": [2000], "filter_order": [4], "filter": ["butter", "ellip"]})
KEYS = {"proc_bw_4000_4_16000": (2000, "butter", 4), "proc_el_4000_4_16000": (2000, "ellip", 4),
        "proc_fft_4000_16000": (2000, "stft_hard", 1), "proc_fft_6000_16000": (3000, "stft_hard", 1)}
LATE = 37


def bits(v):
    return [(k, bits(x)) for k, x in v.items()] if isinstance(v, dict) else np.float64(v).tobytes()


def write_tree(root):
    """A tree shaped like tests/test_gpu_every_family.py's - 16 kHz, eight wav files over three speakers, 0.5 to 0.9 s, no two
    lengths alike - of low-passed noise under a stepped level: a correlation with one peak."""
    from ssr_eval_amd.io import write_wav
    gains = (1.0, 0.5, 1.0, 0.1)
    for s, (spk, lens) in enumerate(LENGTHS.items()):
        (root / spk).mkdir(parents=True)
        for i, n in enumerate(lens):
            env = np.array(gains)[(np.arange(n) // (FS // 10)) % len(gains)]
            x = 0.3 * env * O.lowpassed(n, 10 * s + i, width=33) / 0.4 + 0.005 * O.noise(n, 100 + 10 * s + i)
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), x.astype(np.float32), FS)


class Tree:
    def __init__(self, root):
        self.root, self.runs = root, {}

    def helper(self, late, **options):
        from ssr_eval_amd import SSR_Eval_Helper, BasicTestee

        class Late(BasicTestee):
            """Returns its input LATE samples late: a zero head, the same length and dtype."""
            def infer(self, x):
                y = np.zeros_like(x)
                y[LATE:] = x[:-LATE]
                return y
        return SSR_Eval_Helper(Late() if late else BasicTestee(), test_name="t", input_sr=FS, output_sr=FS, evaluation_sr=FS,
                               test_data_root=str(self.root), **SETTINGS(), **options)

    def run(self, late, batch_files=None, **options):
        tag = (late, batch_files, repr(sorted(options.items())))
        if tag not in self.runs:
            self.runs[tag] = self.helper(late, **options).evaluate(save_json=False, batch_files=batch_files)
        return self.runs[tag]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("align") / "vctk_test"
    write_tree(root)
    return Tree(root)


FAMILIES = {"waveform": True, "phase": True}


def entries(result):
    return [(spk, fn, key, d) for spk in LENGTHS for fn, by_key in result[spk].items() for key, d in by_key.items()]


def test_evaluate_takes_out_a_late_testees_delay(tree):
    from ssr_eval_amd import AudioMetrics
    from ssr_eval_amd.eval import ALIGN_KEYS, _ALL_FAMILIES
    from ssr_eval_amd.io import read_audio
    from ssr_eval_amd.lowpass import lowpass
    on, off = tree.run(True, align=True, **FAMILIES), tree.run(True, **FAMILIES)
    fam_keys = [k for f in _ALL_FAMILIES if f.option in FAMILIES for k in f.keys]
    seen = 0
    for (spk, fn, key, d), (_, _, _, u) in zip(entries(on), entries(off)):
        assert list(d) == list(REFERENCE) + fam_keys + list(ALIGN_KEYS) and list(u) == list(REFERENCE) + fam_keys
        assert d["delay"] == LATE and d["align_corr"] > 0.99, (spk, fn, key, d["delay"], d["align_corr"])
        assert d["snr"] > u["snr"], (spk, fn, key, d["snr"], u["snr"])
        seen += 1
    assert seen == 8 * len(KEYS)
    for block in (on["averaged"], on["each_speaker"]["p361"]):
        for key in KEYS:
            assert list(block[key]) == list(REFERENCE) + fam_keys + list(ALIGN_KEYS) and block[key]["delay"] == LATE
    # every value is the direct AudioMetrics call on the NumPy-shifted output
    am = AudioMetrics(FS)
    files = [(spk, fn) for spk in LENGTHS for fn in on[spk]]
    tgts = [np.asarray(read_audio(str(tree.root / spk / fn))[0], np.float32) for spk, fn in files]
    for key, (cut, kind, order) in KEYS.items():
        outs = [np.asarray(lowpass(x, cut, FS, order=order, _type=kind), np.float32 if kind == "stft_hard" else np.float64) for x in tgts]
        outs = [O.shift(O.delayed(y, LATE), LATE) for y in outs]              # the testee's output, then the stage's copy
        want = [dict(a, **b, **c) for a, b, c in zip(am.evaluation_batch(outs, tgts), am.waveform_batch(outs, tgts), am.phase_distance_batch(outs, tgts))]
        for (spk, fn), w in zip(files, want):
            for m in list(REFERENCE) + fam_keys:
                assert bits(on[spk][fn][key][m]) == bits(w[m]), (key, spk, fn, m, on[spk][fn][key][m], w[m])
    # the files per batch change nothing
    for b in (1, 3):
        assert bits(tree.run(True, batch_files=b, align=True, **FAMILIES)) == bits(on), b
    # the dict form and a narrower search that still holds the delay: the same delay; save_processed_result keeps the aligned output
    h = tree.helper(True, align={"max_lag": 64}, save_processed_result=False)
    spk, fn = files[0]
    one = h.evaluate_single(str(tree.root / spk / fn))
    assert all(one[key]["delay"] == LATE and bits(one[key]["lsd"]) == bits(on[spk][fn][key]["lsd"]) for key in KEYS)


def test_evaluate_with_a_punctual_testee_and_without_the_option(tree):
    from ssr_eval_amd.eval import ALIGN_KEYS, _ALL_FAMILIES
    fam_keys = [k for f in _ALL_FAMILIES if f.option in FAMILIES for k in f.keys]
    on, off = tree.run(False, align=True, **FAMILIES), tree.run(False, **FAMILIES)
    explicit = tree.run(False, align=None, **FAMILIES)
    assert bits(explicit) == bits(off)
    for (spk, fn, key, d), (_, _, _, u) in zip(entries(on), entries(off)):
        assert list(u) == list(REFERENCE) + fam_keys                          # without the option: the keys of today
        assert d["delay"] == 0 and d["align_corr"] > 0.9
        rest = {m: v for m, v in d.items() if m not in ALIGN_KEYS}
        assert bits(rest) == bits(u), (spk, fn, key)
    for key in KEYS:
        assert list(off["averaged"][key]) == list(REFERENCE) + fam_keys
    # a sub-sample search on a punctual testee stays inside half a sample
    sub = tree.run(False, align={"subsample": True, "max_lag": 16})
    assert all(abs(d["delay"]) <= 0.5 for _, _, _, d in entries(sub))
