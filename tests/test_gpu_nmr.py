"""GPU tests (-m gpu) of the noise-to-mask family (ssr_nmr): the comparisons of tests/test_nmr_host.py on the
device, against the float64 oracle (tests/nmr_oracle.py) with the same bars - M within 1e-9 relative, Pn within 1e-9 of the frame's
largest G W2 |X|^2, every dB column within 1e-6 dB, frames equal, rdf equal under the oracle's own margin assertion - at the smallest
shapes that can go wrong: lengths N - 1 (NaN), N (one frame) and 33 N / 2 + N + 7 (two chunks: the seam at frame 32) plus an odd
frame count behind the seam (the half-filled last transform), N = 256 at 8 kHz and N = 2048 at 48 kHz, the dtype mixes, one target
shared by three estimates with three splits, y == x; every device buffer of ssr_nmr between guard bands, on poisoned inputs, and the
one-byte-less workspace; AudioMetrics.nmr / _batch / _multi / masking_threshold; SSR_Eval_Helper(nmr=...) on a three-file wav tree.
Worst differences seen on an MI355X: see DESIGN.md section 28."""
import numpy as np
import pytest
import torch

import guarded as G
import nmr_oracle as O
from test_nmr_host import DTYPES, DTYPE_IDS, check, design, split_bands

pytestmark = pytest.mark.gpu

DEV = "cuda"
FR = O.FR


def B():
    from ssr_eval_amd import backend
    return backend


class Dev:
    pass


def run(tgts, ests, idx, fs, N=None, splits=None, with_bands=True, with_mask=True, level_db=92.0):
    """-> out [n_est, 6], bands [n_est, Nc] or None, M per target [K, Nc] or None, as run_emu of the host file."""
    N = design(fs, N, level_db)["N"]
    r = Dev()
    r.out, r.bands, M = B().nmr_metrics(tgts, ests, idx, fs, N, level_db, split_bands(fs, N, splits, len(ests), level_db), with_bands, with_mask)
    edges = np.concatenate(([0], np.cumsum([O.frames(len(t), N) for t in tgts])))
    r.M = [M[edges[i]:edges[i + 1]] for i in range(len(tgts))] if with_mask else None
    return r


def _shapes(fs, N, dt):
    """Targets of N - 1, N, 33 N / 2 + N + 7 samples (K = 0, 1, 34) and of FR + 1 and FR + 3 frames; the K = 34 one has three
    estimates with three splits, the last of them the target itself."""
    lens = [N - 1, N, 33 * N // 2 + N + 7, O.len_for_frames(FR + 1, N, 3), O.len_for_frames(FR + 3, N, 0)]
    xs = [O.music_like(n, fs, 300 + i) for i, n in enumerate(lens)]
    tg = [x.astype(dt[0]) for x in xs]
    idx = [0, 1, 2, 2, 2, 3, 4]
    ests = [O.noisy(xs[0], 30.0, 1), O.noisy(xs[1], 30.0, 2), O.noisy(xs[2], 30.0, 3), O.clipped(xs[2]), xs[2], O.noisy(xs[3], 40.0, 4),
            O.clipped(xs[4])]
    ests = [y.astype(dt[1]) for y in ests]
    if dt[0] == np.float32:
        ests[4] = tg[2].astype(dt[1])                                        # y == x bit for bit in every mix that can hold it
    splits = [fs / 8.0, fs / 8.0, fs / 16.0, None, fs / 4.0, 1e9, 50.0]
    return tg, ests, idx, splits


@pytest.mark.parametrize("fs,N", [(8000, 256), (48000, 2048)])
@pytest.mark.parametrize("dt", DTYPES, ids=DTYPE_IDS)
def test_shapes_dtype_mixes_and_bit_level_properties(fs, N, dt):
    tg, ests, idx, splits = _shapes(fs, N, dt)
    r = run(tg, ests, idx, fs, N, splits)
    w = check(r, tg, ests, idx, fs, N, splits, what="shapes %d %s" % (fs, dt))
    print("worst so far: M %.3g relative, Pn %.3g of the frame's peak, a dB column %.3g dB" % (w["M"], w["Pn"], w["dB"]))
    assert r.out[:, 5].tolist() == [0, 1, 34, 34, 34, FR + 1, FR + 3] and np.isnan(r.out[0, :5]).all() and not np.isinf(r.out).any()
    if dt != (np.float64, np.float32):
        assert r.out[4].tolist() == [-200.0, -200.0, 0.0, -200.0, -200.0, 34.0] and np.all(r.bands[4] == 0.0)
    assert np.isnan(r.out[3, 3:5]).all() and np.isnan(r.out[5, 3]) and np.isfinite(r.out[5, 4]) and np.isnan(r.out[6, 4]) and np.isfinite(r.out[6, 3])
    again = run(tg, ests, idx, fs, N, splits)
    assert again.out.tobytes() == r.out.tobytes() and again.bands.tobytes() == r.bands.tobytes()
    for e in (1, 3, 6):                                                      # alone = in the batch; one estimate or three: the same mask
        a = run([tg[idx[e]]], [ests[e]], [0], fs, N, [splits[e]])
        assert a.out.tobytes() == r.out[e:e + 1].tobytes() and a.bands.tobytes() == r.bands[e:e + 1].tobytes(), e
        assert a.M[0].tobytes() == r.M[idx[e]].tobytes()
    order = list(range(len(ests)))[::-1]
    b = run(tg, [ests[e] for e in order], [idx[e] for e in order], fs, N, [splits[e] for e in order])
    assert b.out[::-1].tobytes() == r.out.tobytes() and b.bands[::-1].tobytes() == r.bands.tobytes()
    assert run(tg, ests, idx, fs, N, splits, with_bands=False, with_mask=False).out.tobytes() == r.out.tobytes()


def test_one_frame_pairs_give_pn_and_the_empty_batch():
    """On a one-frame pair mean_t R is R of that frame: Pn = R M within 1e-9 of the frame's largest weighted power."""
    fs, N = 16000, 512
    d = design(fs, N)
    xs = [O.music_like(N + e, fs, 330 + e) for e in (0, 1, 255)]
    ys = [O.noisy(x, 30.0, 5 + i) for i, x in enumerate(xs)]
    r = run(xs, ys, [0, 1, 2], fs, N)
    check(r, xs, ys, [0, 1, 2], fs, N, what="one frame")
    for i, (x, y) in enumerate(zip(xs, ys)):
        peak = (d["G"] * d["W2"] * np.abs(O.stft(x, N)[0]) ** 2).max()
        err = float(np.max(np.abs(r.bands[i] * r.M[i][0] - O.noise(x, y, d)[0])) / peak)
        print("one-frame pair %d: Pn within %.3g of the frame's peak" % (i, err))
        assert err <= O.TOL_REL
    e = run(xs, [], [], fs, N)
    assert e.out.shape == (0, 6) and e.bands.shape == (0, d["Nc"])


def test_audio_metrics_single_batch_multi_resident_and_masking_threshold():
    """AudioMetrics(16000): the dict of nmr() is the oracle's; _batch and _multi give the bits of the single call, per-pair and
    per-key split frequencies included; device tensors give the bits of host arrays; masking_threshold is the oracle's mask in dB."""
    from ssr_eval_amd import AudioMetrics
    fs = 16000
    am = AudioMetrics(fs)
    d = design(fs)
    xs = [O.music_like(n, fs, 20 + i) for i, n in enumerate((9000, 12000, 10007))]
    tgts = [x.astype(np.float32) for x in xs]
    ests = [O.noisy(x, 28.0 + i, 30 + i).astype(np.float32 if i != 1 else np.float64) for i, x in enumerate(xs)]
    q = am.nmr(ests[0], tgts[0], split_hz=3000, return_bands=True)
    assert list(q) == ["nmr", "nmr_seg", "rdf", "nmr_hf", "nmr_lf", "band_ratio", "centre_hz", "frames"]
    want, bands, frame_db, M, _ = O.nmr(tgts[0], ests[0], fs, d=d, split_hz=3000)
    assert O.rdf_margin(frame_db) >= 1e-4 and q["rdf"] == want[2] and q["frames"] == want[5] and np.array_equal(q["centre_hz"], B().nmr_design(fs)["fc"])
    for k, c in (("nmr", 0), ("nmr_seg", 1), ("nmr_hf", 3), ("nmr_lf", 4)):
        assert abs(q[k] - want[c]) <= O.TOL_DB, (k, q[k], want[c])
    assert np.max(np.abs(q["band_ratio"] - bands) / bands) < 1e-6
    assert list(am.nmr(ests[0], tgts[0], names=("rdf", "nmr"))) == ["nmr", "rdf"]
    bits = lambda v: np.array([x for x in v.values()]).tobytes()      # noqa: E731
    splits = [4000, None, 2500.5]
    batch = am.nmr_batch(ests, tgts, split_hz=splits)
    for i in range(3):
        assert bits(am.nmr(ests[i], tgts[i], split_hz=splits[i])) == bits(batch[i]), i
    assert np.isnan(batch[1]["nmr_hf"]) and np.isfinite(batch[0]["nmr_hf"])
    by_key = [ests, [O.clipped(x).astype(np.float32) for x in xs], [t.copy() for t in tgts]]
    multi = am.nmr_multi(by_key, tgts, split_hz=[3000, None, 1000.0])
    for i in range(3):
        assert bits(multi[i][0]) == bits(am.nmr(by_key[0][i], tgts[i], split_hz=3000)), i
        assert bits(multi[i][1]) == bits(am.nmr(by_key[1][i], tgts[i])), i
        assert list(multi[i][2].values()) == [-200.0, -200.0, 0.0, -200.0, -200.0]
    dev = am.nmr_batch([torch.from_numpy(e).to(DEV) for e in ests], [torch.from_numpy(t).to(DEV) for t in tgts], split_hz=splits, resident=True)
    assert [bits(v) for v in dev] == [bits(v) for v in batch]
    mask_db, fc = am.masking_threshold(tgts[0])
    assert mask_db.shape == M.shape and np.array_equal(fc, q["centre_hz"]) and np.max(np.abs(mask_db - 10.0 * np.log10(M))) < 1e-8


# ---- where the kernels touch memory ---------------------------------------------------------------------------------------------
def _nmr_inputs(dtype):
    N = 256
    lens = [1, N - 1, N, O.len_for_frames(2, N, 0), O.len_for_frames(FR + 1, N, 7)]
    xs = [O.music_like(n, 8000, 600 + i) + 1e-3 for i, n in enumerate(lens)]
    tgt = [x.astype(dtype) for x in xs]
    idx = list(range(len(lens))) + [len(lens) - 1]                        # two estimates of the last target
    est = [O.noisy(xs[i], 30.0, 610 + k).astype(dtype) for k, i in enumerate(idx)]
    return tgt, est, idx


@pytest.mark.parametrize("placement", ["odd", "quad"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("outputs", [(True, True), (False, False)], ids=["bands_mask_out", "null"])
def test_guard_bands_and_poison(monkeypatch, dtype, placement, outputs):
    """ssr_nmr on separate device tensors, then on views into NaN-filled arenas with `out`, `bands_out`, `mask_out` and the workspace
    between 0xFF guard bands and 0xFF inside: the same bits, no guard damaged, no arena written, the signals read where they lie,
    and every value finite where K >= 1 (a read outside an item or of an unwritten workspace byte would be NaN)."""
    bk = B()
    gaps = {"odd": G.GAPS_ODD, "quad": G.GAPS_QUAD}[placement]
    tgt, est, idx = _nmr_inputs(dtype)

    def call(put):
        return bk.nmr_metrics(put(tgt), put(est), idx, 8000, 256, 92.0, [30] * len(est), outputs[0], outputs[1])
    plain = G.bits([a for a in call(lambda arrays: [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]) if a is not None])
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        got = call(lambda arrays: g.arena(arrays, gaps, torch.from_numpy(np.asarray(arrays[0])).dtype, DEV)[0])
        assert len(g.blocks) >= (4 if outputs[0] else 2)                   # out, bands_out, mask_out and the workspace
        assert g.arenas and g.read_in_place()
        g.check()
        got = G.bits([a for a in got if a is not None])
    G.assert_same_bits(plain, got, "nmr")
    rows = np.frombuffer(got[0][2], np.float64).reshape(got[0][0])
    assert np.isnan(rows[:2, :5]).all() and np.isfinite(rows[2:]).all() and rows[:, 5].tolist() == [0, 0, 1, 2, FR + 1, FR + 1], rows
    if outputs[0]:
        bands, mask = (np.frombuffer(b[2], np.float64).reshape(b[0]) for b in got[1:3])
        assert np.isnan(bands[:2]).all() and np.isfinite(bands[2:]).all() and mask.shape == (1 + 2 + FR + 1, 65) and np.all(mask > 0.0)


def test_one_byte_less_than_reported_is_refused(monkeypatch):
    """With ssr_nmr_workspace_bytes reporting one byte less than it should the call is SSR_ERR_WORKSPACE and nothing is enqueued:
    `out`, `bands_out`, `mask_out` and the workspace still hold only 0xFF."""
    bk = B()
    lib = bk._lib.load()
    real = lib.ssr_nmr_workspace_bytes
    asked = []

    def one_less(*a):
        n = int(real(*a))
        assert n > 0
        asked.append(n)
        return n - 1
    tgt, est, idx = _nmr_inputs(np.float32)
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        m.setattr(lib, "ssr_nmr_workspace_bytes", one_less)
        with pytest.raises(bk.SsrHipError, match=r"libssrhip error -4\b"):
            bk.nmr_metrics(g.arena(tgt, G.GAPS_ODD, torch.float32, DEV)[0], g.arena(est, G.GAPS_ODD, torch.float32, DEV)[0], idx, 8000, 256,
                           return_bands=True, return_mask=True)
        assert asked
        g.check()
        assert g.untouched_payloads(("backend.py:put", "backend.py:_uniform_images")) == []


# ---- SSR_Eval_Helper(nmr=...) ----------------------------------------------------------------------------------------------------
FS = 16000
LENGTHS = {"p360": (8000, 8411), "p361": (9001,)}
KEYS = ("nmr", "rdf", "nmr_hf")


def _bits(v):
    return np.float64(v).tobytes()                                        # NaN equals NaN


def test_evaluate_with_nmr_on_the_three_file_tree(tmp_path, monkeypatch):
    """evaluate() on a three-file 16 kHz tree with an FFT key and an IIR key: the three keys sit behind every_key_order()'s and in
    front of ALIGN_KEYS; the values are a direct AudioMetrics.nmr_multi call's on the arrays the helper scored, bit for bit, each
    key split at its own cutoff; with nmr=None the result is what it is without the keyword."""
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee, AudioMetrics
    from ssr_eval_amd.eval import ALIGN_KEYS, every_key_order, key_cutoff_hz, open_key_order
    from ssr_eval_amd.io import write_wav
    root = tmp_path / "vctk_test"
    for s, (spk, lens) in enumerate(LENGTHS.items()):
        (root / spk).mkdir(parents=True)
        for i, n in enumerate(lens):
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), O.music_like(n, FS, 700 + 10 * s + i).astype(np.float32), FS)
    seen = []

    def go(**kw):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=FS, output_sr=FS, evaluation_sr=FS, test_data_root=str(root),
                            setting_fft={"cutoff_freq": [2000]}, setting_lowpass_filtering={"cutoff_freq": [3000], "filter_order": [4], "filter": ["butter"]},
                            **kw)
        real = h.audio_metrics.nmr_multi

        def spy(by_key, targets, split_hz, *a, **k):
            keep = lambda a: a.clone() if isinstance(a, torch.Tensor) else np.array(a)      # noqa: E731
            seen.append(([[keep(e) for e in es] for es in by_key], [keep(t) for t in targets], list(split_hz)))
            return real(by_key, targets, split_hz, *a, **k)
        monkeypatch.setattr(h.audio_metrics, "nmr_multi", spy)
        return h.evaluate(save_json=False)
    none, off, on, both = go(), go(nmr=None), go(nmr=True), go(nmr=True, csii=True, align=True)
    assert off == none and len(seen) == 2
    order = every_key_order()
    assert open_key_order() == order + KEYS + ALIGN_KEYS
    by_key, targets, split_hz = seen[0]
    keys = list(next(iter(on["p360"].values())))
    assert sorted(keys) == ["proc_bw_6000_4_16000", "proc_fft_4000_16000"] and split_hz == [key_cutoff_hz(k) for k in keys]
    assert sorted(split_hz) == [2000, 3000] and len(by_key) == 2
    to_host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else t      # noqa: E731
    want = AudioMetrics(FS).nmr_multi([[to_host(e) for e in es] for es in by_key], [to_host(t) for t in targets], split_hz=split_hz, names=KEYS)
    files = [(spk, fn) for spk in LENGTHS for fn in on[spk]]
    assert len(files) == 3 == len(want)
    row_of = {int(t.shape[0]): i for i, t in enumerate(targets)}             # the batch's file order, by the files' distinct lengths
    matched = 0
    for spk, fn in files:
        n = len(next(iter(on[spk][fn].values())))
        i = row_of[LENGTHS[spk][int(fn.split("_")[1])]]
        for k, key in enumerate(keys):
            got, b = on[spk][fn][key], both[spk][fn][key]
            assert list(got) == list(order[:4]) + list(KEYS), (spk, fn, key, list(got))
            assert list(b) == list(order[:4]) + ["csii", "csii_mid", "i3", "csii_hf"] + list(KEYS) + list(ALIGN_KEYS)
            assert [_bits(got[m]) for m in order[:4]] == [_bits(none[spk][fn][key][m]) for m in order[:4]]
            assert [_bits(got[m]) for m in KEYS] == [_bits(want[i][k][m]) for m in KEYS], (spk, fn, key, got, want[i][k])
            matched += 1
            assert all(np.isfinite(got[m]) for m in KEYS) and got["nmr"] > -150.0 and 0.0 <= got["rdf"] <= 1.0 and got["nmr_hf"] > got["nmr"], (key, got)
        assert n == 4 + len(KEYS)
    assert matched == 6
    for key in keys:
        assert list(on["averaged"][key]) == list(order[:4]) + list(KEYS)
