"""Where the kernels touch memory: every device-pointer entry point of include/ssr_hip.h run twice on identical inputs -

(a) plain: inputs packed as the other GPU tests pack them, buffers allocated as shipped;
(b) guarded: every workspace and output between two 64 KiB guards, everything pre-filled with 0xFF (tests/guarded.py), every
    input a view into a NaN-filled arena with NaN in front, between (gaps of 1, 3, 5 elements, or 4, 8, 12) and behind.

The guards must stay 0xFF, the arenas unchanged, and (b) must equal (a) bit for bit: placement changes no bit, and a value read
from outside an item, or from a buffer before it was written, would be NaN.  What the header promises to be finite is finite in (b).
There are no tolerances.  The second half is the workspace-size contract: one byte less than *_workspace_bytes reports is
SSR_ERR_WORKSPACE with nothing enqueued - outputs and workspace still hold only 0xFF.  COVERAGE at the end of the file maps every
entry point of the header that takes a device pointer to its case; test_the_inventory_is_the_header keeps it complete."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded as G
from ssr_eval_amd._lib import SIGNATURES

pytestmark = pytest.mark.gpu

DEV = "cuda"
PLACEMENTS = {"odd": G.GAPS_ODD, "quad": G.GAPS_QUAD}
M_ALL, M_LSD, M_LOG_SISPEC, M_SISPEC, M_SSIM = 15, 1, 2, 4, 8
MASKS = (M_ALL, M_LSD | M_SSIM, M_LSD, M_SISPEC | M_LOG_SISPEC)
# (n_fft, hop, precision): one transform kernel of tu_stft.inc each
PLANS = [(2048, 512, "f64"), (2048, 512, "f32"), (2229, 480, "f64"), (2229, 480, "f32"), (1486, 320, "f64"), (743, 160, "f64"),
         (2046, 500, "f64"), (256, 64, "f64"), (4096, 1024, "f64"), (3063, 700, "f64"), (100, 25, "f64")]
PLAN_IDS = ["%d-%d-%s" % p for p in PLANS]


def B():
    from ssr_eval_amd import backend
    return backend


def plan_of(p):
    return B().get_plan(*p)


def main_lengths(plan):
    """T = 7 (SSIM's minimum), 17 and 33 frames (a chunk tail of one frame at four units per chunk), and 33 frames + hop - 1."""
    out = []
    for T, extra in ((7, 0), (17, 0), (33, 0), (33, plan.hop - 1)):
        n = (T - 1) * plan.hop + plan.n_fft % 2 + extra
        assert plan.frames(n) == T
        out.append(n)
    return out


def short_lengths(plan):
    return [1, plan.n_fft // 2 + 1, plan.hop]


def signals(lens, dtype=np.float32, seed=0, noise=0.0):
    rng = np.random.default_rng(seed)
    base = [0.1 * rng.standard_normal(n) for n in lens]
    if noise:
        base = [x + noise * rng.standard_normal(len(x)) for x in base]
    return [x.astype(dtype) for x in base]


def pair_of(lens, est_dtype, tgt_dtype, keys=1, seed=0):
    tgt = signals(lens, np.float64, seed)
    rng = np.random.default_rng(seed + 1000)
    ests = [[(t + 0.01 * (k + 1) * rng.standard_normal(len(t))).astype(est_dtype) for t in tgt] for k in range(keys)]
    return ests, [t.astype(tgt_dtype) for t in tgt]


def twice(monkeypatch, call, gaps, what="", in_place=True, blocks=1):
    """call(put) twice: put(arrays) hands the arrays over as separate device tensors (an entry point that takes a list packs them),
    then as views into a poisoned arena of their dtype under guarded allocations.  in_place: the product must build its Ragged
    batches on the arenas as they lie (a wrapper that packed them would lose the poison); False only where the entry point takes
    the tensors' own pointers or where the inputs are not what the case is about.  blocks: how many buffers of the call, at least,
    must have come from the guarded allocator.  -> the guarded result, after the guard / arena check and the bit comparison."""
    plain = G.bits(call(lambda arrays: [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]))
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)

        def put(arrays):
            return g.arena(arrays, gaps, torch.from_numpy(np.asarray(arrays[0])).dtype, DEV)[0]
        got = call(put)
        assert len(g.blocks) >= blocks, "%d allocation(s) of the call went through the guarded allocator, not %d" % (len(g.blocks), blocks)
        assert not in_place or (g.arenas and g.read_in_place()), "%r: an input arena was packed before the library read it" % (what,)
        g.check()
        got = G.bits(got)
    G.assert_same_bits(plain, got, what)
    return [np.frombuffer(b, np.dtype(d)).reshape(s) for s, d, b in got]


def all_finite(arrays, what=""):
    for a in arrays:
        if a.dtype.kind == "f":
            assert np.isfinite(a).all(), (what, a)


def metric_columns(out, mask, what):
    """[..., 4] = lsd, log_sispec, sispec, ssim: finite where asked for, NaN elsewhere."""
    for j in range(4):
        col = out[..., j]
        if mask >> j & 1:
            assert np.isfinite(col).all(), (what, mask, j, col)
        else:
            assert np.isnan(col).all(), (what, mask, j, col)


# ---- the harness itself: torch operations only ----------------------------------------------------------------------------------
def test_harness_reports_a_byte_in_the_back_guard():
    g = G.Guarded()
    p = g.alloc(1000, DEV)
    assert p.numel() == 1000 and p.data_ptr() % 512 == 0 and bool((p == 0xFF).all())
    whole = g.blocks[-1].whole
    assert whole.numel() >= 1000 + 2 * 65536
    g.check()
    whole[G.GUARD + 1000 + 37] = 0            # 37 bytes behind the payload, inside the test's own allocation
    (b, side, first, last), = g.damage()
    assert (b.nbytes, side, first, last) == (1000, "back", 37, 37)
    with pytest.raises(G.GuardError, match=r"back guard of the 1000-byte buffer allocated at test_gpu_memory_discipline.py:\d+ "
                                           r"\(test_harness_reports_a_byte_in_the_back_guard\) damaged: guard bytes 37 \.\. 37"):
        g.check()


def test_harness_reports_a_byte_in_the_front_guard():
    g = G.Guarded()
    t = g.empty((5, 3), torch.float64, DEV)
    assert t.shape == (5, 3) and bool(torch.isnan(t).all())
    g.blocks[-1].whole[G.GUARD - 1] = 1       # the byte in front of the payload
    (b, side, first, last), = g.damage()
    assert (b.nbytes, side, first, last) == (120, "front", G.GUARD - 1, G.GUARD - 1)
    with pytest.raises(G.GuardError, match=r"front guard of the 120-byte buffer .*\(1 \.\. 1 bytes in front of the payload's start"):
        g.check()


def test_harness_passes_an_intact_run_and_sees_a_written_arena(monkeypatch):
    g = G.Guarded()
    with monkeypatch.context() as m:
        g.route(m)
        bk = B()
        w = bk._workspace(0, torch.device(DEV))
        o = bk.torch.empty((4, 4), dtype=torch.float64, device=DEV)
        z = bk.torch.zeros(7, dtype=torch.float32, device=DEV)
        i = bk.torch.full((3,), 5, dtype=torch.int32, device=DEV)
        e = bk.torch.empty_like(z)
        host = bk.torch.empty(8, dtype=torch.uint8)                      # host memory is not routed
    assert len(g.blocks) == 5 and w.numel() == 1 and not host.is_cuda
    assert bool((i == 5).all()) and bool((z == 0).all()) and bool(torch.isnan(e).all()) and bool((o.view(torch.int64) == -1).all())
    o.fill_(1.0); w.fill_(3)                                             # writes inside the payloads
    views, offs, arena = g.arena([np.arange(5, dtype=np.float32), np.ones((2, 3), np.float32)], G.GAPS_ODD, torch.float32, DEV)
    assert list(offs) == [G.ARENA_PAD + 1, G.ARENA_PAD + 1 + 5 + 1] and views[1].shape == (2, 3)
    assert int(torch.isnan(arena).sum()) == arena.numel() - 11 and arena.numel() >= offs[1] + 6 + G.ARENA_PAD
    g.check()
    arena[offs[0] + 5] = 0.0                                             # the NaN behind item 0
    with pytest.raises(G.GuardError, match=r"input arena of %d elements .* was written: elements %d \.\. %d " % (arena.numel(), offs[0] + 5, offs[0] + 5)):
        g.check()


# ---- pair and image metrics -----------------------------------------------------------------------------------------------------
def _pair_metrics_direct(plan, est, tgt, mask):
    """ssr_pair_metrics itself (PairBatch.run goes through ssr_pair_metrics_stages), float32 pairs."""
    bk = B()
    b = bk.PairBatch(plan, bk.Ragged.from_list(est, plan.device, allow_gaps=True), bk.Ragged.from_list(tgt, plan.device, allow_gaps=True))
    b._workspace(mask)
    e, t = b.est, b.tgt
    bk._lib.check(plan.lib.ssr_pair_metrics(plan.handle, bk._vp(e.data), bk._vp(e.off), bk._vp(t.data), bk._vp(t.off), bk._vp(e.len), bk._vp(b.rows.off),
                                            e.n, e.max_len, b.rows.total, mask, bk._vp(b.out), bk._vp(b.ws), b.ws_bytes, bk._stream()))
    return b.out


@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("dtypes", [(np.float32, np.float32), (np.float64, np.float32), (np.float64, np.float64)], ids=["f32", "est64", "f64"])
@pytest.mark.parametrize("p", PLANS, ids=PLAN_IDS)
def test_pair_metrics(monkeypatch, p, dtypes, placement):
    plan = plan_of(p)
    for lens, masks in ((main_lengths(plan), MASKS), (short_lengths(plan), (M_LSD, M_SISPEC | M_LOG_SISPEC))):
        ests, tgt = pair_of(lens, dtypes[0], dtypes[1])
        for mask in masks:
            if (mask & M_SSIM) and plan.n_bins < 7:
                continue
            out, = twice(monkeypatch, lambda put: B().pair_metrics(plan, put(ests[0]), put(tgt), mask), PLACEMENTS[placement], (p, mask))
            metric_columns(out, mask, (p, lens))
            if dtypes == (np.float32, np.float32):
                direct, = twice(monkeypatch, lambda put: _pair_metrics_direct(plan, put(ests[0]), put(tgt), mask), PLACEMENTS[placement], (p, mask))
                assert direct.tobytes() == out.tobytes()              # stages = 7 IS ssr_pair_metrics


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("p", PLANS, ids=PLAN_IDS)
def test_pair_metrics_multi(monkeypatch, p, K):
    plan = plan_of(p)
    dts = [np.float32] + ([np.float64] if p in ((2229, 480, "f64"), (2048, 512, "f64")) else [])
    for dt in dts:
        for lens, mask in ((main_lengths(plan), M_ALL), (short_lengths(plan), M_LSD | M_SISPEC)):
            ests, tgt = pair_of(lens, dt, np.float32, K)
            n = len(tgt)

            def call(put):
                flat = put([e for key in ests for e in key])              # key-major, ONE buffer: read where they lie
                return B().pair_metrics_multi(plan, [flat[k * n:(k + 1) * n] for k in range(K)], put(tgt), mask)
            out, = twice(monkeypatch, call, G.GAPS_ODD, (p, K, dt))
            assert out.shape == (n, K, 4)
            metric_columns(out, mask, (p, K, dt))


IMG_T, IMG_N = 9, 3


def images(F, seed=3):
    rng = np.random.default_rng(seed)
    tgt = np.abs(rng.standard_normal((IMG_N, IMG_T, F))).astype(np.float32) + 0.01
    est = (tgt * (1 + 0.1 * rng.standard_normal(tgt.shape))).astype(np.float32)
    return np.abs(est) + 0.01, tgt


def fb_of(F, n_mels):
    from ssr_eval_amd import mel
    return mel.mel_filterbank(F, 0.0, 22050.0, n_mels, 44100).contiguous()


def twice_images(monkeypatch, call, lead, what=""):
    """call(place): place(array) -> a device tensor of the array: plain, or inside a poisoned arena whose item base is 16-byte
    aligned (lead 0) or displaced by one float (lead 1)."""
    plain = G.bits(call(lambda a: torch.from_numpy(a).to(DEV)))
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        got = call(lambda a: g.arena([a], (4,), torch.float32, DEV, lead=lead)[0][0])
        for t, _, _ in g.arenas:
            assert (t.data_ptr() + (G.ARENA_PAD + lead) * 4) % 16 == 4 * lead
        assert g.blocks and g.arenas
        g.check()
        got = G.bits(got)
    G.assert_same_bits(plain, got, what)
    out = [np.frombuffer(b, np.dtype(d)).reshape(s) for s, d, b in got]
    all_finite(out, what)
    return out


@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "displaced"])
@pytest.mark.parametrize("F", [1025, 1024])
def test_spectrogram_image_entry_points(monkeypatch, F, lead):
    est, tgt = images(F)
    fb = fb_of(F, 16)
    edges = np.tile(np.array([0, 1, F // 3, F - 1, F], np.int32), (IMG_N, 1))
    bk = B()
    twice_images(monkeypatch, lambda pl: bk.spectrogram_lsd_bands(pl(est), pl(tgt), edges), lead, "lsd_bands")
    twice_images(monkeypatch, lambda pl: bk.spectrogram_mel(pl(est), fb), lead, "mel")
    twice_images(monkeypatch, lambda pl: bk.spectrogram_mel_metrics(pl(est), pl(tgt), fb, 5, 7), lead, "mel_metrics")
    for radius in (0, 31):
        twice_images(monkeypatch, lambda pl: bk.spectrogram_mel_dtw(pl(est), pl(tgt), fb, 5, radius), lead, "mel_dtw")


def _spectrogram_metrics(x, y, off, rows, F, mask):
    """ssr_spectrogram_metrics on two 1-D float32 device tensors whose element 0 is row 0; off / rows: host arrays."""
    bk = B()
    lib = bk._lib.load()
    n, max_T = len(rows), int(max(rows))
    off_d, rows_d = torch.from_numpy(np.asarray(off, np.int64)).to(DEV), torch.from_numpy(np.asarray(rows, np.int32)).to(DEV)
    ws_bytes = int(lib.ssr_spectrogram_metrics_workspace_bytes(n, max_T, F))
    ws = bk._workspace(ws_bytes, torch.device(DEV))
    out = bk.torch.empty((n, 4), dtype=torch.float64, device=DEV)
    bk._lib.check(lib.ssr_spectrogram_metrics(bk._vp(x), bk._vp(y), bk._vp(off_d), bk._vp(rows_d), n, max_T, F, mask, bk._vp(out), bk._vp(ws),
                                              ws_bytes, bk._stream()))
    return out


@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "displaced"])
@pytest.mark.parametrize("F", [1025, 1024, 51])
def test_spectrogram_metrics(monkeypatch, F, lead):
    rng = np.random.default_rng(4)
    rows = [7, 9, 12]
    tgt = [np.abs(rng.standard_normal((T, F))).astype(np.float32) + 0.01 for T in rows]
    est = [(t * (1 + 0.1 * rng.standard_normal(t.shape))).astype(np.float32) for t in tgt]
    packed_off = np.cumsum([0] + rows[:-1])
    for mask in MASKS:
        plain = _spectrogram_metrics(torch.from_numpy(np.concatenate(est).reshape(-1)).to(DEV), torch.from_numpy(np.concatenate(tgt).reshape(-1)).to(DEV),
                                     packed_off, rows, F, mask)
        with monkeypatch.context() as m:
            g = G.Guarded().route(m)
            (_, offs, ae), (_, _, at) = (g.arena(s, (1, 3), torch.float32, DEV, lead=lead, unit=F) for s in (est, tgt))    # gaps of whole rows
            assert (ae.data_ptr() + offs[0] * 4) % 16 == 4 * lead
            got = _spectrogram_metrics(ae[offs[0]:], at[offs[0]:], (offs - offs[0]) // F, rows, F, mask)
            g.check()
        G.assert_same_bits(plain, got, ("spectrogram_metrics", F, mask))
        metric_columns(got.cpu().numpy(), mask, ("spectrogram_metrics", F))


FAMILY_PLANS = [(2048, 512, "f64"), (2229, 480, "f64"), (256, 64, "f64"), (100, 25, "f64")]


@pytest.mark.parametrize("est_dtype", [np.float32, np.float64], ids=["f32", "est64"])
@pytest.mark.parametrize("p", FAMILY_PLANS, ids=["%d-%d-%s" % p for p in FAMILY_PLANS])
def test_pair_image_families(monkeypatch, p, est_dtype):
    """pair_lsd_bands (all keys in one chunk, and keys_per_chunk < K: the scratch plane), pair_mel_metrics, pair_mel_dtw."""
    plan = plan_of(p)
    K, F = 3, plan.n_bins
    ests, tgt = pair_of(main_lengths(plan), est_dtype, np.float32, K)
    n = len(tgt)
    fb = fb_of(F, 16 if F >= 513 else 8)
    edges = np.tile(np.array([0, F // 3, F], np.int32), (K, n, 1))

    def keyed(put):
        flat = put([e for key in ests for e in key])
        return [flat[k * n:(k + 1) * n] for k in range(K)]
    bk = B()
    for kc in (None, 2, 1):
        out, = twice(monkeypatch, lambda put: bk.pair_lsd_bands(plan, keyed(put), put(tgt), edges, keys_per_chunk=kc), G.GAPS_ODD, (p, "lsd_bands", kc))
        all_finite([out], (p, "lsd_bands", kc))
    out, = twice(monkeypatch, lambda put: bk.pair_mel_metrics(plan, keyed(put), put(tgt), fb, 5, 7), G.GAPS_ODD, (p, "mel"))
    all_finite([out], (p, "mel"))
    for radius in (0, 31):
        out, = twice(monkeypatch, lambda put: bk.pair_mel_dtw(plan, keyed(put), put(tgt), fb, 5, radius, keys_per_chunk=2), G.GAPS_QUAD, (p, "dtw", radius))
        all_finite([out], (p, "dtw", radius))


# ---- per-pair families: estimate e against target tgt_index[e] -------------------------------------------------------------------
def family_inputs(fs, dtype, short):
    lens = list(short) + [int(0.3 * fs)]
    tgt = signals(lens, dtype, 7)
    idx = list(range(len(lens))) + [len(lens) - 1]                        # two estimates of the last target
    rng = np.random.default_rng(8)
    est = [(tgt[i] + 0.02 * rng.standard_normal(len(tgt[i]))).astype(dtype) for i in idx]
    return tgt, est, idx


@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_per_pair_families(monkeypatch, dtype, placement):
    bk, gaps = B(), PLACEMENTS[placement]
    fs = 16000
    tgt, est, idx = family_inputs(fs, dtype, (1, 2))
    last = len(est) - 2                                                    # the two estimates of the 0.3 s target

    def run(fn, what, finite=True, in_place=True):
        out = twice(monkeypatch, lambda put: fn(put(tgt), put(est)), gaps, what, in_place)[0]
        if finite:
            assert np.isfinite(out[last:]).all(), (what, out)
        return out
    # (stoi, pitch_metrics and f0_track resample first and so pack their lists: outputs and workspaces only here, the kernels'
    # own reads in test_stoi_and_pitch_read_where_the_signals_lie)
    run(lambda t, e: bk.stoi(t, e, idx, fs, which=bk._lib.STOI_BOTH), "stoi", in_place=False)
    run(lambda t, e: bk.wave_metrics(t, e, idx, fs), "wave")
    run(lambda t, e: bk.quality_metrics(t, e, idx, fs), "quality")
    for n_fft in (256, 2048):
        run(lambda t, e: bk.phase_metrics(t, e, idx, n_fft=n_fft), ("phase", n_fft))
    run(lambda t, e: bk.mrstft_metrics(t, e, idx), "mrstft")
    run(lambda t, e: bk.mrstft_metrics(t, e, idx, resolutions=((256, 64, 256),)), "mrstft-256")
    run(lambda t, e: bk.pitch_metrics(t, e, idx, fs), "pitch", finite=False, in_place=False)     # (B may be empty on noise: NaN by the header)
    tracks = twice(monkeypatch, lambda put: [list(tr) for tr in bk.f0_track(put(tgt), fs)], gaps, "f0_track", in_place=False)
    for f0, vo, ap, en in zip(*[iter(tracks)] * 4):
        assert np.isfinite(ap).all() and np.isfinite(en).all() and np.isfinite(f0[en > 0]).all()


TILE = 16384                                                              # ssr_bss_sdr's tile, in samples


def bss_inputs(dtype):
    rng = np.random.default_rng(7)
    lens = [1, 2, 700, TILE + 3]
    tgt = [(0.1 * rng.standard_normal(n)).astype(dtype) for n in lens]
    idx = list(range(len(lens))) + [len(lens) - 1]                        # two estimates of the last target
    est = [(tgt[i] + 0.02 * rng.standard_normal(len(tgt[i]))).astype(dtype) for i in idx]
    return tgt, est, idx


@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("with_filter", [True, False], ids=["filt", "null"])
def test_guard_bands_and_poison(monkeypatch, dtype, placement, with_filter):
    """ssr_bss_sdr on separate device tensors, then on views into NaN-filled arenas with `out`, `filt` and the workspace between
    0xFF guard bands and 0xFF inside: the same bits, no guard damaged, no arena written, everything finite."""
    bk = B()
    tgt, est, idx = bss_inputs(dtype)
    for taps in (512, 5):
        got = twice(monkeypatch, lambda put: bk.bss_sdr(put(tgt), put(est), idx, taps, return_filter=with_filter), PLACEMENTS[placement],
                    ("bss", taps), blocks=3 if with_filter else 2)            # out, filt and the workspace
        all_finite(got, ("bss", taps))


def twice_direct(monkeypatch, call, groups, gaps, what="", unit=1, lead=None):
    """For the C-ABI drivers: call(places), places[i] = (data, offsets) of groups[i] (a list of host arrays of one dtype) - packed
    back to back in an ordinary tensor, then inside a poisoned arena under guarded allocations.  -> the guarded result."""
    def packed(arrays):
        sizes = np.array([a.size for a in arrays], np.int64)
        return torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in arrays])).to(DEV), np.cumsum(sizes) - sizes
    plain = G.bits(call([packed(a) for a in groups]))
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        places = []
        for arrays in groups:
            _, offs, arena = g.arena(arrays, gaps, torch.from_numpy(np.asarray(arrays[0])).dtype, DEV, lead=lead, unit=unit)
            places.append((arena, offs))
        got = call(places)
        assert g.blocks
        g.check()
        got = G.bits(got)
    G.assert_same_bits(plain, got, what)
    return [np.frombuffer(b, np.dtype(d)).reshape(s) for s, d, b in got]


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _host(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


def _stoi(tgt, tgt_len, est, tgt_index, which):
    """ssr_stoi on 10 kHz float64 signals where they lie: tgt / est = (data, offsets)."""
    bk = B()
    lib = bk._lib.load()
    (td, to), (ed, eo) = tgt, est
    tl, tlp = _host(tgt_len)
    idx, idxp = _host(tgt_index)
    el, elp = _host(tl[idx])
    n_t, n_e = len(tl), len(idx)
    to_d, eo_d = _dev(to, np.int64), _dev(eo, np.int64)
    ws_bytes = int(lib.ssr_stoi_workspace_bytes(tlp, n_t, idxp, n_e))
    ws = bk._workspace(ws_bytes, torch.device(DEV))
    out = bk.torch.empty((n_e, 2 if which == 3 else 1), dtype=torch.float64, device=DEV)
    bk._lib.check(lib.ssr_stoi(bk._vp(td), bk._vp(to_d), tlp, n_t, bk._vp(ed), bk._vp(eo_d), elp, idxp, n_e, which, bk._vp(out), bk._vp(ws),
                               ws_bytes, bk._stream()))
    return out.cpu()                                  # (the copy waits for the stream: the host arrays live until here)


def _f0_track(sig, lens, fmin=50.0, fmax=500.0):
    """ssr_f0_track on 16 kHz float64 signals where they lie."""
    bk = B()
    lib = bk._lib.load()
    data, offs = sig
    ln, lnp = _host(lens)
    n = len(ln)
    T = np.array([bk.pitch_frames(m) for m in ln], np.int64)
    tot = int(T.sum())
    off_d, foff_d = _dev(offs, np.int64), _dev(np.cumsum(T) - T, np.int64)
    f0, ap, en = (bk.torch.empty(tot, dtype=torch.float64, device=DEV) for _ in range(3))
    vo = bk.torch.empty(tot, dtype=torch.uint8, device=DEV)
    ws_bytes = int(lib.ssr_f0_track_workspace_bytes(lnp, n, fmin, fmax))
    ws = bk._workspace(ws_bytes, torch.device(DEV))
    bk._lib.check(lib.ssr_f0_track(bk._vp(data), bk._vp(off_d), lnp, n, fmin, fmax, bk._vp(f0), bk._vp(ap), bk._vp(en), bk._vp(vo), bk._vp(foff_d),
                                   bk._vp(ws), ws_bytes, bk._stream()))
    return [t.cpu() for t in (f0, ap, en, vo)]


def _f0_metrics(tgt, tgt_len, est, tgt_index, which=31, fmin=50.0, fmax=500.0):
    """ssr_f0_metrics on 16 kHz float64 signals where they lie."""
    bk = B()
    lib = bk._lib.load()
    (td, to), (ed, eo) = tgt, est
    tl, tlp = _host(tgt_len)
    idx, idxp = _host(tgt_index)
    n_t, n_e = len(tl), len(idx)
    to_d, eo_d = _dev(to, np.int64), _dev(eo, np.int64)
    ws_bytes = int(lib.ssr_f0_metrics_workspace_bytes(tlp, n_t, idxp, n_e, fmin, fmax, which))
    ws = bk._workspace(ws_bytes, torch.device(DEV))
    out = bk.torch.empty((n_e, bin(which).count("1")), dtype=torch.float64, device=DEV)
    bk._lib.check(lib.ssr_f0_metrics(bk._vp(td), bk._vp(to_d), tlp, n_t, bk._vp(ed), bk._vp(eo_d), idxp, n_e, fmin, fmax, which, bk._vp(out),
                                     bk._vp(ws), ws_bytes, bk._stream()))
    return out.cpu()


def voiced_like(n, fs, f, seed):
    """A harmonic signal with a little noise: frames that YIN calls voiced, so that the pitch metrics have frames to score."""
    t = np.arange(n) / fs
    rng = np.random.default_rng(seed)
    return 0.3 * np.sin(2 * np.pi * f * t) + 0.1 * np.sin(4 * np.pi * f * t) + 0.005 * rng.standard_normal(n)


@pytest.mark.parametrize("placement", list(PLACEMENTS))
def test_stoi_and_pitch_read_where_the_signals_lie(monkeypatch, placement):
    """ssr_stoi (10 kHz), ssr_f0_track and ssr_f0_metrics (16 kHz) take float64 signals by offset: driven through the C ABI on
    poisoned float64 arenas (the Python wrappers resample first, into a packed buffer)."""
    gaps = PLACEMENTS[placement]
    for fs, lens in ((10000, [1, 2, 5000]), (16000, [1, 159, 160, 4800])):
        idx = list(range(len(lens))) + [len(lens) - 1]
        tgt = [voiced_like(n, fs, 120.0 + 10 * i, i) for i, n in enumerate(lens)]
        rng = np.random.default_rng(30)
        est = [tgt[i] + 0.01 * rng.standard_normal(len(tgt[i])) for i in idx]
        if fs == 10000:
            out, = twice_direct(monkeypatch, lambda pl: _stoi(pl[0], lens, pl[1], idx, 3), [tgt, est], gaps, "ssr_stoi")
            assert np.isfinite(out).all(), out
        else:
            f0, ap, en, vo = twice_direct(monkeypatch, lambda pl: _f0_track(pl[0], lens), [tgt], gaps, "ssr_f0_track")
            assert np.isfinite(ap).all() and np.isfinite(en).all() and np.isfinite(f0[en > 0]).all() and vo.max() <= 1
            out, = twice_direct(monkeypatch, lambda pl: _f0_metrics(pl[0], lens, pl[1], idx), [tgt, est], gaps, "ssr_f0_metrics")
            assert np.isfinite(out[-2:, 3:]).all(), out              # VDE and FFE of the 0.3 s pairs: T > 0


# ---- statistics, elementwise helpers --------------------------------------------------------------------------------------------
def test_bootstrap(monkeypatch):
    bk = B()
    rng = np.random.default_rng(9)
    table = rng.standard_normal((8, 3))
    spk_off = [0, 1, 3, 8]
    for scheme in ("utterance", "speaker"):
        def call(put):
            reps = bk.bootstrap_means(put([table])[0], spk_off, 64, seed=11, scheme=scheme)
            return [reps] + list(bk.bootstrap_summary(reps, [0.025, 0.5, 0.975]))
        all_finite(twice(monkeypatch, call, G.GAPS_ODD, scheme, in_place=False), scheme)        # (the table's own pointer is passed)


def test_elementwise_helpers(monkeypatch):
    bk = B()
    rng = np.random.default_rng(10)
    for n in (1, 1027, 4 * 1025 + 3):
        x = np.abs(rng.standard_normal(n)).astype(np.float32) + 0.1
        y = rng.standard_normal(n).astype(np.float32)
        for gaps in PLACEMENTS.values():
            all_finite(twice(monkeypatch, lambda put: list(bk.magphase(*put([x, y]), 1e-8)), gaps, "magphase", in_place=False))
            all_finite(twice(monkeypatch, lambda put: bk.elementwise("to_log", put([x])[0]), gaps, "to_log", in_place=False))
            all_finite(twice(monkeypatch, lambda put: bk.elementwise("from_log", put([y])[0]), gaps, "from_log", in_place=False))
    for per in (1, 1027, 5000):
        a, b = (rng.standard_normal((3, per)).astype(np.float32) for _ in range(2))
        mul, div = (np.abs(rng.standard_normal(3)).astype(np.float32) + 0.5 for _ in range(2))
        for gaps in PLACEMENTS.values():
            all_finite(twice(monkeypatch, lambda put: bk.energy_sums(*put([a, b]), 3), gaps, "energy_sums", in_place=False))
            all_finite(twice(monkeypatch, lambda put: bk.scale_items(*put([a, mul, div])), gaps, "scale_items", in_place=False))
    e, t = (np.abs(rng.standard_normal((2, 3, 7, 129))).astype(np.float32) + 0.01 for _ in range(2))
    for log_domain in (False, True):
        for gaps in PLACEMENTS.values():
            all_finite(twice(monkeypatch, lambda put: bk.sispec_multichannel(*put([e, t]), log_domain), gaps, "sispec_multichannel", in_place=False))


# ---- transforms -----------------------------------------------------------------------------------------------------------------
def hand_ragged(g, arrays, gaps):
    """A Ragged whose items lie in a poisoned arena (packed = False): for the entry points whose Python wrapper would pack a list."""
    bk = B()
    views, offs, arena = g.arena(arrays, gaps, torch.from_numpy(arrays[0]).dtype, DEV)
    lens = np.array([len(a) for a in arrays], np.int64)
    r = bk.Ragged(arena, torch.from_numpy(offs).to(DEV), torch.from_numpy(lens.astype(np.int32)).to(DEV), lens)
    r.packed = False
    return r, offs


def twice_ragged(monkeypatch, call, arrays, gaps, what=""):
    """call(ragged, offsets) on the packed batch, then on the same items inside a poisoned arena under guarded allocations."""
    bk = B()
    lens = np.array([len(a) for a in arrays], np.int64)
    plain = G.bits(call(bk.Ragged.from_list(arrays, DEV, torch.from_numpy(arrays[0]).dtype), np.cumsum(lens) - lens))
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        r, offs = hand_ragged(g, arrays, gaps)
        got = call(r, offs)
        assert g.blocks and g.arenas
        g.check()
        got = G.bits(got)
    G.assert_same_bits(plain, got, what)
    out = [np.frombuffer(b, np.dtype(d)).reshape(s) for s, d, b in got]
    all_finite(out, what)
    return out


@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("p", PLANS, ids=PLAN_IDS)
def test_stft(monkeypatch, p, placement):
    plan = plan_of(p)
    sigs = signals(main_lengths(plan) + short_lengths(plan), np.float32, 12)
    for kind in ("mag", "complex"):
        twice_ragged(monkeypatch, lambda r, _: B().stft(plan, r, kind), sigs, PLACEMENTS[placement], (p, kind))


LOWPASS_PLANS = ["segments", "fused", "conv-2048", "conv-512", "ex-nocenter", "ex-constant"]


def lowpass_plan(name):
    """-> (plan, item lengths): the three engines of ssr_fft_lowpass / ssr_istft, and two ssr_plan_create_ex plans (a Hamming window
    without centring, zero padding)."""
    from scipy.signal import get_window
    bk = B()
    plan = {"segments": lambda: bk.get_plan(1024, 256, "f64"),
            "fused": lambda: bk.get_plan(2048, 441, "f64", lowpass_engine="fused"),
            "conv-2048": lambda: bk.get_plan(2048, 441, "f64", lowpass_engine="conv"),
            "conv-512": lambda: bk.get_plan(512, 110, "f64", lowpass_engine="conv"),
            "ex-nocenter": lambda: bk.get_plan_ex(512, 128, "hamming", get_window("hamming", 512, fftbins=True), False, "reflect"),
            "ex-constant": lambda: bk.get_plan_ex(512, 128, "hann", None, True, "constant")}[name]()
    shortest = plan.n_fft if name == "ex-nocenter" else plan.n_fft // 2 + 1
    return plan, [shortest, 16 * plan.hop, 32 * plan.hop + plan.hop - 1]


@pytest.mark.parametrize("name", LOWPASS_PLANS)
def test_fft_lowpass(monkeypatch, name):
    bk = B()
    plan, lens = lowpass_plan(name)
    F = plan.n_bins
    sigs = signals(lens, np.float32, 13)
    def items(flat, offs):
        if G.routed():                                # the output has the input's layout: its gaps must stay as they were handed out
            G.assert_only_items_written(flat, offs, lens, name)
        return [flat[..., o:o + n] for o, n in zip(offs, lens)]
    for gaps in PLACEMENTS.values():
        twice_ragged(monkeypatch, lambda r, offs: items(bk.LowpassBatch(plan, r, [1, F // 3, F]).run(), offs), sigs, gaps, (name, "per item"))
        twice_ragged(monkeypatch, lambda r, offs: items(bk.LowpassBatch(plan, r, F // 3).run(), offs), sigs, gaps, (name, "one cut"))
        twice_ragged(monkeypatch, lambda r, offs: items(bk.MultiLowpassBatch(plan, r, [1, F // 3, F]).run(), offs), sigs, gaps, (name, "multi"))


def _istft(plan, re, im, rows, lens):
    """ssr_istft on spectra where they lie: re / im = (data, element offsets of each item's first row) in ONE row grid (both sides
    placed alike), row 0 = the first item's first row; total_rows spans the gaps."""
    bk = B()
    (rd, ro), (idt, io) = re, im
    F = plan.n_bins
    assert np.array_equal(ro, io) and not ((ro - ro[0]) % F).any()
    frame_off = (ro - ro[0]) // F
    total_rows = int(frame_off[-1] + rows[-1])
    lens = np.asarray(lens, np.int64)
    foff_d, len_d, ooff_d = _dev(frame_off, np.int64), _dev(lens, np.int32), _dev(np.cumsum(lens) - lens, np.int64)
    ws_bytes = int(plan.lib.ssr_ola_workspace_bytes(plan.handle, total_rows))
    ws = bk._workspace(ws_bytes, torch.device(DEV))
    out = bk.torch.empty(int(lens.sum()), dtype=torch.float32, device=DEV)
    bk._lib.check(plan.lib.ssr_istft(plan.handle, bk._vp(rd[ro[0]:]), bk._vp(idt[ro[0]:]), bk._vp(foff_d), bk._vp(len_d), bk._vp(ooff_d), len(lens),
                                     int(lens.max()), total_rows, bk._vp(out), bk._vp(ws), ws_bytes, bk._stream()))
    return out


@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "displaced"])
@pytest.mark.parametrize("name", LOWPASS_PLANS)
def test_istft(monkeypatch, name, lead):
    """ssr_stft (complex) of the plan at hand on poisoned signals - the conv engine and the ssr_plan_create_ex plans - then
    ssr_istft through the C ABI on those spectra inside poisoned arenas: NaN in front, gaps of one and three whole rows between the
    items, NaN behind, the base 16-byte aligned or displaced by one float."""
    bk = B()
    plan, lens = lowpass_plan(name)
    sigs = signals(lens, np.float32, 14)
    if not lead:
        for gaps in PLACEMENTS.values():
            twice_ragged(monkeypatch, lambda r, _: bk.stft(plan, r, "complex"), sigs, gaps, (name, "stft"))
    re, im = bk.stft(plan, sigs, "complex")
    re, im = [t.cpu().numpy() for t in re], [t.cpu().numpy() for t in im]
    rows = [r.shape[0] for r in re]
    assert rows == [plan.frames(n) for n in lens]
    out, = twice_direct(monkeypatch, lambda pl: _istft(plan, pl[0], pl[1], rows, lens), [re, im], (1, 3), (name, "istft"), unit=plan.n_bins, lead=lead)
    all_finite([out], name)
    assert np.array_equal(out, np.concatenate([t.cpu().numpy() for t in bk.istft(plan, [torch.from_numpy(r) for r in re], [torch.from_numpy(i) for i in im], lens)]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("updown", [(160, 147), (147, 160)])
def test_resample_poly(monkeypatch, updown, dtype):
    bk = B()
    sigs = signals([1, 2, 147, 1000, 4411], dtype, 15)
    for exact in (True, False):
        for gaps in PLACEMENTS.values():
            twice_ragged(monkeypatch, lambda r, _: bk.resample_poly(r, *updown, exact=exact), sigs, gaps, (updown, exact))


def test_resample_poly_chain_and_sinc(monkeypatch):
    bk = B()
    sigs = signals([1, 160, 1601, 4800], np.float32, 16)
    for gaps in PLACEMENTS.values():
        for fused in (None, False):
            twice_ragged(monkeypatch, lambda r, _: bk.resample_poly_chain(r, 16000, 44100, 48000, fused=fused), sigs, gaps, ("chain", fused))
        for a, b in ((44100, 48000), (48000, 16000)):
            twice_ragged(monkeypatch, lambda r, _: bk.resample_sinc(r, a, b), sigs, gaps, ("sinc", a, b))


def test_upload_decoded(monkeypatch):
    """ssr_pcm16_to_float: 16-bit mono and stereo cross as int16 (the device twin of the staging arena and the float output are
    guarded); 24-bit input is uploaded as the float32 mono array it already is."""
    from ssr_eval_amd.io import RawAudio
    bk = B()
    rng = np.random.default_rng(17)
    mono = rng.integers(-32768, 32767, 1001, dtype=np.int16)
    stereo = rng.integers(-32768, 32767, 2 * 777, dtype=np.int16)
    x24 = (rng.integers(-2 ** 23, 2 ** 23, 333).astype(np.float64) / 2 ** 23).astype(np.float32)
    raw = lambda: [RawAudio(mono, None, 1, 44100), RawAudio(stereo, None, 2, 44100), RawAudio(None, x24, 1, 44100)]      # noqa: E731
    plain = G.bits(bk.upload_decoded(raw(), DEV))
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        m.setattr(bk._Staging, "_by_dev", {})             # fresh staging arenas: this run allocates its own device twin, guarded
        got = bk.upload_decoded(raw(), DEV)
        assert any(b.fn == "backend.py:_h2d_arena" and b.nbytes >= 2 * (1001 + 2 * 777) for b in g.blocks), [b.fn for b in g.blocks]
        assert any(b.fn == "backend.py:_pcm_to_float" and b.nbytes == 4 * (1001 + 777) for b in g.blocks), [b.fn for b in g.blocks]
        g.check()
        got = G.bits(got)
    G.assert_same_bits(plain, got, "upload_decoded")
    assert [s_[0] for s_, _, _ in got] == [1001, 777, 333]


def _pcm16(pcm, frames, chans):
    """ssr_pcm16_to_float on interleaved int16 frames where they lie: pcm = (data, offsets)."""
    bk = B()
    data, offs = pcm
    frames = np.asarray(frames, np.int64)
    n = len(frames)
    in_off, out_off = _dev(offs, np.int64), _dev(np.cumsum(frames) - frames, np.int64)
    fr, ch = _dev(frames, np.int32), _dev(chans, np.int32)
    out = bk.torch.empty(int(frames.sum()), dtype=torch.float32, device=DEV)
    bk._lib.check(bk._lib.load().ssr_pcm16_to_float(bk._vp(data), bk._vp(in_off), bk._vp(fr), bk._vp(ch), n, int(frames.max()), bk._vp(out),
                                                    bk._vp(out_off), bk._stream()))
    return out


@pytest.mark.parametrize("placement", list(PLACEMENTS))
def test_pcm16_to_float_reads_where_the_frames_lie(monkeypatch, placement):
    """Mono, stereo and three-channel items inside an int16 arena (0x7F7F outside the items: a stray sample moves the mono mix)."""
    rng = np.random.default_rng(23)
    frames, chans = [1001, 777, 1, 100], [1, 2, 2, 3]
    pcm = [rng.integers(-32768, 32767, f * c, dtype=np.int16) for f, c in zip(frames, chans)]
    out, = twice_direct(monkeypatch, lambda pl: _pcm16(pl[0], frames, chans), [pcm], PLACEMENTS[placement], "ssr_pcm16_to_float")
    assert out.shape == (sum(frames),) and np.isfinite(out).all() and np.abs(out).max() <= 1.0


def test_allreduce_sums_in_place():
    """ssr_allreduce_sums on a one-rank communicator: the caller's buffer is the output - in place, inside a guarded block."""
    bk = B()
    lib = bk._lib.load()
    uid = (C.c_char * 128)()
    bk._lib.check(lib.ssr_comm_unique_id(uid))
    comm = C.c_void_p()
    bk._lib.check(lib.ssr_comm_init_rank(uid, 1, 0, C.byref(comm)))
    try:
        g = G.Guarded()
        buf = g.empty((5,), torch.float64, DEV)
        want = torch.tensor([1.5, -2.0, 1e-300, 3.0, 0.0], dtype=torch.float64)
        buf.copy_(want)
        bk._lib.check(lib.ssr_allreduce_sums(buf.data_ptr(), buf.numel(), comm, torch.cuda.current_stream().cuda_stream))
        g.check()
        G.assert_same_bits(want, buf, "allreduce")
    finally:
        bk._lib.check(lib.ssr_comm_destroy(comm))


# ---- IIR and cross-correlation: driven through the C ABI so that the gaps survive ------------------------------------------------
def _sosfiltfilt(name, data, offs, lens, sos_list):
    """One launch of ssr_sosfiltfilt(_f64) (one design) or ssr_sosfiltfilt_multi / _fast(_f64) (several) over the items at
    data[offs[i] : offs[i] + lens[i]]; y has x's layout.  -> [design][item]."""
    from scipy.signal import sosfilt_zi
    bk = B()
    lib = bk._lib.load()
    dev = torch.device(DEV)
    total, n = int(data.numel()), len(lens)
    off_d, len_d = torch.from_numpy(np.asarray(offs, np.int64)).to(DEV), torch.from_numpy(np.asarray(lens, np.int32)).to(DEV)
    edges = np.array([bk._sos_edge(s) for s in sos_list], np.int32)
    D = len(sos_list)
    if name in ("ssr_sosfiltfilt", "ssr_sosfiltfilt_f64"):
        sos = sos_list[0]
        sos_d, zi_d = torch.from_numpy(sos).to(DEV), torch.from_numpy(np.ascontiguousarray(sosfilt_zi(sos))).to(DEV)
        ws_bytes = int(lib.ssr_sosfiltfilt_workspace_bytes(total, n, int(edges[0])))
        ws = bk._workspace(ws_bytes, dev)
        y = bk.torch.empty((1, total), dtype=torch.float64, device=DEV)
        bk._lib.check(getattr(lib, name)(bk._vp(data), bk._vp(off_d), bk._vp(len_d), n, total, bk._vp(sos_d), bk._vp(zi_d), sos.shape[0],
                                         int(edges[0]), bk._vp(y), bk._vp(ws), ws_bytes, bk._stream()))
    else:
        sos_h, zi_h = np.zeros((D, 8, 6)), np.zeros((D, 8, 2))
        for d, s_ in enumerate(sos_list):
            sos_h[d, :s_.shape[0]], zi_h[d, :s_.shape[0]] = s_, sosfilt_zi(s_)
        ns = np.array([s_.shape[0] for s_ in sos_list], np.int32)
        sos_d, zi_d = torch.from_numpy(sos_h).to(DEV), torch.from_numpy(zi_h).to(DEV)
        ws_name = "ssr_sosfiltfilt_multi_workspace_bytes" if name == "ssr_sosfiltfilt_multi" else "ssr_sosfiltfilt_fast_workspace_bytes"
        ws_bytes = int(getattr(lib, ws_name)(total, n, edges.ctypes.data_as(C.c_void_p), D))
        ws = bk._workspace(ws_bytes, dev)
        y = bk.torch.empty((D, total), dtype=torch.float64, device=DEV)
        bk._lib.check(getattr(lib, name)(bk._vp(data), bk._vp(off_d), bk._vp(len_d), n, total, bk._vp(sos_d), bk._vp(zi_d),
                                         ns.ctypes.data_as(C.c_void_p), edges.ctypes.data_as(C.c_void_p), D, bk._vp(y), total,
                                         bk._vp(ws), ws_bytes, bk._stream()))
    if G.routed():                                    # y has x's layout: nothing but the items may have been written
        G.assert_only_items_written(y, offs, lens, name)
    return [[y[d, o:o + m] for o, m in zip(offs, lens)] for d in range(D)]


def sos_designs():
    from scipy.signal import butter
    return {2: np.ascontiguousarray(butter(2, 0.2, output="sos")), 10: np.ascontiguousarray(butter(10, 0.3, output="sos")),
            18: np.ascontiguousarray(butter(18, 0.4, output="sos"))}          # 1, 5 and 9 sections


@pytest.mark.parametrize("placement", list(PLACEMENTS))
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_sosfiltfilt(monkeypatch, dtype, placement):
    bk = B()
    des = sos_designs()
    f64 = dtype == np.float64
    cases = [("ssr_sosfiltfilt_f64" if f64 else "ssr_sosfiltfilt", [des[o]]) for o in (2, 10, 18)]
    cases.append(("ssr_sosfiltfilt_fast_f64" if f64 else "ssr_sosfiltfilt_fast", [des[2], des[10]]))
    if not f64:
        cases.append(("ssr_sosfiltfilt_multi", [des[2], des[10]]))
    for name, sos_list in cases:
        edge = max(bk._sos_edge(s) for s in sos_list)
        lens = [edge + 1, 128 * 3 + 1, 1000]              # padlen + 1; the segment edge of the fast path
        sigs = signals(lens, dtype, 18)
        twice_ragged(monkeypatch, lambda r, offs: _sosfiltfilt(name, r.data, offs, lens, sos_list), sigs, PLACEMENTS[placement], (name, len(sos_list)))
    # the Python entry points on the packed batch (they refuse views with gaps): outputs and workspaces guarded; 9 sections = the fallback
    sigs = signals([bk._sos_edge(des[18]) + 1, 385, 1000], dtype, 19)
    for exact in (True, False):
        all_finite(twice(monkeypatch, lambda put: bk.sosfiltfilt_multi([des[2], des[10], des[18]], list(sigs), exact=exact), G.GAPS_ODD, ("py multi", exact),
                         in_place=False))
        all_finite(twice(monkeypatch, lambda put: bk.sosfiltfilt(des[10], list(sigs), exact=exact), G.GAPS_ODD, ("py single", exact), in_place=False))


def _xcorr(ra, rb):
    bk = B()
    lib = bk._lib.load()
    ws_bytes = int(lib.ssr_xcorr_workspace_bytes(ra.n, ra.max_len))
    ws = bk._workspace(ws_bytes, torch.device(DEV))
    out = bk.torch.empty(ra.n, dtype=torch.int64, device=DEV)
    bk._lib.check(lib.ssr_xcorr_argmax(bk._vp(ra.data), bk._vp(ra.off), bk._vp(rb.data), bk._vp(rb.off), bk._vp(ra.len), ra.n, ra.max_len,
                                       bk._vp(out), bk._vp(ws), ws_bytes, bk._stream()))
    return out


@pytest.mark.parametrize("placement", list(PLACEMENTS))
def test_xcorr_argmax(monkeypatch, placement):
    bk = B()
    lens = [1, 3, 2048, 2049, 5000]                       # the last three straddle the 2048-lag block
    a = signals(lens, np.float32, 20)
    b = [np.roll(x, k % max(len(x), 1)).astype(np.float32) for k, x in enumerate(a)]
    plain = _xcorr(bk.Ragged.from_list(a, DEV), bk.Ragged.from_list(b, DEV))
    assert np.array_equal(plain.cpu().numpy(), bk.xcorr_argmax(a, b))
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        got = _xcorr(hand_ragged(g, a, PLACEMENTS[placement])[0], hand_ragged(g, b, PLACEMENTS[placement])[0])
        g.check()
    G.assert_same_bits(plain, got, "xcorr")
    assert (got.cpu().numpy() >= 0).all() and (got.cpu().numpy() <= 2 * np.array(lens) - 2).all()


# ---- the workspace-size contract ------------------------------------------------------------------------------------------------
WS_QUERIES = [n for n in SIGNATURES if "_workspace_bytes" in n]
# buffers a refused call may leave written: descriptor uploads, and the resampling launch in front of ssr_stoi / ssr_f0_*
WRITTEN_OK = ("backend.py:put", "backend.py:_uniform_images", "backend.py:_resample_f64")


def refused(monkeypatch, query, call, written_ok=WRITTEN_OK):
    """call(g) under guarded allocations with `query` reporting one byte less than it should: SSR_ERR_WORKSPACE, nothing enqueued -
    every payload but those allocated in the functions `written_ok` names still holds only 0xFF."""
    bk = B()
    lib = bk._lib.load()
    real = getattr(lib, query)
    asked = []

    def one_less(*a):
        n = int(real(*a))
        assert n > 0, (query, a)
        asked.append(n)
        return n - 1
    with monkeypatch.context() as m:
        g = G.Guarded().route(m)
        m.setattr(lib, query, one_less)
        with pytest.raises(bk.SsrHipError, match=r"libssrhip error -4\b"):
            call(g)
        assert asked, query
        g.check()
        assert g.untouched_payloads(written_ok) == [], query


def _ws_cases():
    """query -> a call that sizes its workspace with it (g: the Guarded of the run, for poisoned inputs)."""
    bk = B()
    plan = bk.get_plan(2048, 512, "f64")
    plan3 = bk.get_plan(2229, 480, "f64")
    lens = main_lengths(plan)[:2]
    e32, t32 = pair_of(lens, np.float32, np.float32, 2)
    e64, t3 = pair_of(main_lengths(plan3)[:2], np.float64, np.float32, 2)
    fb = fb_of(plan.n_bins, 16)
    F = plan.n_bins
    est, tgt = images(1025)
    edges = np.tile(np.array([0, F // 3, F], np.int32), (2, len(t32), 1))
    wt, we, idx = family_inputs(16000, np.float32, (1, 2))
    des = sos_designs()
    sig = signals([100, 385, 1000], np.float32, 21)
    dev = lambda a: torch.from_numpy(a).to(DEV)                           # noqa: E731
    rag = lambda arrs: bk.Ragged.from_list(arrs, DEV)                     # noqa: E731
    offs = np.cumsum([0, 100, 385])
    lp = bk.get_plan(1024, 256, "f64")
    lsig = signals([2000, 3000], np.float32, 22)
    w64 = [x.astype(np.float64) for x in sig]
    re, im = ([torch.zeros((lp.frames(n), lp.n_bins), dtype=torch.float32) for n in (2000, 3000)] for _ in range(2))
    bt, be, bidx = bss_inputs(np.float32)
    return {
        "ssr_pair_metrics_workspace_bytes_for": [lambda g: bk.pair_metrics(plan, e32[0], t32, M_LSD), lambda g: bk.pair_metrics(plan, e32[0], t32, M_ALL),
                                                 lambda g: bk.pair_metrics(plan3, e64[0], t3, M_ALL),
                                                 lambda g: bk.pair_metrics(plan3, e64[0], [t.astype(np.float64) for t in t3], M_ALL)],
        "ssr_pair_metrics_multi_workspace_bytes": lambda g: bk.pair_metrics_multi(plan, e32, t32),
        "ssr_pair_metrics_multi_est64_workspace_bytes": lambda g: bk.pair_metrics_multi(plan3, e64, t3),
        "ssr_spectrogram_metrics_workspace_bytes": lambda g: bk.spectrogram_metrics(list(est), list(tgt)),
        "ssr_spectrogram_lsd_bands_workspace_bytes": lambda g: bk.spectrogram_lsd_bands(dev(est), dev(tgt), np.tile(np.array([0, 5, 1025], np.int32), (IMG_N, 1))),
        "ssr_pair_lsd_bands_workspace_bytes": [lambda g: bk.pair_lsd_bands(plan, e32, t32, edges),
                                               lambda g: bk.pair_lsd_bands(plan3, e64, t3, np.tile(np.array([0, 9, plan3.n_bins], np.int32), (2, len(t3), 1)))],
        "ssr_spectrogram_mel_workspace_bytes": lambda g: bk.spectrogram_mel(dev(est), fb),
        "ssr_spectrogram_mel_metrics_workspace_bytes": lambda g: bk.spectrogram_mel_metrics(dev(est), dev(tgt), fb, 5, 7),
        "ssr_pair_mel_metrics_workspace_bytes": lambda g: bk.pair_mel_metrics(plan, e32, t32, fb, 5, 7),
        "ssr_spectrogram_mel_dtw_workspace_bytes": lambda g: bk.spectrogram_mel_dtw(dev(est), dev(tgt), fb, 5, 3),
        "ssr_pair_mel_dtw_workspace_bytes": lambda g: bk.pair_mel_dtw(plan, e32, t32, fb, 5, 3),
        "ssr_stoi_workspace_bytes": lambda g: bk.stoi(wt, we, idx, 16000),
        "ssr_wave_metrics_workspace_bytes": lambda g: bk.wave_metrics(wt, we, idx, 16000),
        "ssr_bss_sdr_workspace_bytes": lambda g: bk.bss_sdr(bt, be, bidx, 512, return_filter=True),
        "ssr_quality_metrics_workspace_bytes": lambda g: bk.quality_metrics(wt, we, idx, 16000),
        "ssr_phase_metrics_workspace_bytes": lambda g: bk.phase_metrics(wt, we, idx),
        "ssr_mrstft_workspace_bytes": lambda g: bk.mrstft_metrics(wt, we, idx),
        "ssr_f0_track_workspace_bytes": lambda g: bk.f0_track(wt, 16000),
        "ssr_f0_metrics_workspace_bytes": lambda g: bk.pitch_metrics(wt, we, idx, 16000),
        "ssr_ola_workspace_bytes": [lambda g: bk.fft_lowpass(lp, lsig, [5, 100]), lambda g: bk.fft_lowpass(lp, lsig, 5),
                                    lambda g: bk.fft_lowpass_multi(lp, lsig, [5, 100, 513]), lambda g: bk.istft(lp, re, im, [2000, 3000])],
        "ssr_xcorr_workspace_bytes": lambda g: bk.xcorr_argmax(sig, sig),
        "ssr_sosfiltfilt_workspace_bytes": [lambda g: bk.sosfiltfilt(des[10], sig), lambda g: bk.sosfiltfilt(des[10], w64)],
        "ssr_sosfiltfilt_multi_workspace_bytes": lambda g: bk.sosfiltfilt_multi([des[2], des[10]], sig),
        "ssr_sosfiltfilt_fast_workspace_bytes": [lambda g: _sosfiltfilt("ssr_sosfiltfilt_fast", rag(sig).data, offs, [100, 385, 1000], [des[2], des[10]]),
                                                 lambda g: bk.sosfiltfilt_multi([des[2], des[10]], w64, exact=False)],
    }


@pytest.mark.parametrize("query", WS_QUERIES)
def test_one_byte_less_than_reported_is_refused(monkeypatch, query):
    bk = B()
    if query == "ssr_pair_metrics_workspace_bytes":
        # the unmasked query is the masked one at SSR_METRIC_ALL; ssr_pair_metrics itself (not _stages) with one byte less
        plan = bk.get_plan(2048, 512, "f64")
        lens = main_lengths(plan)[:2]
        ests, tgt = pair_of(lens, np.float32, np.float32)
        lib = plan.lib
        with monkeypatch.context() as m:
            g = G.Guarded().route(m)
            b = bk.PairBatch(plan, bk.Ragged.from_list(ests[0], DEV), bk.Ragged.from_list(tgt, DEV))
            need = int(lib.ssr_pair_metrics_workspace_bytes(plan.handle, b.est.n, b.est.max_len, b.rows.total))
            assert need == int(lib.ssr_pair_metrics_workspace_bytes_for(plan.handle, b.est.n, b.est.max_len, b.rows.total, M_ALL))
            ws = bk._workspace(need - 1, torch.device(DEV))
            e, t = b.est, b.tgt
            for fn, extra in ((lib.ssr_pair_metrics, ()), (lib.ssr_pair_metrics_stages, (7,))):
                rc = fn(plan.handle, bk._vp(e.data), bk._vp(e.off), bk._vp(t.data), bk._vp(t.off), bk._vp(e.len), bk._vp(b.rows.off), e.n,
                        e.max_len, b.rows.total, M_ALL, bk._vp(b.out), bk._vp(ws), need - 1, bk._stream(), *extra)
                assert rc == bk._lib.ERR_WORKSPACE
            g.check()
            assert g.untouched_payloads(WRITTEN_OK) == []
        return
    cases = _ws_cases()
    assert query in cases, "a *_workspace_bytes query of the header without a refusal case: %s" % query
    # (nothing is resampled in front of ssr_bss_sdr: its refused call may leave the descriptor uploads written and nothing else)
    written_ok = WRITTEN_OK[:2] if query == "ssr_bss_sdr_workspace_bytes" else WRITTEN_OK
    for call in (cases[query] if isinstance(cases[query], list) else [cases[query]]):
        refused(monkeypatch, query, call, written_ok)


def test_every_workspace_query_of_the_header_has_a_refusal_case():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssr_hip.h")).read()
    declared = set(re.findall(r"size_t (ssr_\w*_workspace_bytes\w*)\(", header))
    assert declared == set(WS_QUERIES)
    assert declared - {"ssr_pair_metrics_workspace_bytes"} == set(_ws_cases())


# ---- the inventory: every entry point of include/ssr_hip.h that takes a device pointer -> the case that runs it guarded -----------
HOST_ONLY = {"ssr_last_error", "ssr_version", "ssr_plan_create", "ssr_plan_create_ex", "ssr_plan_destroy", "ssr_plan_query",
             "ssr_plan_set_lowpass_engine", "ssr_plan_set_tl_weights", "ssr_tl_weights", "ssr_tl_weights_ex", "ssr_num_frames",
             "ssr_stoi_band_edges", "ssr_quality_bands", "ssr_resample_plan", "ssr_flac_info", "ssr_flac_decode_pcm16",
             "ssr_flac_decode_i32", "ssr_bootstrap_geometry", "ssr_comm_unique_id", "ssr_comm_init_rank", "ssr_comm_destroy"}
COVERAGE = {
    "ssr_stft": "test_stft, test_istft (conv engine, ssr_plan_create_ex plans)",
    "ssr_magphase": "test_elementwise_helpers",
    "ssr_pair_metrics": "test_pair_metrics (f32: _pair_metrics_direct)",
    "ssr_pair_metrics_stages": "test_pair_metrics (f32)",
    "ssr_pair_metrics_est64": "test_pair_metrics (est64)",
    "ssr_pair_metrics_f64": "test_pair_metrics (f64)",
    "ssr_pair_metrics_multi": "test_pair_metrics_multi",
    "ssr_pair_metrics_multi_est64": "test_pair_metrics_multi (2229-480-f64: the fast path, 2048-512-f64: the fallback)",
    "ssr_spectrogram_metrics": "test_spectrogram_metrics",
    "ssr_spectrogram_lsd_bands": "test_spectrogram_image_entry_points",
    "ssr_pair_lsd_bands": "test_pair_image_families (f32)",
    "ssr_pair_lsd_bands_est64": "test_pair_image_families (est64)",
    "ssr_spectrogram_mel": "test_spectrogram_image_entry_points",
    "ssr_spectrogram_mel_metrics": "test_spectrogram_image_entry_points",
    "ssr_pair_mel_metrics": "test_pair_image_families (f32)",
    "ssr_pair_mel_metrics_est64": "test_pair_image_families (est64)",
    "ssr_spectrogram_mel_dtw": "test_spectrogram_image_entry_points",
    "ssr_pair_mel_dtw": "test_pair_image_families (f32)",
    "ssr_pair_mel_dtw_est64": "test_pair_image_families (est64)",
    "ssr_stoi": "test_stoi_and_pitch_read_where_the_signals_lie (inputs), test_per_pair_families (wrapper: outputs, workspace)",
    "ssr_wave_metrics": "test_per_pair_families",
    "ssr_bss_sdr": "test_guard_bands_and_poison",
    "ssr_quality_metrics": "test_per_pair_families",
    "ssr_phase_metrics": "test_per_pair_families",
    "ssr_mrstft_metrics": "test_per_pair_families",
    "ssr_f0_track": "test_stoi_and_pitch_read_where_the_signals_lie (inputs), test_per_pair_families (wrapper: outputs, workspace)",
    "ssr_f0_metrics": "test_stoi_and_pitch_read_where_the_signals_lie (inputs), test_per_pair_families (wrapper: outputs, workspace)",
    "ssr_bootstrap_means": "test_bootstrap",
    "ssr_bootstrap_summary": "test_bootstrap (its input is ssr_bootstrap_means' guarded output)",
    "ssr_to_log": "test_elementwise_helpers",
    "ssr_from_log": "test_elementwise_helpers",
    "ssr_energy_sums": "test_elementwise_helpers",
    "ssr_scale_items": "test_elementwise_helpers",
    "ssr_sispec_multichannel": "test_elementwise_helpers",
    "ssr_fft_lowpass": "test_fft_lowpass (per item)",
    "ssr_fft_lowpass_multi": "test_fft_lowpass (one cut, multi)",
    "ssr_istft": "test_istft (C ABI, row gaps)",
    "ssr_resample_poly": "test_resample_poly (f32, exact), test_resample_poly_chain_and_sinc (fused=False)",
    "ssr_resample_poly_mfma": "test_resample_poly (f32, exact=False)",
    "ssr_resample_poly_f64": "test_resample_poly (f64)",
    "ssr_resample_poly_chain": "test_resample_poly_chain_and_sinc",
    "ssr_resample_sinc": "test_resample_poly_chain_and_sinc",
    "ssr_pcm16_to_float": "test_pcm16_to_float_reads_where_the_frames_lie (inputs), test_upload_decoded (wrapper: device twin, output)",
    "ssr_xcorr_argmax": "test_xcorr_argmax",
    "ssr_sosfiltfilt": "test_sosfiltfilt (f32)",
    "ssr_sosfiltfilt_f64": "test_sosfiltfilt (f64)",
    "ssr_sosfiltfilt_multi": "test_sosfiltfilt (f32)",
    "ssr_sosfiltfilt_fast": "test_sosfiltfilt (f32)",
    "ssr_sosfiltfilt_fast_f64": "test_sosfiltfilt (f64)",
    "ssr_allreduce_sums": "test_allreduce_sums_in_place",
}


def test_the_inventory_is_the_header():
    """Every symbol the header declares is host-only, a workspace query (test_one_byte_less_than_reported_is_refused) or has a case."""
    assert set(SIGNATURES) == HOST_ONLY | set(WS_QUERIES) | set(COVERAGE)
    for name, cases in COVERAGE.items():
        for case in cases.replace(",", " ").split():
            if case.startswith("test_"):
                assert case in globals(), (name, case)
