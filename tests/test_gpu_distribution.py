"""GPU tests of the distribution family (fd, kd): ssr_frechet, ssr_kernel_distance and ssr_pairwise_distances
through the C ABI at the shapes, bars and bit-level properties of tests/test_distribution_host.py; the public functions on host and
resident, NumPy and torch inputs; the median bandwidth against the oracle's; guard bands, poisoned gaps and a poisoned workspace; the
workspace queries; and SSR_Eval_Helper(distribution=...) end to end.

Bars: distribution_oracle.TOL_* (means 1e-12 max |x|, covariance 1e-10 of the largest diagonal entry, fd 1e-9 S on full-rank and 1e-6 S
on rank-deficient inputs, kernel means and mmd2 1e-10).  Each test prints the worst differences it saw; on an MI355X: mean 3.6e-16
max |x|, covariance 1.1e-15 of the largest diagonal entry, fd 1.2e-14 S on full-rank sets (D = 128) and 2.4e-8 S on rank-deficient
ones, kernel means 3.3e-14, at most 15 sweeps (the emulated bodies: 3.6e-16, 1.1e-15, 1.2e-14, 2.3e-8, 3.3e-14)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import distribution_oracle as O
import guarded as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
same_bits = O.same_bits
HP = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
DP = lambda t: None if t is None else C.c_void_p(t.data_ptr())            # noqa: E731


def _lib():
    from ssr_eval_amd import _lib as L
    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def abi_fd(sets, dtype=np.float64, max_sweeps=60, moments=True, ld_extra=0, gap=0, g=None):
    """ssr_frechet on sets = [ref, est_0, ...] packed with NaN between rows and sets -> (out [K][8], moments or None); g: a
    guarded.Guarded that supplies the outputs and the workspace."""
    L, lib = _lib()
    buf, off, rows, d, ld = O.pack(sets, dtype, ld_extra, gap)
    K = len(sets) - 1
    data = torch.from_numpy(buf).to(DEV)
    need = int(lib.ssr_frechet_workspace_bytes(HP(rows), K, d))
    assert need > 0
    if g is None:
        out = torch.full((K, 8), -123.0, dtype=torch.float64, device=DEV)
        mom = torch.full((K + 1, d + d * d), -123.0, dtype=torch.float64, device=DEV) if moments else None
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    else:
        out = g.empty((K, 8), torch.float64, DEV)
        mom = g.empty((K + 1, d + d * d), torch.float64, DEV) if moments else None
        ws = g.alloc(need, DEV)
    L.check(lib.ssr_frechet(DP(data), int(dtype == np.float64), HP(off), HP(rows), K, d, ld, max_sweeps, DP(out), DP(mom), DP(ws), need, _stream()))
    torch.cuda.synchronize()
    assert same_bits(data.cpu().numpy(), buf)
    return out.cpu().numpy(), None if mom is None else mom.cpu().numpy()


def abi_kd(sets, gammas, dtype=np.float64, scale=1000.0, ld_extra=0, gap=0, g=None):
    L, lib = _lib()
    buf, off, rows, d, ld = O.pack(sets, dtype, ld_extra, gap)
    K, gm = len(sets) - 1, np.ascontiguousarray(gammas, np.float64)
    data = torch.from_numpy(buf).to(DEV)
    need = int(lib.ssr_kernel_distance_workspace_bytes(HP(rows), K, d, len(gm)))
    assert need > 0
    if g is None:
        out, ws = torch.full((K, len(gm), 4), -123.0, dtype=torch.float64, device=DEV), torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    else:
        out, ws = g.empty((K, len(gm), 4), torch.float64, DEV), g.alloc(need, DEV)
    L.check(lib.ssr_kernel_distance(DP(data), int(dtype == np.float64), HP(off), HP(rows), K, d, ld, HP(gm), len(gm), scale, DP(out), DP(ws), need,
                                    _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _kernel_case(n, m, d):
    r, e = O.gaussian_set(n, d, 1, 10.0, scale=1.0 / math.sqrt(d)), O.gaussian_set(m, d, 2, 10.0, shift=0.1, scale=1.0 / math.sqrt(d))
    return r, e, O.kernel_means(r, e, O.GAMMAS8)


# ---- the C ABI at the host test's shapes and bars ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,m", O.FRECHET_SHAPES + O.DEFICIENT_SHAPES, ids=lambda v: str(v))
def test_frechet_shapes(d, n, m):
    deficient = (d, n, m) in O.DEFICIENT_SHAPES
    r, e = O.frechet_sets(d, n, m)
    rank, cond = O.rank_and_cond(r)
    assert rank == min(d, n - 1) and cond <= (1e6 if deficient else 1e4)
    out, mom = abi_fd([r, e])
    worst = O.check_frechet(out, mom, [r, e], deficient=deficient, name=(d, n, m))
    print((d, n, m), "worst mean %.3g max|x|, cov %.3g, fd %.3g S; sweeps %d / %d, rank %d" % (worst + tuple(out[0, 5:])))
    assert out[0, 7] == rank and out[0, 5] <= 30 and out[0, 6] <= 30
    assert same_bits(abi_fd([r, e], moments=False)[0], out)                    # moments_out = NULL changes no bit


def test_frechet_special_rows_and_bounded_exit():
    d = 8
    r, e = O.frechet_sets(d, 40, 33, seed=5)
    rc, ec = r.copy(), e.copy()
    rc[:, 3], ec[:, 3] = 2.5, 2.5
    out, mom = abi_fd([rc, ec])
    O.check_frechet(out, mom, [rc, ec], deficient=True, name="constant column")
    assert out[0, 7] == d - 1
    big = [O.gaussian_set(60, d, 7, 10.0) + 1e4, O.gaussian_set(50, d, 8, 10.0, scale=1.1) + 1e4]
    out, mom = abi_fd(big)
    print("means of 1e4: cov %.3g of the largest diagonal entry, fd %.3g S" % O.check_frechet(out, mom, big, name="means of 1e4")[1:])
    out, _ = abi_fd([r, r.copy()])
    assert abs(out[0, 0]) <= 1e-12 * (out[0, 2] + out[0, 3]) and out[0, 1] == 0.0
    out, mom = abi_fd([r[:2], e])
    O.check_frechet(out, mom, [r[:2], e], deficient=True, name="n = 2")
    for sets in ([r[:1], e], [r, e[:1]], [r, e[:0]]):
        out, mom = abi_fd(sets)
        assert np.isnan(out[0, 0]) and np.isnan(out[0, 4]) and not np.isinf(out).any() and not np.isinf(mom).any()
    bad = e.copy()
    bad[5, 2] = np.inf
    out, _ = abi_fd([r, bad, e])
    assert np.isnan(out[0, 0]) and out[0, 6] == -1 and not np.isinf(out).any() and same_bits(out[1], abi_fd([r, e])[0][0])
    # the bounded exit: max_sweeps = 1 on a D = 32 case
    r, e = O.frechet_sets(32, 150, 140)
    out, _ = abi_fd([r, e], max_sweeps=1)
    assert np.isnan(out[0, 0]) and np.isnan(out[0, 4]) and out[0, 5] == -1 and np.isfinite(out[0, 1:4]).all()


def test_frechet_layouts_and_bit_level_properties():
    d = 33
    chunk = max(256, 4 * d)
    r = O.gaussian_set(chunk + 1, d, 11, 1e2)
    ests = [O.gaussian_set(m, d, 20 + m, 1e2, shift=0.1 * m / 70, scale=1.0 + m / 700) for m in (70, 2 * chunk, 131)]
    base, mom = abi_fd([r] + ests)
    O.check_frechet(base, mom, [r] + ests, name="K = 3")
    for k in range(3):
        alone, mom1 = abi_fd([r, ests[k]])
        assert same_bits(alone[0], base[k]) and same_bits(mom1[1], mom[1 + k]) and same_bits(mom1[0], mom[0])
    back, _ = abi_fd([r] + ests[::-1], ld_extra=3, gap=7)
    assert same_bits(back[::-1], base)
    r32, e32 = r[:90].astype(np.float32), ests[0].astype(np.float32)
    out32, mom32 = abi_fd([r32, e32], np.float32, ld_extra=3, gap=5)
    O.check_frechet(out32, mom32, [r32, e32], np.float32, name="float32")
    assert same_bits(out32, abi_fd([r32.astype(np.float64), e32.astype(np.float64)])[0])
    for p2 in (2.0 ** -7, 2.0 ** 10):
        sc, _ = abi_fd([p2 * r] + [p2 * x for x in ests])
        assert same_bits(sc[:, :5], base[:, :5] * p2 * p2) and same_bits(sc[:, 5:], base[:, 5:])


@pytest.mark.parametrize("n,m,d", O.KERNEL_SHAPES, ids=lambda v: str(v))
def test_kernel_distance_shapes(n, m, d):
    r, e, want = _kernel_case(n, m, d)
    got8 = abi_kd([r, e], O.GAMMAS8, ld_extra=3, gap=5)
    worst = float(np.max(np.abs(got8[0, :, 1:] - want[:, 1:])))
    print((n, m, d), "worst kernel mean / mmd2 difference %.3g" % worst)
    assert worst <= O.TOL_KERNEL and same_bits(got8[0, :, 0], 1000.0 * got8[0, :, 1])
    for j in (0, 5):
        assert same_bits(abi_kd([r, e], [O.GAMMAS8[j]])[0, 0], got8[0, j])
    e2 = O.gaussian_set(m + 3, d, 3, 10.0, scale=1.0 / math.sqrt(d))
    many = abi_kd([r, e2, e, e2[:1]], O.GAMMAS8[:2])
    assert same_bits(many[1], got8[0, :2]) and same_bits(many[0], abi_kd([r, e2], O.GAMMAS8[:2])[0]) and np.isnan(many[2]).all()
    got32 = abi_kd([r.astype(np.float32), e.astype(np.float32)], O.GAMMAS8[:1], np.float32)
    assert np.max(np.abs(got32[0, :, 1:] - O.kernel_means(O.as_read(r, np.float32), O.as_read(e, np.float32), O.GAMMAS8[:1])[:, 1:])) <= O.TOL_KERNEL
    assert np.isnan(abi_kd([r[:1], e], [0.1])).all() and np.isnan(abi_kd([r, e[:0]], [0.1])).all()


@pytest.mark.parametrize("n", [2, 65, 130])
def test_pairwise_distances(n):
    L, lib = _lib()
    d = 5
    x = O.gaussian_set(n + 9, d, n, 10.0)
    index = (np.arange(n, dtype=np.int64) * 7) % (n + 9)
    for dtype in (np.float64, np.float32):
        buf, off, rows, _, ld = O.pack([x], dtype, ld_extra=2, gap=3)
        data = torch.from_numpy(buf).to(DEV)
        g = G.Guarded()
        out, ws = g.empty((n * (n - 1) // 2,), torch.float64, DEV), g.alloc(L.DISTRIBUTION_PAIRWISE_WORKSPACE, DEV)
        L.check(lib.ssr_pairwise_distances(DP(data), int(dtype == np.float64), int(off[0]), n + 9, d, ld, HP(index), n, DP(out), DP(ws),
                                           L.DISTRIBUTION_PAIRWISE_WORKSPACE, _stream()))
        g.check()
        got, want = out.cpu().numpy(), O.pairwise(O.as_read(x, dtype), index)
        assert np.max(np.abs(got - want)) <= 1e-14 * max(1.0, want.max())
        assert O.lower_median(got)[1] == O.lower_median(want)[1]


# ---- the public functions ---------------------------------------------------------------------------------------------------------
def test_public_functions_inputs_lists_and_median():
    import ssr_eval_amd as S
    from ssr_eval_amd import backend as B
    from ssr_eval_amd import distribution as DM
    d = 16
    r = O.gaussian_set(300, d, 1, 1e2)
    ests = [O.gaussian_set(m, d, 2 + m, 1e2, shift=0.2, scale=1.1) for m in (130, 77)]
    o = [O.frechet(r, e) for e in ests]
    fd = S.frechet_distance(ests, r)
    assert isinstance(fd, list) and all(abs(v - w["fd"]) <= O.TOL_FD * w["S"] for v, w in zip(fd, o))
    # a list of estimate sets equals the sets one by one, bit for bit; host / resident, NumPy / torch
    t = lambda a: torch.from_numpy(a)      # noqa: E731
    for k, e in enumerate(ests):
        for est, ref in ((e, r), (t(e), t(r)), (t(e).to(DEV), t(r).to(DEV)), (e, t(r).to(DEV))):
            one = S.frechet_distance(est, ref)
            assert isinstance(one, float) and np.float64(one).tobytes() == np.float64(fd[k]).tobytes()
    st = S.frechet_distance(ests[0], r, return_stats=True)
    assert list(st) == ["fd", "dmu2", "tr_ref", "tr_est", "tr_sqrt", "sweeps_ref", "sweeps_est", "rank_ref"] and st["rank_ref"] == d and st["fd"] == fd[0]
    assert math.isnan(S.frechet_distance(ests[0], r, max_sweeps=1))
    out, mom = B.frechet_stats(r.astype(np.float32), [e.astype(np.float32) for e in ests], return_moments=True)
    O.check_frechet(out, mom, [r] + ests, np.float32, name="float32 through backend")
    # the median bandwidth: the oracle's pair, gamma within 1e-12 relative
    gamma = DM.median_gamma(r)
    want = O.median_gamma(r)
    dist = B.pairwise_distances(r, O.subsample_index(len(r)))
    assert O.lower_median(dist)[1] == O.lower_median(O.pairwise(r, O.subsample_index(len(r))))[1] and abs(gamma / want - 1.0) <= 1e-12
    big = O.gaussian_set(2500, 3, 9, 10.0)                                       # more rows than the cap: evenly strided
    assert abs(DM.median_gamma(big) / O.median_gamma(big) - 1.0) <= 1e-12
    assert math.isnan(DM.median_gamma(np.ones((5, 3)))) and math.isnan(S.kernel_distance(np.ones((5, 3)), np.ones((5, 3))))
    kd = S.kernel_distance(ests, r)
    km = [O.kernel_means(r, e, [want])[0] for e in ests]
    assert all(abs(v - 1000.0 * w[1]) <= 1000.0 * O.TOL_KERNEL for v, w in zip(kd, km))
    for k, e in enumerate(ests):
        assert np.float64(S.kernel_distance(t(e).to(DEV), r)).tobytes() == np.float64(kd[k]).tobytes()
    assert abs(S.kernel_distance(ests[0], r, bandwidth=2.0, scale=1.0) - O.kernel_means(r, ests[0], [0.125])[0, 1]) <= O.TOL_KERNEL
    both = S.distribution_distance(ests, r)
    assert list(both) == ["fd", "kd"] and both["fd"] == fd and both["kd"] == kd and list(S.distribution_distance(ests[0], r, metrics=("kd",))) == ["kd"]


# ---- memory discipline --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("moments", [True, False], ids=["moments_out", "null"])
@pytest.mark.parametrize("d", [33, 128])
def test_guard_bands_and_poison(d, moments, dtype):
    """ssr_frechet, ssr_kernel_distance on sets with NaN between their rows (ld = D + 3) and between the sets, the outputs and the
    workspace between 0xFF guard bands and 0xFF inside: the same bits as the plain run, no guard damaged, the input untouched, NaN
    nowhere in the results (a read outside a row or of an unwritten workspace byte would be NaN)."""
    chunk = max(256, 4 * d)
    sets = [O.gaussian_set(chunk + 3, d, 1, 1e2), O.gaussian_set(2 * d + 5, d, 2, 1e2, shift=0.1), O.gaussian_set(65, d, 3, 1e2, scale=1.2)]
    sets = [s.astype(dtype) for s in sets]
    plain = abi_fd(sets, dtype, moments=moments, ld_extra=3, gap=5)
    g = G.Guarded()
    got = abi_fd(sets, dtype, moments=moments, ld_extra=3, gap=5, g=g)
    g.check()
    G.assert_same_bits([p for p in plain if p is not None], [p for p in got if p is not None], "ssr_frechet")
    assert np.isfinite(got[0]).all() and (got[1] is None or np.isfinite(got[1]).all())
    O.check_frechet(got[0], got[1] if moments else abi_fd(sets, dtype, ld_extra=3, gap=5)[1], sets, dtype, deficient=True, name="guarded")
    kp = abi_kd(sets, O.GAMMAS8[:3], dtype, ld_extra=3, gap=5)
    g = G.Guarded()
    kg = abi_kd(sets, O.GAMMAS8[:3], dtype, ld_extra=3, gap=5, g=g)
    g.check()
    G.assert_same_bits(kp, kg, "ssr_kernel_distance")
    assert np.isfinite(kg).all()


def test_one_byte_less_than_reported_is_refused(monkeypatch):
    """With a workspace query reporting one byte less than it should the call is SSR_ERR_WORKSPACE and nothing is enqueued: the
    outputs and the workspace still hold only 0xFF."""
    from ssr_eval_amd import backend as B
    L, lib = _lib()
    r, e = O.frechet_sets(8, 40, 33)
    for name, call in (("ssr_frechet_workspace_bytes", lambda: B.frechet_stats(r, [e], return_moments=True)),
                       ("ssr_kernel_distance_workspace_bytes", lambda: B.kernel_sums(r, [e], [0.5, 1.0]))):
        real, asked = getattr(lib, name), []

        def one_less(*a, real=real, asked=asked):
            n = int(real(*a))
            assert n > 0
            asked.append(n)
            return n - 1
        with monkeypatch.context() as m:
            g = G.Guarded().route(m)
            m.setattr(lib, name, one_less)
            with pytest.raises(B.SsrHipError, match=r"libssrhip error -4\b"):
                call()
            assert asked and len(g.blocks) >= 2
            g.check()
            assert g.untouched_payloads() == []


# ---- SSR_Eval_Helper(distribution=...) -----------------------------------------------------------------------------------------------
FS = 16000


def _write_tree(root):
    """Two speakers x six short files: a tone with harmonics under a slow level movement, plus noise; every file its own pitch."""
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(12)
    for s, spk in enumerate(("p360", "p361")):
        (root / spk).mkdir(parents=True)
        for i in range(6):
            n = 6000 + 331 * i + 97 * s
            t = np.arange(n) / FS
            f0 = 150.0 + 35.0 * i + 60.0 * s
            x = sum(a * np.sin(2 * np.pi * f0 * h * t) for h, a in ((1, 0.3), (2, 0.1), (8, 0.05), (16, 0.03)))
            x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 5.0 * t + i))
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), (x + 0.02 * rng.standard_normal(n)).astype(np.float32), FS)


def test_evaluate_with_distribution(tmp_path, monkeypatch):
    """evaluate() on a 2 x 6-file tree with two FFT cutoffs: per_key equals distribution_distance on the embeddings recomputed
    outside evaluate() from the very waves the helper embedded; every other entry of the result is, bit for bit, the run without the
    option; a callable embed with D = 8 is honoured."""
    import ssr_eval_amd as S
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd import eval as E
    root = tmp_path / "vctk_test"
    _write_tree(root)
    cutoffs = [2000, 3000]
    keys = ["proc_fft_%d_%d" % (2 * c, FS) for c in cutoffs]
    seen = []
    real = E.embed_waves

    def recording(settings, am, waves, sr):
        out = real(settings, am, waves, sr)
        seen.append(([w.detach().cpu().clone() for w in waves], sr, out.copy()))
        return out
    monkeypatch.setattr(E, "embed_waves", recording)

    def go(**kw):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=FS, output_sr=FS, evaluation_sr=FS, test_data_root=str(root),
                            setting_fft={"cutoff_freq": list(cutoffs)}, **kw)
        return h, h.evaluate(save_json=False, batch_files=5)
    h, on = go(distribution=True)
    kept, _ = list(seen), seen.clear()
    _, none = go()
    assert not seen and go(distribution=None)[1] == none
    block = on.pop("distribution")
    assert on == none and list(on) == list(none)                                 # every other entry, bit for bit (floats compare by value: NaN-free here)
    for spk in ("p360", "p361"):
        for f in none[spk]:
            for k in keys:
                for m, v in none[spk][f][k].items():
                    assert np.float64(v).tobytes() == np.float64(on[spk][f][k][m]).tobytes()
    assert list(block) == ["settings", "dim", "n", "per_key"] and block["n"] == 12 and list(block["per_key"]) == keys
    n_mels = block["dim"] // 2
    assert block["dim"] == 2 * n_mels and block["settings"] == {"embed": "logmel_stats", "bandwidth": "median", "scale": 1000.0, "max_sweeps": 60,
                                                                "metrics": ["fd", "kd"]}
    # the embeddings recomputed outside evaluate(): per batch the targets (one per file), then the outputs file-major, key-minor
    ref, est = [], [[], []]
    for waves, sr, _ in kept:
        assert sr == FS and len(waves) % 3 == 0
        nf = len(waves) // 3
        emb = S.embed_logmel_stats(h.audio_metrics, [w.to(DEV) for w in waves]).cpu().numpy()
        assert emb.shape == (3 * nf, block["dim"]) and emb.dtype == np.float64
        L = [10.0 * np.log10(np.maximum(h.audio_metrics.mel_spectrogram(w.numpy()).numpy().reshape(-1, n_mels).astype(np.float64), 1e-10)) for w in waves[:2]]
        assert all(np.max(np.abs(emb[i] - np.concatenate([l.mean(0), l.std(0)]))) <= 1e-9 for i, l in enumerate(L))
        ref += list(emb[:nf])
        for i in range(nf):
            for k in range(2):
                est[k].append(emb[nf + 2 * i + k])
    assert len(ref) == 12
    want = S.distribution_distance([np.array(e) for e in est], np.array(ref))
    for k, key in enumerate(keys):
        got = block["per_key"][key]
        print(key, got, "recomputed", want["fd"][k], want["kd"][k])
        assert list(got) == ["fd", "kd"]
        assert np.float64(got["fd"]).tobytes() == np.float64(want["fd"][k]).tobytes() and np.float64(got["kd"]).tobytes() == np.float64(want["kd"][k]).tobytes()
    # the harder cutoff is further from the targets
    assert block["per_key"][keys[0]]["fd"] > block["per_key"][keys[1]]["fd"] > 0.0
    # a callable embed with D = 8 is honoured
    seen.clear()

    def embed8(waves, sr):
        assert sr == FS and all(isinstance(w, torch.Tensor) and w.dim() == 1 for w in waves)
        return torch.stack([torch.stack([w.double().abs().mean() * (j + 1) + 0.01 * j * w.double().std() for j in range(8)]) for w in waves])
    _, res8 = go(distribution={"embed": embed8, "metrics": ("fd",), "max_sweeps": 100})
    b8 = res8.pop("distribution")
    assert res8 == none and b8["dim"] == 8 and b8["n"] == 12 and b8["settings"]["embed"] == "callable" and b8["settings"]["metrics"] == ["fd"]
    assert all(list(v) == ["fd"] and math.isfinite(v["fd"]) for v in b8["per_key"].values())
    assert S.compare_results is not None
