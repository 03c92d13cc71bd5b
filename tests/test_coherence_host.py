"""CPU tests of the magnitude-squared coherence family (msc, coh_sdr, coh_bw): the float64 oracle
(tests/coherence_oracle.py) pinned to scipy.signal.coherence, a g++ build of the kernel bodies (ssr_coherence.h) against the oracle -
the input list, the shapes where the geometry can go wrong, the exact facts, the bit-level properties -, the C ABI's argument
checks (they return before anything touches a device), the header / ctypes table / library agreement, and AudioMetrics /
SSR_Eval_Helper(coherence=...) validation and key order.

Tolerances: msc and the per-bin coherence within 1e-9, the bar of the phase and multi-resolution kernels on the same transform;
coh_sdr within 1e-6 dB, the bar of sdr; coh_bins equal.  The transform's rounding error is a few 1e-16 log2(N) of a segment's
largest bin, so a bin whose Sxx and Syy are at ratio r of their maxima has a relative error of about 1e-15 / r in g2: every
compared pair is asserted to have r >= 1e-4 and no bin within 1e-6 of the counting threshold (coherence_oracle.conditioning).
Worst differences seen in emulation: msc 2.0e-15, per bin 2.2e-15, coh_sdr 3.7e-13 dB (on an MI355X: 2.0e-15, 2.0e-15, 4.8e-13 dB)."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import coherence_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, TOL_DB, R_MIN, THR_MARGIN, FR = O.TOL, O.TOL_DB, O.R_MIN, O.THR_MARGIN, O.FR
band_table, check_rows, _len_for_segments = O.band_table, O.check_rows, O.len_for_segments


# ---- the oracle against SciPy -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(O.CASES)))
def test_oracle_coherence_is_scipys(case):
    from scipy.signal import coherence
    n, N, H = O.CASES[case]
    x, y = O.input_pair(n, 100 + case)
    g2, _ = O.gamma2(x, y, N, H)
    _, want = coherence(x, y, window="hann", nperseg=N, noverlap=N - H, detrend=False)
    print(n, N, H, "worst difference to scipy.signal.coherence", np.max(np.abs(g2 - want)))
    assert want.shape == g2.shape and np.max(np.abs(g2 - want)) <= 1e-12


def test_oracle_nan_cases_zero_rule_and_bias():
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal(4000), rng.standard_normal(4000)
    assert [O.segments(n, 256, 64) for n in (0, 255, 256, 319, 320, 4000)] == [0, 0, 1, 1, 2, 59]
    for n in (255, 256, 319):                                  # K = 0 and K = 1
        rows, g2 = O.coherence(x[:n], y[:n], 256, 64)
        assert np.isnan(rows).all() and np.isnan(g2).all()
    rows, g2 = O.coherence(x, y, 256, 64, [(3, 2), (0, 128)])
    assert np.isnan(rows[0]).all() and np.isfinite(rows[1]).all()
    one = O.gamma2(x[:256], y[:256], 256, 64)[0]               # one segment: identically 1 (why K < 2 is NaN)
    assert np.max(np.abs(one - 1.0)) < 1e-12
    # unrelated signals: E[g2] is about 1 / K
    K = O.segments(4000, 256, 256)
    assert K == 15 and abs(O.coherence(x, y, 256, 256)[0][0, 0] * K - 1.0) < 0.25
    # digital silence is incoherent, not NaN; a linear filter on the estimate changes nothing
    z = np.zeros(4000)
    rows0, g0 = O.coherence(x, z, 256, 64)
    assert np.all(g0 == 0.0) and rows0[0, 0] == 0.0 and rows0[0, 2] == 0.0
    same, _ = O.coherence(x, x, 256, 64)
    assert same[0, 0] >= 1 - 1e-12 and same[0, 1] >= 120.0 and same[0, 2] == 129


# ---- the kernel bodies compiled for the host ------------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "coherence_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libcoherence_emu.so")


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    lib = C.CDLL(EMU_SO)
    lib.coherence_emu.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    return lib


def run_emu(lib, tgts, ests, idx, n_fft, hop, bands, thr=0.5, spectrum=True):
    """-> (out [n_est, n_bands, 3], g2 [n_est, n_fft / 2 + 1] or None)"""
    tdt, edt = tgts[0].dtype, (ests[0].dtype if ests else tgts[0].dtype)
    t64, e64 = tdt == np.float64, edt == np.float64
    P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    tl = np.array([len(t) for t in tgts], np.int32)
    el = np.array([len(e) for e in ests], np.int64)
    to = np.concatenate(([0], np.cumsum(tl)[:-1])).astype(np.int64)
    eo = np.concatenate(([0], np.cumsum(el)[:-1])).astype(np.int64)
    td = np.concatenate(list(tgts) + [np.zeros(1, tdt)])
    ed = np.concatenate(list(ests) + [np.zeros(1, edt)])
    idx = np.ascontiguousarray(idx, np.int32)
    tab = band_table(bands, len(ests))
    out = np.full((len(ests), tab.shape[1], 3), -123.0)
    g2 = np.full((len(ests), n_fft // 2 + 1), -7.0) if spectrum else None
    assert lib.coherence_emu(P(td), int(t64), P(to), P(tl), len(tgts), P(ed), int(e64), P(eo), P(idx), len(ests), n_fft, hop,
                             tab.shape[1], P(tab), thr, P(out), P(g2) if spectrum else None) == 0
    return out, g2


@pytest.mark.parametrize("case", range(len(O.CASES)))
def test_emulated_kernels_match_the_oracle_on_the_input_list(emu, case):
    """The seeded pair (coherent below half Nyquist, incoherent above) at 16 kHz, as float64 and as float32 signals, on the full band,
    the two halves and an interior band; what the numbers mean: full-band coh_sdr a few dB, the upper half well below 0 dB."""
    n, N, H = O.CASES[case]
    x, y = O.input_pair(n, 100 + case)
    bands = O.input_bands(N)
    margin, rx, ry = O.conditioning(x, y, N, H)
    print("n %d N %d H %d: min |g2 - 0.5| %.3g, min Sxx / max %.3g, min Syy / max %.3g" % (n, N, H, margin, rx, ry))
    assert margin >= THR_MARGIN and rx >= R_MIN and ry >= R_MIN
    for dt in (np.float64, np.float32):
        tg, es = [x.astype(dt)], [y.astype(dt)]
        out, g2 = run_emu(emu, tg, es, [0], N, H, bands)
        worst = check_rows(out, g2, tg, es, [0], N, H, bands, what="inputs")
        print("worst msc %.3g, per bin %.3g, coh_sdr %.3g dB" % tuple(worst))
        assert 3.0 < out[0, 0, 1] < 6.0 and -14.0 < out[0, 2, 1] < -5.0 and out[0, 1, 1] > 12.0
        assert out[0, 1, 0] > 0.9 and out[0, 2, 0] < 0.3


@pytest.mark.parametrize("dt", [(np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64), (np.float64, np.float64)],
                         ids=["f32-f32", "f64-f32", "f32-f64", "f64-f64"])
def test_emulated_geometry_shapes_and_bit_level_properties(emu, dt):
    """N = 256, hop 64, in ONE batch: n = 255 (K = 0) and n = 256 (K = 1), both NaN; K = 2, K = the chunk length, the chunk length
    plus one, three chunks; three estimates sharing one target in a run, then one with its own target; the four input bands, the
    empty band, bin 0 alone and bin N / 2 alone.  Then: a pair alone and at another position gives the bits it gives in the batch,
    a band's row does not depend on the other bands, and msc_out = NULL changes no bit of out."""
    N, H = 256, 64
    lens = [255, 256, _len_for_segments(2, N, H), _len_for_segments(FR, N, H, 5), _len_for_segments(FR + 1, N, H),
            _len_for_segments(2 * FR + 1, N, H, 63)]
    pairs = [O.input_pair(n, 200 + i) for i, n in enumerate(lens)]
    tg = [x.astype(dt[0]) for x, _ in pairs]
    ests, idx = [], []
    for i, (x, y) in enumerate(pairs):
        for k in range(3 if i == 4 else 1):
            ests.append((y + 0.1 * k * np.random.default_rng(300 + k).standard_normal(len(y))).astype(dt[1]))
            idx.append(i)
    bands = O.input_bands(N) + [(5, 4), (0, 0), (N // 2, N // 2)]
    out, g2 = run_emu(emu, tg, ests, idx, N, H, bands)
    worst = check_rows(out, g2, tg, ests, idx, N, H, bands, what="shapes")
    print("worst msc %.3g, per bin %.3g, coh_sdr %.3g dB" % tuple(worst))
    assert np.isnan(out[:2]).all() and np.isnan(g2[:2]).all() and np.isfinite(out[2:, [0, 1, 2, 3, 5, 6]]).all()
    assert np.isnan(out[:, 4]).all()                                              # the empty band
    assert out[3, 5, 0] == g2[3, 0] and out[3, 6, 0] == g2[3, N // 2]             # one-bin bands: msc is that bin's coherence
    for e in (2, 3, 5, len(ests) - 1):
        alone, ga = run_emu(emu, [tg[idx[e]]], [ests[e]], [0], N, H, bands)
        assert alone.tobytes() == out[e:e + 1].tobytes() and ga.tobytes() == g2[e:e + 1].tobytes(), e
    order = list(range(len(ests)))[::-1]
    back, gb = run_emu(emu, tg, [ests[e] for e in order], [idx[e] for e in order], N, H, bands)
    assert back[::-1].tobytes() == out.tobytes() and gb[::-1].tobytes() == g2.tobytes()
    for b in (0, 2, 3, 6):                                                        # a band alone, and bands in another order
        sub, _ = run_emu(emu, tg, ests, idx, N, H, [bands[b]])
        assert sub[:, 0].tobytes() == np.ascontiguousarray(out[:, b]).tobytes(), b
    swapped, _ = run_emu(emu, tg, ests, idx, N, H, bands[::-1])
    assert np.ascontiguousarray(swapped[:, ::-1]).tobytes() == out.tobytes()
    assert run_emu(emu, tg, ests, idx, N, H, bands, spectrum=False)[0].tobytes() == out.tobytes()
    # bands per estimate: every estimate its own split, as SSR_Eval_Helper asks for them
    per_est = [[(0, N // 2), (10 + 7 * e, N // 2)] for e in range(len(ests))]
    po, _ = run_emu(emu, tg, ests, idx, N, H, per_est)
    check_rows(po, None, tg, ests, idx, N, H, per_est, what="per-estimate bands")
    assert np.ascontiguousarray(po[:, 0]).tobytes() == np.ascontiguousarray(out[:, 0]).tobytes()


@pytest.mark.parametrize("n_fft,hop,K", [(2048, 1024, 3), (1024, 341, FR + 1), (512, 512, 4), (256, 1, FR), (2048, 2048, 2)])
def test_emulated_other_transform_sizes(emu, n_fft, hop, K):
    """N = 2048 with K = 3, a hop that does not divide N across a chunk boundary, no overlap, hop 1, K = 2 at the largest size -
    float32 targets with float64 estimates, next to a pair that is too short."""
    n = _len_for_segments(K, n_fft, hop, min(3, hop - 1))
    x, y = O.input_pair(n, 400 + n_fft + hop)
    tg = [x.astype(np.float32), x[:n_fft - 1].astype(np.float32)]
    ests = [y, y[:n_fft - 1]]
    bands = O.input_bands(n_fft) + [(n_fft // 2, n_fft // 2)]
    out, g2 = run_emu(emu, tg, ests, [0, 1], n_fft, hop, bands, thr=0.25)
    worst = check_rows(out, g2, tg, ests, [0, 1], n_fft, hop, bands, thr=0.25, what="sizes")
    print("worst msc %.3g, per bin %.3g, coh_sdr %.3g dB" % tuple(worst))
    assert np.isnan(out[1]).all() and np.isfinite(out[0]).all()


def test_emulated_exact_facts(emu):
    """y == x: msc >= 1 - 1e-12, coh_sdr >= 120 dB, every bin counted.  y = 0: msc == 0 and no bin counted - and so for a target of
    zeros.  A stretch of exact zeros longer than a segment in one signal: its segments add their exact zero."""
    N, H, n = 512, 128, 6000
    x, y = O.input_pair(n, 7)
    xf = x.astype(np.float32)
    bands = [(0, N // 2), (40, 200), (N // 2, N // 2)]
    for same in (xf, xf.astype(np.float64)):
        out, g2 = run_emu(emu, [xf], [same], [0], N, H, bands)
        print("y == x", out[0])
        assert (out[0, :, 0] >= 1 - 1e-12).all() and (out[0, :, 1] >= 120.0).all() and out[0, :, 2].tolist() == [257.0, 161.0, 1.0]
    z = np.zeros(n, np.float32)
    for tg, es in (([xf], [z]), ([z], [xf]), ([z], [z])):
        out, g2 = run_emu(emu, tg, es, [0], N, H, bands)
        assert np.all(out[0, :, 0] == 0.0) and np.all(out[0, :, 2] == 0.0) and np.all(g2 == 0.0), out
    assert run_emu(emu, [z], [z], [0], N, H, bands)[0][0, 0, 1] == 0.0          # 10 log10(EPS / EPS)
    x2, y2, y3 = x.copy(), y.copy(), y.copy()
    x2[700:700 + 3 * N] = 0.0
    y2[700:700 + 3 * N] = 0.0
    y3[2500:2500 + 2 * N + 17] = 0.0
    tg, es, idx = [x2, x], [y2, y3, y2], [0, 1, 1]
    out, g2 = run_emu(emu, tg, es, idx, N, H, bands)
    check_rows(out, g2, tg, es, idx, N, H, bands, what="silent stretches")


def test_emulated_threshold_and_empty_batch(emu):
    N, H = 256, 128
    x, y = O.input_pair(4000, 100)
    g2 = O.gamma2(x, y, N, H)[0]
    for thr in (0.05, 0.5, 0.95, 1.0):
        out, _ = run_emu(emu, [x], [y], [0], N, H, [(0, N // 2)], thr=thr)
        assert np.min(np.abs(g2 - thr)) > 1e-6 and out[0, 0, 2] == np.sum(g2 >= thr), thr
    out, _ = run_emu(emu, [x], [], [], N, H, np.zeros((0, 1, 2), np.int32))        # n_est = 0
    assert out.shape == (0, 1, 3)


def test_emulated_segment_geometry(emu):
    res = np.zeros(3, np.int64)
    for n_fft, hop in ((256, 64), (1024, 1024), (2048, 683), (512, 1)):
        for n in (0, 1, n_fft - 1, n_fft, n_fft + hop - 1, n_fft + hop, n_fft + (FR - 1) * hop, n_fft + FR * hop, 48000 * 60):
            emu.coherence_geometry(n, n_fft, hop, res.ctypes.data_as(C.c_void_p))
            K = O.segments(n, n_fft, hop)
            assert tuple(res) == (K, -(-K // FR), FR)


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


def _call(lib, tl, idx, n_fft=1024, hop=512, bands=((0, 512),), thr=0.5, n_bands=None, n_est=None, ws=_DUMMY, ws_bytes=1 << 40,
          out=_DUMMY, null_bands=False):
    tl, tp = _i32(tl)
    idx, ip = _i32(idx)
    tab, bp = _i32(np.broadcast_to(np.asarray(bands, np.int32), (max(len(idx), 1),) + np.asarray(bands).shape))
    return lib.ssr_coherence(_DUMMY, 0, _DUMMY, tp, len(tl), _DUMMY, 0, _DUMMY, ip, len(idx) if n_est is None else n_est, n_fft, hop,
                             len(bands) if n_bands is None else n_bands, None if null_bands else bp, thr, out, None, ws, ws_bytes, None)


def test_coherence_rejects_bad_arguments_before_launch():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E = _lib.ERR_INVALID_ARG
    for n_fft in (0, 128, 255, 1000, 4096, -1024):
        assert _call(lib, [4000], [0], n_fft=n_fft, hop=64, bands=((0, 0),)) == E and "n_fft" in err()
    for hop in (0, -1, 1025):
        assert _call(lib, [4000], [0], hop=hop) == E and "hop" in err()
    for n_bands in (0, -1, 9):
        assert _call(lib, [4000], [0], n_bands=n_bands) == E and "n_bands" in err()
    for band in ((-1, 5), (0, 513), (513, 513), (-3, -2)):
        assert _call(lib, [4000], [0], bands=(band,)) == E and "bands" in err()
        assert _call(lib, [4000], [0], bands=((0, 512), band)) == E and "bands" in err()
    for thr in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert _call(lib, [4000], [0], thr=thr) == E and "thr" in err()
    assert _call(lib, [4000, 5000], [2]) == E and "tgt_index" in err()
    assert _call(lib, [4000, 5000], [0, -1]) == E and "tgt_index" in err()
    assert _call(lib, [-3], [0]) == E and "lengths" in err()
    assert _call(lib, [1 << 29], [0]) == E and "lengths" in err()
    assert _call(lib, [4000], [0], out=None) == E and "null" in err()
    assert _call(lib, [4000], [0], null_bands=True) == E and "null" in err()
    tl, tp = _i32([4000, 9000])
    idx, ip = _i32([1, 1, 0])
    need = lib.ssr_coherence_workspace_bytes(tp, 2, ip, 3, 1024, 512, 2)
    assert need > 0 and lib.ssr_coherence_workspace_bytes(tp, 2, ip, 3, 1024, 128, 2) > need
    two = ((0, 512), (6, 5))                          # (the empty band is accepted)
    assert _call(lib, [4000, 9000], [1, 1, 0], bands=two, ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in err()
    assert _call(lib, [4000, 9000], [1, 1, 0], bands=two, ws=None) == _lib.ERR_WORKSPACE
    bad, bp = _i32([2])
    assert lib.ssr_coherence_workspace_bytes(tp, 2, bp, 1, 1024, 512, 2) == 0
    assert lib.ssr_coherence_workspace_bytes(tp, 2, ip, 3, 1000, 512, 2) == 0
    assert lib.ssr_coherence_workspace_bytes(tp, 2, ip, 3, 1024, 0, 2) == 0
    assert lib.ssr_coherence_workspace_bytes(tp, 2, ip, 3, 1024, 512, 0) == 0
    assert lib.ssr_coherence_workspace_bytes(tp, 2, ip, 3, 1024, 512, 9) == 0
    neg, np_ = _i32([4000, -1])
    assert lib.ssr_coherence_workspace_bytes(np_, 2, ip, 3, 1024, 512, 2) == 0
    # one workgroup of n_fft / 8 threads per chunk of 32 segments: 2^32 threads are refused before anything is queued
    many, mp = _i32([(1 << 29) - 1])
    rep, rp = _i32([0] * 70)
    assert lib.ssr_coherence_workspace_bytes(mp, 1, rp, 70, 2048, 1, 1) > 0
    tab, bp2 = _i32(np.zeros((70, 1, 2)))
    assert lib.ssr_coherence(_DUMMY, 0, _DUMMY, mp, 1, _DUMMY, 0, _DUMMY, rp, 70, 2048, 1, 1, bp2, 0.5, _DUMMY, None, _DUMMY, 1 << 60,
                             None) == _lib.ERR_UNSUPPORTED and "too large" in err()
    assert _call(lib, [4000], [], n_est=0, ws=None, ws_bytes=0, out=None, null_bands=True) == 0     # nothing to score: nothing queued


def test_header_ctypes_table_and_library_agree():
    from ssr_eval_amd import _lib
    path = os.path.join(ROOT, "ssr_eval_amd", "csrc", "ssr_hip_coherence.h")
    header = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    declared = set(re.findall(r"\b(ssr_[a-z_0-9]+)\s*\(", header))
    assert declared == {"ssr_coherence", "ssr_coherence_workspace_bytes"} == set(_lib.COHERENCE_SIGNATURES)
    assert not set(_lib.COHERENCE_SIGNATURES) & set(_lib.SIGNATURES)
    lib = _lib.load()
    for name, (res, args) in _lib.COHERENCE_SIGNATURES.items():
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    main = open(os.path.join(ROOT, "include", "ssr_hip.h")).read()
    assert main.count("#include \"../ssr_eval_amd/csrc/ssr_hip_coherence.h\"") == 1
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T ssr_coherence\n" in exported and " T ssr_coherence_workspace_bytes\n" in exported
    # the header is C99 on its own behind the main one
    src = "#include \"%s\"\nint main(void) { return ssr_coherence_workspace_bytes(0, 0, 0, 0, 1024, 512, 1) != 0; }\n" % \
        os.path.join(ROOT, "include", "ssr_hip.h")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-"], input=src, text=True, check=True)


# ---- AudioMetrics / SSR_Eval_Helper options --------------------------------------------------------------------------------------
def test_audio_metrics_coherence_options():
    from ssr_eval_amd import AudioMetrics
    from ssr_eval_amd import backend as B
    am = AudioMetrics(16000)
    assert B.check_coherence_frames(1024, None) == (1024, 512) and B.check_coherence_frames(np.int64(256), 256) == (256, 256)
    assert B.check_coherence_frames(2048, 1) == (2048, 1)
    for bad in ((1000, None), (4096, None), (1024.0, None), (True, None), (1024, 0), (1024, 1025), (1024, 2.0), (1024, True)):
        with pytest.raises(ValueError):
            B.check_coherence_frames(*bad)
    assert B.check_coherence_threshold(1) == 1.0 and B.check_coherence_threshold(np.float32(0.25)) == 0.25
    for bad in (0, 0.0, -0.1, 1.5, float("nan"), None, "0.5", True):
        with pytest.raises(ValueError):
            B.check_coherence_threshold(bad)
    # bands: the family's band by _phase_bins' rule, the split's first bin ceil(split N / rate)
    assert am._coh_bands(1024, None, None, 1) == [[(0, 512)]]
    assert am._coh_bands(1024, (1000, 6000), None, 2) == [[(64, 384)]] * 2
    assert am._coh_bands(1024, None, 4000, 2) == [[(0, 512), (256, 512)]] * 2
    assert am._coh_bands(1024, (0, 7000), [4000.5, None, 7001, 0], 4) == [[(0, 448), (257, 448)], [(0, 448), (1, 0)], [(0, 448), (1, 0)],
                                                                          [(0, 448), (0, 448)]]
    for bad in ("4000", True, -1.0, float("nan"), float("inf"), (4000,), [4000, "x"]):
        with pytest.raises(ValueError):
            am._coh_bands(1024, None, bad, 2)
    with pytest.raises(ValueError):
        am._coh_bands(1024, None, [4000], 2)                                     # one split per pair
    x = np.zeros(3000, np.float32)
    for kw in ({"n_fft": 300}, {"hop": 0}, {"band": (5, 1)}, {"threshold": 0}, {"threshold": 1.1}, {"split_hz": -5}, {"split_hz": "x"}):
        with pytest.raises(ValueError):                                          # rejected before any device is touched
            am.coherence(x, x, **kw)
        with pytest.raises(ValueError):
            am.coherence_batch([x], [x], **kw)
        with pytest.raises(ValueError):
            am.coherence_multi([[x]], [x], **kw)
    # rows -> dicts: coh_bw = coh_bins rate / N, the split's two values behind the band's three, the spectrum last
    dicts = am._coh_dicts(1024, True, True)
    got = dicts((np.array([[[0.5, 3.0, 64.0], [0.25, -2.0, 7.0]]]), np.arange(513.0)[None]))
    assert list(got[0]) == ["msc", "coh_sdr", "coh_bw", "msc_hf", "coh_sdr_hf", "msc_spectrum"]
    assert got[0]["coh_bw"] == 1000.0 and got[0]["msc_hf"] == 0.25 and got[0]["coh_sdr_hf"] == -2.0 and got[0]["msc_spectrum"].shape == (513,)
    assert am._coh_dicts(1024, False, False)((np.array([[[0.5, 3.0, 64.0]]]), None)) == [{"msc": 0.5, "coh_sdr": 3.0, "coh_bw": 1000.0}]
    assert np.isnan(am._coh_dicts(256, False, False)((np.full((1, 1, 3), np.nan), None))[0]["coh_bw"])


def test_helper_coherence_option_and_key_order():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd import eval as E
    mk = lambda **kw: SSR_Eval_Helper(BasicTestee(), 44100, 44100, test_data_root=None, **kw)      # noqa: E731
    assert mk().coherence is None and mk(coherence=None).coherence is None
    for ok in (True, {"n_fft": 2048}, {"hop": 100}, {"band": (0, 1e6)}, {"threshold": 0.9}, {"split": 4000}, {"split": 0},
               {"n_fft": 512, "hop": 512, "band": (1000, 16000), "threshold": np.float32(0.25), "split": 8000.5}):
        assert mk(coherence=ok).coherence == ok
    for bad in (False, 1, "all", "msc", (), ("msc",), [1024], {}, {"fft": 512}, {"n_fft": 1000}, {"n_fft": 4096}, {"hop": 0},
                {"hop": 1025}, {"hop": 2.5}, {"n_fft": 256, "hop": 257}, {"band": (8000, 4000)}, {"band": 4000}, {"threshold": 0},
                {"threshold": 1.5}, {"threshold": None}, {"split": -1}, {"split": "4000"}, {"split": True}, {"split": None},
                {"which": "msc"}, {"split_hz": 4000}):
        with pytest.raises(ValueError):
            mk(coherence=bad)
    # the earlier registry and order are what they were; the new family is queued behind them and its keys close the order
    assert E._COH_KEYS == ("msc", "coh_sdr", "coh_bw", "msc_hf", "coh_sdr_hf")
    assert [f.option for f in E._LATER_FAMILIES] == ["coherence"] and E._LATER_FAMILIES[0].per_key is True
    assert [f[0] for f in E._FAMILIES] == ["lsd_split", "stoi", "waveform", "mel", "mel_dtw", "quality", "pitch", "phase", "mrstft", "bss_sdr"]
    assert len(E.result_key_order()) == 33
    assert E.all_key_order() == E.result_key_order() + E._COH_KEYS and len(set(E.all_key_order())) == 38
    args = E._LATER_FAMILIES[0].arguments
    keys = ["proc_fft_8000_44100", "proc_mp3_64_44100", "proc_bw_22050_4_44100"]
    assert args(mk(coherence=True), keys) == ((1024, None, None, [4000, None, 11025], 0.5), {})
    assert args(mk(coherence={"n_fft": 512, "hop": 100, "band": (0, 9000), "threshold": 0.7, "split": 3000}), keys) == \
        ((512, 100, (0, 9000), [3000.0, 3000.0, 3000.0], 0.7), {})
