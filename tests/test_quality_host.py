"""CPU tests of the objective quality measures (LLR, LPC cepstral distance, WSS, fwSNRseg): frame / transform / order geometry, the
critical-band table and the library's filters, properties of the float64 oracle (tests/quality_oracle.py), the C ABI's argument
checks (they return before anything touches a device), SSR_Eval_Helper(quality=...) validation and metric order, and a g++ build
of the kernel bodies (ssr_quality.h) against the oracle."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import quality_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,L,R,N,P", [(8000, 240, 60, 512, 10), (16000, 480, 120, 1024, 16), (22050, 662, 165, 2048, 16),
                                        (44100, 1323, 330, 4096, 16), (48000, 1440, 360, 4096, 16)])
def test_geometry(fs, L, R, N, P):
    assert O.frame_geometry(fs, 0)[:2] == (L, R)
    assert O.frame_geometry(fs, L + R - 1)[2] == 0 and O.frame_geometry(fs, L + R)[2] == 1
    assert O.nfft(fs) == N and O.default_order(fs) == P
    assert O.frame_geometry(48000, 60 * 48000)[2] == 7996 and O.trim_count(7996) == 7596


def test_band_table_has_no_typo():
    # bw[i] = cent[i + 1] - cent[i] up to the printed precision: the centres carry 6 significant digits, so above 1 kHz the
    # difference of two printed centres is only good to about half a unit of their second decimal (up to 6e-3: 1148.30 - 1020.38
    # against 127.914); below 1 kHz it holds to 1e-3
    assert len(O.CENT) == 25 and len(O.BW) == 25
    for i in range(24):
        d = abs(O.BW[i] - (O.CENT[i + 1] - O.CENT[i]))
        if O.CENT[i + 1] < 1000:
            assert d < 1e-3, i
        half_units = 0.5 * 10.0 ** (np.floor(np.log10(O.CENT[i + 1])) - 5) + 0.5 * 10.0 ** (np.floor(np.log10(O.CENT[i])) - 5)
        assert d <= half_units + 1e-9, i


@pytest.mark.parametrize("fs", [8000, 16000, 22050, 44100, 48000])
def test_library_filters_match_the_oracle(fs):
    from ssr_eval_amd import backend as B
    n, cent, bw, filt = B.quality_bands(fs)
    assert n == O.nfft(fs)
    np.testing.assert_array_equal(cent, O.CENT)
    np.testing.assert_array_equal(bw, O.BW)
    want = O.filters(fs)
    assert filt.shape == want.shape and np.max(np.abs(filt - want)) <= 1e-15
    top = np.nonzero(filt[24])[0][-1] * fs / n
    assert 3500 < top < 4100                                       # the bands stop below about 4 kHz at every rate


# ---- oracle properties ---------------------------------------------------------------------------------------------------------
def _speechy(rng, n):
    e = rng.standard_normal(n + 200)
    z = np.zeros_like(e)
    a1, a2 = 2 * 0.95 * np.cos(2 * np.pi * 0.06), -0.95 ** 2
    for i in range(2, len(e)):
        z[i] = e[i] + a1 * z[i - 1] + a2 * z[i - 2]
    return 0.05 * z[200:]


@pytest.fixture(scope="module")
def sig():
    rng = np.random.default_rng(3)
    x = _speechy(rng, 8000)
    return x, x + 0.05 * rng.standard_normal(x.shape)


def test_identities_of_identical_signals(sig):
    x, _ = sig
    assert O.quality(x, x, 16000) == {"llr": 0.0, "cep_dist": 0.0, "wss": 0.0, "fwseg_snr": 35.0}


def test_llr_is_not_negative_on_random_frames():
    rng = np.random.default_rng(5)
    for _ in range(40):
        a, b = rng.standard_normal(480), rng.standard_normal(480)
        rx, ry = O.lags(a, 16), O.lags(b, 16)
        assert O.llr_frame(rx, O.levinson(rx, 16), O.levinson(ry, 16)) >= -1e-12


def test_trimmed_mean_against_a_sort():
    rng = np.random.default_rng(6)
    for M in (1, 2, 3, 19, 20, 21, 100, 529):
        v = rng.standard_normal(M)
        v[: M // 3] = np.round(v[: M // 3], 1)                    # ties
        K = int(np.floor(0.95 * M + 0.5))
        assert K >= 1
        assert abs(O.trimmed_mean(v) - np.mean(np.sort(v)[:K])) < 1e-15


def test_nan_without_frames():
    assert all(np.isnan(v) for v in O.quality(np.zeros(0), np.zeros(0), 16000).values())
    x = np.ones(480 + 119)
    assert all(np.isnan(v) for v in O.quality(x, 0.5 * x, 16000).values())


def test_levinson_against_solve_toeplitz():
    solve_toeplitz = pytest.importorskip("scipy.linalg").solve_toeplitz
    rng = np.random.default_rng(8)
    w = O.window(480)
    for _ in range(10):
        f = w * _speechy(rng, 480)
        r = O.lags(f, 16)
        a = O.levinson(r, 16)
        alpha = solve_toeplitz(r[:16], r[1:17])
        assert np.max(np.abs(-a[1:] - alpha)) < 1e-9


def test_levinson_guard_on_a_singular_frame():
    r = np.zeros(17)
    r[0] = 1.0
    r[1] = 1.0                                                     # E_1 = (1 - 1) E_0 = 0: the recursion stops at order 2
    a = O.levinson(r, 16)
    assert np.all(np.isfinite(a)) and a[1] == -1.0 and np.all(a[2:] == 0.0)
    assert O.llr_frame(r, a, a) == O.LLR_CLIP                      # a' R a = 0: the ratio guard gives 2, even for y == x
    z = np.zeros(17)
    a0 = O.levinson(z, 16)
    assert np.all(a0[1:] == 0) and O.llr_frame(z, a0, a0) == O.LLR_CLIP     # zero forms: the clip value
    assert np.isfinite(O.cep_frame(O.cepstrum(a), O.cepstrum(a0)))


# ---- C ABI argument checks (no device call happens before any of these errors) ------------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


def _call(lib, tl, idx, which=15, fs=16000, order=0, n_est=None, ws=_DUMMY, ws_bytes=1 << 30, out=_DUMMY):
    tl, tp = _i32(tl)
    idx, ip = _i32(idx)
    return lib.ssr_quality_metrics(_DUMMY, 0, _DUMMY, tp, len(tl), _DUMMY, 0, _DUMMY, ip, len(idx) if n_est is None else n_est, fs,
                                   order, which, out, ws, ws_bytes, None)


def test_quality_metrics_rejects_bad_arguments_before_launch():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E = _lib.ERR_INVALID_ARG
    for w in (0, 16, -1, 31):
        assert _call(lib, [4000], [0], which=w) == E and "which" in err()
    for fs in (0, -16000, 7999, 48001, 96000):
        assert _call(lib, [4000], [0], fs=fs) == E and "fs" in err()
    for order in (-1, 33):
        assert _call(lib, [4000], [0], order=order) == E and "lpc_order" in err()
    assert _call(lib, [4000, 5000], [2]) == E and "tgt_index" in err()
    assert _call(lib, [4000, 5000], [0, -1]) == E and "tgt_index" in err()
    assert _call(lib, [-3], [0]) == E and "lengths" in err()
    assert _call(lib, [4000], [0], out=None) == E and "null" in err()
    tl, tp = _i32([4000, 9000])
    idx, ip = _i32([1, 1, 0])
    need = lib.ssr_quality_metrics_workspace_bytes(tp, 2, ip, 3, 16000, 0, 15)
    assert need > 0
    assert lib.ssr_quality_metrics_workspace_bytes(tp, 2, ip, 3, 16000, 0, 3) < need      # no bands: no twiddles, no filters
    assert _call(lib, [4000, 9000], [1, 1, 0], ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in err()
    assert _call(lib, [4000, 9000], [1, 1, 0], ws=None) == _lib.ERR_WORKSPACE
    bad, bp = _i32([2])
    assert lib.ssr_quality_metrics_workspace_bytes(tp, 2, bp, 1, 16000, 0, 15) == 0
    assert lib.ssr_quality_metrics_workspace_bytes(tp, 2, ip, 3, 0, 0, 15) == 0
    assert lib.ssr_quality_metrics_workspace_bytes(tp, 2, ip, 3, 16000, 40, 15) == 0
    assert _call(lib, [4000], [], n_est=0, ws=None, ws_bytes=0, out=None) == 0     # nothing to score: nothing queued
    n = C.c_int32(0)
    assert lib.ssr_quality_bands(4000, C.byref(n), None, None, None, 0) == E and "fs" in err()
    small = np.zeros(10)
    assert lib.ssr_quality_bands(16000, C.byref(n), None, None, small.ctypes.data_as(C.c_void_p), 10) == E and "filters" in err()


# ---- SSR_Eval_Helper / AudioMetrics options ----------------------------------------------------------------------------------
def test_helper_quality_option_and_metric_order():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.eval import _METRIC_KEYS, _WAVEFORM_KEYS, _MEL_KEYS, _QUALITY_KEYS
    mk = lambda v: SSR_Eval_Helper(BasicTestee(), 44100, 44100, test_data_root=None, quality=v)      # noqa: E731
    for ok in (None, True, "llr", "wss", ("llr", "fwseg_snr"), {"which": "cep_dist"}, {"lpc_order": 12},
               {"which": ("wss",), "lpc_order": 1}):
        assert mk(ok).quality == ok
    for bad in (False, "LLR", 1, ["llr"], (), ("llr", "pesq"), ("llr", True), {}, {"order": 12}, {"lpc_order": 0},
                {"lpc_order": 33}, {"lpc_order": 12.0}, {"which": "x"}):
        with pytest.raises(ValueError):
            mk(bad)
    assert _QUALITY_KEYS == ("llr", "cep_dist", "wss", "fwseg_snr")
    assert _MEL_KEYS == ("mel_lsd", "mel_l1", "mcd") and _WAVEFORM_KEYS == ("snr", "si_sdr", "seg_snr")
    assert len(_METRIC_KEYS) == 8


def test_audio_metrics_which_values():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(16000)
    assert am._quality_which("all") == 15 and am._quality_which("llr") == 1 and am._quality_which("cep_dist") == 2
    assert am._quality_which("wss") == 4 and am._quality_which(("fwseg_snr", "llr")) == 9 and am._quality_which(["wss"]) == 4
    for bad in (None, True, 0, 15, "LLR", (), ("llr", "x")):
        with pytest.raises(ValueError):
            am._quality_which(bad)
    assert am._quality_order(None) == 0 and am._quality_order(12) == 12
    for bad in (0, 33, True, 1.5, "16"):
        with pytest.raises(ValueError):
            am._quality_order(bad)
    assert am._quality_dicts(np.array([[1.0, 2.0]]), 6) == [{"cep_dist": 1.0, "wss": 2.0}]


# ---- the kernel bodies compiled for the host ---------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "quality_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libquality_emu.so")


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    lib = C.CDLL(EMU_SO)
    lib.quality_trimmed_mean.restype = C.c_double
    return lib


@pytest.mark.parametrize("fs", [8000, 16000, 22050, 44100, 48000])
def test_emulated_geometry(emu, fs):
    res = np.zeros(6, np.int64)
    for n in (0, 1, 4095, 12345, 48000 * 3 + 7):
        emu.quality_geometry(fs, C.c_int64(n), res.ctypes.data_as(C.c_void_p))
        L, R, M = O.frame_geometry(fs, n)
        assert tuple(res) == (L, R, M, O.nfft(fs), O.default_order(fs), O.trim_count(M))


def test_emulated_trimmed_mean_is_the_sorted_prefix(emu):
    rng = np.random.default_rng(9)
    for M in (1, 2, 7, 20, 255, 256, 257, 1000, 7996):
        v = rng.standard_normal(M) * 3
        v[::3] = np.round(v[::3])                                  # ties, and +-0
        v[1::7] = -0.0
        got = emu.quality_trimmed_mean(v.ctypes.data_as(C.c_void_p), C.c_int64(M))
        assert abs(got - O.trimmed_mean(v)) < 1e-12, M


def test_emulated_levinson(emu):
    rng = np.random.default_rng(10)
    for P in (1, 10, 16, 32):
        f = O.window(1440) * _speechy(rng, 1440)
        r = np.ascontiguousarray(O.lags(f, P))
        a = np.zeros(P + 1)
        emu.quality_levinson(r.ctypes.data_as(C.c_void_p), P, a.ctypes.data_as(C.c_void_p))
        np.testing.assert_array_equal(a, O.levinson(r, P))


def run_emu(lib, tgts, ests, idx, fs, which=15, order=0):
    t64, e64 = tgts[0].dtype == np.float64, ests[0].dtype == np.float64
    P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    tl = np.array([len(t) for t in tgts], np.int32)
    el = np.array([len(e) for e in ests], np.int64)
    to = np.concatenate(([0], np.cumsum(tl)[:-1])).astype(np.int64)
    eo = np.concatenate(([0], np.cumsum(el)[:-1])).astype(np.int64)
    td = np.concatenate(tgts + [np.zeros(1, tgts[0].dtype)])
    ed = np.concatenate(ests + [np.zeros(1, ests[0].dtype)])
    idx = np.ascontiguousarray(idx, np.int32)
    out = np.full((len(ests), bin(which).count("1")), -123.0)
    assert lib.quality_emu(P(td), int(t64), P(to), P(tl), len(tgts), P(ed), int(e64), P(eo), P(idx), len(ests), fs, order, which,
                           P(out)) == 0
    return out


@pytest.mark.parametrize("fs", [8000, 16000, 48000])
@pytest.mark.parametrize("dt", [(np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64), (np.float64, np.float64)])
def test_emulated_kernels_match_the_oracle(emu, fs, dt):
    rng = np.random.default_rng(fs + 10 * (dt[0] == np.float64) + (dt[1] == np.float64))
    L, R, _ = O.frame_geometry(fs, 0)
    lens = [fs // 4 + 11, L + R - 1, L + R, 0, L + 4 * R]
    # (float32 values in either dtype: the estimate `t` is then the target exactly, whichever dtype it has)
    tg = [_speechy(rng, n).astype(np.float32).astype(dt[0]) for n in lens]
    ests, idx = [], []
    for i, t in enumerate(tg):        # three estimates per target, next to each other (one run), then one more for target 0
        ests += [(t + 0.01 * rng.standard_normal(len(t))).astype(dt[1]), t.astype(dt[1]),
                 (t + 0.2 * rng.standard_normal(len(t))).astype(dt[1])]
        idx += [i, i, i]
    ests.append((0.7 * tg[0] + 0.005 * rng.standard_normal(lens[0])).astype(dt[1]))
    idx.append(0)
    got = run_emu(emu, tg, ests, idx, fs)
    for e, (y, i) in enumerate(zip(ests, idx)):
        want = O.quality(tg[i], y, fs)
        for j, m in enumerate(O.NAMES):
            if np.isnan(want[m]):
                assert np.isnan(got[e, j]), (e, m)
            else:
                assert abs(got[e, j] - want[m]) < 1e-10, (e, m, got[e, j], want[m])
    assert got[1].tolist() == [0.0, 0.0, 0.0, 35.0]                # y == x
    # subsets: the same values in bit order
    for which in (1, 2, 4, 8, 3, 12, 5, 10, 7, 14):
        sub = run_emu(emu, tg, ests, idx, fs, which)
        cols = [j for j in range(4) if which & (1 << j)]
        np.testing.assert_array_equal(sub, got[:, cols])
    # a pair alone gives the bits it has in the batch
    alone = run_emu(emu, [tg[4]], [ests[12]], [0], fs)
    np.testing.assert_array_equal(alone[0], got[12])


def test_emulated_lpc_order_override(emu):
    rng = np.random.default_rng(12)
    fs = 16000
    x = _speechy(rng, 6000)
    y = x + 0.01 * rng.standard_normal(len(x))
    for order in (4, 12, 32):
        got = run_emu(emu, [x], [y], [0], fs, 3, order)
        want = O.quality(x, y, fs, order)
        assert abs(got[0, 0] - want["llr"]) < 1e-10 and abs(got[0, 1] - want["cep_dist"]) < 1e-10
