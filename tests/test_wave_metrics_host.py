"""CPU tests of the waveform metrics (SNR, SI-SDR, segmental SNR): frame geometry, properties of the float64 oracle
(tests/wave_oracle.py), the C ABI's argument checks (they return before anything touches a device), SSR_Eval_Helper(waveform=...)
validation and metric order, and a g++ build of the kernel bodies (ssr_wave_metrics.h) against the oracle."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import wave_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- frame geometry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,L,R", [(8000, 240, 60), (16000, 480, 120), (22050, 662, 165), (44100, 1323, 330), (48000, 1440, 360)])
def test_frame_geometry(fs, L, R):
    assert O.frame_geometry(fs, 0)[:2] == (L, R)
    assert O.frame_geometry(fs, L + R - 1)[2] == 0              # one whole frame and a bit: comp_snr.m's loop does not run
    assert O.frame_geometry(fs, L + R)[2] == 1
    assert O.frame_geometry(fs, 50 * R)[2] == (50 * R - L) // R
    assert O.frame_geometry(fs, L - 1)[2] == 0


# ---- oracle properties --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sig():
    rng = np.random.default_rng(3)
    x = np.convolve(rng.standard_normal(20000), np.hanning(31), "same")
    return x, x + 0.3 * np.std(x) * rng.standard_normal(x.shape)


def test_si_sdr_is_scale_and_offset_invariant_snr_is_not(sig):
    x, y = sig
    d = O.si_sdr(x, y)
    assert abs(O.si_sdr(x, 3.7 * y) - d) < 1e-9
    assert abs(O.si_sdr(x, y + 0.8) - d) < 1e-9
    assert abs(O.si_sdr(x - 0.5, y) - d) < 1e-9
    s = O.snr(x, y)
    assert abs(O.snr(x, 3.7 * y) - s) > 1
    assert abs(O.snr(x, y + 0.8) - s) > 1


def test_seg_snr_clamps(sig):
    x, y = sig
    assert O.seg_snr(x, x, 16000) == 35.0                     # no error at all: every frame at the upper bound
    assert O.seg_snr(x, x + 1e6 * np.std(x), 16000) == -10.0  # error swamps the signal: every frame at the lower bound
    assert O.seg_snr(np.zeros_like(x), y, 16000) == -10.0    # no signal
    assert -10 < O.seg_snr(x, y, 16000) < 35


def test_identical_signals_are_finite(sig):
    x, _ = sig
    w = O.waveform(x, x, 16000)
    assert all(np.isfinite(v) for v in w.values())
    assert abs(w["snr"] - 10 * np.log10(np.sum(x * x) / O.EPS + 1)) < 1e-9
    z = np.zeros(5000)
    assert O.snr(z, z) == 0.0 and O.si_sdr(z, z) == 0.0


def test_nan_cases():
    e = np.zeros(0)
    assert all(np.isnan(v) for v in O.waveform(e, e, 16000).values())
    x = np.ones(480 + 119)                                    # M = 0 at 16 kHz
    w = O.waveform(x, 0.5 * x, 16000)
    assert np.isnan(w["seg_snr"]) and np.isfinite(w["snr"]) and np.isfinite(w["si_sdr"])


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


def _call(lib, tl, idx, which=7, fs=16000, n_est=None, ws=_DUMMY, ws_bytes=1 << 30, out=_DUMMY):
    tl, tp = _i32(tl)
    idx, ip = _i32(idx)
    return lib.ssr_wave_metrics(_DUMMY, 0, _DUMMY, tp, len(tl), _DUMMY, 0, _DUMMY, ip, len(idx) if n_est is None else n_est, fs,
                                which, out, ws, ws_bytes, None)


def test_wave_metrics_rejects_bad_arguments_before_launch():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E = _lib.ERR_INVALID_ARG
    for w in (0, 8, -1, 15):
        assert _call(lib, [4000], [0], which=w) == E and "which" in err()
    for fs in (0, -16000):
        assert _call(lib, [4000], [0], fs=fs) == E and "fs" in err()
    assert _call(lib, [4000, 5000], [2]) == E and "tgt_index" in err()
    assert _call(lib, [4000, 5000], [0, -1]) == E and "tgt_index" in err()
    assert _call(lib, [-3], [0]) == E and "lengths" in err()
    assert _call(lib, [4000], [0], out=None) == E and "null" in err()
    tl, tp = _i32([4000, 9000])
    idx, ip = _i32([1, 1, 0])
    need = lib.ssr_wave_metrics_workspace_bytes(tp, 2, ip, 3, 16000, 7)
    assert need > 0
    assert lib.ssr_wave_metrics_workspace_bytes(tp, 2, ip, 3, 16000, 1) < need      # no SI-SDR: no pass-2 records
    assert _call(lib, [4000, 9000], [1, 1, 0], ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in err()
    assert _call(lib, [4000, 9000], [1, 1, 0], ws=None) == _lib.ERR_WORKSPACE
    bad, bp = _i32([2])
    assert lib.ssr_wave_metrics_workspace_bytes(tp, 2, bp, 1, 16000, 7) == 0
    assert lib.ssr_wave_metrics_workspace_bytes(tp, 2, ip, 3, 0, 7) == 0
    assert _call(lib, [4000], [], n_est=0, ws=None, ws_bytes=0, out=None) == 0     # nothing to score: nothing queued


# ---- SSR_Eval_Helper / AudioMetrics options -----------------------------------------------------------------------------------
def test_helper_waveform_option_and_metric_order():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.eval import _METRIC_KEYS, _WAVEFORM_KEYS
    mk = lambda v: SSR_Eval_Helper(BasicTestee(), 44100, 44100, test_data_root=None, waveform=v)      # noqa: E731
    for ok in (None, True, "snr", "si_sdr", "seg_snr", ("snr", "seg_snr"), ("si_sdr",)):
        assert mk(ok).waveform == ok
    for bad in (False, "SNR", "all", 1, ["snr"], (), ("snr", "pesq"), ("snr", True)):
        with pytest.raises(ValueError):
            mk(bad)
    assert _METRIC_KEYS == ("lsd", "log_sispec", "sispec", "ssim", "lsd_lf", "lsd_hf", "stoi", "estoi")
    assert _WAVEFORM_KEYS == ("snr", "si_sdr", "seg_snr")


def test_audio_metrics_which_values():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(16000)
    assert am._wave_which("all") == 7 and am._wave_which("snr") == 1 and am._wave_which("si_sdr") == 2
    assert am._wave_which("seg_snr") == 4 and am._wave_which(("seg_snr", "snr")) == 5 and am._wave_which(["si_sdr"]) == 2
    for bad in (None, True, 0, 7, "SNR", (), ("snr", "x")):
        with pytest.raises(ValueError):
            am._wave_which(bad)
    assert am._wave_dicts(np.array([[1.0, 2.0]]), 5) == [{"snr": 1.0, "seg_snr": 2.0}]


# ---- the kernel bodies compiled for the host ---------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "wave_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libwave_emu.so")


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    return C.CDLL(EMU_SO)


@pytest.mark.parametrize("fs", [8000, 16000, 22050, 44100, 48000])
def test_emulated_geometry(emu, fs):
    res = np.zeros(5, np.int64)
    for n in (0, 1, 4095, 4096, 12345, 48000 * 3 + 7):
        emu.wave_geometry(fs, C.c_int64(n), res.ctypes.data_as(C.c_void_p))
        L, R, M = O.frame_geometry(fs, n)
        assert tuple(res[:3]) == (L, R, M)
        assert res[3] % R == 0 and res[3] >= 4096 > res[3] - R and res[4] == -(-n // res[3])


def run_emu(lib, tgts, ests, idx, fs, which):
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
    assert lib.wave_emu(P(td), int(t64), P(to), P(tl), len(tgts), P(ed), int(e64), P(eo), P(idx), len(ests), fs, which, P(out)) == 0
    return out


@pytest.mark.parametrize("fs", [16000, 44100])
@pytest.mark.parametrize("dt", [(np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64), (np.float64, np.float64)])
def test_emulated_kernels_match_the_oracle(emu, fs, dt):
    rng = np.random.default_rng(fs + 10 * (dt[0] == np.float64) + (dt[1] == np.float64))
    L, R, _ = O.frame_geometry(fs, 0)
    lens = [30000, 12345, L + R - 1, 0, 9000, 4 * 4096 + 17]
    # (float32 values in either dtype: the estimate `t` is then the target exactly, whichever dtype it has)
    tg = [np.convolve(rng.standard_normal(n), np.hanning(9), "same").astype(np.float32).astype(dt[0]) if n else np.zeros(0, dt[0])
          for n in lens]
    tg[4] = (0.5 + 1e-3 * rng.standard_normal(lens[4])).astype(np.float32).astype(dt[0])       # DC offset on a small signal
    tg[5] = np.zeros(lens[5], dt[0])                                        # all-zero target
    ests, idx = [], []
    for i, t in enumerate(tg):        # three estimates per target, next to each other (one run), then one more for target 0
        sd = float(np.std(t)) if len(t) else 0.0
        ests += [(t + 0.3 * (sd + 1e-3) * rng.standard_normal(len(t))).astype(dt[1]), t.astype(dt[1]),
                 (0.2 * t.astype(np.float64) + 1e-5 * (sd + 1e-3) * rng.standard_normal(len(t))).astype(dt[1])]
        idx += [i, i, i]
    ests.append((0.7 * tg[0] + 0.05 * rng.standard_normal(lens[0])).astype(dt[1]))
    idx.append(0)
    got = run_emu(emu, tg, ests, idx, fs, 7)
    for e, (y, i) in enumerate(zip(ests, idx)):
        want = O.waveform(tg[i], y, fs)
        for j, m in enumerate(("snr", "si_sdr", "seg_snr")):
            if np.isnan(want[m]):
                assert np.isnan(got[e, j]), (e, m)
            else:
                assert abs(got[e, j] - want[m]) < 1e-10, (e, m, got[e, j], want[m])
    # subsets: the same values in bit order
    for which in (1, 2, 4, 3, 5, 6):
        sub = run_emu(emu, tg, ests, idx, fs, which)
        cols = [j for j in range(3) if which & (1 << j)]
        np.testing.assert_array_equal(sub, got[:, cols])
    # a pair alone gives the bits it has in the batch
    alone = run_emu(emu, [tg[1]], [ests[4]], [0], fs, 7)
    np.testing.assert_array_equal(alone[0], got[4])
