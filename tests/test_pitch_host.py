"""CPU tests of the pitch metrics (YIN F0 tracking, F0 RMSE, F0 correlation, GPE, VDE, FFE): frame and lag geometry, known answers
of the float64 oracle (tests/pitch_oracle.py), the C ABI's argument checks (they return before anything touches a device),
SSR_Eval_Helper(pitch=...) validation and metric order, and a g++ build of the kernel bodies (ssr_pitch.h) against the oracle."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import pitch_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def harmonic(f0, fs, n, phase=0.0):
    """Six harmonics of f0 (Hz, a scalar or one value per sample) with falling amplitudes."""
    f = np.broadcast_to(np.asarray(f0, np.float64), (n,))
    ph = 2 * np.pi * np.cumsum(f) / fs + phase
    return 0.3 * sum((0.6 ** k) * np.sin((k + 1) * ph + k) for k in range(6))


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def test_lag_range_and_frames():
    assert O.lag_range() == (32, 320)
    assert O.lag_range(40, 1000) == (16, 400)
    assert O.lag_range(60, 400) == (40, 267)
    assert O.valid_range(50, 500) and O.valid_range(40, 1000)
    for fmin, fmax in ((39.9, 500), (50, 1000.5), (500, 500), (600, 500), (990, 1000), (float("nan"), 500)):
        assert not O.valid_range(fmin, fmax)
    assert [O.n_frames(n) for n in (0, 1, 159, 160, 161, 16000)] == [0, 1, 1, 2, 2, 101]


# ---- oracle known answers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [16000, 44100, 48000])
@pytest.mark.parametrize("f0", [80.0, 125.0, 210.0, 400.0])
def test_harmonic_complex_is_tracked_within_one_cent(fs, f0):
    tr = O.track(harmonic(f0, fs, int(0.6 * fs)), fs)
    T = len(tr["f0"])
    inner = np.arange(3, T - 3)                  # frames whose window lies inside the signal
    assert tr["voiced"][inner].all()
    assert tr["stable"].mean() >= 0.99
    cents = 1200 * np.log2(tr["f0"][inner] / f0)
    assert np.abs(cents).max() < 1.0, np.abs(cents).max()


def test_noise_is_unvoiced_and_zeros_are_silent():
    x = np.random.default_rng(5).standard_normal(32000)
    tr = O.track(x, 16000)
    assert np.mean(~tr["voiced"]) >= 0.95
    z = O.track(np.zeros(16000), 16000)
    assert not z["voiced"].any() and np.isnan(z["f0"]).all() and (z["energy"] == 0).all()


def test_identical_gliding_tracks_score_perfectly():
    fs = 16000
    x = harmonic(np.linspace(110, 240, fs), fs, fs)
    m, stable = O.pitch(x, x.copy(), fs)
    assert stable
    assert m["f0_rmse"] == 0 and m["gpe"] == 0 and m["vde"] == 0 and m["ffe"] == 0 and m["f0_corr"] == 1.0


def test_octave_down_estimate_is_a_gross_error():
    fs = 16000
    x, y = harmonic(200.0, fs, fs), harmonic(100.0, fs, fs)
    m, stable = O.pitch(x, y, fs)
    assert stable
    # (the edge frames, half outside the signal, are a few cents off: the RMSE over every frame of B is 1200 within 25 cents,
    # the interior frames within one)
    assert m["gpe"] == 1.0 and abs(m["f0_rmse"] - 1200) < 25 and m["ffe"] > 0.9
    tx, ty = O.track(x, fs), O.track(y, fs)
    inner = slice(3, len(tx["f0"]) - 3)
    assert np.abs(1200 * np.log2(tx["f0"][inner] / ty["f0"][inner]) - 1200).max() < 1


def test_nan_cases():
    e = np.zeros(0)
    m, _ = O.pitch(e, e, 16000)
    assert all(np.isnan(v) for v in m.values())
    z = np.zeros(8000)
    m, _ = O.pitch(z, z, 16000)                  # T > 0, nothing voiced: only vde / ffe are defined
    assert m["vde"] == 0 and m["ffe"] == 0 and np.isnan(m["f0_rmse"]) and np.isnan(m["gpe"]) and np.isnan(m["f0_corr"])


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


def _metrics(lib, tl, idx, which=31, fmin=50.0, fmax=500.0, n_est=None, ws=_DUMMY, ws_bytes=1 << 30, out=_DUMMY):
    tl, tp = _i32(tl)
    idx, ip = _i32(idx)
    return lib.ssr_f0_metrics(_DUMMY, _DUMMY, tp, len(tl), _DUMMY, _DUMMY, ip, len(idx) if n_est is None else n_est, fmin, fmax,
                              which, out, ws, ws_bytes, None)


def _track(lib, ln, fmin=50.0, fmax=500.0, ws=_DUMMY, ws_bytes=1 << 30, f0=_DUMMY, n=None):
    ln, lp = _i32(ln)
    return lib.ssr_f0_track(_DUMMY, _DUMMY, lp, len(ln) if n is None else n, fmin, fmax, f0, _DUMMY, _DUMMY, _DUMMY, _DUMMY, ws,
                            ws_bytes, None)


def test_c_abi_rejects_bad_arguments_before_launch():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E = _lib.ERR_INVALID_ARG
    for w in (0, 32, -1, 64):
        assert _metrics(lib, [4000], [0], which=w) == E and "which" in err()
    for fmin, fmax in ((30.0, 500.0), (50.0, 1001.0), (500.0, 400.0), (990.0, 1000.0), (float("nan"), 500.0)):
        assert _metrics(lib, [4000], [0], fmin=fmin, fmax=fmax) == E and "fmin" in err()
        assert _track(lib, [4000], fmin=fmin, fmax=fmax) == E and "fmin" in err()
    assert _metrics(lib, [4000, 5000], [2]) == E and "tgt_index" in err()
    assert _metrics(lib, [4000, 5000], [0, -1]) == E and "tgt_index" in err()
    assert _metrics(lib, [-3], [0]) == E and "lengths" in err()
    assert _metrics(lib, [1 << 29], [0]) == E and "lengths" in err()
    assert _track(lib, [100, 1 << 29]) == E and "lengths" in err()
    assert _metrics(lib, [4000], [0], out=None) == E and "null" in err()
    assert _track(lib, [4000], f0=None) == E and "null" in err()
    tl, tp = _i32([4000, 9000])
    idx, ip = _i32([1, 1, 0])
    need = lib.ssr_f0_metrics_workspace_bytes(tp, 2, ip, 3, 50.0, 500.0, 31)
    assert need > 0
    assert _metrics(lib, [4000, 9000], [1, 1, 0], ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in err()
    assert _metrics(lib, [4000, 9000], [1, 1, 0], ws=None) == _lib.ERR_WORKSPACE
    tneed = lib.ssr_f0_track_workspace_bytes(tp, 2, 50.0, 500.0)
    assert 0 < tneed < need
    assert _track(lib, [4000, 9000], ws_bytes=tneed - 1) == _lib.ERR_WORKSPACE
    bad, bp = _i32([2])
    assert lib.ssr_f0_metrics_workspace_bytes(tp, 2, bp, 1, 50.0, 500.0, 31) == 0
    assert lib.ssr_f0_metrics_workspace_bytes(tp, 2, ip, 3, 50.0, 500.0, 0) == 0
    assert lib.ssr_f0_track_workspace_bytes(tp, 2, 500.0, 50.0) == 0
    assert _metrics(lib, [4000], [], n_est=0, ws=None, ws_bytes=0, out=None) == 0     # nothing to score: nothing queued
    assert _track(lib, [], ws=None, ws_bytes=0, f0=None) == 0


# ---- SSR_Eval_Helper / AudioMetrics options -----------------------------------------------------------------------------------
def test_helper_pitch_option_and_metric_order():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.eval import _METRIC_KEYS, _WAVEFORM_KEYS, _MEL_KEYS, _QUALITY_KEYS, _PITCH_KEYS
    mk = lambda v, sr=44100: SSR_Eval_Helper(BasicTestee(), 44100, 44100, evaluation_sr=sr, test_data_root=None, pitch=v)  # noqa: E731
    for ok in (None, True, "all", "gpe", ("vde", "f0_rmse"), {"which": "ffe"}, {"fmin": 60, "fmax": 400.0},
               {"which": ("gpe",), "fmin": 40.0, "fmax": 1000.0}):
        assert mk(ok).pitch == ok
    for bad in (False, "GPE", 1, ["gpe"], (), ("gpe", "pesq"), {}, {"which": "gpe", "lpc_order": 3}, {"fmin": 30},
                {"fmin": 500, "fmax": 400}, {"fmin": True}, {"fmax": "500"}):
        with pytest.raises(ValueError):
            mk(bad)
    for sr in (4000,):
        with pytest.raises(ValueError):
            mk(True, sr)
    assert _PITCH_KEYS == ("f0_rmse", "f0_corr", "gpe", "vde", "ffe")
    assert not set(_PITCH_KEYS) & set(_METRIC_KEYS + _WAVEFORM_KEYS + _MEL_KEYS + _QUALITY_KEYS)


def test_audio_metrics_pitch_which_values():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(16000)
    assert am._pitch_which("all") == 31 and am._pitch_which("f0_rmse") == 1 and am._pitch_which("ffe") == 16
    assert am._pitch_which(("ffe", "f0_corr")) == 18 and am._pitch_which(["gpe", "vde"]) == 12
    for bad in (None, True, 0, 31, "F0", (), ("gpe", "x")):
        with pytest.raises(ValueError):
            am._pitch_which(bad)
    assert am._pitch_dicts(np.array([[1.0, 2.0]]), 18) == [{"f0_corr": 1.0, "ffe": 2.0}]
    assert am._pitch_range(50, 500) == (50.0, 500.0)
    with pytest.raises(ValueError):
        am._pitch_range(50, 50)


# ---- the kernel bodies compiled for the host ---------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "pitch_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libpitch_emu.so")
P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    return C.CDLL(EMU_SO)


@pytest.mark.parametrize("fmin,fmax", [(50.0, 500.0), (40.0, 1000.0), (60.0, 400.0)])
def test_emulated_geometry(emu, fmin, fmax):
    res = np.zeros(5, np.int64)
    for n in (0, 1, 159, 160, 12345, 16000 * 3 + 7):
        emu.pitch_geometry(C.c_double(fmin), C.c_double(fmax), C.c_int64(n), P(res))
        lo, hi = O.lag_range(fmin, fmax)
        T = O.n_frames(n)
        assert tuple(res) == (lo, hi, T, -(-T // 8), -(-hi // 5))


def _ragged(sigs):
    lens = np.array([len(s) for s in sigs], np.int32)
    off = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    return np.concatenate(list(sigs) + [np.zeros(1)]).astype(np.float64), off, lens


def _signals(rng):
    fs = 16000
    n = 12000
    return [harmonic(np.linspace(90, 300, n), fs, n) * (1 + 0.5 * np.sin(np.arange(n) / 900.0)),
            harmonic(170.0, fs, 5000) + 0.02 * rng.standard_normal(5000),
            rng.standard_normal(3000),
            np.zeros(2000),
            np.zeros(0),
            harmonic(420.0, fs, 100),
            np.concatenate((np.zeros(2500), harmonic(65.0, fs, 6000), np.zeros(1500)))]


@pytest.mark.parametrize("fmin,fmax", [(50.0, 500.0), (40.0, 1000.0)])
def test_emulated_tracker_matches_the_oracle(emu, fmin, fmax):
    sigs = _signals(np.random.default_rng(11))
    data, off, lens = _ragged(sigs)
    T = np.array([O.n_frames(int(n)) for n in lens])
    tot = int(T.sum())
    f0, ap, en = np.zeros(tot + 1), np.zeros(tot + 1), np.zeros(tot + 1)
    vo = np.zeros(tot + 1, np.uint8)
    assert emu.pitch_track_emu(P(data), P(off), P(lens), len(sigs), C.c_double(fmin), C.c_double(fmax), P(f0), P(ap), P(en), P(vo)) == 0
    a = 0
    for s, t in zip(sigs, T):
        want = O.track16(s, fmin, fmax)
        st = want["stable"]
        assert st.mean() >= 0.99 if t else True
        sl = slice(a, a + t)
        np.testing.assert_array_equal(vo[sl].astype(bool)[st], want["voiced"][st])
        np.testing.assert_array_equal(np.isnan(f0[sl]), np.isnan(want["f0"]))
        ok = st & ~np.isnan(want["f0"])
        np.testing.assert_allclose(f0[sl][ok], want["f0"][ok], rtol=1e-10, atol=0)
        np.testing.assert_allclose(ap[sl][st], want["aperiodicity"][st], rtol=1e-10, atol=0)
        np.testing.assert_allclose(en[sl], want["energy"], rtol=1e-10, atol=0)
        a += t


def test_emulated_metrics_match_the_oracle(emu):
    rng = np.random.default_rng(12)
    fs = 16000
    tg = _signals(rng)
    ests, idx = [], []
    for i, x in enumerate(tg):        # per target: itself, a detuned copy, an octave below, a noisy copy (one run), ...
        n = len(x)
        f = np.linspace(90, 300, n) if i == 0 else 170.0
        ests += [x.copy(), harmonic(np.asarray(f) * 1.03, fs, n) if n else x.copy(), harmonic(np.asarray(f) / 2, fs, n) if n else x.copy(),
                 x + 0.05 * rng.standard_normal(n)]
        idx += [i] * 4
    ests.append(0.5 * tg[0])          # ... and one more for target 0, away from its run
    idx.append(0)
    td, to, tl = _ragged(tg)
    ed, eo, _ = _ragged(ests)
    ix = np.ascontiguousarray(idx, np.int32)
    out = np.full((len(ests), 5), -123.0)
    assert emu.pitch_metrics_emu(P(td), P(to), P(tl), len(tg), P(ed), P(eo), P(ix), len(ests), C.c_double(50.0), C.c_double(500.0), 31,
                                 P(out)) == 0
    checked = 0
    for e, (y, i) in enumerate(zip(ests, idx)):
        want, stable = O.pitch(tg[i], y, fs)
        if not stable:
            continue
        checked += 1
        for j, m in enumerate(O.NAMES):
            if np.isnan(want[m]):
                assert np.isnan(out[e, j]), (e, m, out[e, j])
            else:
                assert abs(out[e, j] - want[m]) <= 1e-10 * max(1.0, abs(want[m])), (e, m, out[e, j], want[m])
    assert checked >= len(ests) - 3
    for which in (1, 2, 4, 8, 16, 5, 24, 19):     # subsets: the same values in bit order
        sub = np.full((len(ests), bin(which).count("1")), -123.0)
        emu.pitch_metrics_emu(P(td), P(to), P(tl), len(tg), P(ed), P(eo), P(ix), len(ests), C.c_double(50.0), C.c_double(500.0), which,
                              P(sub))
        np.testing.assert_array_equal(sub, out[:, [j for j in range(5) if which & (1 << j)]])
    alone = np.zeros((1, 5))                       # a pair alone gives the bits it has in the batch
    d1, o1, l1 = _ragged([tg[1]])
    e1, eo1, _ = _ragged([ests[5]])
    emu.pitch_metrics_emu(P(d1), P(o1), P(l1), 1, P(e1), P(eo1), P(np.zeros(1, np.int32)), 1, C.c_double(50.0), C.c_double(500.0), 31,
                          P(alone))
    np.testing.assert_array_equal(alone[0], out[5])
