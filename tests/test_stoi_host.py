"""CPU tests of STOI / ESTOI: the Octave tap design and the custom-filter resampling plan against SciPy's own bookkeeping, the
band matrix, properties of the float64 oracle (tests/stoi_oracle.py), the C ABI's argument checks (they return before anything
touches a device), SSR_Eval_Helper(stoi=...) validation, and a g++ build of the kernel bodies (ssr_stoi.h) against the oracle."""
import ctypes as C
import glob
import os
import subprocess
from math import gcd

import numpy as np
import pytest

import stoi_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- resampling plan --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,taps", [(48000, 1741), (16000, 581), (44100, 31947)])
def test_octave_taps_match_the_oracle_and_the_issue_table(fs, taps):
    from ssr_eval_amd.backend import octave_taps
    g = gcd(10000, fs)
    h = octave_taps(10000 // g, fs // g)
    assert len(h) == taps
    assert np.array_equal(h, O.octave_window(10000 // g, fs // g))
    assert abs(np.sum(h) - 1.0) < 1e-12


def _scipy_plan(n_in, up, down, h):
    """scipy.signal.resample_poly's integer bookkeeping for an array window (SciPy 1.15, _signaltools.resample_poly)."""
    half_len = (h.size - 1) // 2
    n_out = n_in * up // down + bool(n_in * up % down)
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    out_len = lambda nh: ((n_in - 1) * up + nh - 1) // down + 1     # noqa: E731
    n_post_pad = 0
    while out_len(len(h) + n_pre_pad + n_post_pad) < n_out + n_pre_remove:
        n_post_pad += 1
    return half_len, n_pre_pad, n_pre_remove, n_out, n_post_pad


@pytest.mark.parametrize("fs", [16000, 44100, 48000, 8000, 22050])
def test_custom_filter_plan_matches_scipy(fs):
    from scipy.signal import resample_poly
    from ssr_eval_amd.backend import StoiResamplePlan
    p = StoiResamplePlan(fs, "cpu")
    g = gcd(10000, fs)
    assert (p.up, p.down) == (10000 // g, fs // g)
    h = O.octave_window(p.up, p.down)
    for n_in in (1, 257, 4000, 12345, 48000):
        hl, pre, rem, n_out, post = _scipy_plan(n_in, p.up, p.down, h)
        assert (p.half_len, p.n_pre_pad, p.n_pre_remove, p.n_out(n_in), p.n_post_pad(n_in)) == (hl, pre, rem, n_out, post)
        assert len(resample_poly(np.ones(n_in), p.up, p.down, window=h)) == n_out
    assert np.array_equal(p.taps_host[p.n_pre_pad:], h * p.up) and not p.taps_host[:p.n_pre_pad].any()


def test_identity_plan_at_10k():
    from ssr_eval_amd.backend import StoiResamplePlan
    p = StoiResamplePlan(10000, "cpu")
    assert p.identity and p.n_out(777) == 777


def test_scipy_keeps_the_array_window_in_float64():
    """The reason a float32 signal is widened before ssr_resample_poly_f64: SciPy resamples it in float64."""
    from scipy.signal import resample_poly
    x = np.random.default_rng(1).standard_normal(3000).astype(np.float32)
    h = O.octave_window(5, 24)
    y = resample_poly(x, 5, 24, window=h)
    assert y.dtype == np.float64 and np.array_equal(y, resample_poly(x.astype(np.float64), 5, 24, window=h))


# ---- band matrix --------------------------------------------------------------------------------------------------------------
def test_band_edges_of_the_library_and_the_oracle():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    lo, hi = np.zeros(15, np.int32), np.zeros(15, np.int32)
    assert lib.ssr_stoi_band_edges(lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)) == 0
    obm, olo, ohi = O.thirdoct()
    assert np.array_equal(lo, olo) and np.array_equal(hi, ohi)
    assert lo.tolist() == [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]
    assert hi.tolist() == lo.tolist()[1:] + [219]
    assert obm.shape == (15, 257) and np.array_equal(obm.sum(axis=1), hi - lo)


# ---- oracle properties ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def speech():
    rng = np.random.default_rng(7)
    x = O.speech_like(rng, 30000, 10000)
    return x, x + 0.5 * np.abs(x).max() * rng.standard_normal(x.shape)


def test_oracle_identity_scores_one(speech):
    x, _ = speech
    assert abs(O.stoi_10k(x, x) - 1) < 1e-12
    assert abs(O.stoi_10k(x, x, True) - 1) < 1e-12


def test_oracle_is_invariant_to_estimate_scale(speech):
    x, y = speech
    for ext in (False, True):
        d = O.stoi_10k(x, y, ext)
        assert 0 < d < 1
        assert abs(O.stoi_10k(x, 3.7 * y, ext) - d) < 1e-12


def test_oracle_all_zero_target_scores_zero(speech):
    _, y = speech
    assert O.stoi_10k(np.zeros_like(y), y) == 0.0
    assert O.stoi_10k(np.zeros_like(y), y, True) == 0.0


def test_oracle_short_signals_score_1e5(speech):
    x, y = speech
    # 31 frames of 128-sample hop -> 30 kept frames at most -> 29 STFT frames: below N = 30
    n = 256 + 30 * 128
    assert O.stoi_10k(x[:n], y[:n]) == 1e-5 and O.stoi_10k(x[:n], y[:n], True) == 1e-5
    assert O.stoi_10k(x[:n + 128], y[:n + 128]) != 1e-5
    assert O.stoi_10k(x[:200], y[:200]) == 1e-5


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


def _call(lib, tl, el, idx, which=1, n_tgt=None, n_est=None, ws=_DUMMY, ws_bytes=1 << 30, out=_DUMMY, est=_DUMMY):
    tl, tp = _i32(tl)
    el, ep = _i32(el)
    idx, ip = _i32(idx)
    return lib.ssr_stoi(_DUMMY, _DUMMY, tp, len(tl) if n_tgt is None else n_tgt, est, _DUMMY, ep, ip,
                        len(el) if n_est is None else n_est, which, out, ws, ws_bytes, None)


def test_stoi_rejects_bad_arguments_before_launch():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E = _lib.ERR_INVALID_ARG
    assert _call(lib, [4000, 5000], [4000], [2]) == E and "tgt_index" in err()
    assert _call(lib, [4000, 5000], [4000], [-1]) == E and "tgt_index" in err()
    assert _call(lib, [4000, 5000], [4001], [0]) == E and "length" in err()
    assert _call(lib, [4000, 5000], [4000, 4000], [0, 1]) == E and "length" in err()
    assert _call(lib, [-3], [-3], [0]) == E and "lengths" in err()
    assert _call(lib, [1 << 29], [1 << 29], [0]) == E and "lengths" in err()
    for w in (0, 4, -1):
        assert _call(lib, [4000], [4000], [0], which=w) == E and "which" in err()
    assert _call(lib, [4000], [4000], [0], out=None) == E and "null" in err()
    assert _call(lib, [4000], [4000], [0], est=None) == E and "null" in err()
    assert _call(lib, [4000], [4000], [0], n_tgt=-1) == E
    tl, tp = _i32([4000, 9000])
    idx, ip = _i32([1, 0, 1])
    need = lib.ssr_stoi_workspace_bytes(tp, 2, ip, 3)
    assert need > 0
    assert _call(lib, [4000, 9000], [9000, 4000, 9000], [1, 0, 1], ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in err()
    assert _call(lib, [4000, 9000], [9000, 4000, 9000], [1, 0, 1], ws=None) == _lib.ERR_WORKSPACE
    bad, bp = _i32([2])
    assert lib.ssr_stoi_workspace_bytes(tp, 2, bp, 1) == 0
    assert _call(lib, [4000], [], [], n_est=0) == 0           # nothing to score: nothing queued


# ---- SSR_Eval_Helper option ---------------------------------------------------------------------------------------------------
def test_helper_stoi_option():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.eval import _METRIC_KEYS
    mk = lambda v: SSR_Eval_Helper(BasicTestee(), 44100, 44100, test_data_root=None, stoi=v)      # noqa: E731
    for ok in (None, "stoi", "estoi", "both"):
        assert mk(ok).stoi == ok
    for bad in (True, False, "STOI", 1, ["stoi"]):
        with pytest.raises(ValueError):
            mk(bad)
    assert _METRIC_KEYS == ("lsd", "log_sispec", "sispec", "ssim", "lsd_lf", "lsd_hf", "stoi", "estoi")


def test_audio_metrics_extended_values():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(16000)
    assert am._stoi_which(False) == 1 and am._stoi_which(True) == 2 and am._stoi_which("both") == 3
    for bad in (None, 0, 1, "estoi"):
        with pytest.raises(ValueError):
            am._stoi_which(bad)


# ---- the kernel bodies compiled for the host ---------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "stoi_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libstoi_emu.so")


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    return C.CDLL(EMU_SO)


def run_emu(lib, tgts, ests, idx, which):
    sig = list(tgts) + list(ests)
    lens = np.array([len(s) for s in sig], np.int32)
    off = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    data = np.concatenate(sig).astype(np.float64)
    nt = len(tgts)
    out = np.zeros((len(ests), 2 if which == 3 else 1))
    idx = np.ascontiguousarray(idx, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    to, eo = off[:nt].copy(), off[nt:].copy()
    assert lib.stoi_emu(P(data), P(to), P(data), P(eo), P(lens), P(idx), nt, len(ests), which, P(out)) == 0
    return out


def test_emulated_kernels_match_the_oracle(emu):
    rng = np.random.default_rng(3)
    lens = [8000, 12345, 20000, 3000, 4000, 9999, 6000]
    tg = [O.speech_like(rng, n, 10000) for n in lens[:-1]] + [np.zeros(lens[-1])]
    ests, idx = [], []
    for i, t in enumerate(tg):               # two estimates per target: noisy, and scaled + filtered
        ests.append(t + 0.3 * (np.abs(t).max() + 1e-3) * rng.standard_normal(len(t)))
        ests.append(0.2 * np.convolve(t, [0.5, 0.3, 0.2], "same") + 0.01 * rng.standard_normal(len(t)))
        idx += [i, i]
    got = run_emu(emu, tg, ests, idx, 3)
    for e, (y, i) in enumerate(zip(ests, idx)):
        assert abs(got[e, 0] - O.stoi_10k(tg[i], y)) < 1e-12
        assert abs(got[e, 1] - O.stoi_10k(tg[i], y, True)) < 1e-12
    assert np.array_equal(run_emu(emu, tg, ests, idx, 1)[:, 0], got[:, 0])
    assert np.array_equal(run_emu(emu, tg, ests, idx, 2)[:, 0], got[:, 1])
