"""CPU tests of the anti-wrapping phase distances (phase_ip, phase_gd, phase_iaf): properties of the float64
oracle (tests/phase_oracle.py), a g++ build of the kernel bodies (ssr_phase.h) against the oracle, the C ABI's argument checks
(they return before anything touches a device), AudioMetrics / SSR_Eval_Helper(phase=...) validation and metric order.

The bound of the emulated-kernel comparison, 1e-9 rad, comes from an argument: the transform's rounding error is a few
1e-16 log2(N) of the frame's largest bin, so a cell at ratio r of that maximum has a phase error of about 1e-15 / r; the tests use
seeded Gaussian float32 noise of one level in both signals and assert through phase_oracle.conditioning() that every scored cell
has r >= 1e-6."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import phase_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
R_MIN = 1e-6


def _noise(rng, n, dtype=np.float32):
    return rng.standard_normal(n).astype(np.float32).astype(dtype)


# ---- oracle properties -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    rng = np.random.default_rng(17)
    return _noise(rng, 6000), _noise(rng, 6000)


@pytest.mark.parametrize("n_fft,hop,band", [(1024, 256, None), (512, 200, (3, 200)), (256, 256, (0, 128)), (2048, 512, (7, 7))])
def test_product_form_is_the_literal_anti_wrapping_form(pair, n_fft, hop, band):
    x, y = pair
    got, want = O.phase_distance(x, y, n_fft, hop, band), O.phase_distance_literal(x, y, n_fft, hop, band)
    for m in O.NAMES:
        assert abs(got[m] - want[m]) < 1e-12 or (np.isnan(got[m]) and np.isnan(want[m])), (m, got[m], want[m])
    assert all(0.0 <= got[m] <= np.pi for m in O.NAMES if not np.isnan(got[m]))


def test_identical_and_negated_estimates(pair):
    x, _ = pair
    same, neg = O.phase_distance(x, x, 512, 128), O.phase_distance(x, -x, 512, 128)
    assert all(same[m] <= 1e-12 for m in O.NAMES)
    assert abs(neg["phase_ip"] - np.pi) <= 1e-12 and neg["phase_gd"] <= 1e-12 and neg["phase_iaf"] <= 1e-12


def test_a_power_of_two_on_the_estimate_changes_no_bit(pair):
    x, y = pair
    assert O.phase_distance(x, 4.0 * y.astype(np.float64)) == O.phase_distance(x, y)


def test_zero_rule_and_nan_cases():
    assert O.a(np.array([-0.0 + 0j, complex(0.0, -0.0), complex(-0.0, -0.0), -1.0 + 0j, 1j]))[:3].tolist() == [0.0, 0.0, 0.0]
    assert O.a(np.array([complex(-1.0, -0.0)]))[0] == np.pi
    z = np.zeros(4000)
    assert O.phase_distance(z, z, 512, 128) == {m: 0.0 for m in O.NAMES}             # digital silence scores 0 and is counted
    for n in (0, 1, 512):                                                            # n <= N / 2: no reflect padding
        assert all(np.isnan(v) for v in O.phase_distance(np.ones(n), np.ones(n), 1024).values())
    one = O.phase_distance(np.ones(513), -np.ones(513), 1024, 1024)                  # T = 1: no time difference
    assert O.num_frames(513, 1024, 1024) == 1 and np.isnan(one["phase_iaf"]) and not np.isnan(one["phase_ip"])
    rng = np.random.default_rng(2)
    single = O.phase_distance(_noise(rng, 900), _noise(rng, 900), 256, 64, (5, 5))   # one bin: no frequency difference
    assert np.isnan(single["phase_gd"]) and not np.isnan(single["phase_ip"]) and not np.isnan(single["phase_iaf"])
    assert [O.num_frames(n, 1024, 256) for n in (512, 513, 767, 768, 48000)] == [0, 3, 3, 4, 188]


# ---- the kernel bodies compiled for the host -------------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "phase_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libphase_emu.so")


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    return C.CDLL(EMU_SO)


def run_emu(lib, tgts, ests, idx, n_fft, hop, band=None, which=7):
    t64, e64 = tgts[0].dtype == np.float64, ests[0].dtype == np.float64
    P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    tl = np.array([len(t) for t in tgts], np.int32)
    el = np.array([len(e) for e in ests], np.int64)
    to = np.concatenate(([0], np.cumsum(tl)[:-1])).astype(np.int64)
    eo = np.concatenate(([0], np.cumsum(el)[:-1])).astype(np.int64)
    td = np.concatenate(tgts + [np.zeros(1, tgts[0].dtype)])
    ed = np.concatenate(ests + [np.zeros(1, ests[0].dtype)])
    idx = np.ascontiguousarray(idx, np.int32)
    lo, hi = (0, n_fft // 2) if band is None else band
    out = np.full((len(ests), bin(which).count("1")), -123.0)
    assert lib.phase_emu(P(td), int(t64), P(to), P(tl), len(tgts), P(ed), int(e64), P(eo), P(idx), len(ests), n_fft, hop, lo, hi, which,
                         P(out)) == 0
    return out


def check_rows(got, tgts, ests, idx, n_fft, hop, band=None):
    """Every value within TOL of the oracle (NaN where it has NaN), every scored cell at r >= R_MIN -> the worst difference."""
    worst = 0.0
    for e, (y, i) in enumerate(zip(ests, idx)):
        want = O.phase_distance(tgts[i], y, n_fft, hop, band)
        assert min(O.conditioning(tgts[i], y, n_fft, hop, band)) >= R_MIN, (e, O.conditioning(tgts[i], y, n_fft, hop, band))
        for j, m in enumerate(O.NAMES):
            if np.isnan(want[m]):
                assert np.isnan(got[e, j]), (e, m, got[e, j])
            else:
                worst = max(worst, abs(got[e, j] - want[m]))
                assert abs(got[e, j] - want[m]) <= TOL, (e, m, got[e, j], want[m])
    return worst


def test_emulated_geometry(emu):
    res = np.zeros(3, np.int64)
    for n_fft, hop in ((256, 64), (1024, 1024), (2048, 683)):
        for n in (0, 1, n_fft // 2, n_fft // 2 + 1, 15 * hop, 16 * hop, 16 * hop + n_fft, 48000 * 60):
            emu.phase_geometry(n, n_fft, hop, res.ctypes.data_as(C.c_void_p))
            T = O.num_frames(n, n_fft, hop)
            assert tuple(res) == (T, -(-T // 16), 16)


def _len_for_frames(T, n_fft, hop):
    """The smallest valid n with T frames, plus a few samples (T = 1 + n // hop, n > n_fft / 2)."""
    n = max((T - 1) * hop, n_fft // 2 + 1)
    n = min(n + 3, T * hop - 1)
    assert O.num_frames(n, n_fft, hop) == T, (T, n_fft, hop, n)
    return n


@pytest.mark.parametrize("n_fft", O.N_FFTS)
def test_emulated_kernels_match_the_oracle(emu, n_fft):
    """One batch per transform size: T = 1 and 2 (hop = n_fft), the chunk edges T = FR, FR + 1 and 2 FR + 1 (hop = n_fft / 4: IAF
    across a chunk boundary and the warm-up frame), a hop that does not divide n_fft, the shortest valid length, and a signal too
    short for its padding; then the bands, on the same batch."""
    rng = np.random.default_rng(100 + n_fft)
    FR, q, odd = 16, n_fft // 4, n_fft // 3 + 1
    for hop, frames in ((n_fft, (1, 2, 5)), (q, (FR, FR + 1, 2 * FR + 1)), (odd, (2, FR + 1))):
        lens = [_len_for_frames(T, n_fft, hop) for T in frames] +[n_fft // 2 + 1, n_fft // 2, 0]
        tg = [_noise(rng, n) for n in lens]
        ests = [_noise(rng, n) for n in lens] + [_noise(rng, lens[0])]
        idx = list(range(len(lens))) + [0]
        got = run_emu(emu, tg, ests, idx, n_fft, hop)
        check_rows(got, tg, ests, idx, n_fft, hop)
        assert np.isnan(got[len(lens) - 2:len(lens)]).all()                        # n = N / 2 and n = 0
        # subsets: IP alone and IP | GD give the IP (and GD) bits of the full call; IAF alone its bits
        np.testing.assert_array_equal(run_emu(emu, tg, ests, idx, n_fft, hop, which=1), got[:, :1])
        np.testing.assert_array_equal(run_emu(emu, tg, ests, idx, n_fft, hop, which=3), got[:, :2])
        np.testing.assert_array_equal(run_emu(emu, tg, ests, idx, n_fft, hop, which=6), got[:, 1:])
        # a pair alone gives the bits it has in the batch
        np.testing.assert_array_equal(run_emu(emu, [tg[1]], [ests[1]], [0], n_fft, hop)[0], got[1])
    # bands, on the last batch: the full range again, the two edge bins alone, an interior band
    for band in ((0, n_fft // 2), (0, 0), (n_fft // 2, n_fft // 2), (n_fft // 8 + 1, n_fft // 4 + 2)):
        sub = run_emu(emu, tg, ests, idx, n_fft, odd, band)
        check_rows(sub, tg, ests, idx, n_fft, odd, band)
        if band[0] == band[1]:
            assert np.isnan(sub[:, 1]).all() and not np.isnan(sub[0, 0]) and not np.isnan(sub[0, 2])


def test_emulated_mixed_dtypes_and_y_equal_x(emu):
    rng = np.random.default_rng(5)
    n_fft, hop, n = 512, 128, 3000
    for dt in ((np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)):
        x = _noise(rng, n, dt[0])
        ests = [_noise(rng, n, dt[1]), x.astype(dt[1]), (-x).astype(dt[1])]
        got = run_emu(emu, [x], ests, [0, 0, 0], n_fft, hop)
        check_rows(got, [x], ests, [0, 0, 0], n_fft, hop)
        assert (got[1] <= 1e-12).all()                                             # y = x: not exactly 0, the packed split rounds
        assert abs(got[2, 0] - np.pi) <= 1e-12 and (got[2, 1:] <= 1e-12).all()     # y = -x


def test_emulated_zero_rule(emu):
    """A stretch of exact zeros longer than n_fft in both signals, and one in the estimate only: the silent frames score 0 and are
    counted (the packed transform alone would return the loud frame's rounding error as the silent frame's spectrum)."""
    rng = np.random.default_rng(6)
    n_fft, hop, n = 256, 64, 40 * 64
    x, y, y2 = _noise(rng, n), _noise(rng, n), _noise(rng, n)
    x[700:700 + 3 * n_fft] = 0.0
    y[700:700 + 3 * n_fft] = 0.0
    y2[1500:1500 + 2 * n_fft + 17] = 0.0
    z = np.zeros(n, np.float32)
    ests = [y, y2, z]
    got = run_emu(emu, [x], ests, [0, 0, 0], n_fft, hop)
    check_rows(got, [x], ests, [0, 0, 0], n_fft, hop)
    assert got[2].tolist() == [0.0, 0.0, 0.0]
    # independent noise has a mean phase distance of pi / 2; the 8 silent frames of 41 pull it down to about 0.8 of that
    assert got[0, 0] < 0.9 * np.pi / 2


# ---- C ABI argument checks (no device call happens before any of these errors) ------------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


def _call(lib, tl, idx, which=7, n_fft=1024, hop=256, lo=0, hi=None, n_est=None, ws=_DUMMY, ws_bytes=1 << 30, out=_DUMMY):
    tl, tp = _i32(tl)
    idx, ip = _i32(idx)
    return lib.ssr_phase_metrics(_DUMMY, 0, _DUMMY, tp, len(tl), _DUMMY, 0, _DUMMY, ip, len(idx) if n_est is None else n_est, n_fft,
                                 hop, lo, n_fft // 2 if hi is None else hi, which, out, ws, ws_bytes, None)


def test_phase_metrics_rejects_bad_arguments_before_launch():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E = _lib.ERR_INVALID_ARG
    for w in (0, 8, -1, 15):
        assert _call(lib, [4000], [0], which=w) == E and "which" in err()
    for n_fft in (0, 128, 255, 1000, 4096, -1024):
        assert _call(lib, [4000], [0], n_fft=n_fft, hop=64, hi=0) == E and "n_fft" in err()
    for hop in (0, -1, 1025):
        assert _call(lib, [4000], [0], hop=hop) == E and "hop" in err()
    for lo, hi in ((-1, 5), (6, 5), (0, 513), (513, 513)):
        assert _call(lib, [4000], [0], lo=lo, hi=hi) == E and "bin" in err()
    assert _call(lib, [4000, 5000], [2]) == E and "tgt_index" in err()
    assert _call(lib, [4000, 5000], [0, -1]) == E and "tgt_index" in err()
    assert _call(lib, [-3], [0]) == E and "lengths" in err()
    assert _call(lib, [1 << 29], [0]) == E and "lengths" in err()
    assert _call(lib, [4000], [0], out=None) == E and "null" in err()
    tl, tp = _i32([4000, 9000])
    idx, ip = _i32([1, 1, 0])
    need = lib.ssr_phase_metrics_workspace_bytes(tp, 2, ip, 3, 1024, 256, 7)
    assert need > 0 and lib.ssr_phase_metrics_workspace_bytes(tp, 2, ip, 3, 1024, 256, 1) == need
    assert _call(lib, [4000, 9000], [1, 1, 0], ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in err()
    assert _call(lib, [4000, 9000], [1, 1, 0], ws=None) == _lib.ERR_WORKSPACE
    bad, bp = _i32([2])
    assert lib.ssr_phase_metrics_workspace_bytes(tp, 2, bp, 1, 1024, 256, 7) == 0
    assert lib.ssr_phase_metrics_workspace_bytes(tp, 2, ip, 3, 1000, 256, 7) == 0
    assert lib.ssr_phase_metrics_workspace_bytes(tp, 2, ip, 3, 1024, 0, 7) == 0
    assert lib.ssr_phase_metrics_workspace_bytes(tp, 2, ip, 3, 1024, 256, 0) == 0
    assert _call(lib, [4000], [], n_est=0, ws=None, ws_bytes=0, out=None) == 0     # nothing to score: nothing queued


# ---- AudioMetrics / SSR_Eval_Helper options --------------------------------------------------------------------------------------
def test_audio_metrics_phase_options():
    from ssr_eval_amd import AudioMetrics
    from ssr_eval_amd import backend as B
    am = AudioMetrics(48000)
    assert am._phase_which("all") == 7 and am._phase_which("phase_ip") == 1 and am._phase_which(("phase_iaf", "phase_gd")) == 6
    for bad in (None, True, 0, 7, "ip", (), ("phase_ip", "x")):
        with pytest.raises(ValueError):
            am._phase_which(bad)
    assert am._phase_dicts(np.array([[1.0, 2.0]]), 5) == [{"phase_ip": 1.0, "phase_iaf": 2.0}]
    assert B.check_phase_frames(1024, None) == (1024, 256) and B.check_phase_frames(np.int64(256), 256) == (256, 256)
    for bad in ((1000, None), (4096, None), (1024.0, None), (True, None), (1024, 0), (1024, 1025), (1024, 2.0), (1024, True)):
        with pytest.raises(ValueError):
            B.check_phase_frames(*bad)
    # band -> bins: k_lo = ceil(lo N / rate), k_hi = floor(hi N / rate), clamped to [0, N / 2]
    assert am._phase_bins(48000, 1024, None) is None
    assert am._phase_bins(48000, 1024, (0, 24000)) == (0, 512) and am._phase_bins(48000, 1024, (-5.0, 1e9)) == (0, 512)
    assert am._phase_bins(48000, 1024, (4000, 8000)) == (86, 170) and am._phase_bins(48000, 1024, (3000, 3000)) == (64, 64)
    assert am._phase_bins(48000, 2048, (23437.5, 24000)) == (1000, 1024)
    for bad in ((8000, 4000), (3001, 3040), (24001, 30000), (1, 2, 3), "all", (None, 5), (0, float("nan")), (True, 5)):
        with pytest.raises(ValueError):
            am._phase_bins(48000, 1024, bad)
    for kw in ({"which": "x"}, {"n_fft": 300}, {"hop": 0}, {"band": (5, 1)}):        # rejected before any device is touched
        with pytest.raises(ValueError):
            am.phase_distance(np.zeros(2000, np.float32), np.zeros(2000, np.float32), **kw)


def test_helper_phase_option_and_metric_order():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.eval import _FAMILIES, _METRIC_KEYS, _WAVEFORM_KEYS, _MEL_KEYS, _MEL_DTW_KEYS, _QUALITY_KEYS, _PITCH_KEYS, \
        _PHASE_KEYS, result_key_order
    mk = lambda v: SSR_Eval_Helper(BasicTestee(), 44100, 44100, test_data_root=None, phase=v)      # noqa: E731
    for ok in (None, True, "phase_ip", ("phase_gd", "phase_iaf"), {"which": "phase_iaf"}, {"n_fft": 2048}, {"hop": 100},
               {"which": ("phase_ip",), "n_fft": 512, "hop": 512, "band": (4000, 16000)}, {"band": (0, 1e6)}):
        assert mk(ok).phase == ok
    for bad in (False, "ip", 1, ["phase_ip"], (), ("phase_ip", "lsd"), ("phase_ip", True), {}, {"fft": 512}, {"n_fft": 1000},
                {"n_fft": 4096}, {"hop": 0}, {"hop": 1025}, {"hop": 2.5}, {"band": (8000, 4000)}, {"band": 4000}, {"which": "x"},
                {"n_fft": 256, "hop": 257}):
        with pytest.raises(ValueError):
            mk(bad)
    assert _PHASE_KEYS == ("phase_ip", "phase_gd", "phase_iaf")
    names = [f[0] for f in _FAMILIES]
    assert names.index("phase") == names.index("pitch") + 1
    order = result_key_order()
    at = order.index("phase_ip")
    assert order[at:at + 3] == _PHASE_KEYS
    assert order[:at] == _METRIC_KEYS + _WAVEFORM_KEYS + _MEL_KEYS + _MEL_DTW_KEYS + _QUALITY_KEYS + _PITCH_KEYS
    assert order[:at] == ("lsd", "log_sispec", "sispec", "ssim", "lsd_lf", "lsd_hf", "stoi", "estoi", "snr", "si_sdr", "seg_snr",
                        "mel_lsd", "mel_l1", "mcd", "mcd_dtw", "dtw_dev", "llr", "cep_dist", "wss", "fwseg_snr", "f0_rmse", "f0_corr",
                        "gpe", "vde", "ffe")
    assert len(set(order)) == len(order)
