"""CPU tests of the filter-invariant SDR (BSS Eval's SDR, 1 .. 512-tap distortion filter): self-checks of the
float64 oracle (tests/bss_oracle.py), a g++ build of the kernel bodies (ssr_bss.h) against it - the input list, the shapes where
the geometry can go wrong, the exact facts -, the C ABI's argument checks (they return before anything touches a device), the
header / ctypes table / library agreement, and SSR_Eval_Helper(bss_sdr=...) validation and metric order.

The bar on `sdr` is 1e-6 dB: the dense solve and Levinson's recursion agree to 1e-9 dB on these inputs, and three orders are left
for the kernels' summation order.  The worst difference seen in emulation is 6.1e-10 dB."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import bss_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_DB = 1e-6
TILE = 16384
targets, estimates, exact_fir_pair = O.targets, O.estimates, O.exact_fir_pair


# ---- oracle self-checks -------------------------------------------------------------------------------------------------------
def test_one_tap_is_the_closed_form():
    for name, x in targets(n=6000).items():
        for kind, y in estimates(x).items():
            got, want = O.bss_sdr(x, y, 1)[0], O.closed_form_one_tap(x, y)
            print(name, kind, got, want)
            assert abs(got - want) < 1e-12, (name, kind, got, want)


def test_levinson_route_agrees_with_the_dense_solve():
    worst = 0.0
    for name, x in targets().items():
        for kind, y in estimates(x).items():
            a, b = O.bss_sdr(x, y)[0], O.bss_sdr(x, y, levinson=True)[0]
            print(name, kind, "%.9f %.9f" % (a, b))
            worst = max(worst, abs(a - b))
            assert abs(a - b) < 1e-8, (name, kind, a, b)
    print("worst", worst)


def test_oracle_uses_only_the_terms_that_exist():
    rng = np.random.default_rng(2)
    x, y = rng.standard_normal(5), rng.standard_normal(5)
    r, b = O.correlations(x, y, 512)
    assert np.all(r[5:] == 0.0) and np.all(b[5:] == 0.0) and r[4] == x[0] * x[4] and b[4] == x[0] * y[4]
    full = np.correlate(np.concatenate([y, np.zeros(511)]), x, "valid")       # the zero-padded support of n + L - 1 samples
    np.testing.assert_allclose(b, full, atol=1e-15)
    assert np.isfinite(O.bss_sdr(x, y)[0])
    assert all(np.isnan(v) for v in O.bss_sdr(np.zeros(0), np.zeros(0))[:2])
    assert all(np.isnan(v) for v in O.bss_sdr(np.zeros(9), np.ones(9))[:2]) and np.all(O.bss_sdr(np.zeros(9), np.ones(9))[2] == 0.0)


# ---- the kernel bodies compiled for the host -----------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "bss_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libbss_emu.so")


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    return C.CDLL(EMU_SO)


def run_emu(lib, tgts, ests, idx, taps, filt=True):
    """-> (out [n_est, 2], filt [n_est, taps] or None)"""
    t64, e64 = tgts[0].dtype == np.float64, ests[0].dtype == np.float64
    P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    tl = np.array([len(t) for t in tgts], np.int32)
    el = np.array([len(e) for e in ests], np.int64)
    to = np.concatenate(([0], np.cumsum(tl)[:-1])).astype(np.int64)
    eo = np.concatenate(([0], np.cumsum(el)[:-1])).astype(np.int64)
    td = np.concatenate(list(tgts) + [np.zeros(1, tgts[0].dtype)])
    ed = np.concatenate(list(ests) + [np.zeros(1, ests[0].dtype)])
    idx = np.ascontiguousarray(idx, np.int32)
    out = np.full((len(ests), 2), -123.0)
    f = np.full((len(ests), taps), -7.0) if filt else None
    assert lib.bss_emu(P(td), int(t64), P(to), P(tl), len(tgts), P(ed), int(e64), P(eo), P(idx), len(ests), taps, P(out),
                       P(f) if filt else None) == 0
    return out, f


def check_rows(out, tgts, ests, idx, taps, what=""):
    """every row against the oracle: sdr within TOL_DB (NaN where it has NaN), sdr_lag equal -> the worst sdr difference"""
    worst = 0.0
    for e, (y, i) in enumerate(zip(ests, idx)):
        sdr, lag, _ = O.bss_sdr(tgts[i], y, taps)
        print(what, "pair", e, "n", len(y), "taps", taps, "got", out[e], "want", sdr, lag)
        if np.isnan(sdr):
            assert np.isnan(out[e]).all(), (what, e, out[e])
            continue
        assert abs(out[e, 0] - sdr) < TOL_DB, (what, e, out[e, 0], sdr)
        assert out[e, 1] == lag, (what, e, out[e, 1], lag)
        worst = max(worst, abs(out[e, 0] - sdr))
    return worst


@pytest.mark.parametrize("dt", [(np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64), (np.float64, np.float64)],
                         ids=["f32-f32", "f64-f32", "f32-f64", "f64-f64"])
def test_emulated_kernels_match_the_oracle_on_the_input_list(emu, dt):
    """The five targets with three estimates each, next to each other (a run per target), at 512 taps."""
    tg = [x.astype(dt[0]) for x in targets().values()]
    names = list(targets())
    ests, idx = [], []
    for i, x in enumerate(tg):
        for y in estimates(x.astype(np.float64)).values():
            ests.append(y.astype(dt[1]))
            idx.append(i)
    out, filt = run_emu(emu, tg, ests, idx, 512)
    worst = check_rows(out, tg, ests, idx, 512, "inputs")
    print("worst sdr difference", worst)
    # the delayed estimates: tap 37 - except on the sine, whose every shift is a combination of two others (the oracle's least-squares
    # filter peaks at tap 0 there, and check_rows has held the kernels to it)
    assert [out[3 * i + 2, 1] for i, m in enumerate(names) if m != "sine"] == [37.0] * 4
    for e in range(3):                                                                         # the white target: condition about 2
        c = O.bss_sdr(tg[0], ests[e], 512)[2]
        assert names[0] == "white" and np.max(np.abs(filt[e] - c)) <= 1e-10 * np.max(np.abs(c)), e
    # what the numbers mean: the noise levels, and for the delayed estimate the 37 samples of 0.7 x that fall behind the estimate's
    # end (10 log10(24000 / 37) = 28 dB; snr and si_sdr give about 0 dB here)
    assert 19.9 < out[0, 0] < 20.3 and 99.0 < out[1, 0] < 101.0 and 26.0 < out[2, 0] < 30.0


@pytest.mark.parametrize("L", [1, 2, 64, 511, 512])
def test_emulated_geometry_shapes(emu, L):
    """n in {0, 1, 5, L - 1, L, L + 1, one tile - 1, one tile + 1, 4099} in ONE batch, three estimates sharing the 4099 target in a
    run next to the singletons; float32 targets, float64 estimates.  n < L uses only the terms that exist."""
    rng = np.random.default_rng(100 + L)
    lens = [0, 1, 5, max(L - 1, 0), L, L + 1, TILE - 1, TILE + 1, 4099]
    tg = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    ests, idx = [], []
    for i, x in enumerate(tg):
        for k in range(3 if lens[i] == 4099 else 1):
            d = min(k + 1, len(x))
            ests.append(0.7 * np.concatenate([np.zeros(d), x[:len(x) - d].astype(np.float64)]) + 0.01 * (k + 1) * rng.standard_normal(len(x)))
            idx.append(i)
    out, filt = run_emu(emu, tg, ests, idx, L)
    check_rows(out, tg, ests, idx, L, "shapes")
    assert np.isnan(out[0]).all() and np.all(filt[0] == 0.0)
    # a pair gives the bits it has in the batch alone, and without the filter output
    for e in (2, 6, 7, len(ests) - 2):
        alone, fa = run_emu(emu, [tg[idx[e]]], [ests[e]], [0], L)
        assert alone.tobytes() == out[e:e + 1].tobytes() and fa.tobytes() == filt[e:e + 1].tobytes(), e
    assert run_emu(emu, tg, ests, idx, L, filt=False)[0].tobytes() == out.tobytes()
    # ... and at another position, among other pairs
    order = list(range(len(ests)))[::-1]
    back, _ = run_emu(emu, tg, [ests[e] for e in order], [idx[e] for e in order], L)
    assert back[::-1].tobytes() == out.tobytes()


def test_emulated_five_samples_against_512_taps(emu):
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal(5), rng.standard_normal(5)
    out, filt = run_emu(emu, [x], [y], [0], 512)
    sdr, lag, c = O.bss_sdr(x, y, 512)
    print(out, sdr, lag)
    assert abs(out[0, 0] - sdr) < TOL_DB and out[0, 1] == lag and np.isfinite(filt).all()
    assert abs(sdr - (-0.7360544)) < 1e-6 and lag == 0.0          # the oracle's own value on this seed, pinned


def test_emulated_exact_facts(emu):
    rng = np.random.default_rng(7)
    x = (0.1 * rng.standard_normal(4099)).astype(np.float32)
    # y == x: the EPS ceiling, lag 0, the filter a unit impulse
    for y in (x, x.astype(np.float64)):
        out, filt = run_emu(emu, [x], [y], [0], 512)
        sxx = float(np.sum(x.astype(np.float64) ** 2))
        assert abs(out[0, 0] - 10.0 * np.log10((sxx + O.EPS) / O.EPS)) < TOL_DB and out[0, 1] == 0.0, out
        assert filt[0, 0] == 1.0 and np.all(filt[0, 1:] == 0.0)
    # an exact FIR image of the target
    for L in (2, 64, 512):
        xf, yf, h = exact_fir_pair(L)
        out, filt = run_emu(emu, [xf], [yf], [0], L)
        print("exact FIR", L, out, np.max(np.abs(filt[0] - h)))
        assert out[0, 0] >= 120.0, (L, out)
        if L in (2, 64):
            assert np.max(np.abs(filt[0] - h)) <= 1e-10, L
    # n = 0 and an all-zero target: NaN in both columns, the neighbours untouched
    tg = [x, np.zeros(0, np.float32), x[:700], np.zeros(900, np.float32), x[:300]]
    ests = [t + np.float32(0.01) for t in tg]
    out, filt = run_emu(emu, tg, ests, list(range(5)), 64)
    assert np.isnan(out[[1, 3]]).all() and np.isfinite(out[[0, 2, 4]]).all() and np.all(filt[[1, 3]] == 0.0)
    for e in (0, 2, 4):
        assert run_emu(emu, [tg[e]], [ests[e]], [0], 64)[0].tobytes() == out[e:e + 1].tobytes()
    check_rows(out, tg, ests, list(range(5)), 64, "nan neighbours")


def test_emulated_sdr_is_monotone_in_the_tap_count(emu):
    x = targets(n=6000)["lowpass"]
    y = estimates(x)["20dB"] + 0.3 * np.concatenate([np.zeros(11), x[:-11]])
    prev = -np.inf
    for L in (1, 2, 8, 16, 64, 512):
        sdr = run_emu(emu, [x], [y], [0], L)[0][0, 0]
        print(L, sdr)
        assert sdr >= prev - 1e-9, (L, sdr, prev)
        prev = sdr


def test_emulated_tile_geometry(emu):
    res = np.zeros(2, np.int64)
    for n in (0, 1, TILE - 1, TILE, TILE + 1, 60 * 48000):
        emu.bss_geometry(C.c_int64(n), res.ctypes.data_as(C.c_void_p))
        assert res[0] == TILE and res[1] == -(-n // TILE)


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


def _call(lib, tl, idx, taps=512, n_est=None, ws=_DUMMY, ws_bytes=1 << 40, out=_DUMMY, filt=None):
    tl, tp = _i32(tl)
    idx, ip = _i32(idx)
    return lib.ssr_bss_sdr(_DUMMY, 0, _DUMMY, tp, len(tl), _DUMMY, 0, _DUMMY, ip, len(idx) if n_est is None else n_est, taps, out,
                           filt, ws, ws_bytes, None)


def test_bss_sdr_rejects_bad_arguments_before_launch():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E = _lib.ERR_INVALID_ARG
    for taps in (0, 513, -1):
        assert _call(lib, [4000], [0], taps=taps) == E and "taps" in err()
    assert _call(lib, [4000, 5000], [2]) == E and "tgt_index" in err()
    assert _call(lib, [4000, 5000], [0, -1]) == E and "tgt_index" in err()
    assert _call(lib, [-3], [0]) == E and "lengths" in err()
    assert _call(lib, [1 << 29], [0]) == E and "lengths" in err()
    assert _call(lib, [4000], [0], out=None) == E and "null" in err()
    tl, tp = _i32([4000, 40000])
    idx, ip = _i32([1, 1, 0])
    need = lib.ssr_bss_sdr_workspace_bytes(tp, 2, ip, 3, 512)
    assert need > lib.ssr_bss_sdr_workspace_bytes(tp, 2, ip, 3, 64) > 0
    idx2, ip2 = _i32([1, 0, 1])                      # no run of two: the target's autocorrelation rows twice
    assert lib.ssr_bss_sdr_workspace_bytes(tp, 2, ip2, 3, 512) > need
    assert _call(lib, [4000, 40000], [1, 1, 0], ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in err()
    assert _call(lib, [4000, 40000], [1, 1, 0], ws=None) == _lib.ERR_WORKSPACE
    bad, bp = _i32([2])
    assert lib.ssr_bss_sdr_workspace_bytes(tp, 2, bp, 1, 512) == 0
    assert lib.ssr_bss_sdr_workspace_bytes(tp, 2, ip, 3, 0) == 0 and lib.ssr_bss_sdr_workspace_bytes(tp, 2, ip, 3, 513) == 0
    neg, np_ = _i32([4000, -1])
    assert lib.ssr_bss_sdr_workspace_bytes(np_, 2, ip, 3, 512) == 0
    assert _call(lib, [4000], [], n_est=0, ws=None, ws_bytes=0, out=None) == 0     # nothing to score: nothing queued


def test_header_ctypes_table_and_library_agree():
    from ssr_eval_amd import _lib
    inc = os.path.join(ROOT, "include")
    assert os.listdir(inc) == ["ssr_hip.h"]                         # one header: the family has none of its own
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "ssr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ssr_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load()
    for name in ("ssr_bss_sdr", "ssr_bss_sdr_workspace_bytes"):
        assert name in declared and name in _lib.SIGNATURES, name
        assert hasattr(lib, name) and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert "#define SSR_BSS_MAX_TAPS 512" in header and _lib.BSS_MAX_TAPS == 512
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T ssr_bss_sdr\n" in exported and " T ssr_bss_sdr_workspace_bytes\n" in exported


# ---- AudioMetrics / SSR_Eval_Helper options --------------------------------------------------------------------------------------
def test_audio_metrics_bss_options():
    from ssr_eval_amd import AudioMetrics
    from ssr_eval_amd import backend as B
    am = AudioMetrics(48000)
    assert B.BSS_TAPS == 512 and B.check_bss_taps(np.int64(64)) == 64
    x = np.zeros(100, np.float32)
    for bad in (0, 513, -1, 64.0, True, None, "512", (512,)):
        with pytest.raises(ValueError):
            B.check_bss_taps(bad)
        with pytest.raises(ValueError):
            am.bss_sdr(x, x, taps=bad)
        with pytest.raises(ValueError):
            am.bss_sdr_batch([x], [x], bad)
        with pytest.raises(ValueError):
            am.bss_sdr_multi([[x]], [x], bad)
    call, dicts = am._bss_family(8, True)
    got = dicts((np.array([[1.5, 3.0]]), np.arange(8.0)[None]))
    assert list(got[0]) == ["sdr", "sdr_lag", "filter"] and got[0]["sdr"] == 1.5 and got[0]["sdr_lag"] == 3.0
    assert am._bss_family(8, False)[1]((np.array([[1.5, 3.0]]), None)) == [{"sdr": 1.5, "sdr_lag": 3.0}]


def test_helper_bss_option_and_metric_order():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd import eval as E
    mk = lambda **kw: SSR_Eval_Helper(BasicTestee(), 44100, 44100, test_data_root=None, **kw)      # noqa: E731
    assert mk().bss_sdr is None and mk(bss_sdr=None).bss_sdr is None
    for ok in (True, {"taps": 512}, {"taps": 1}, {"taps": np.int32(64)}):
        assert mk(bss_sdr=ok).bss_sdr == ok
    for bad in (False, 1, 512, "all", (), {}, {"taps": 0}, {"taps": 513}, {"taps": 64.0}, {"taps": True}, {"taps": None},
                {"which": "all"}, {"taps": 64, "which": "sdr"}, ("sdr",), [512]):
        with pytest.raises(ValueError):
            mk(bss_sdr=bad)
    # the one registry in queue order, and the one order a result is listed in: this family and its keys close both
    assert E._BSS_KEYS == ("sdr", "sdr_lag")
    assert [f[0] for f in E._FAMILIES] == ["lsd_split", "stoi", "waveform", "mel", "mel_dtw", "quality", "pitch", "phase", "mrstft", "bss_sdr"]
    order = E.result_key_order()
    assert order == ("lsd", "log_sispec", "sispec", "ssim", "lsd_lf", "lsd_hf", "stoi", "estoi", "snr", "si_sdr", "seg_snr", "mel_lsd",
                     "mel_l1", "mcd", "mcd_dtw", "dtw_dev", "llr", "cep_dist", "wss", "fwseg_snr", "f0_rmse", "f0_corr", "gpe", "vde",
                     "ffe", "phase_ip", "phase_gd", "phase_iaf", "mrstft_sc", "mrstft_mag", "mrstft", "sdr", "sdr_lag")
    assert len(order) == 33 and len(set(order)) == len(order)
    assert order == E._METRIC_KEYS[:4] + tuple(k for f in E._FAMILIES for k in f.keys)      # every row's keys, in row order
    args = E._FAMILIES[-1].arguments
    assert args(mk(bss_sdr=True), ["k"]) == ((512,), {}) and args(mk(bss_sdr={"taps": 64}), ["k"]) == ((64,), {})


def test_compare_results_pairs_the_new_columns():
    """The host half of compare_results (_paired_tables; the bootstrap behind it runs on the GPU: tests/test_gpu_bss.py): two results
    that carry sdr / sdr_lag per file are matched column for column, the new columns last, one result without them drops them."""
    from ssr_eval_amd.stats import _paired_tables

    def result(shift, with_bss=True):
        r = {}
        for s, spk in enumerate(("p360", "p361")):
            r[spk] = {}
            for f in range(2):
                d = {"lsd": 1.0 + s + f, "snr": 3.0 * f}
                if with_bss:
                    d.update({"sdr": 20.0 + s + 0.5 * f + shift, "sdr_lag": 37.0})
                r[spk]["f%d.wav" % f] = {"proc_fft_8000_44100": d}
        r["averaged"] = {}
        return r
    ta, tb, speakers, columns = _paired_tables(result(0.0), result(-2.0))
    assert columns == [("proc_fft_8000_44100", m) for m in ("lsd", "snr", "sdr", "sdr_lag")] and speakers == ["p360"] * 2 + ["p361"] * 2
    assert ta.shape == (4, 4) and np.all(ta[:, 2] - tb[:, 2] == 2.0) and np.all(ta[:, 3] == 37.0) and np.all((ta - tb)[:, [0, 1, 3]] == 0.0)
    assert _paired_tables(result(0.0), result(0.0, False))[3] == [("proc_fft_8000_44100", m) for m in ("lsd", "snr")]
