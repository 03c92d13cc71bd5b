"""CPU tests of the delay stage: the float64 oracle (tests/align_oracle.py) against np.correlate, a g++ build of
the kernel bodies (ssr_align.h) against the oracle - lengths around a tile, lag counts around a lag block, both signs of delay, both
dtypes, unequal lengths, the degenerate pairs, the bit-level properties -, the C ABI's argument checks (they return before anything
touches a device), the header / ctypes table / library agreement, the option checks of SSR_Eval_Helper(align=...) and the registry
facts that stay as they were.

Bars (the issue's): c within 1e-10 sqrt(Ex Ey) of the oracle; d* and edge equal where the oracle's peak leads its runner-up by more
than 2e-10 sqrt(Ex Ey); frac within 1e-8 where the oracle's denominator is at least 1e-3 c[d*]; corr within 1e-10; the integer-mode
output bit-identical to slicing; the fractional-mode output within 1e-12 max|y| (float64) or one float32 ulp of max|y| (float32)."""
import ctypes as C
import glob
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import align_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 16384


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def test_oracle_sums_are_np_correlate_and_the_tie_rule():
    x, y = O.noise(301, 1), O.noise(257, 2)
    L = 40
    full = np.correlate(y, x, "full")                        # lag d at index d + len(x) - 1
    c = O.xcorr(x, y, L)
    assert np.max(np.abs(c - full[len(x) - 1 - L:len(x) + L])) <= 1e-12 * np.sqrt(np.dot(x, x) * np.dot(y, y))
    assert np.all(O.xcorr(x[:3], y[:2], 5)[[0, 1, 9, 10]] == 0.0)      # lags without a term
    assert O.scan_order(3) == [0, 1, -1, 2, -2, 3, -3]
    flat = np.ones(7)
    assert O.peak(flat, 3)[0] == 0
    two = np.zeros(7); two[3 + 2] = two[3 - 2] = 5.0
    assert O.peak(two, 3)[0] == 2                                     # equal values: the non-negative lag
    two[3 - 1] = 5.0
    assert O.peak(two, 3)[0] == -1                                    # ... after the smallest |d|
    h = O.taps(0.3)
    assert len(h) == 33 and abs(h.sum() - 1.0) < 1e-15 and np.argmax(np.abs(h)) == 16
    # the taps delay a slow sine by delta: z[t] = y[t + delta]
    t = np.arange(400.0)
    z = O.shift(np.sin(0.05 * t), 0, 0.3)
    assert np.max(np.abs(z[40:-40] - np.sin(0.05 * (t[40:-40] + 0.3)))) < 1e-4
    y32 = O.noise(50, 3).astype(np.float32)
    assert O.shift(y32, 3).dtype == np.float32 and np.array_equal(O.shift(y32, 3)[:47], y32[3:]) and np.all(O.shift(y32, 3)[47:] == 0)
    assert np.array_equal(O.shift(y32, -3)[3:], y32[:47]) and np.all(O.shift(y32, 60) == 0) and np.array_equal(O.delayed(y32, 3)[3:], y32[:47])
    r = O.estimate(np.zeros(10), y32[:10], 4)
    smooth = O.lowpassed(500, 4)                              # its autocorrelation is positive up to lag 8
    assert r["degenerate"] and r["delay"] == 0 and np.isnan(r["corr"]) and O.estimate(smooth, -smooth, 4)["degenerate"]
    assert O.estimate(y32[:0], y32, 4)["degenerate"]


# ---- the kernel bodies compiled for the host ------------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "align_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libalign_emu.so")


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    lib = C.CDLL(EMU_SO)
    lib.align_emu.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def run_emu(lib, tgts, ests, idx, L, subsample=False, gaps=(0,)):
    """-> (rows [n_est, 4], the shifted estimates, c [n_est, 2 L + 1], taps [n_est, 33]).  gaps: poisoned elements in front of each
    signal and output (cycled), so that the 16-byte paths meet every alignment."""
    P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    tdt, edt = tgts[0].dtype, ests[0].dtype

    def pack(sigs, dt):
        off, pos = [], 0
        for i, s in enumerate(sigs):
            pos += gaps[i % len(gaps)]
            off.append(pos); pos += len(s)
        buf = np.full(pos + 8, np.nan, dt)
        for o, s in zip(off, sigs):
            buf[o:o + len(s)] = s
        return buf, np.array(off, np.int64), np.array([len(s) for s in sigs], np.int32)
    td, to, tl = pack(tgts, tdt)
    ed, eo, el = pack(ests, edt)
    idx = np.ascontiguousarray(idx, np.int32)
    rows = np.full((len(ests), 4), -123.0)
    sh = np.full(len(ed), np.nan, edt)
    c = np.full((len(ests), 2 * L + 1), np.nan)
    tp = np.full((len(ests), 33), np.nan)
    rc = lib.align_emu(P(td), int(tdt == np.float64), P(to), P(tl), len(tgts), P(ed), int(edt == np.float64), P(eo), P(el), P(idx), len(ests),
                       L, int(subsample), P(rows), P(sh), P(eo), P(c), P(tp))
    assert rc == 0, rc
    inside = np.zeros(len(sh), bool)
    for o, n in zip(eo, el):
        inside[o:o + n] = True
    assert np.isnan(sh[~inside]).all() and not np.isnan(sh[inside]).any()        # every output sample written, nothing else
    return rows, [sh[o:o + n] for o, n in zip(eo, el)], c, tp


def check_pair(x, y, L, row, z, c, subsample, exempt_ok=False):
    """One pair against the oracle at the issue's bars; -> True where d* was compared (the oracle's margin qualifies)."""
    zo, r = O.align(x, y, L, subsample)
    s = r["scale"]
    assert np.max(np.abs(c - r["c"])) <= 1e-10 * s, ("c", np.max(np.abs(c - r["c"])), s)
    qualifies = r["degenerate"] or r["margin"] > 2e-10 * s
    assert qualifies or exempt_ok
    if not qualifies:
        return False
    assert (row[0], row[3]) == (r["delay"], r["edge"]), (row, r["delay"], r["edge"])
    if r["degenerate"]:
        assert np.isnan(row[2]) and row[1] == 0.0 and np.array_equal(z, y)
        return True
    assert abs(row[2] - r["corr"]) <= 1e-10
    if not r["edge"]:
        assert abs(r["den"]) >= 1e-3 * r["c"][r["delay"] + L], "the input does not qualify for the parabola's bar"
        assert abs(row[1] - r["frac"]) <= 1e-8
    # the shift is judged with the frac the kernel reported (it met its own bar above): frac == 0 exactly is the copy's path, and
    # where the oracle's parabola gives 0 the kernel's may give 1e-16
    if not subsample or row[1] == 0.0:
        assert z.dtype == y.dtype and z.tobytes() == O.shift(y, r["delay"]).tobytes()
    else:
        zo = O.shift(y, r["delay"], row[1])
        peak = np.max(np.abs(y)).astype(np.float64)
        bar = 1e-12 * peak if y.dtype == np.float64 else float(np.spacing(np.float32(peak)))
        assert np.max(np.abs(z.astype(np.float64) - zo.astype(np.float64))) <= bar
    return True


LENGTHS = [(7, 8, 1), (64, 9, -3), (1023, 1024, 37), (1025, 1024, -37), (TILE - 1, 64, 37), (TILE, 64, -63), (TILE + 1, 64, 64),
           (40000, 64, -64), (20000, 2047, 2046), (20000, 2049, -2048), (9000, 4096, 4095), (9000, 4096, -4096), (30000, 1024, 1029),
           (5000, 1, 0), (5000, 1, 1), (5000, 1, -1), (5000, 8, 0), (1, 1, 0)]


@pytest.mark.parametrize("n,L,d", LENGTHS, ids=["n%d-L%d-d%d" % c for c in LENGTHS])
def test_emulated_kernels_match_the_oracle(emu, n, L, d):
    for k, dt in enumerate((np.float32, np.float64)):
        x = O.lowpassed(n, 10 * n + L + k).astype(dt)
        y = O.delayed(x, d)
        for sub in (False, True):
            rows, sh, c, _ = run_emu(emu, [x], [y], [0], L, sub, gaps=(k + 1,))
            assert check_pair(x, y, L, rows[0], sh[0], c[0], sub)
            if abs(d) < L and n > 4 * abs(d) + 100:
                assert rows[0][0] == d and rows[0][2] > 0.9


def test_emulated_unequal_lengths_shared_target_and_mixed_dtypes(emu):
    x = O.lowpassed(TILE + 700, 5)
    # three estimates with different delays name one target; shorter and longer than it, in both dtypes
    for tdt, edt in ((np.float32, np.float64), (np.float64, np.float32)):
        tg = [x.astype(tdt), O.lowpassed(3000, 6).astype(tdt)]
        es = [O.delayed(tg[0], 5, TILE + 100).astype(edt), O.delayed(tg[0], -200, TILE + 2000).astype(edt),
              O.delayed(tg[0], 333).astype(edt), O.delayed(tg[1], 40, 2500).astype(edt), O.delayed(tg[1], -41, 6000).astype(edt)]
        idx = [0, 0, 0, 1, 1]
        for sub in (False, True):
            rows, sh, c, _ = run_emu(emu, tg, es, idx, 512, sub, gaps=(1, 2, 3, 4))
            assert list(rows[:, 0]) == [5, -200, 333, 40, -41]
            for e in range(5):
                assert check_pair(tg[idx[e]], es[e], 512, rows[e], sh[e], c[e], sub)
            # a pair alone gives the bits of its row in the batch
            for e in (1, 4):
                r1, s1, c1, _ = run_emu(emu, [tg[idx[e]]], [es[e]], [0], 512, sub)
                assert r1[0].tobytes() == rows[e].tobytes() and s1[0].tobytes() == sh[e].tobytes() and c1[0].tobytes() == c[e].tobytes()


def test_emulated_degenerate_pairs_and_taps(emu):
    x = O.lowpassed(3000, 9).astype(np.float32)
    zero = np.zeros(3000, np.float32)
    # (lag 4: the autocorrelation of the low-passed noise is positive that far, so y = -x has no positive c)
    rows, sh, c, tp = run_emu(emu, [x, zero, x[:0]], [zero, x, -x, x, x[:0]], [0, 1, 0, 2, 0], 4, True)
    for e in range(5):
        assert rows[e][0] == 0 and rows[e][1] == 0 and np.isnan(rows[e][2]) and rows[e][3] == 0
        assert np.array_equal(tp[e], np.eye(33)[16])
    assert np.array_equal(sh[1], x) and np.array_equal(sh[2], -x) and np.array_equal(sh[3], x) and np.all(c[3] == 0)
    # the taps of a real fractional delay are the oracle's
    y = np.convolve(O.delayed(x, 7), [0.5, 0.5])[:3000].astype(np.float32)
    rows, sh, c, tp = run_emu(emu, [x], [y], [0], 16, True)
    assert rows[0][0] in (7, 8) and rows[0][1] != 0 and np.max(np.abs(tp[0] - O.taps(rows[0][1]))) < 1e-15


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


def _call(lib, tl, el, idx, L=64, n_est=None, ws=_DUMMY, ws_bytes=1 << 40, rows=_DUMMY, shifted=_DUMMY, shifted_off=_DUMMY, est_len=True):
    tl, tp = _i32(tl)
    el, ep = _i32(el)
    idx, ip = _i32(idx)
    return lib.ssr_align(_DUMMY, 0, _DUMMY, tp, len(tl), _DUMMY, 0, _DUMMY, ep if est_len else None, ip, len(idx) if n_est is None else n_est, L, 0,
                         rows, shifted, shifted_off, None, ws, ws_bytes, None)


def test_align_rejects_bad_arguments_before_launch():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E = _lib.ERR_INVALID_ARG
    for L in (0, -1, 4097, 1 << 20):
        assert _call(lib, [4000], [4000], [0], L=L) == E and "max_lag" in err()
    assert _call(lib, [4000, 5000], [4000], [2]) == E and "tgt_index" in err()
    assert _call(lib, [4000, 5000], [4000, 1], [0, -1]) == E and "tgt_index" in err()
    assert _call(lib, [-3], [10], [0]) == E and "lengths" in err()
    assert _call(lib, [1 << 29], [10], [0]) == E and "lengths" in err()
    assert _call(lib, [10], [-1], [0]) == E and "lengths" in err()
    assert _call(lib, [10], [1 << 29], [0]) == E and "lengths" in err()
    assert _call(lib, [10], [10], [0], est_len=False) == E and "null" in err()
    assert _call(lib, [10], [10], [0], rows=None) == E and "null" in err()
    assert _call(lib, [10], [10], [0], shifted_off=None) == E and "null" in err()
    tl, tp = _i32([4000, 40000])
    el, ep = _i32([3000, 41000, 4000])
    idx, ip = _i32([1, 1, 0])
    need = lib.ssr_align_workspace_bytes(tp, 2, ep, ip, 3, 64)
    assert need > 0
    # one row of 2 L + 1 doubles per tile of 16384 target samples of every pair: 3 + 3 + 1 tiles
    more = lib.ssr_align_workspace_bytes(tp, 2, ep, ip, 3, 65) - need
    assert abs(more - 7 * 2 * 8) <= 256
    assert _call(lib, [4000, 40000], [3000, 41000, 4000], [1, 1, 0], ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in err()
    assert _call(lib, [4000, 40000], [3000, 41000, 4000], [1, 1, 0], ws=None) == _lib.ERR_WORKSPACE
    bad, bp = _i32([2, 0, 0])
    assert lib.ssr_align_workspace_bytes(tp, 2, ep, bp, 3, 64) == 0
    assert lib.ssr_align_workspace_bytes(tp, 2, ep, ip, 3, 0) == 0 and lib.ssr_align_workspace_bytes(tp, 2, ep, ip, 3, 4097) == 0
    assert lib.ssr_align_workspace_bytes(tp, 2, None, ip, 3, 64) == 0
    # one workgroup of 256 threads per (tile, block of 2048 lags), four blocks at 4096: 2^32 threads are refused before anything is queued
    assert _call(lib, [(1 << 29) - 1], [10] * 140, [0] * 140, L=4096, ws_bytes=1 << 62) == _lib.ERR_UNSUPPORTED and "too large" in err()
    assert _call(lib, [(1 << 29) - 1], [10] * 100, [0] * 100, L=4096, ws_bytes=1 << 30) == _lib.ERR_WORKSPACE
    assert _call(lib, [4000], [], [], n_est=0, ws=None, ws_bytes=0, rows=None, shifted=None, shifted_off=None) == 0      # nothing queued


def test_header_ctypes_table_and_library_agree():
    from ssr_eval_amd import _lib
    path = os.path.join(ROOT, "ssr_eval_amd", "csrc", "ssr_hip_align.h")
    header = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    declared = set(re.findall(r"\b(ssr_[a-z_0-9]+)\s*\(", header))
    assert declared == {"ssr_align", "ssr_align_workspace_bytes"} == set(_lib.ALIGN_SIGNATURES)
    others = set(_lib.SIGNATURES) | set(_lib.COHERENCE_SIGNATURES) | set(_lib.LOUDNESS_SIGNATURES) | set(_lib.SPECTRUM_SIGNATURES) | \
        set(_lib.AUDITORY_SIGNATURES) | set(_lib.MODULATION_SIGNATURES) | set(_lib.DISTRIBUTION_SIGNATURES) | set(_lib.CSII_SIGNATURES)
    assert not set(_lib.ALIGN_SIGNATURES) & others
    assert "#define SSR_ALIGN_MAX_LAG 4096" in header and "#define SSR_ALIGN_COLUMNS 4" in header and (_lib.ALIGN_MAX_LAG, _lib.ALIGN_COLUMNS) == (4096, 4)
    for name, n in (("ssr_align", 20), ("ssr_align_workspace_bytes", 6)):
        n_args = len(re.search(r"\b%s\((.*?)\);" % name, header, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.ALIGN_SIGNATURES[name][1]) == n, name
    lib = _lib.load()
    for name, (res, args) in _lib.ALIGN_SIGNATURES.items():
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    main = open(os.path.join(ROOT, "include", "ssr_hip.h")).read()
    assert main.count("#include \"../ssr_eval_amd/csrc/ssr_hip_align.h\"") == 1
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T ssr_align\n" in exported and " T ssr_align_workspace_bytes\n" in exported
    # the header is C99 on its own behind the main one
    src = "#include \"%s\"\nint main(void) { return ssr_align_workspace_bytes(0, 0, 0, 0, 0, 64) != 0 || SSR_ALIGN_MAX_LAG != 4096; }\n" % \
        os.path.join(ROOT, "include", "ssr_hip.h")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-"], input=src, text=True, check=True)


# ---- AudioMetrics / SSR_Eval_Helper options --------------------------------------------------------------------------------------
def test_backend_and_audio_metrics_align_options():
    """Everything here is refused before any device is touched (this test runs without one)."""
    from ssr_eval_amd import AudioMetrics, backend as bk
    assert bk.check_align_lag(1) == 1 and bk.check_align_lag(np.int64(4096)) == 4096 and bk.ALIGN_LAG == 1024
    x = np.zeros(3000, np.float32)
    for bad in (0, 4097, -5, 64.0, True, None, "64"):
        with pytest.raises(ValueError, match="max_lag must be an integer"):
            bk.align([x], [x], [0], max_lag=bad)
        with pytest.raises(ValueError, match="max_lag must be an integer"):
            AudioMetrics(16000).align(x, x, max_lag=bad)
        with pytest.raises(ValueError, match="max_lag must be an integer"):
            AudioMetrics(16000).delay(x, x, max_lag=bad)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="subsample must be True or False"):
            bk.align([x], [x], [0], subsample=bad)
        with pytest.raises(ValueError, match="subsample must be True or False"):
            AudioMetrics(16000).align_batch([x], [x], subsample=bad)
        with pytest.raises(ValueError, match="subsample must be True or False"):
            AudioMetrics(16000).align_multi([[x]], [x], subsample=bad)
    with pytest.raises(ValueError, match="return_corr"):
        bk.align([x], [x], [0], return_corr=1)
    with pytest.raises(ValueError, match="tgt_index out of range"):
        bk.align([x], [x], [1])
    with pytest.raises(ValueError, match="one target index per estimate"):
        bk.align([x], [x], [0, 0])
    with pytest.raises(ValueError, match="1-D"):
        AudioMetrics(16000).align(np.zeros((2, 30), np.float32), x)


def test_helper_align_option_and_registry_facts():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd import eval as E
    mk = lambda **kw: SSR_Eval_Helper(BasicTestee(), 16000, 16000, evaluation_sr=16000, test_data_root=None, **kw)      # noqa: E731
    assert mk().align is None and mk()._align is None and mk(align=None)._align is None
    assert mk(align=True)._align == (1024, False) and mk(align={"max_lag": 37})._align == (37, False)
    assert mk(align={"subsample": True})._align == (1024, True) and mk(align={"max_lag": 4096, "subsample": False})._align == (4096, False)
    for bad in (False, 1, "all", (), {}, [True], {"lag": 3}, {"max_lag": 64, "taps": 3}):
        with pytest.raises(ValueError, match="align must be None, True or a dict"):
            mk(align=bad)
    for bad in ({"max_lag": 0}, {"max_lag": 4097}, {"max_lag": 64.0}, {"max_lag": None}, {"max_lag": True}):
        with pytest.raises(ValueError, match="max_lag must be an integer"):
            mk(align=bad)
    for bad in ({"subsample": 1}, {"subsample": None}, {"subsample": "yes"}):
        with pytest.raises(ValueError, match="subsample must be True or False"):
            mk(align=bad)
    # the option is checked before the caller's settings are touched
    setting = {"cutoff_freq": [1000, 2000]}
    with pytest.raises(ValueError):
        mk(align={"max_lag": 0}, setting_fft=setting)
    assert setting == {"cutoff_freq": [1000, 2000]}
    assert inspect.signature(SSR_Eval_Helper.__init__).parameters["align"].kind is inspect.Parameter.KEYWORD_ONLY
    # the stage is no registry family: with it in the build the registries are what they were
    assert len(E._ALL_FAMILIES) == 16 and len(E.every_key_order()) == 56 and "align" not in [f.option for f in E._ALL_FAMILIES]
    assert E.ALIGN_KEYS == ("delay", "align_corr") and not set(E.ALIGN_KEYS) & set(E.every_key_order())


# ---- the GPU test's geometry batches on the emulated kernels: the same inputs, the same bars --------------------------------------
@pytest.mark.parametrize("L", O.LAGS)
def test_emulated_geometry_batches(emu, L):
    dt = (np.float32, np.float64)[O.LAGS.index(L) % 2]
    tgts, ests, idx = O.geometry_batch(L, dt, dt)
    assert len(ests) == 2 * len(tgts) and {len(e) for e in ests} - {len(t) for t in tgts}
    for sub in (False, True):
        rows, sh, c, _ = run_emu(emu, tgts, ests, idx, L, sub, gaps=(1, 2, 3, 4))
        compared = sum(check_pair(tgts[idx[e]], ests[e], L, rows[e], sh[e], c[e], sub) for e in range(len(ests)))
        assert compared == len(ests)                      # no pair is exempt: every peak leads its runner-up by the margin
        assert {int(r[3]) for r in rows} == {0, 1}          # edges among them
