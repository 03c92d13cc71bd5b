"""CPU tests of the coherence speech intelligibility index (csii, csii_low, csii_mid, csii_high, i3 and the values above a split;
DESIGN.md section 26): the float64 oracle (tests/csii_oracle.py) against the coherence oracle and the closed form of its weights, a
g++ build of the kernel bodies (ssr_csii.h) against the oracle - rates, transform sizes, the shapes where the geometry can go wrong,
the exact facts, the bit-level properties -, the C ABI's argument checks (they return before anything touches a device), the header /
ctypes table / library agreement, and AudioMetrics / SSR_Eval_Helper(csii=...) validation and key order.

Tolerances: the CSII values and the values above a split within 1e-7 - section 20's coh_sdr bar of 1e-6 dB over the 30 dB per unit of
a band value is 3.4e-8, the importance weights sum to 1, the bar is three times that; i3 within 3e-7 - the logistic's slope is at most
0.25, times 9.99 + 1.84; the segment counts equal.  Counts can only be equal where no segment level lies on a class threshold: every
compared target is asserted, with the oracle alone, to have every level at least 1e-6 dB from 0, -10 and -30 dB
(csii_oracle.check_rows); a target of exactly one segment's length has its one level at 0 dB by definition - every value is NaN
there and its counts must be one segment in all, none low, one in mid or in high.  Worst differences seen in emulation: CSII 4.4e-16, i3 1.1e-16, a band value
3.0e-15 (on an MI355X: 4.4e-16, 2.2e-16, 2.2e-15)."""
import ctypes as C
import glob
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import coherence_oracle as CO
import csii_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FR = O.FR
DTYPES = [(np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64), (np.float64, np.float64)]
DTYPE_IDS = ["f32-f32", "f64-f32", "f32-f64", "f64-f64"]


def B():
    from ssr_eval_amd import backend
    return backend


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def test_oracle_design_bands_weights_and_default_nfft():
    assert len(O.CENTRES) == len(O.IMPORTANCE) == 21 and abs(sum(O.IMPORTANCE) - 1.0) < 1e-12
    assert [O.default_nfft(fs) for fs in (8000, 16000, 22050, 44100, 48000, 96000, 192000)] == [256, 256, 512, 1024, 1024, 2048, 2048]
    for fs, n_bands in ((8000, 17), (16000, 20), (44100, 21), (48000, 21)):
        N = O.default_nfft(fs)
        fc, imp, W = O.design(fs, N)
        assert len(fc) == n_bands and W.shape == (n_bands, N // 2 + 1) and abs(imp.sum() - 1.0) < 1e-15 and np.all(W[:, 0] == 0.0)
        assert np.all(W >= 0.0) and np.all(W <= 1.0)
        # the closed form at f_c, where W = 1: a rate and a size that put a bin on every centre that is a multiple of fs / N
        for j, f in enumerate(fc):
            k = f * N / fs
            if k == int(k):
                assert W[j, int(k)] == 1.0
    fc, _, W = O.design(16000, 2048)                           # bins every 7.8125 Hz: 250, 1000, 2500 ... lie on a bin
    on = [j for j, f in enumerate(fc) if (f * 2048 / 16000) == int(f * 2048 / 16000)]
    assert len(on) >= 5 and all(W[j, int(fc[j] * 2048 / 16000)] == 1.0 for j in on)
    fc, imp, W = O.design(48000, 1024, (1000, 4000))
    assert list(fc) == [1000., 1170., 1370., 1600., 1850., 2150., 2500., 2900., 3400., 4000.] and abs(imp.sum() - 1.0) < 1e-15
    # the backend's vectorised design is the oracle's loop
    for fs, N, band in ((8000, 256, None), (16000, 512, None), (44100, 1024, (300, 9000)), (48000, 2048, None)):
        fo, io, Wo = O.design(fs, N, band)
        fb, ib, Wb = B().csii_design(fs, N, band)
        assert np.array_equal(fo, fb) and np.max(np.abs(io - ib)) <= 1e-16 and np.max(np.abs(Wo - Wb)) <= 1e-15


@pytest.mark.parametrize("case", range(len(CO.CASES)))
def test_oracle_all_set_spectra_are_the_coherence_oracles(case):
    n, N, H = CO.CASES[case]
    x, y = CO.input_pair(n, 100 + case)
    sxx, syy, sxy, cnt = O.set_spectra(x, y, N, H)
    wxx, wyy, wxy = CO.auto_cross(x, y, N, H)
    scale = np.max(wxx) + np.max(wyy)
    assert cnt[0] == CO.segments(n, N, H) and cnt[1:].sum() <= cnt[0]
    assert max(np.max(np.abs(sxx[0] - wxx)), np.max(np.abs(syy[0] - wyy)), np.max(np.abs(sxy[0] - wxy))) <= 1e-12 * scale
    # the class sets partition what they hold
    assert np.max(np.abs(sxx[1:].sum(0) - wxx)) <= 1e-12 * scale or cnt[1:].sum() < cnt[0]


def test_oracle_levels_classes_nan_cases_and_meaning():
    fs, N, H = 16000, 256, 128
    x = O.speech_like(24000, fs, 1)
    L, c = O.levels(x, N, H), O.classes(x, N, H)
    assert len(L) == CO.segments(len(x), N, H) == len(c)
    assert all(np.all(c[(L >= lo) & (L < hi)] == k) for lo, hi, k in ((0, np.inf, 3), (-10, 0, 2), (-30, -10, 1), (-np.inf, -30, 0)))
    assert min(np.sum(c == k) for k in (0, 1, 2, 3)) >= 2 and O.level_margin(x, N, H) >= O.LEVEL_MARGIN
    z = np.zeros(4000)
    assert np.all(O.classes(z, N, H) == -1) and np.isnan(O.csii(z, x[:4000], fs)[0]).all()
    v, cnt, T = O.csii(x[:4000], z, fs)                                            # a silent estimate: incoherent, not NaN
    assert v[0] == 0.0 and np.all(T[0] == 0.0)
    for n in (255, 256, 256 + 127):                                                # K = 0 and K = 1
        v, cnt, _ = O.csii(x[:n], x[:n], fs, N, H)
        assert np.isnan(v).all() and cnt[0] == (n >= 256)
    v, cnt, T = O.csii(x, x, fs, N, H, split_hz=4000)
    assert np.all(np.delete(v, 4) == 1.0) and np.all(T == 1.0)                     # y == x: 1 exactly
    assert v[4] == 1.0 / (1.0 + np.exp(-(-3.47 + 1.84 + 9.99)))
    assert np.isnan(O.csii(x, x, fs, N, H)[0][5:]).all() and np.isnan(O.csii(x, x, fs, N, H, split_hz=8000)[0][5:]).all()
    # white noise at 0 dB: the louder the target's segments, the better their local signal-to-noise ratio
    v, cnt, _ = O.csii(x, O.noisy(x, 0.0, 5), fs, N, H)
    print("white noise at 0 dB: csii_high, csii_mid, csii_low", v[3], v[2], v[1])
    assert 1.0 > v[3] > v[2] > v[1] > 0.0
    g, _, _ = O.csii(x, 0.5 * O.noisy(x, 0.0, 5), fs, N, H)
    assert g.tobytes() == v.tobytes()                                              # the estimate's gain changes no bit


# ---- the kernel bodies compiled for the host ------------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "csii_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libcsii_emu.so")


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    lib = C.CDLL(EMU_SO)
    lib.csii_emu.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                             C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def split_bands(fs, n_fft, band, splits, n_est):
    """One split frequency per estimate (None: none) -> the int32 first band of the upper part, -1 for no split."""
    fc = O.design(fs, n_fft, band)[0]
    if splits is None:
        return np.full(n_est, -1, np.int32)
    return np.array([-1 if s is None else int(np.searchsorted(fc, float(s), side="left")) for s in splits], np.int32)


def run_emu(lib, tgts, ests, idx, fs, n_fft, hop, band=None, splits=None, with_bands=True):
    """-> (out [n_est, 13], T [n_est, 4, n_bands] or None, the class row of every target)"""
    tdt, edt = tgts[0].dtype, (ests[0].dtype if ests else tgts[0].dtype)
    P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    tl = np.array([len(t) for t in tgts], np.int32)
    el = np.array([len(e) for e in ests], np.int64)
    to = np.concatenate(([0], np.cumsum(tl)[:-1])).astype(np.int64)
    eo = np.concatenate(([0], np.cumsum(el)[:-1])).astype(np.int64)
    td = np.concatenate(list(tgts) + [np.zeros(1, tdt)])
    ed = np.concatenate(list(ests) + [np.zeros(1, edt)])
    idx = np.ascontiguousarray(idx, np.int32)
    _, imp, W = B().csii_design(fs, n_fft, band)
    sp = split_bands(fs, n_fft, band, splits, len(ests))
    out = np.full((len(ests), 13), -123.0)
    T = np.full((len(ests), 4, len(imp)), -7.0) if with_bands else None
    Ks = [CO.segments(int(n), n_fft, hop) for n in tl]
    cls = np.full(sum(Ks) + 1, 77, np.int8)
    assert lib.csii_emu(P(td), int(tdt == np.float64), P(to), P(tl), len(tgts), P(ed), int(edt == np.float64), P(eo), P(idx), len(ests),
                        n_fft, hop, len(imp), P(W), P(imp), P(sp), P(out), P(T) if with_bands else None, P(cls)) == 0
    assert cls[-1] == 77
    edges = np.concatenate(([0], np.cumsum(Ks)))
    return out, T, [cls[edges[i]:edges[i + 1]].copy() for i in range(len(tgts))]


def _classes_match(rows, tgts, n_fft, hop):
    for t, row in zip(tgts, rows):
        if len(t) == n_fft:              # (one segment as long as the target lies on the 0 dB threshold by definition: mid or high)
            assert row.tolist() in ([2], [3])
        else:
            assert np.array_equal(row, O.classes(t, n_fft, hop))


@pytest.mark.parametrize("fs,n_bands,seconds,seed", [(8000, 17, 2.0, 11), (16000, 20, 1.5, 12), (44100, 21, 1.0, 13), (48000, 21, 1.0, 14)])
def test_emulated_kernels_match_the_oracle_at_every_rate(emu, fs, n_bands, seconds, seed):
    """A synthetic voiced signal with pauses at the four rates, default n_fft and hop: a noisy and a clipped estimate of one target
    (with a third, the target itself), the four dtype mixes, a split at a quarter of the rate; every class holds segments."""
    N = O.default_nfft(fs)
    assert N == B().csii_default_nfft(fs) and len(O.design(fs, N)[0]) == n_bands
    x = O.speech_like(int(seconds * fs), fs, seed)
    ys = [O.noisy(x, 5.0, seed), O.distorted(x, seed), x.copy()]
    for dt in DTYPES:
        tg, es = [x.astype(dt[0])], [y.astype(dt[1]) for y in ys]
        out, T, rows = run_emu(emu, tg, es, [0, 0, 0], fs, N, N // 2, splits=[fs / 8.0, None, fs / 8.0])
        worst = O.check_rows(out, tg, es, [0, 0, 0], fs, N, N // 2, None, [fs / 8.0, None, fs / 8.0], T, what="rate %d" % fs)
        print("fs %d %s-%s: worst CSII %.3g, i3 %.3g, band value %.3g" % ((fs, np.dtype(dt[0]).name, np.dtype(dt[1]).name) + tuple(worst)))
        _classes_match(rows, tg, N, N // 2)
        assert np.all(out[0, 10:] >= 2) and np.isfinite(out[0]).all() and np.isnan(out[1, 5:9]).all()
        assert 0.0 < out[0, 0] < 1.0 and 0.0 < out[0, 4] < 1.0 and out[0, 3] > out[0, 1]
        if dt[0] == dt[1]:
            assert np.all(out[2, :4] == 1.0) and np.all(out[2, 5:9] == 1.0) and np.all(T[2] == 1.0)       # y == x: 1 exactly


def _geometry_batch(dt):
    """N = 256, hop 64 at 16 kHz: n = N - 1 (K = 0), n = N (K = 1), K = 2, 31, 32, 33, 65; the K = 33 target has three estimates."""
    fs, N, H = 16000, 256, 64
    lens = [255, 256] + [CO.len_for_segments(K, N, H, e) for K, e in ((2, 0), (FR - 1, 5), (FR, 63), (FR + 1, 0), (2 * FR + 1, 17))]
    xs = [O.speech_like(n, fs, 40 + i) for i, n in enumerate(lens)]
    tg = [x.astype(dt[0]) for x in xs]
    ests, idx = [], []
    for i, x in enumerate(xs):
        for k in range(3 if i == 5 else 1):
            ests.append(O.noisy(x, 3.0 + 4.0 * k, 50 + i + k).astype(dt[1]))
            idx.append(i)
    return fs, N, H, tg, ests, idx


# one split per estimate of the geometry batch; 7500 Hz and 1e9 Hz lie above the last centre at 16 kHz (7000 Hz): the empty _hf
GEOMETRY_SPLITS = [2000.0, 2500.0, 3000.0, 3500.0, 4000.0, 4500.0, 7500.0, 5500.0, 1e9]


@pytest.mark.parametrize("dt", DTYPES, ids=DTYPE_IDS)
def test_emulated_geometry_shapes_and_bit_level_properties(emu, dt):
    """The ragged geometry batch; then: a pair alone and at another position gives the bits it gives in the batch, a target's class
    row is the same with one and with three estimates, a gain of 0.5 changes no bit, bands_out = NULL changes no bit of out."""
    fs, N, H, tg, ests, idx = _geometry_batch(dt)
    splits = GEOMETRY_SPLITS
    assert split_bands(fs, N, None, splits, len(ests)).tolist() == [12, 13, 15, 16, 16, 17, 20, 18, 20]      # (20 = n_bands: no band above)
    out, T, rows = run_emu(emu, tg, ests, idx, fs, N, H, splits=splits)
    worst = O.check_rows(out, tg, ests, idx, fs, N, H, None, splits, T, what="shapes")
    print("worst CSII %.3g, i3 %.3g, band value %.3g" % tuple(worst))
    _classes_match(rows, tg, N, H)
    assert np.isnan(out[:2, :9]).all() and out[:2, 9].tolist() == [0.0, 1.0] and np.isfinite(out[3:, 0]).all()
    # the empty upper part, next to estimates of the same target and batch that have one: NaN in the four _hf columns only
    assert np.isnan(out[[6, 8], 5:9]).all() and np.isfinite(out[[6, 8], 0]).all() and np.isfinite(out[[5, 7], 5]).all()
    assert out[:, 9].tolist() == [0, 1, 2, FR - 1, FR, FR + 1, FR + 1, FR + 1, 2 * FR + 1]
    for e in (2, 3, 5, 6, len(ests) - 1):
        alone, Ta, ra = run_emu(emu, [tg[idx[e]]], [ests[e]], [0], fs, N, H, splits=[splits[e]])
        assert alone.tobytes() == out[e:e + 1].tobytes() and Ta.tobytes() == T[e:e + 1].tobytes(), e
        assert np.array_equal(ra[0], rows[idx[e]])                                 # one estimate or three: the same class row
    order = list(range(len(ests)))[::-1]
    back, Tb, _ = run_emu(emu, tg, [ests[e] for e in order], [idx[e] for e in order], fs, N, H, splits=[splits[e] for e in order])
    assert back[::-1].tobytes() == out.tobytes() and Tb[::-1].tobytes() == T.tobytes()
    half, Th, _ = run_emu(emu, tg, [(0.5 * e.astype(np.float64)).astype(dt[1]) for e in ests], idx, fs, N, H, splits=splits)
    assert half.tobytes() == out.tobytes() and Th.tobytes() == T.tobytes()
    assert run_emu(emu, tg, ests, idx, fs, N, H, splits=splits, with_bands=False)[0].tobytes() == out.tobytes()
    # a band option and no split at all: the columns that do not depend on them keep their bits
    sub, Ts, _ = run_emu(emu, tg, ests, idx, fs, N, H, band=(500, 5000))
    O.check_rows(sub, tg, ests, idx, fs, N, H, (500, 5000), None, Ts, what="band option")
    assert Ts.shape[2] == 14 and np.isnan(sub[:, 5:9]).all() and sub[:, 9:].tobytes() == out[:, 9:].tobytes()
    none, _, _ = run_emu(emu, tg, ests, idx, fs, N, H)
    assert none[:, :5].tobytes() == out[:, :5].tobytes() and np.isnan(none[:, 5:9]).all()


@pytest.mark.parametrize("fs,n_fft,hop,K", [(48000, 2048, 1024, 3), (44100, 1024, 341, FR + 1), (16000, 512, 512, 4), (16000, 256, 1, FR + 2),
                                            (48000, 2048, 2048, 2), (8000, 512, 77, 2 * FR + 1), (16000, 1024, 1, 3)])
def test_emulated_other_transform_sizes_and_hops(emu, fs, n_fft, hop, K):
    """Every n_fft; hop = 1 on a short signal, N / 2, N and odd values across chunk boundaries - float32 targets with float64
    estimates, next to a pair one sample too short for a segment."""
    n = CO.len_for_segments(K, n_fft, hop, min(3, hop - 1))
    x = O.speech_like(n, fs, 70 + n_fft // 256 + hop)
    tg = [x.astype(np.float32), x[:n_fft - 1].astype(np.float32)]
    ests = [O.noisy(x, 6.0, 3), O.distorted(x)[:n_fft - 1]]
    out, T, rows = run_emu(emu, tg, ests, [0, 1], fs, n_fft, hop, splits=[1500.0, 1500.0])
    worst = O.check_rows(out, tg, ests, [0, 1], fs, n_fft, hop, None, [1500.0, 1500.0], T, what="sizes")
    print("worst CSII %.3g, i3 %.3g, band value %.3g" % tuple(worst))
    _classes_match(rows, tg, n_fft, hop)
    assert np.isnan(out[1, :9]).all() and np.isfinite(out[0, 0]) and out[:, 9].tolist() == [K, 0]


def _stepped(gains_db, N, fs, seed, tail_db=None, tail=0):
    """Segments without overlap (hop = N) at the given levels, and `tail` samples behind the last one that no segment covers."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(len(gains_db) * N + tail)
    for i, g in enumerate(gains_db):
        x[i * N:(i + 1) * N] *= 10.0 ** (g / 20.0)
    if tail:
        x[len(gains_db) * N:] *= 10.0 ** (tail_db / 20.0)
    return 0.1 * x


def test_emulated_class_populations(emu):
    """A class with no segment and a class with one: NaN there and in i3; all segments in one class; every class dropped."""
    fs, N = 16000, 256
    cases = {
        "low empty": ([0, 0, 0, -4, -4, -4, -4, -60, -60], None, 0),
        "low one": ([0, 0, 0, -4, -4, -4, -4, -20, -60], None, 0),
        "mid one": ([0, 0, 0, 0, -5, -25, -25, -25, -25], None, 0),
        "all mid": ([0, 0, 0, 0, 0, 0], 14.0, 200),
        "all low": ([0, 0, 0, 0, 0], 30.0, 255),
        "all dropped": ([0, 0, 0], 50.0, 255),
    }
    for name, (gains, tail_db, tail) in cases.items():
        x = _stepped(gains, N, fs, 80, tail_db, tail)
        y = O.noisy(x, 10.0, 81)
        out, T, rows = run_emu(emu, [x], [y], [0], fs, N, N, splits=[3000.0])
        O.check_rows(out, [x], [y], [0], fs, N, N, None, [3000.0], T, what=name)
        cnt = out[0, 9:].tolist()
        print(name, cnt, out[0, :5])
        if name == "low empty":
            assert cnt[1] == 0 and np.isnan(out[0, 1]) and np.isnan(out[0, 4]) and np.isfinite(out[0, [0, 2, 3]]).all()
        elif name == "low one":
            assert cnt[1] == 1 and np.isnan(out[0, 1]) and np.isnan(out[0, 4]) and np.isnan(T[0, 1]).all()
        elif name == "mid one":
            assert cnt[2] == 1 and np.isnan(out[0, 2]) and np.isnan(out[0, 4]) and np.isfinite(out[0, [0, 1, 3]]).all()
        elif name == "all mid":
            assert cnt == [6, 0, 6, 0] and np.isfinite(out[0, [0, 2]]).all() and np.isnan(out[0, [1, 3, 4]]).all()
        elif name == "all low":
            assert cnt == [5, 5, 0, 0] and np.isfinite(out[0, [0, 1]]).all() and np.isnan(out[0, [2, 3, 4]]).all()
        else:
            assert cnt == [3, 0, 0, 0] and np.isfinite(out[0, 0]) and np.isnan(out[0, 1:5]).all()


def test_emulated_exact_facts_and_silence(emu):
    """y == x: 1.0 exactly in every set that holds two segments.  A digitally silent target: every value NaN; a silent estimate: 0,
    not NaN.  Stretches of exact zeros inside a loud signal, in the target, in the estimate and in both: their segments are dropped
    from the class sets and add their exact zero to `all`."""
    fs, N, H, n = 16000, 512, 256, 12000
    x = O.speech_like(n, fs, 90)
    xf = x.astype(np.float32)
    for same in (xf, xf.astype(np.float64)):
        out, T, _ = run_emu(emu, [xf], [same], [0], fs, N, H, splits=[2000.0])
        assert np.all(out[0, 9:] >= 2) and np.all(out[0, :4] == 1.0) and np.all(out[0, 5:9] == 1.0) and np.all(T == 1.0), out
        assert out[0, 4] == 1.0 / (1.0 + np.exp(-(-3.47 + 1.84 + 9.99)))
    z = np.zeros(n, np.float32)
    out, T, rows = run_emu(emu, [z], [xf], [0], fs, N, H, splits=[2000.0])
    assert np.isnan(out[0, :9]).all() and np.isnan(T).all() and out[0, 9:].tolist() == [CO.segments(n, N, H), 0, 0, 0] and np.all(rows[0] == -1)
    out, T, _ = run_emu(emu, [z], [z], [0], fs, N, H)
    assert np.isnan(out[0, :9]).all()
    out, T, _ = run_emu(emu, [xf], [z], [0], fs, N, H, splits=[2000.0])
    assert np.all(out[0, :4] == 0.0) and np.all(out[0, 5:9] == 0.0) and np.all(T == 0.0) and out[0, 4] == 1.0 / (1.0 + np.exp(3.47))
    x2, y, y2, y3 = x.copy(), O.noisy(x, 8.0, 91), None, None
    x2[3000:3000 + 3 * N] = 0.0
    y2, y3 = y.copy(), y.copy()
    y2[3000:3000 + 3 * N] = 0.0
    y3[7000:7000 + 2 * N + 17] = 0.0
    tg, es, idx = [x2, x], [y2, y, y3, y2], [0, 0, 1, 1]
    out, T, rows = run_emu(emu, tg, es, idx, fs, N, H, splits=[2000.0] * 4)
    O.check_rows(out, tg, es, idx, fs, N, H, None, [2000.0] * 4, T, what="silent stretches")
    _classes_match(rows, tg, N, H)
    assert np.sum(rows[0] == 0) > np.sum(rows[1] == 0) and np.isfinite(out[:, :9]).all()


def test_emulated_white_noise_orders_the_levels_and_empty_batch(emu):
    fs, N, H = 16000, 256, 128
    x = O.speech_like(24000, fs, 1)
    y = O.noisy(x, 0.0, 5)
    out, T, _ = run_emu(emu, [x], [y], [0], fs, N, H)
    O.check_rows(out, [x], [y], [0], fs, N, H, None, None, T, what="white noise at 0 dB")
    print("white noise at 0 dB: csii_high %.3f csii_mid %.3f csii_low %.3f i3 %.3f" % (out[0, 3], out[0, 2], out[0, 1], out[0, 4]))
    assert 1.0 > out[0, 3] > out[0, 2] > out[0, 1] > 0.0
    out, T, _ = run_emu(emu, [x], [], [], fs, N, H)                                # n_est = 0: the target is still classified
    assert out.shape == (0, 13)


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


def _call(lib, tl, idx, n_fft=256, hop=128, n_bands=20, imp=None, split=None, n_est=None, ws=_DUMMY, ws_bytes=1 << 40, out=_DUMMY,
          weights=_DUMMY, null=()):
    tl, tp = _i32(tl)
    idx, ip = _i32(idx)
    imp = np.ascontiguousarray(np.full(max(n_bands, 1), 1.0 / max(n_bands, 1)) if imp is None else imp, np.float64)
    sp, spp = _i32(np.full(max(len(idx), 1), -1) if split is None else split)
    return lib.ssr_csii(_DUMMY, 0, _DUMMY, tp, len(tl), _DUMMY, 0, _DUMMY, ip, len(idx) if n_est is None else n_est, n_fft, hop, n_bands,
                        None if "weights" in null else weights, None if "imp" in null else imp.ctypes.data_as(C.c_void_p),
                        None if "split" in null else spp, out, None, ws, ws_bytes, None)


def test_csii_rejects_bad_arguments_before_launch():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E = _lib.ERR_INVALID_ARG
    for n_fft in (0, 128, 255, 1000, 4096, -1024):
        assert _call(lib, [4000], [0], n_fft=n_fft, hop=64) == E and "n_fft" in err()
    for hop in (0, -1, 257):
        assert _call(lib, [4000], [0], hop=hop) == E and "hop" in err()
    for n_bands in (0, -1, 22):
        assert _call(lib, [4000], [0], n_bands=n_bands) == E and "n_bands" in err()
    for bad in (0.0, -0.1, 1.5, float("nan")):
        assert _call(lib, [4000], [0], n_bands=2, imp=[0.5, bad]) == E and "importance" in err()
    for bad in (-2, 21):
        assert _call(lib, [4000], [0], split=[bad]) == E and "split" in err()
    assert _call(lib, [4000], [0], split=[20], ws_bytes=0) == _lib.ERR_WORKSPACE                 # (n_bands itself: no band above)
    assert _call(lib, [4000, 5000], [2]) == E and "tgt_index" in err()
    assert _call(lib, [4000, 5000], [0, -1]) == E and "tgt_index" in err()
    assert _call(lib, [-3], [0]) == E and "lengths" in err()
    assert _call(lib, [1 << 29], [0]) == E and "lengths" in err()
    assert _call(lib, [4000], [0], out=None) == E and "null" in err()
    for name in ("weights", "imp", "split"):
        assert _call(lib, [4000], [0], null=(name,)) == E and "null" in err()
    tl, tp = _i32([4000, 9000])
    idx, ip = _i32([1, 1, 0])
    need = lib.ssr_csii_workspace_bytes(tp, 2, ip, 3, 256, 128, 20)
    assert need > 0 and lib.ssr_csii_workspace_bytes(tp, 2, ip, 3, 256, 32, 20) > need
    # four sets of [bin][4] doubles per chunk of 32 segments
    one, op = _i32([256 + 32 * 128])
    z, zp = _i32([0])
    more = lib.ssr_csii_workspace_bytes(op, 1, zp, 1, 256, 128, 20) - lib.ssr_csii_workspace_bytes(op, 1, zp, 1, 256, 129, 20)
    assert abs(more - 4 * 129 * 4 * 8) < 256                                        # (33 segments against 32; areas are rounded to 256 bytes)
    assert _call(lib, [4000, 9000], [1, 1, 0], ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in err()
    assert _call(lib, [4000, 9000], [1, 1, 0], ws=None) == _lib.ERR_WORKSPACE
    bad, bp = _i32([2])
    assert lib.ssr_csii_workspace_bytes(tp, 2, bp, 1, 256, 128, 20) == 0
    assert lib.ssr_csii_workspace_bytes(tp, 2, ip, 3, 1000, 128, 20) == 0
    assert lib.ssr_csii_workspace_bytes(tp, 2, ip, 3, 256, 0, 20) == 0
    assert lib.ssr_csii_workspace_bytes(tp, 2, ip, 3, 256, 128, 0) == 0
    assert lib.ssr_csii_workspace_bytes(tp, 2, ip, 3, 256, 128, 22) == 0
    neg, np_ = _i32([4000, -1])
    assert lib.ssr_csii_workspace_bytes(np_, 2, ip, 3, 256, 128, 20) == 0
    # one workgroup of n_fft / 8 threads per chunk of 32 segments: 2^32 threads are refused before anything is queued
    many, mp = _i32([(1 << 29) - 1])
    rep, rp = _i32([0] * 70)
    assert lib.ssr_csii_workspace_bytes(mp, 1, rp, 70, 2048, 1, 1) > 0
    assert _call(lib, [(1 << 29) - 1], [0] * 70, n_fft=2048, hop=1, n_bands=1, ws_bytes=1 << 62) == _lib.ERR_UNSUPPORTED and "too large" in err()
    assert _call(lib, [4000], [], n_est=0, ws=None, ws_bytes=0, out=None, null=("weights", "imp", "split")) == 0      # nothing queued


def test_header_ctypes_table_and_library_agree():
    from ssr_eval_amd import _lib
    path = os.path.join(ROOT, "ssr_eval_amd", "csrc", "ssr_hip_csii.h")
    header = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    declared = set(re.findall(r"\b(ssr_[a-z_0-9]+)\s*\(", header))
    assert declared == {"ssr_csii", "ssr_csii_workspace_bytes"} == set(_lib.CSII_SIGNATURES)
    others = set(_lib.SIGNATURES) | set(_lib.COHERENCE_SIGNATURES) | set(_lib.LOUDNESS_SIGNATURES) | set(_lib.SPECTRUM_SIGNATURES) | \
        set(_lib.AUDITORY_SIGNATURES) | set(_lib.MODULATION_SIGNATURES) | set(_lib.DISTRIBUTION_SIGNATURES)
    assert not set(_lib.CSII_SIGNATURES) & others
    assert "#define SSR_CSII_BANDS 21" in header and "#define SSR_CSII_COLUMNS 13" in header and (_lib.CSII_BANDS, _lib.CSII_COLUMNS) == (21, 13)
    for name, n in (("ssr_csii", 21), ("ssr_csii_workspace_bytes", 7)):
        n_args = len(re.search(r"\b%s\((.*?)\);" % name, header, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.CSII_SIGNATURES[name][1]) == n, name
    lib = _lib.load()
    for name, (res, args) in _lib.CSII_SIGNATURES.items():
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    main = open(os.path.join(ROOT, "include", "ssr_hip.h")).read()
    inc = "#include \"../ssr_eval_amd/csrc/ssr_hip_csii.h\""
    assert main.count(inc) == 1 and main.index(inc) > max(main.index(line) for line in re.findall(r"#include \"../ssr_eval_amd/csrc/ssr_hip_(?!csii)\w+\.h\"", main))
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T ssr_csii\n" in exported and " T ssr_csii_workspace_bytes\n" in exported
    # the header is C99 on its own behind the main one
    src = "#include \"%s\"\nint main(void) { return ssr_csii_workspace_bytes(0, 0, 0, 0, 256, 128, 20) != 0 || SSR_CSII_BANDS != 21; }\n" % \
        os.path.join(ROOT, "include", "ssr_hip.h")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-"], input=src, text=True, check=True)


# ---- AudioMetrics / SSR_Eval_Helper options --------------------------------------------------------------------------------------
def test_audio_metrics_csii_options():
    """Everything here is refused before any device is touched (this test runs without one)."""
    from ssr_eval_amd import AudioMetrics
    bk = B()
    assert [bk.csii_default_nfft(fs) for fs in (8000, 16000, 16001, 44100, 48000, 192000)] == [256, 256, 512, 1024, 1024, 2048]
    for bad in (300, 0, -1, True, None, "16000", float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rate above 300 Hz"):
            bk.csii_default_nfft(bad)
    assert bk.check_csii_frames(16000, None, None) == (256, 128) and bk.check_csii_frames(48000, None, 100) == (1024, 100)
    assert bk.check_csii_frames(16000, 2048, 2048) == (2048, 2048)
    for bad in ((1000, None), (4096, None), (256.0, None), (256, 0), (256, 257), (256, 2.0)):
        with pytest.raises(ValueError):
            bk.check_csii_frames(16000, *bad)
    fc, imp, W = bk.csii_design(16000, 256)
    assert fc.shape == (20,) and imp.shape == (20,) and W.shape == (20, 129) and W.dtype == np.float64 and W.flags.c_contiguous
    assert len(bk.csii_design(8000, 256)[0]) == 17 and len(bk.csii_design(44100, 1024)[0]) == 21 and len(bk.csii_design(48000, 1024)[0]) == 21
    assert list(bk.csii_design(16000, 256, (150, 250))[0]) == [150.0, 250.0] and list(bk.csii_design(48000, 512, (8000, 1e6))[0]) == [8500.0]
    for band in ((0, 100), (9000, 20000), (5, 1), (4000,), 4000, ("a", "b"), (True, 4000), (-1, 4000)):
        with pytest.raises(ValueError, match="band must be None or"):
            bk.csii_design(16000, 256, band)
    with pytest.raises(ValueError):
        bk.csii_design(16000, 300)
    am = AudioMetrics(16000)
    names = ("csii", "csii_low", "csii_mid", "csii_high", "i3", "csii_hf", "csii_mid_hf")
    assert am._csii_names(None) == names and am._csii_names(["i3", "csii"]) == ("csii", "i3")
    assert am._csii_splits(fc, None, 2) == [-1, -1] and am._csii_splits(fc, 4000.0, 2) == [16, 16]
    assert am._csii_splits(fc, [None, 1e9, 0.0, 4000.5, 7000], 5) == [-1, 20, 0, 17, 19]
    x = np.zeros(3000, np.float32)
    for kw in ({"n_fft": 300}, {"n_fft": 1024.0}, {"hop": 0}, {"hop": 257}, {"band": (5, 1)}, {"band": (0, 100)}, {"split_hz": -5}, {"split_hz": "x"},
               {"split_hz": True}, {"split_hz": float("inf")}, {"split_hz": [4000.0, 2000.0]}, {"names": ()}, {"names": "csii"}, {"names": ("nope",)},
               {"return_bands": 1}, {"return_counts": "yes"}):
        with pytest.raises(ValueError):                                          # rejected before any device is touched
            am.csii(x, x, **kw)
        with pytest.raises(ValueError):
            am.csii_batch([x], [x], **kw)
        with pytest.raises(ValueError):
            am.csii_multi([[x]], [x], **kw)
    with pytest.raises(ValueError):
        am.csii_multi([[x], [x]], [x], split_hz=[1000.0])
    with pytest.raises(ValueError):
        am.csii(np.zeros((2, 3000), np.float32), x)
    with pytest.raises(ValueError, match="rate above 300 Hz"):
        AudioMetrics(200).csii(x, x)
    for kw in ({"split_bands": [-2]}, {"split_bands": [21]}, {"split_bands": [1, 2]}, {"n_fft": 100}, {"hop": 0}, {"band": (1, 2)}, {"return_bands": "yes"}):
        with pytest.raises(ValueError):
            bk.csii_metrics([x], [x], [0], 16000, **kw)
    with pytest.raises(ValueError, match="tgt_index out of range"):
        bk.csii_metrics([x], [x], [1], 16000)
    with pytest.raises(ValueError, match="one target index per estimate"):
        bk.csii_metrics([x], [x], [0, 0], 16000)


def test_helper_csii_option_and_key_order():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd import eval as E
    mk = lambda sr=44100, **kw: SSR_Eval_Helper(BasicTestee(), sr, sr, evaluation_sr=sr, test_data_root=None, **kw)      # noqa: E731
    assert mk().csii is None and mk(csii=None).csii is None and mk(csii=True).csii is True
    ok = {"n_fft": 2048, "hop": 100, "band": (300.0, 9000.0), "split": 4000.0}
    assert mk(csii=ok).csii == ok and mk(csii={"split": 0}).csii == {"split": 0} and mk(16000, csii={"band": (150, 150)}).csii == {"band": (150, 150)}
    messages = {"csii must be None, True or a dict": (False, 1, "all", "csii", (), ("i3",), {}, {"which": "i3"}, [True], {"split_hz": 4000}, {"threshold": 0.5}),
                "n_fft must be one of": ({"n_fft": 1000}, {"n_fft": 4096}, {"n_fft": 1024.0}, {"n_fft": None}),
                "hop must be": ({"hop": 0}, {"hop": 2.5}, {"n_fft": 256, "hop": 257}, {"hop": 1025}),
                "band must be None or": ({"band": (8000, 4000)}, {"band": 4000}, {"band": (30000.0, 40000.0)}, {"band": (0.0, 100.0)}),
                "split must be a frequency": ({"split": None}, {"split": "4000"}, {"split": [4000.0]}, {"split": True}),
                "a split frequency is a finite number": ({"split": -5.0}, {"split": float("inf")})}
    for message, values in messages.items():
        for bad in values:
            with pytest.raises(ValueError, match=message):
                mk(csii=bad)
    with pytest.raises(ValueError, match="rate above 300 Hz"):
        mk(200, csii=True)
    params = inspect.signature(SSR_Eval_Helper.__init__).parameters
    assert params["csii"].kind is inspect.Parameter.KEYWORD_ONLY and list(params)[-5:] == ["csii", "auditory", "modulation", "loudness", "bandwidth"]
    # the three pinned tuples and their order functions are what they were; the new tuple is queued behind them
    assert [f.option for f in E._TAIL_FAMILIES] == ["loudness", "bandwidth", "modulation", "auditory"]
    assert [f.option for f in E._LATER_FAMILIES] == ["coherence"] and len(E._FAMILIES) == 10
    assert [f.option for f in E._NEWER_FAMILIES] == ["csii"]
    fam = E._NEWER_FAMILIES[0]
    assert fam.keys == ("csii", "csii_mid", "i3", "csii_hf") and fam.per_key is True and (fam.multi, fam.batch) == ("csii_multi", "csii_batch")
    assert E._ALL_FAMILIES == E._FAMILIES + E._LATER_FAMILIES + E._TAIL_FAMILIES + E._NEWER_FAMILIES
    full = E.full_key_order()
    assert len(full) == 52 and full[-2:] == ("nsim", "nsim_hf") and not set(fam.keys) & set(full)
    assert full == E.all_key_order() + tuple(k for f in E._TAIL_FAMILIES for k in f.keys)
    assert E.every_key_order() == full + fam.keys and len(set(E.every_key_order())) == 56
    keys = ["proc_fft_8000_44100", "proc_mp3_32k_44100"]
    args, kw = fam.arguments(mk(csii=True), keys)
    assert args == ([4000, None], None, None, None) and kw == {"names": fam.keys}
    args, kw = fam.arguments(mk(csii=ok), keys)
    assert args == ([4000.0, 4000.0], 2048, 100, (300.0, 9000.0)) and kw == {"names": fam.keys}
