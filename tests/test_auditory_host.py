"""CPU tests of the auditory family (nsim, nsim_hf, nsim_lf, fvnsim): the float64 oracle
(tests/auditory_oracle.py) pinned to scipy.signal.lfilter, to |H(f_c)| = 2 and to its anchors, a g++ build of the kernel bodies
(ssr_auditory.h) against the oracle - the shapes where the geometry can go wrong, the NaN rules, the bit-level properties -, the C
ABI's argument checks (they return before anything touches a device), the header / ctypes table / library agreement, and
AudioMetrics.nsim* / SSR_Eval_Helper(auditory=...) validation and key order.

Bars (auditory_oracle.TOL_*): P within 1e-9 of the target's largest cell; the NSIM values within 1e-9 - the worst difference to the
oracle measured on the emulated bodies is 1.1e-14, at most 1e-11, so the bar is the project's customary 1e-9 -; the dB images
within 1e-6 dB.  An input must keep every scored value finite (auditory_oracle.assert_conditioned): where that fails the input is
wrong, not the kernel.  Worst differences seen in emulation: P 1.2e-14 of the target's largest cell, NSIM values 1.1e-14, dB images
2.5e-12 dB; on an MI355X: P 1.2e-14, NSIM values 1.1e-14, dB images 2.5e-12 dB (tests/test_gpu_auditory.py).  The geometry cases
include hop-blocks of more than one staging tile (8 CP samples), with and without a partial last tile."""
import ctypes as C
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest

import auditory_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 16000


# ---- the oracle's pins ------------------------------------------------------------------------------------------------------------
def test_oracle_cascade_is_four_lfilter_passes():
    from scipy.signal import lfilter
    fc, coef = O.design(FS, 32)
    x = O.harmonic(1500, FS, 1) + O.noise(1500, 2, 0.05)
    z = O.filterbank(x, coef)
    worst = 0.0
    for c in range(32):
        a = complex(coef[c, 0], coef[c, 1])
        y = coef[c, 2] * x.astype(np.complex128)
        for _ in range(4):
            y = lfilter([1.0], [1.0, -a], y)
        worst = max(worst, float(np.max(np.abs(z[c] - y)) / np.max(np.abs(y))))
    print("worst difference to four lfilter passes re the band's peak", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("fs", [8000, 16000, 44100, 48000])
def test_oracle_gain_at_the_centre_frequency_is_two(fs):
    from scipy.signal import freqz
    fc, coef = O.design(fs)
    assert len(fc) == 32 and abs(fc[0] - 50.0) < 1e-9 and abs(fc[-1] - 0.45 * fs) < 1e-6 and np.all(np.diff(O.erb_scale(fc)) > 0)
    assert np.allclose(np.diff(O.erb_scale(fc)), np.diff(O.erb_scale(fc))[0], rtol=1e-10) and abs(O.A_GAMMA - 0.9817477042468103) < 1e-15
    worst = 0.0
    for c in range(32):
        a = complex(coef[c, 0], coef[c, 1])
        assert abs(a) < 1.0
        # (section by section: the expanded 4th-order polynomial of a pole this close to the unit circle loses 1e-6 to cancellation)
        _, h = freqz([1.0], [1.0, -a], worN=[2.0 * np.pi * fc[c] / fs])
        worst = max(worst, abs(coef[c, 2] * abs(h[0]) ** 4 - 2.0))
    print(fs, "worst | |H(f_c)| - 2 |", worst)
    assert worst <= 1e-6


def test_oracle_anchors_and_nan_rules():
    fc, coef = O.design(FS, 32)
    hop = 160
    # a sine of amplitude A at f_c: |z|^2 / 2 -> A^2 / 2 (the sine's power) once the filter has settled
    c, A = 16, 0.3
    s = A * np.sin(2.0 * np.pi * fc[c] * np.arange(8000) / FS)
    P = O.power_image(s, coef, hop)
    print("sine anchor: P / (A^2 / 2) in the last rows", P[-3:, c] / (A * A / 2.0))
    assert np.all(np.abs(P[-10:, c] / (A * A / 2.0) - 1.0) < 1e-3)
    x = O.harmonic(4000, FS, 3)
    y = O.lowpassed(x, 0.25)
    same = O.analyse(x, x.copy(), coef, hop, split=O.split_band(fc, 2000.0))
    assert np.all(np.abs(same["pair"] - 1.0) <= 1e-12) and np.all(np.abs(same["bands"][1:-1] - 1.0) <= 1e-12) and np.isnan(same["bands"][[0, -1]]).all()
    full, half = O.analyse(x, y, coef, hop, split=10), O.analyse(x, 0.5 * y, coef, hop, split=10)
    assert np.max(np.abs(full["pair"] - half["pair"])) <= 1e-12 and full["pair"][1] < full["pair"][2] < 1.0
    loud = O.analyse(x, 0.5 * y, coef, hop, match_level=False, split=10)
    assert abs(loud["pair"][0] - full["pair"][0]) > 1e-3
    # the NaN rules: T < 3, a digitally silent target; a silent estimate is scored; the split's three cases
    assert np.isnan(O.analyse(x[:3 * hop + hop - 1], y[:3 * hop + hop - 1], coef, hop, split=10)["pair"]).all() and O.rows(4 * hop - 1, hop) == 2
    assert np.isfinite(O.analyse(x[:4 * hop], y[:4 * hop], coef, hop, split=10)["pair"]).all() and O.rows(4 * hop, hop) == 3
    assert np.isnan(O.analyse(np.zeros(4000), y, coef, hop, split=10)["pair"]).all()
    quiet = O.analyse(x, np.zeros(4000), coef, hop, split=10)
    assert np.isfinite(quiet["pair"]).all() and quiet["pair"][0] < 0.5
    for sp, nan in ((-1, [1, 2]), (1, [2]), (31, [1])):
        p = O.analyse(x, y, coef, hop, split=sp)["pair"]
        assert [j for j in range(3) if math.isnan(p[j])] == nan, (sp, p)
    assert O.split_band(fc, None) == -1 and O.split_band(fc, 0.0) == 1 and O.split_band(fc, 1e9) == 31 and O.split_band(fc, fc[5]) == 5
    assert [O.rows(n, 160) for n in (319, 320, 479, 480, 640, 641)] == [0, 1, 1, 2, 3, 3]


# ---- the kernel bodies compiled for the host ------------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "auditory_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libauditory_emu.so")
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    lib = C.CDLL(EMU_SO)
    lib.auditory_emu.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                 C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int] + [C.c_void_p] * 5
    return lib


def run(c, lib, bands=True, images=True, gap=3):
    """The emulation on Case c -> (pair_out, band_out or None, the dB images per signal or None, the power images per signal);
    gap: unused samples between the signals."""
    n_t, n_e, nb = len(c.tgts), len(c.ests), len(c.coef)
    td, to, tl = O.pack(c.tgts, gap, c.tdt)
    ed, eo, _ = O.pack(c.ests, gap + 1, c.edt)
    idx, sp = np.array(c.index, np.int32), np.array(c.splits, np.int32)
    r = c.rows()
    edges = np.concatenate(([0], np.cumsum(r))).astype(np.int64)
    pair, bd = np.full((n_e, 3), -123.0), (np.full((n_e, nb), -123.0) if bands else None)
    img, pw = (np.full((int(edges[-1]), nb), -123.0) if images else None), np.full((int(edges[-1]), nb), -123.0)
    rc = lib.auditory_emu(P(td), int(c.tdt == np.float64), P(to), P(tl), n_t, P(ed), int(c.edt == np.float64), P(eo), P(idx), n_e, c.hop, nb,
                          P(c.coef), c.range_db, int(c.match), P(sp), P(pair), P(bd), P(img), P(pw))
    assert rc == 0
    cut = lambda a: None if a is None else [a[edges[i]:edges[i + 1]] for i in range(len(r))]      # noqa: E731
    return pair, bd, cut(img), cut(pw)


def same_bits(a, b):
    return all((x is None and y is None) or np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("fs,hop,n_bands,ks", [(16000, 160, 32, (8, 9, 64)), (16000, 8, 3, (8, 9, 64, 512, 513)), (16000, 8, 32, (8, 9, 16, 64, 65, 128)),
                                               (16000, 8, 64, (8, 9, 32, 33, 64)), (16000, 100, 3, (8, 9, 64)), (48000, 480, 32, (8, 9)),
                                               (16000, 513, 64, (8, 9))],
                         ids=["hop160-32", "hop8-3", "hop8-32", "hop8-64", "hop100-3-4tiles", "48k-hop480-32-2tiles", "hop513-64-2tiles"])
def test_emulated_geometry_shapes_and_bit_level_properties(emu, fs, hop, n_bands, ks):
    """The geometry batch against the oracle in two dtype combinations; then: a pair alone gives the bits it gives in the batch, so
    does the batch reversed with other gaps, and band_out = image_out = NULL changes no bit of pair_out."""
    c = O.geometry_case(fs, hop, n_bands, ks)
    got = run(c, emu)
    worst = c.check(*got, name="hop %d C %d" % (hop, n_bands))
    print(hop, n_bands, "worst P %.3g, NSIM %.3g, dB image %.3g" % worst)
    pair, bd, img, pw = got
    n_t = len(c.tgts)
    assert np.isnan(pair[:3]).all() and np.isfinite(pair[3, 0]) and [len(i) for i in img[:4]] == [0, 1, 2, 3]
    assert np.isfinite(pair[4:, 0]).all() and not np.isinf(pair).any() and np.isnan(bd[:, [0, -1]]).all() and np.isfinite(bd[3:, 1:-1]).all()
    f64 = O.geometry_case(fs, hop, n_bands, ks[:2], tdt=np.float32, edt=np.float64)
    print("f32 / f64: worst P %.3g, NSIM %.3g, dB image %.3g" % f64.check(*run(f64, emu), name="f32/f64"))
    for e in (3, 5, n_t - 1, n_t, n_t + 1):
        one = run(O.Case([c.tgts[c.index[e]]], [c.ests[e]], [0], c.coef, hop, splits=[c.splits[e]], edt=np.float32, fs=fs), emu, gap=0)
        assert one[0].tobytes() == pair[e:e + 1].tobytes() and one[1].tobytes() == bd[e:e + 1].tobytes(), e
        assert same_bits(one[2], [img[c.index[e]], img[n_t + e]]) and same_bits(one[3], [pw[c.index[e]], pw[n_t + e]]), e
    back = run(O.Case(c.tgts[::-1], c.ests[::-1], [n_t - 1 - t for t in c.index[::-1]], c.coef, hop, splits=c.splits[::-1], edt=np.float32, fs=fs), emu, gap=7)
    assert back[0][::-1].tobytes() == pair.tobytes() and back[1][::-1].tobytes() == bd.tobytes() and same_bits(back[2][::-1], img[n_t:] + img[:n_t])
    off = run(c, emu, bands=False, images=False)
    assert off[0].tobytes() == pair.tobytes() and same_bits(off[3], pw)
    half = run(c, emu, bands=True, images=False)
    assert half[0].tobytes() == pair.tobytes() and half[1].tobytes() == bd.tobytes()


@pytest.mark.parametrize("tdt,edt", [(np.float64, np.float64), (np.float32, np.float32)], ids=["f64", "f32"])
def test_emulated_ragged_batch_and_three_estimates_per_target(emu, tdt, edt):
    """Six signals of 0.5 s or less at 16 kHz, hop 160, 32 bands: harmonic tones and noise, each with K = 1 estimate and the first
    with K = 3 (low-passed, noisy, unrelated) at three different splits - none, above every band, 2 kHz; with and without level
    matching; range_db away from its default."""
    fc, coef = O.design(FS, 32)
    lens = (8000, 6123, 4801, 3000, 1777, 640)
    tgts = [O.harmonic(n, FS, 10 + i) if i % 2 == 0 else O.noise(n, 10 + i) for i, n in enumerate(lens)]
    ests = [O.lowpassed(tgts[0], 0.25), tgts[0] + O.noise(lens[0], 30, 0.02), O.noise(lens[0], 31)] + \
        [0.7 * t + O.noise(len(t), 40 + i, 0.01) for i, t in enumerate(tgts[1:])]
    index = [0, 0, 0, 1, 2, 3, 4, 5]
    splits = [-1, 31, O.split_band(fc, 2000.0), 5, 1, 30, -1, 17]
    power = None
    for match, rdb in ((True, 60.0), (False, 60.0), (True, 35.5)):
        c = O.Case(tgts, ests, index, coef, 160, range_db=rdb, match=match, splits=splits, tdt=tdt, edt=edt, power=power)
        got = run(c, emu)
        print(np.dtype(tdt).name, match, rdb, "worst P %.3g, NSIM %.3g, dB image %.3g" % c.check(*got, name="ragged"), got[0][:3, 0])
        pair, power = got[0], c.power          # (the oracle's power images do not depend on the options that change)
        assert np.isnan(pair[0, 1:]).all() and np.isnan(pair[1, 1]) and np.isfinite(pair[1, 2]) and np.isfinite(pair[2]).all()
        assert pair[2, 0] < pair[1, 0] < 1.0 and pair[0, 0] < pair[1, 0] and np.isnan(pair[4, 2]) and np.isfinite(pair[5]).all()


def test_emulated_silence_identity_and_gain(emu):
    """A silent target: NaN everywhere, NaN images.  A silent estimate: scored, finite.  A denormal estimate with level
    matching: NaN, no infinity.  Estimate = target: 1 within 1e-12.  Level matching: a
    gain of 0.5 (a power of two) changes no bit; without it the value moves."""
    fc, coef = O.design(FS, 32)
    x = O.harmonic(3000, FS, 5)
    y = O.lowpassed(x, 0.3)
    z = np.zeros(3000)
    # (1e-160 y: its image is denormal and the level factor overflows - the pair's NaN rule, no infinity)
    c = O.Case([x, z], [z, x.copy(), y, 0.5 * y, y, 1e-160 * y], [0, 0, 0, 0, 1, 0], coef, 160, splits=[9] * 6)
    pair, bd, img, _ = run(c, emu)
    c.check(pair, bd, img, name="silence")
    assert np.isnan(pair[5]).all() and np.isnan(bd[5]).all() and np.isnan(img[2 + 5]).all() and not any(np.isinf(i).any() for i in img)
    assert np.isfinite(pair[0]).all() and pair[0, 0] < 0.5 and np.max(np.abs(pair[1] - 1.0)) <= 1e-12 and np.max(np.abs(bd[1, 1:-1] - 1.0)) <= 1e-12
    assert pair[2].tobytes() == pair[3].tobytes() and np.isnan(pair[4]).all() and np.isnan(bd[4]).all()
    assert np.isnan(img[1]).all() and np.isnan(img[2 + 4]).all() and not np.any(img[2 + 0] - img[2 + 0][0, 0]) and not np.isinf(pair).any()
    assert abs(np.max(img[0]) - 10.0 * math.log10(np.max(O.power_image(x, coef, 160)))) < 1e-9 and np.min(img[0]) >= np.max(img[0]) - 60.0
    loud = run(O.Case([x], [y, 0.5 * y], [0, 0], coef, 160, match=False, splits=[9, 9]), emu)[0]
    assert abs(loud[0, 0] - loud[1, 0]) > 1e-3 and abs(loud[0, 0] - pair[2, 0]) < 0.05
    res = np.zeros(7, np.int64)
    emu.auditory_geometry(48000 * 600, 480, 32, P(res))
    assert list(res) == [60000, 59999, 7500, 938, 8, 65536, 32]
    emu.auditory_geometry(319, 160, 3, P(res))
    assert list(res[:4]) == [0, 0, 0, 0] and res[6] == 4
    # the block transition of the scan: a^L binom(L - 1 + d, d), against a^L from the polar form
    tab = np.zeros((32, 12))
    emu.auditory_tables(P(coef), 32, 160, P(tab))
    a = coef[:, 0] + 1j * coef[:, 1]
    L = 8 * 160
    aL = np.abs(a) ** L * np.exp(1j * L * np.angle(a))
    for d, b in enumerate((1.0, L, L * (L + 1) / 2.0, L * (L + 1) * (L + 2) / 6.0)):
        got = tab[:, 4 + 2 * d] + 1j * tab[:, 5 + 2 * d]
        assert np.max(np.abs(got - aL * b)) <= 1e-9 * np.max(np.abs(aL * b)), d


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first
_COEF = O.design(FS, 32)[1]


def _call(lib, lens, index, hop=160, coef=_COEF, n_bands=None, range_db=60.0, match=1, split=None, n_tgt=None, n_est=None, tgt=_DUMMY, est=_DUMMY,
          toff=_DUMMY, eoff=_DUMMY, pair=_DUMMY, ws=_DUMMY, ws_bytes=1 << 40, null=()):
    ln, ix = np.ascontiguousarray(lens, np.int32), np.ascontiguousarray(index, np.int32)
    cf = np.ascontiguousarray(coef, np.float64)
    sp = np.full(len(ix), -1, np.int32) if split is None else np.ascontiguousarray(split, np.int32)
    return lib.ssr_auditory(tgt, 0, toff, None if "len" in null else P(ln), len(ln) if n_tgt is None else n_tgt, est, 0, eoff,
                            None if "index" in null else P(ix), len(ix) if n_est is None else n_est, hop, len(cf) if n_bands is None else n_bands,
                            None if "coef" in null else P(cf), range_db, match, None if "split" in null else P(sp), pair, None, None, ws, ws_bytes, None)


def test_auditory_rejects_bad_arguments_before_launch():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E = _lib.ERR_INVALID_ARG
    for hop in (0, -1, -160):
        assert _call(lib, [4000], [0], hop=hop) == E and "hop" in err()
    for nb in (0, 2, 65, -3):
        assert _call(lib, [4000], [0], n_bands=nb) == E and "n_bands" in err()
    for rdb in (0.0, -3.0, 150.5, float("nan"), float("inf")):
        assert _call(lib, [4000], [0], range_db=rdb) == E and "range_db" in err()
    for j, v in ((0, 1.0), (1, 1.0), (0, float("nan")), (1, float("inf")), (2, float("nan")), (2, float("inf"))):
        bad = _COEF.copy()
        bad[7, j] = v
        assert _call(lib, [4000], [0], coef=bad) == E and "coef" in err(), (j, v)
    for sp in (-2, 0, 32, 100):
        assert _call(lib, [4000], [0], split=[sp]) == E and "split_band" in err()
    assert _call(lib, [4000, -1], [0]) == E and "lengths" in err()
    assert _call(lib, [1 << 29], [0]) == E and "lengths" in err()
    assert _call(lib, [4000], [1]) == E and "tgt_index" in err()
    assert _call(lib, [4000], [-1]) == E and "tgt_index" in err()
    assert _call(lib, [4000], [0], n_tgt=-1) == E and _call(lib, [4000], [0], n_est=-1) == E
    for name in ("len", "index", "coef", "split"):
        assert _call(lib, [4000], [0], null=(name,)) == E and "null" in err(), name
    for kw in ({"tgt": None}, {"est": None}, {"toff": None}, {"eoff": None}, {"pair": None}):
        assert _call(lib, [4000], [0], **kw) == E and "null" in err(), kw
    ln, ix = np.array([4000, 0, 319, 320], np.int32), np.array([0, 0, 3], np.int32)
    need = lib.ssr_auditory_workspace_bytes(P(ln), 4, P(ix), 3, 160, 32)
    assert need > 0 and lib.ssr_auditory_workspace_bytes(P(ln), 4, P(ix), 0, 160, 32) < need
    assert _call(lib, ln, ix, ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in err()
    assert _call(lib, ln, ix, ws=None) == _lib.ERR_WORKSPACE
    for bad in ((P(ln), 4, P(ix), 3, 0, 32), (P(ln), 4, P(ix), 3, 160, 2), (P(ln), 4, P(ix), 3, 160, 65), (None, 4, P(ix), 3, 160, 32),
                (P(ln), -1, P(ix), 3, 160, 32), (P(ln), 2, P(ix), 3, 160, 32)):
        assert lib.ssr_auditory_workspace_bytes(*bad) == 0
    # the block limit: ten minutes at 48 kHz fit, 65537 blocks do not - refused before anything is enqueued
    ten = np.array([48000 * 600], np.int32)
    assert lib.ssr_auditory_workspace_bytes(P(ten), 1, P(ix), 0, 480, 32) > 0
    assert _call(lib, [65537 * 160], [0]) == _lib.ERR_UNSUPPORTED and "65536" in err()
    assert lib.ssr_auditory_workspace_bytes(P(np.array([65537], np.int32)), 1, P(ix), 0, 1, 32) == 0
    assert _call(lib, [], [], tgt=None, est=None, toff=None, eoff=None, pair=None, ws=None, ws_bytes=0) == 0      # nothing queued


def test_header_ctypes_table_and_library_agree():
    from ssr_eval_amd import _lib
    path = os.path.join(ROOT, "ssr_eval_amd", "csrc", "ssr_hip_auditory.h")
    header = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    declared = set(re.findall(r"\b(ssr_[a-z_0-9]+)\s*\(", header))
    assert declared == {"ssr_auditory", "ssr_auditory_workspace_bytes"} == set(_lib.AUDITORY_SIGNATURES)
    others = set(_lib.SIGNATURES) | set(_lib.COHERENCE_SIGNATURES) | set(_lib.LOUDNESS_SIGNATURES) | set(_lib.SPECTRUM_SIGNATURES)
    assert not set(_lib.AUDITORY_SIGNATURES) & others
    assert "#define SSR_AUDITORY_MAX_BANDS 64" in header and "#define SSR_AUDITORY_MIN_BANDS 3" in header and "#define SSR_AUDITORY_MAX_BLOCKS 65536" in header
    assert (_lib.AUDITORY_MIN_BANDS, _lib.AUDITORY_MAX_BANDS, _lib.AUDITORY_MAX_BLOCKS) == (3, 64, 65536)
    lib = _lib.load()
    for name, (res, args) in _lib.AUDITORY_SIGNATURES.items():
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    main = open(os.path.join(ROOT, "include", "ssr_hip.h")).read()
    inc = "#include \"../ssr_eval_amd/csrc/ssr_hip_auditory.h\""
    assert main.count(inc) == 1 and main.index(inc) > main.index("#include \"../ssr_eval_amd/csrc/ssr_hip_spectrum.h\"")
    assert os.listdir(os.path.join(ROOT, "include")) == ["ssr_hip.h"]
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T ssr_auditory\n" in exported and " T ssr_auditory_workspace_bytes\n" in exported
    # the header is C99 on its own behind the main one
    src = "#include \"%s\"\nint main(void) { return ssr_auditory_workspace_bytes(0, 0, 0, 0, 160, 32) != 0; }\n" % os.path.join(ROOT, "include", "ssr_hip.h")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-"], input=src, text=True, check=True)


# ---- AudioMetrics / SSR_Eval_Helper options --------------------------------------------------------------------------------------
def test_audio_metrics_nsim_options():
    """Everything here is refused before any device is touched (this test runs without one)."""
    from ssr_eval_amd import AudioMetrics
    from ssr_eval_amd import backend as B
    for fs, nb, band in ((8000, 32, None), (16000, 3, None), (44100, 64, (100.0, 18000.0)), (48000, 32, None)):
        fc, coef = B.gammatone_design(fs, nb, band)
        fo, co = O.design(fs, nb, band)
        assert coef.shape == (nb, 3) and coef.dtype == np.float64 and np.max(np.abs(fc - fo)) <= 1e-9 and np.max(np.abs(coef - co)) <= 1e-14
    assert [B.auditory_hop(fs) for fs in (8000, 16000, 22050, 44100, 48000)] == [80, 160, 221, 441, 480]
    assert B.check_auditory_range(150) == 150.0 and B.check_auditory_bands(3) == 3
    for bad in (2, 65, 32.0, True, None, "32"):
        with pytest.raises(ValueError):
            B.check_auditory_bands(bad)
    for bad in (0, -1.0, 150.1, True, None, "60", float("nan"), float("inf")):
        with pytest.raises(ValueError):
            B.check_auditory_range(bad)
    for band in ((0.0, 4000.0), (50.0, 8000.0), (4000.0, 50.0), (50.0,), "50-4000", (50.0, 4000.0, 1.0), (True, 4000.0), (50.0, float("nan"))):
        with pytest.raises(ValueError):
            B.gammatone_design(16000, 32, band)
    for fs in (0, -16000, 10, None, "16000", float("inf")):
        with pytest.raises(ValueError):
            B.gammatone_design(fs)
    x = np.zeros(6000, np.float32)
    am = AudioMetrics(16000)
    fc, _ = B.gammatone_design(16000)
    assert am._nsim_names(None) == ("nsim", "nsim_hf", "nsim_lf") and am._nsim_names(["nsim_hf", "nsim"]) == ("nsim", "nsim_hf")
    assert am._nsim_splits(fc, None, 2) == [-1, -1] and am._nsim_splits(fc, 2000.0, 2) == [O.split_band(fc, 2000.0)] * 2
    assert am._nsim_splits(fc, [None, 1e9, 0.0, float(fc[7])], 4) == [-1, 31, 1, 7]
    for kw in ({"n_bands": 2}, {"n_bands": 65}, {"n_bands": 32.0}, {"band": (0.0, 1000.0)}, {"band": (50.0, 8000.0)}, {"band": (1, 2, 3)},
               {"range_db": 0}, {"range_db": 151}, {"range_db": "60"}, {"match_level": 1}, {"match_level": None}, {"return_bands": 1},
               {"split_hz": -1.0}, {"split_hz": "4000"}, {"split_hz": [4000.0, 2000.0]}, {"split_hz": float("inf")}, {"split_hz": True},
               {"names": ()}, {"names": "nsim"}, {"names": ("nope",)}):
        with pytest.raises(ValueError):
            am.nsim_batch([x], [x], **kw)
    with pytest.raises(ValueError):
        am.nsim_multi([[x], [x]], [x], split_hz=[1000.0])
    with pytest.raises(ValueError):
        am.nsim(np.zeros((2, 6000), np.float32), np.zeros(6000, np.float32))
    for kw in ({"split_bands": [-2]}, {"split_bands": [0]}, {"split_bands": [32]}, {"split_bands": [1, 2]}, {"range_db": -1}, {"n_bands": 100},
               {"hop": 0}, {"hop": 1.5}, {"match_level": "yes"}):
        with pytest.raises(ValueError):
            B.auditory_metrics([x], [x], [0], 16000, **kw)
    with pytest.raises(ValueError):
        B.auditory_metrics([x], [x], [1], 16000)
    with pytest.raises(ValueError):
        B.auditory_metrics([x], [x], [0, 0], 16000)


def test_helper_auditory_option_and_key_order():
    import inspect
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd import eval as E
    mk = lambda sr=44100, **kw: SSR_Eval_Helper(BasicTestee(), sr, sr, evaluation_sr=sr, test_data_root=None, **kw)      # noqa: E731
    assert mk().auditory is None and mk(auditory=None).auditory is None and mk(auditory=True).auditory is True
    ok = {"n_bands": 24, "band": (100.0, 18000.0), "range_db": 50.0, "split": 4000.0, "match_level": False}
    assert mk(auditory=ok).auditory == ok and mk(auditory={"split": 8000}).auditory == {"split": 8000}
    for bad in (False, 1, "all", "nsim", (), ("nsim",), {}, {"which": "nsim"}, [True], {"n_bands": 2}, {"n_bands": 65}, {"n_bands": 32.5},
                {"band": (30000.0, 40000.0)}, {"band": (0.0, 100.0)}, {"split": None}, {"split": -5.0}, {"split": "4000"}, {"split": [4000.0]},
                {"split": {4000.0}}, {"split": 4000j}, {"split": object()}, {"split": float("inf")}, {"range_db": 0.0}, {"range_db": 200}, {"match_level": 1}, {"threshold": 0.5}, {"hop": 160}):
        with pytest.raises(ValueError):
            mk(auditory=bad)
    params = inspect.signature(SSR_Eval_Helper.__init__).parameters
    assert params["auditory"].kind is inspect.Parameter.KEYWORD_ONLY and list(params)[-2:] == ["loudness", "bandwidth"]
    # the family is a member of the open-ended tail, after bandwidth, and its keys end full_key_order()
    tail = [f.option for f in E._TAIL_FAMILIES]
    assert "auditory" in tail and tail.index("auditory") > tail.index("bandwidth") > tail.index("loudness")
    fam = E._TAIL_FAMILIES[tail.index("auditory")]
    assert fam.keys == ("nsim", "nsim_hf") and fam.per_key is True and (fam.multi, fam.batch) == ("nsim_multi", "nsim_batch")
    assert "auditory" not in [f.option for f in E._FAMILIES + E._LATER_FAMILIES]
    full = E.full_key_order()
    assert full[:len(E.all_key_order())] == E.all_key_order() and len(set(full)) == len(full) and full[-2:] == fam.keys
    assert full[len(E.all_key_order()):] == tuple(k for f in E._TAIL_FAMILIES for k in f.keys)
    keys = ["proc_fft_8000_44100", "proc_mp3_32k_44100"]
    args, kw = fam.arguments(mk(auditory=True), keys)
    assert args == ([4000.0, None], 32, None, 60.0, True) and kw == {"names": fam.keys}
    args, kw = fam.arguments(mk(auditory=ok), keys)
    assert args == ([4000.0, 4000.0], 24, (100.0, 18000.0), 50.0, False)
