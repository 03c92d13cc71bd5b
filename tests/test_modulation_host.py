"""CPU tests of the modulation family (srmr, srmr_diff, mod_dist, mod_dist_hf, mod_dist_lf): the float64 oracle
(tests/modulation_oracle.py) pinned to its anchors - unit gain at every modulation centre, zeros at DC and Nyquist, an AM tone
lands in its own column, AM noise moves SRMR the way the measure is meant to - and its monotone approach to a full-rate SRMR; a g++
build of the kernel bodies (ssr_modulation.h on ssr_auditory.h's sweeps) against the oracle - the shapes where the geometry can go
wrong, the NaN rules, the bit-level properties -, the C ABI's argument checks (they return before anything touches a device), the
header / ctypes table / library agreement, and AudioMetrics.srmr / modulation* / SSR_Eval_Helper(modulation=...) validation and
key order.

Bars (modulation_oracle.TOL_*): Ebar within 1e-9 of the signal's largest cell, srmr within 1e-9 max(1, |srmr|), c90 and K* equal,
mod_dist* within 1e-6 dB, srmr_diff within 2e-9 max(1, |srmr|).  An input must keep c90 away from rounding
(modulation_oracle.assert_conditioned): where that fails the input is wrong, not the kernel.  Worst differences seen in emulation:
Ebar 7.7e-13 of the largest cell, srmr 2.4e-13, mod_dist* 3.1e-13 dB, srmr_diff 6.2e-13 (all in the hop_e = 1 case); on an MI355X:
Ebar 9.1e-13, srmr 2.0e-13, mod_dist* 2.6e-13 dB, srmr_diff 1.2e-12 (tests/test_gpu_modulation.py)."""
import ctypes as C
import glob
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import auditory_oracle as A
import modulation_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 16000
SHAPES, SHAPE_IDS, same_bits, sub_case = O.SHAPES, O.SHAPE_IDS, O.same_bits, O.sub_case

# ---- the oracle's pins ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fe", [1600.0, 44100 / 27, 800.0, 48000 / 7, 8000.0])
def test_oracle_bank_has_unit_gain_at_its_centres_and_zeros_at_dc_and_nyquist(fe):
    from scipy.signal import freqz
    mod, fk = O.mod_design(fe), O.mod_centres()
    assert abs(fk[0] - 4.0) < 1e-12 and abs(fk[-1] - 128.0) < 1e-9 and np.allclose(fk[1:] / fk[:-1], 32.0 ** (1.0 / 7.0))
    worst = 0.0
    for k in range(O.K):
        b, a = mod[k, :3], np.concatenate(([1.0], mod[k, 3:]))
        _, h = freqz(b, a, worN=[2.0 * np.pi * fk[k] / fe, 0.0, np.pi])
        worst = max(worst, abs(abs(h[0]) - 1.0))
        assert abs(h[1]) <= 1e-12 and abs(h[2]) <= 1e-12 and mod[k, 1] == 0.0 and mod[k, 0] == -mod[k, 2]
        assert abs(mod[k, 4]) < 1.0 and abs(mod[k, 3]) < 1.0 + mod[k, 4]
    print(fe, "worst | |H_k(f_k)| - 1 |", worst)
    assert worst <= 1e-12
    assert [O.hop_e(fs) for fs in (8000, 16000, 44100, 48000)] == [5, 10, 27, 30] and (O.hop_e(48000, 800), O.hop_e(8000, 6400)) == (60, 1)
    assert [O.frame_step(fs / O.hop_e(fs)) for fs in (8000, 44100, 48000)] == [102, 105, 102]
    assert [O.frames(nb, 102) for nb in (407, 408, 509, 510, 612)] == [0, 1, 1, 2, 3] and [O.blocks(n, 5) for n in (9, 10, 14)] == [0, 2, 2]


def test_oracle_am_tone_lands_in_its_own_column_and_am_noise_moves_srmr():
    fc, coef = A.design(FS, 32)
    hop = O.hop_e(FS)
    c = 24                                    # a band wide enough for the sidebands at +- 128 Hz
    t = np.arange(FS) / FS
    sigs = [(1.0 + 0.8 * np.sin(2.0 * np.pi * f * t)) * np.sin(2.0 * np.pi * fc[c] * t) for f in O.mod_centres()]
    for k, d in enumerate(O.analyses_of(sigs, FS, hop, 32)):
        print("AM at %.1f Hz: band %d's Ebar" % (O.mod_centres()[k], c), d["E"][c])
        assert int(np.argmax(d["E"][c])) == k, (k, d["E"][c])
    noise = A.noise(2 * FS, 7)
    t = np.arange(2 * FS) / FS
    plain, slow, fast = O.analyses_of([noise, (1.0 + 0.8 * np.sin(2.0 * np.pi * 4.0 * t)) * noise,
                                       (1.0 + 0.8 * np.sin(2.0 * np.pi * 64.0 * t)) * noise], FS, hop, 32)
    print("srmr of noise: AM 4 Hz %.3f, none %.3f, AM 64 Hz %.3f" % (slow["srmr"], plain["srmr"], fast["srmr"]))
    assert slow["srmr"] > plain["srmr"] > fast["srmr"] > 0.0
    # K* grows with the band's width; a constant replaces the table
    tab = O.kstar_table(fc)
    assert tab[0] == 5 and tab[-1] == 8 and np.all(np.diff(tab) >= 0) and list(O.kstar_table(fc, 6)) == [6] * 32
    assert O.split_band(fc, None) == -1 and O.split_band(fc, 0.0) == 0 and O.split_band(fc, 1e9) == 32 and O.split_band(fc, fc[5]) == 5


def test_oracle_approaches_the_full_rate_srmr_monotonically():
    """The block envelope against |z| at the signal's own rate: the gap shrinks with every doubling of env_rate (two seeds; the
    figures are DESIGN section 24's stated distance, not a bar)."""
    for seed in (1, 2):
        x = O.voiced(FS, FS, seed) + 0.3 * O.reverberated(O.voiced(FS, FS, seed), FS, 10 + seed)
        full = O.full_rate_srmr(x, FS)
        got = [O.analyses_of([x], FS, O.hop_e(FS, r), 32)[0]["srmr"] for r in (800, 1600, 3200)]
        gaps = [abs(g - full) / full for g in got]
        print("seed %d: full-rate srmr %.4f; env_rate 800 / 1600 / 3200: %s; relative gaps %s" % (seed, full, got, gaps))
        assert gaps[0] > gaps[1] > gaps[2]


# ---- the kernel bodies compiled for the host ------------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "modulation_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libmodulation_emu.so")
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    lib = C.CDLL(EMU_SO)
    lib.modulation_emu.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double] + [C.c_void_p] * 4
    return lib


def run(c, lib, spec=True, gap=3):
    """The emulation on Case c -> (signal_out, pair_out, spectrum_out or None); gap: unused (NaN) samples between the signals."""
    n_t, n_e, nb = len(c.tgts), len(c.ests), c.n_bands
    td, to, tl = A.pack(c.tgts, gap, c.tdt)
    ed, eo, _ = A.pack(c.ests, gap + 1, c.edt) if n_e else (None, None, None)
    idx, sp = np.array(c.index, np.int32), np.array(c.splits, np.int32)
    sig, pair = np.full((n_t + n_e, 4), -123.0), np.full((n_e, 4), -123.0)
    sx = np.full((n_t + n_e, nb, 8), -123.0) if spec else None
    rc = lib.modulation_emu(P(td), int(c.tdt == np.float64), P(to), P(tl), n_t, P(ed), int(c.edt == np.float64), P(eo), P(idx), n_e, c.hop, nb,
                            P(c.coef), P(c.mod), c.S, P(c.ktab), c.range_db, P(sp), P(sig), P(pair), P(sx))
    assert rc == 0
    return sig, pair, sx


@pytest.mark.parametrize("fs,n_bands,env_rate", SHAPES, ids=SHAPE_IDS)
def test_emulated_geometry_shapes_and_bit_level_properties(emu, fs, n_bands, env_rate):
    """The geometry batch (float64 targets, float32 estimates) against the oracle; then: a pair alone gives the bits it gives in the
    batch, so does the batch reversed with other gaps, the targets alone (n_est = 0) give their bits, and spectrum_out = NULL changes
    no bit of the other outputs."""
    res = np.zeros(9, np.int64)
    emu.modulation_geometry(0, 1, n_bands, 1, P(res))
    c = O.geometry_case(fs, n_bands, env_rate, tile=int(res[6]))
    got = run(c, emu)
    print(fs, n_bands, env_rate, "hop_e %d S %d: worst Ebar %.3g, srmr %.3g, mod_dist %.3g dB, srmr_diff %.3g" % ((c.hop, c.S) + c.check(*got, name="geometry")))
    sig, pair, sx = got
    n_t = len(c.tgts)
    for i, n in enumerate(len(t) for t in c.tgts):
        emu.modulation_geometry(n, c.hop, n_bands, c.S, P(res))
        assert res[0] == O.blocks(n, c.hop) and res[1] == O.frames(int(res[0]), c.S), (i, n, res)
    assert np.isnan(sig[0]).all() and np.isnan(sx[0]).all() and np.isfinite(sig[1:n_t]).all() and np.isnan(pair[0]).all()
    assert np.isfinite(pair[1:, :2]).all() and [[j for j in range(4) if math.isnan(pair[e, j])] for e in (1, 2, 3, 4)] == [[3], [2], [], [2, 3]]
    for e in (1, 2, 3, 5):
        one = run(sub_case(c, [c.index[e]], [e]), emu, gap=0)
        assert one[1].tobytes() == pair[e:e + 1].tobytes() and same_bits([one[0], one[2]], [sig[[c.index[e], n_t + e]], sx[[c.index[e], n_t + e]]]), e
    back = run(sub_case(c, list(range(n_t))[::-1], list(range(len(c.ests)))[::-1]), emu, gap=7)
    assert back[1][::-1].tobytes() == pair.tobytes()
    assert same_bits([back[0][:n_t][::-1], back[0][n_t:][::-1], back[2][:n_t][::-1]], [sig[:n_t], sig[n_t:], sx[:n_t]])
    alone = run(sub_case(c, list(range(n_t)), []), emu)
    assert alone[1].shape == (0, 4) and same_bits([alone[0], alone[2]], [sig[:n_t], sx[:n_t]])
    off = run(c, emu, spec=False)
    assert off[2] is None and same_bits(off[:2], got[:2])


@pytest.mark.parametrize("tdt,edt", [(np.float32, np.float64), (np.float32, np.float32), (np.float64, np.float64)], ids=["f32-f64", "f32", "f64"])
def test_emulated_dtypes_range_and_constant_kstar(emu, tdt, edt):
    """The short geometry batch at 8 kHz in the other dtype combinations; range_db away from its default; kstar as a constant."""
    c = O.geometry_case(8000, 32, short=True, tdt=tdt, edt=edt)
    print(np.dtype(tdt).name, np.dtype(edt).name, "worst Ebar %.3g, srmr %.3g, mod_dist %.3g dB, srmr_diff %.3g" % c.check(*run(c, emu), name="dtypes"))
    base = run(c, emu)
    for rdb, ks in ((35.5, None), (60.0, 6)):
        v = sub_case(c, list(range(len(c.tgts))), list(range(len(c.ests))))
        v.range_db, v.kstar, v.ktab = rdb, ks, O.kstar_table(c.fc, ks)
        got = run(v, emu)
        v.check(*got, name="range %s kstar %s" % (rdb, ks))
        assert got[2].tobytes() == base[2].tobytes() and (ks is None or (np.all(got[0][1:len(c.tgts), 1] == 6) and not np.array_equal(got[0], base[0])))


def test_emulated_silence_identity_and_gain(emu):
    """A silent target: NaN for the pair, srmr NaN, sum Ebar 0.  A silent estimate: NaN for the pair (the level factor is infinite).  A
    denormal estimate: NaN, no infinity.  Estimate = target: srmr_diff and mod_dist are 0 exactly.  A gain of a power of two keeps
    every bit of srmr; 0.3 keeps it within 1e-12 and keeps mod_dist."""
    hop = O.hop_e(FS)
    x = O.voiced(6000, FS, 5)
    y = O.reverberated(x, FS, 6, 0.2)
    z = np.zeros(6000)
    # (1e-148 y against 1e10 x: every Ebar is a normal number and the level factor overflows - the pair's NaN rule, no infinity)
    c = O.Case([x, z, 0.25 * x, 0.3 * x, 1e10 * x], [z, x.copy(), y, 0.5 * y, y, 1e-148 * y, 0.3 * y, 3e38 * y], [0, 0, 0, 0, 1, 4, 0, 0], FS, hop,
               splits=[9] * 8)
    sig, pair, sx = run(c, emu)
    c.check(sig, pair, sx, name="silence")
    n_t = 5
    assert np.isnan(sig[1, :3]).all() and sig[1, 3] == 0.0 and not np.any(sx[1]) and np.isnan(sig[n_t, :3]).all() and sig[n_t, 3] == 0.0
    assert np.isnan(pair[0]).all() and np.isnan(pair[4]).all() and np.isnan(pair[5]).all() and np.isfinite(sig[n_t + 5]).all()
    assert not np.isinf(sig).any() and not np.isinf(pair).any() and not np.isinf(sx).any()
    assert pair[1, 0] == 0.0 and pair[1, 1] == 0.0 and pair[1, 2] == 0.0 and pair[1, 3] == 0.0
    assert sig[2, :3].tobytes() == sig[0, :3].tobytes() and sig[n_t + 3, :3].tobytes() == sig[n_t + 2, :3].tobytes() and pair[3].tobytes() == pair[2].tobytes()
    for a, b in ((sig[3], sig[0]), (sig[4], sig[0]), (sig[n_t + 6], sig[n_t + 2]), (sig[n_t + 7], sig[n_t + 2])):
        assert abs(a[0] / b[0] - 1.0) <= 1e-12 and a[1:3].tobytes() == b[1:3].tobytes()
    assert np.max(np.abs(pair[6] - pair[2])) <= 1e-9 and np.max(np.abs(pair[7] - pair[2])) <= 1e-9 and pair[2, 1] > 1.0
    res = np.zeros(9, np.int64)
    emu.modulation_geometry(48000 * 4, 30, 32, 102, P(res))
    assert list(res) == [6400, 59, 800, 100, 8, 8, 32, 65536, 1024]
    tab = np.zeros(40 + 408)
    emu.modulation_tables(P(c.mod), 102, P(tab))
    assert tab[:40].tobytes() == c.mod.tobytes() and np.max(np.abs(tab[40:] - O.hamming(408))) <= 1e-15 and abs(tab[40] - 0.08) < 1e-15


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first
_COEF = A.design(FS, 32)[1]
_MOD = O.mod_design(1600.0)
_KSTAR = O.kstar_table(A.design(FS, 32)[0])


def _call(lib, lens, index, hop=10, coef=_COEF, n_bands=None, mod=_MOD, S=102, kstar=_KSTAR, range_db=60.0, split=None, n_tgt=None, n_est=None,
          tgt=_DUMMY, est=_DUMMY, toff=_DUMMY, eoff=_DUMMY, sig=_DUMMY, pair=_DUMMY, ws=_DUMMY, ws_bytes=1 << 40, null=()):
    ln, ix = np.ascontiguousarray(lens, np.int32), np.ascontiguousarray(index, np.int32)
    cf, md, ks = np.ascontiguousarray(coef, np.float64), np.ascontiguousarray(mod, np.float64), np.ascontiguousarray(kstar, np.int32)
    sp = np.full(len(ix), -1, np.int32) if split is None else np.ascontiguousarray(split, np.int32)
    return lib.ssr_modulation(tgt, 0, toff, None if "len" in null else P(ln), len(ln) if n_tgt is None else n_tgt, est, 0, eoff,
                              None if "index" in null else P(ix), len(ix) if n_est is None else n_est, hop, len(cf) if n_bands is None else n_bands,
                              None if "coef" in null else P(cf), None if "mod" in null else P(md), S, None if "kstar" in null else P(ks), range_db,
                              None if "split" in null else P(sp), sig, pair, None, ws, ws_bytes, None)


def test_modulation_rejects_bad_arguments_before_launch():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E = _lib.ERR_INVALID_ARG
    for hop in (0, -1, -10):
        assert _call(lib, [8000], [0], hop=hop) == E and "hop_e" in err()
    for nb in (0, 2, 65, -3):
        assert _call(lib, [8000], [0], n_bands=nb) == E and "n_bands" in err()
    for S in (0, -1, 1025):
        assert _call(lib, [8000], [0], S=S) == E and "S must" in err()
    for rdb in (0.0, -3.0, 150.5, float("nan"), float("inf")):
        assert _call(lib, [8000], [0], range_db=rdb) == E and "range_db" in err()
    for j, v in ((0, 1.0), (1, 1.0), (0, float("nan")), (2, float("inf"))):
        bad = _COEF.copy()
        bad[7, j] = v
        assert _call(lib, [8000], [0], coef=bad) == E and "coef" in err(), (j, v)
    for j, v in ((0, float("nan")), (1, float("inf")), (2, float("-inf")), (3, float("nan")), (4, float("nan")), (4, 1.0), (3, 2.5)):
        bad = _MOD.copy()
        bad[5, j] = v
        assert _call(lib, [8000], [0], mod=bad) == E and "mod must" in err(), (j, v)
    for v in (4, 9, 0, -1):
        bad = _KSTAR.copy()
        bad[31] = v
        assert _call(lib, [8000], [0], kstar=bad) == E and "kstar" in err(), v
    for sp in (-2, 33, 100):
        assert _call(lib, [8000], [0], split=[sp]) == E and "split_band" in err()
    assert _call(lib, [8000, -1], [0]) == E and "lengths" in err()
    assert _call(lib, [1 << 29], [0]) == E and "lengths" in err()
    assert _call(lib, [8000], [1]) == E and "tgt_index" in err()
    assert _call(lib, [8000], [-1]) == E and "tgt_index" in err()
    assert _call(lib, [8000], [0], n_tgt=-1) == E and _call(lib, [8000], [0], n_est=-1) == E
    for name in ("len", "index", "coef", "mod", "kstar", "split"):
        assert _call(lib, [8000], [0], null=(name,)) == E and "null" in err(), name
    for kw in ({"tgt": None}, {"est": None}, {"toff": None}, {"eoff": None}, {"sig": None}, {"pair": None}):
        assert _call(lib, [8000], [0], **kw) == E and "null" in err(), kw
    ln, ix = np.array([8000, 0, 19, 4080], np.int32), np.array([0, 0, 3], np.int32)
    need = lib.ssr_modulation_workspace_bytes(P(ln), 4, P(ix), 3, 10, 32)
    assert need > 0 and lib.ssr_modulation_workspace_bytes(P(ln), 4, P(ix), 0, 10, 32) < need
    assert _call(lib, ln, ix, ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in err()
    assert _call(lib, ln, ix, ws=None) == _lib.ERR_WORKSPACE
    for bad in ((P(ln), 4, P(ix), 3, 0, 32), (P(ln), 4, P(ix), 3, 10, 2), (P(ln), 4, P(ix), 3, 10, 65), (None, 4, P(ix), 3, 10, 32),
                (P(ln), -1, P(ix), 3, 10, 32), (P(ln), 2, P(ix), 3, 10, 32)):
        assert lib.ssr_modulation_workspace_bytes(*bad) == 0
    # the block limit: 65536 envelope samples fit, 65537 do not - refused before anything is enqueued
    assert lib.ssr_modulation_workspace_bytes(P(np.array([65536 * 30 + 29], np.int32)), 1, P(ix), 0, 30, 32) > 0
    assert _call(lib, [65537 * 10], [0]) == _lib.ERR_UNSUPPORTED and "65536" in err()
    assert lib.ssr_modulation_workspace_bytes(P(np.array([65537], np.int32)), 1, P(ix), 0, 1, 32) == 0
    # about 3.3 MB per 4 s signal at 48 kHz and 32 bands
    four = lib.ssr_modulation_workspace_bytes(P(np.array([192000] * 9, np.int32)), 9, P(ix), 0, 30, 32) - \
        lib.ssr_modulation_workspace_bytes(P(np.array([192000], np.int32)), 1, P(ix), 0, 30, 32)
    assert 3.2e6 < four / 8 < 3.4e6
    assert _call(lib, [], [], tgt=None, est=None, toff=None, eoff=None, sig=None, pair=None, ws=None, ws_bytes=0) == 0      # nothing queued


def test_header_ctypes_table_and_library_agree():
    from ssr_eval_amd import _lib
    path = os.path.join(ROOT, "ssr_eval_amd", "csrc", "ssr_hip_modulation.h")
    header = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    declared = set(re.findall(r"\b(ssr_[a-z_0-9]+)\s*\(", header))
    assert declared == {"ssr_modulation", "ssr_modulation_workspace_bytes"} == set(_lib.MODULATION_SIGNATURES)
    others = set(_lib.SIGNATURES) | set(_lib.COHERENCE_SIGNATURES) | set(_lib.LOUDNESS_SIGNATURES) | set(_lib.SPECTRUM_SIGNATURES) | \
        set(_lib.AUDITORY_SIGNATURES)
    assert not set(_lib.MODULATION_SIGNATURES) & others
    assert "#define SSR_MODULATION_BANDS 8" in header and "#define SSR_MODULATION_MAX_BLOCKS 65536" in header
    assert (_lib.MODULATION_BANDS, _lib.MODULATION_MAX_BLOCKS) == (8, 65536)
    n_args = len([a for a in re.search(r"int ssr_modulation\((.*?)\);", header, flags=re.S).group(1).split(",")])
    assert n_args == len(_lib.MODULATION_SIGNATURES["ssr_modulation"][1]) == 24
    lib = _lib.load()
    for name, (res, args) in _lib.MODULATION_SIGNATURES.items():
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    main = open(os.path.join(ROOT, "include", "ssr_hip.h")).read()
    inc = "#include \"../ssr_eval_amd/csrc/ssr_hip_modulation.h\""
    assert main.count(inc) == 1 and main.index(inc) > main.index("#include \"../ssr_eval_amd/csrc/ssr_hip_auditory.h\"")
    assert os.listdir(os.path.join(ROOT, "include")) == ["ssr_hip.h"]
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T ssr_modulation\n" in exported and " T ssr_modulation_workspace_bytes\n" in exported
    # the header is C99 on its own behind the main one
    src = "#include \"%s\"\nint main(void) { return ssr_modulation_workspace_bytes(0, 0, 0, 0, 30, 32) != 0 || SSR_MODULATION_BANDS != 8; }\n" % \
        os.path.join(ROOT, "include", "ssr_hip.h")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-"], input=src, text=True, check=True)


# ---- AudioMetrics / SSR_Eval_Helper options --------------------------------------------------------------------------------------
def test_audio_metrics_modulation_options():
    """Everything here is refused before any device is touched (this test runs without one)."""
    from ssr_eval_amd import AudioMetrics
    from ssr_eval_amd import backend as B
    assert [B.modulation_hop(fs) for fs in (8000, 16000, 44100, 48000)] == [5, 10, 27, 30]
    assert (B.modulation_hop(48000, 800), B.modulation_hop(48000, 6400), B.modulation_hop(8000, 6400), B.modulation_hop(500, 800)) == (60, 7, 1, 1)
    for fs, nb, env in ((8000, 32, 1600), (16000, 3, 800), (44100, 64, 1600), (48000, 32, 6400)):
        hop = B.modulation_hop(fs, env)
        fc, coef, mod, S, ktab = B.modulation_design(fs, hop, nb)
        fo, co = A.design(fs, nb)
        assert coef.shape == (nb, 3) and np.max(np.abs(fc - fo)) <= 1e-9 and np.max(np.abs(coef - co)) <= 1e-14
        assert mod.shape == (8, 5) and mod.dtype == np.float64 and np.max(np.abs(mod - O.mod_design(fs / hop))) <= 1e-15 and S == O.frame_step(fs / hop)
        assert ktab.dtype == np.int32 and np.array_equal(ktab, O.kstar_table(fo))
    assert list(B.modulation_design(16000, 10, 5, None, 7)[4]) == [7] * 5
    assert B.check_modulation_env_rate(800) == 800 and B.check_modulation_env_rate(6400.0) == 6400.0 and B.check_modulation_range(150) == 150.0
    assert B.check_modulation_kstar(None) is None and B.check_modulation_kstar(8) == 8
    for bad in (799, 6401, True, None, "1600", float("nan"), float("inf")):
        with pytest.raises(ValueError):
            B.check_modulation_env_rate(bad)
    for bad in (4, 9, 6.0, True, "6"):
        with pytest.raises(ValueError):
            B.check_modulation_kstar(bad)
    for bad in (0, -1.0, 150.1, True, None, "60", float("nan")):
        with pytest.raises(ValueError):
            B.check_modulation_range(bad)
    for args in ((16000, 0), (16000, 1.5), (16000, True), (16000, 41), (300, 1), (16000, 10, 2), (16000, 10, 32, (0.0, 100.0)), (16000, 10, 32, None, 4)):
        with pytest.raises(ValueError):
            B.modulation_design(*args)
    x = np.zeros(6000, np.float32)
    am = AudioMetrics(16000)
    fc, _ = B.gammatone_design(16000)
    names = ("srmr", "srmr_diff", "mod_dist", "mod_dist_hf", "mod_dist_lf")
    assert am._modulation_names(None) == names and am._modulation_names(["mod_dist", "srmr"]) == ("srmr", "mod_dist")
    assert am._modulation_splits(fc, None, 2) == [-1, -1] and am._modulation_splits(fc, 2000.0, 2) == [O.split_band(fc, 2000.0)] * 2
    assert am._modulation_splits(fc, [None, 1e9, 0.0, float(fc[7])], 4) == [-1, 32, 0, 7]
    for kw in ({"n_bands": 2}, {"n_bands": 65}, {"n_bands": 32.0}, {"band": (0.0, 1000.0)}, {"band": (50.0, 8000.0)}, {"env_rate": 100}, {"env_rate": 7000},
               {"env_rate": "1600"}, {"range_db": 0}, {"range_db": 151}, {"range_db": "60"}, {"kstar": 4}, {"kstar": 9}, {"kstar": 6.5},
               {"return_spectrum": 1}, {"split_hz": -1.0}, {"split_hz": "4000"}, {"split_hz": [4000.0, 2000.0]}, {"split_hz": float("inf")},
               {"split_hz": True}, {"names": ()}, {"names": "srmr"}, {"names": ("nope",)}):
        with pytest.raises(ValueError):
            am.modulation_batch([x], [x], **kw)
    for kw in ({"n_bands": 2}, {"env_rate": 100}, {"kstar": 4}, {"return_spectrum": "yes"}, {"band": (1, 2, 3)}):
        with pytest.raises(ValueError):
            am.srmr(x, **kw)
    with pytest.raises(ValueError):
        am.modulation_multi([[x], [x]], [x], split_hz=[1000.0])
    with pytest.raises(ValueError):
        am.modulation(np.zeros((2, 6000), np.float32), np.zeros(6000, np.float32))
    with pytest.raises(ValueError):
        am.srmr(np.zeros((2, 6000), np.float32))
    for kw in ({"split_bands": [-2]}, {"split_bands": [33]}, {"split_bands": [1, 2]}, {"range_db": -1}, {"n_bands": 100}, {"hop_e": 0}, {"hop_e": 1.5},
               {"env_rate": 10}, {"kstar": 3}, {"return_spectrum": "yes"}):
        with pytest.raises(ValueError):
            B.modulation_metrics([x], [x], [0], 16000, **kw)
    with pytest.raises(ValueError):
        B.modulation_metrics([x], [x], [1], 16000)
    with pytest.raises(ValueError):
        B.modulation_metrics([x], [x], [0, 0], 16000)
    assert B.MODULATION_WORKSPACE_CAP == 1 << 30


def test_helper_modulation_option_and_key_order():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd import eval as E
    mk = lambda sr=44100, **kw: SSR_Eval_Helper(BasicTestee(), sr, sr, evaluation_sr=sr, test_data_root=None, **kw)      # noqa: E731
    assert mk().modulation is None and mk(modulation=None).modulation is None and mk(modulation=True).modulation is True
    ok = {"n_bands": 24, "band": (100.0, 18000.0), "env_rate": 3200, "range_db": 50.0, "kstar": 6, "split": 4000.0}
    assert mk(modulation=ok).modulation == ok and mk(modulation={"split": 8000}).modulation == {"split": 8000}
    for bad in (False, 1, "all", "srmr", (), ("srmr",), {}, {"which": "srmr"}, [True], {"n_bands": 2}, {"n_bands": 65}, {"n_bands": 32.5},
                {"band": (30000.0, 40000.0)}, {"band": (0.0, 100.0)}, {"split": None}, {"split": -5.0}, {"split": "4000"}, {"split": [4000.0]},
                {"split": float("inf")}, {"range_db": 0.0}, {"range_db": 200}, {"env_rate": 799}, {"env_rate": 6401}, {"env_rate": None},
                {"kstar": 4}, {"kstar": 9}, {"kstar": None}, {"kstar": 6.0}, {"match_level": True}, {"hop_e": 30}):
        with pytest.raises(ValueError):
            mk(modulation=bad)
    params = inspect.signature(SSR_Eval_Helper.__init__).parameters
    assert params["modulation"].kind is inspect.Parameter.KEYWORD_ONLY and list(params)[-4:] == ["auditory", "modulation", "loudness", "bandwidth"]
    # the family's row sits in the open-ended tail between bandwidth and auditory, whose keys still end full_key_order()
    tail = [f.option for f in E._TAIL_FAMILIES]
    assert tail == ["loudness", "bandwidth", "modulation", "auditory"]
    fam = E._TAIL_FAMILIES[tail.index("modulation")]
    assert fam.keys == ("srmr", "srmr_diff", "mod_dist", "mod_dist_hf") and fam.per_key is True
    assert (fam.multi, fam.batch) == ("modulation_multi", "modulation_batch")
    assert "modulation" not in [f.option for f in E._FAMILIES + E._LATER_FAMILIES]
    full = E.full_key_order()
    assert full[:len(E.all_key_order())] == E.all_key_order() and len(set(full)) == len(full) and full[-2:] == ("nsim", "nsim_hf")
    assert full[len(E.all_key_order()):] == tuple(k for f in E._TAIL_FAMILIES for k in f.keys) and full[-6:-2] == fam.keys
    keys = ["proc_fft_8000_44100", "proc_mp3_32k_44100"]
    args, kw = fam.arguments(mk(modulation=True), keys)
    assert args == ([4000.0, None], 32, None, 1600, 60.0, None) and kw == {"names": fam.keys}
    args, kw = fam.arguments(mk(modulation=ok), keys)
    assert args == ([4000.0, 4000.0], 24, (100.0, 18000.0), 3200, 50.0, 6)
