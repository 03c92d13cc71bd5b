"""CPU tests of the loudness family (lufs, lra, lufs_m_max, lufs_s_max, peak_db, true_peak_db): the float64
oracle (tests/loudness_oracle.py) pinned to BS.1770-4's tables and to its anchors, a g++ build of the kernel bodies
(ssr_loudness.h) against the oracle - the input list, the shapes where the geometry can go wrong, the exact facts, the bit-level
properties -, the C ABI's argument checks (they return before anything touches a device), the header / ctypes table / library
agreement, and AudioMetrics / SSR_Eval_Helper(loudness=...) validation and key order.

Bars (loudness_oracle.TOL_*): E[s] within 1e-10 of the signal's largest sub-block energy, the four loudness values within 1e-6 LU,
true_peak_db within 1e-9 dB, peak_db within 1e-12 dB.  An input of the list must keep every block 1e-3 LU from a gate and the
values next to the two loudness-range ranks 1e-6 LU apart (loudness_oracle.assert_conditioned): where that fails the input is
wrong, not the kernel.  Worst differences seen in emulation: E 7.7e-15, loudness 8.9e-15 LU, true peak 3.6e-15 dB, peak 0."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import loudness_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle's pins ------------------------------------------------------------------------------------------------------------
def test_oracle_coefficients_are_bs1770s_at_48k_and_anchors_hold():
    (b1, a1), (b2, a2) = O.k_weighting(48000)
    worst = max(np.max(np.abs(b1 - O.B1_48K)), np.max(np.abs(a1 - O.A1_48K)), np.max(np.abs(b2 - O.B2_48K)), np.max(np.abs(a2 - O.A2_48K)))
    print("worst coefficient difference to the tables at 48 kHz", worst)
    assert worst <= 1e-15
    for fs, want in O.ANCHORS.items():
        got = O.analyse(np.sin(2 * np.pi * 997 * np.arange(5 * fs) / fs), fs)["lufs"]
        print(fs, got, want)
        assert abs(got - want) <= 1e-3
    assert [O.sub_len(fs) for fs in (8000, 11025, 22050, 44100, 48000)] == [800, 1103, 2205, 4410, 4800]
    assert [O.rank(m, p) for m, p in ((1, 10), (1, 95), (2, 95), (11, 10), (11, 95), (64, 10), (64, 95))] == [0, 0, 1, 1, 10, 6, 60]


def test_oracle_nan_rules_and_the_sine_at_a_quarter_of_the_rate():
    fs = 16000
    rng = np.random.default_rng(5)
    x = 0.1 * rng.standard_normal(4 * fs)
    h = O.sub_len(fs)
    assert np.isnan(O.row(x[:4 * h - 1], fs)[:4]).all() and np.isfinite(O.row(x[:4 * h - 1], fs)[4:]).all()      # S = 3
    r = O.row(x[:4 * h], fs)                                                                                 # S = 4
    assert np.isfinite(r[[0, 2, 4, 5]]).all() and np.isnan(r[[1, 3]]).all()
    assert np.isnan(O.row(x[:30 * h - 1], fs)[[1, 3]]).all() and np.isfinite(O.row(x[:30 * h], fs)).all()      # S = 29, 30
    assert np.isnan(O.row(np.zeros(4 * fs), fs)).all() and np.isnan(O.row(np.zeros(0), fs)).all()
    assert np.isnan(O.row(1e-5 * x, fs)[:4]).all()                                                           # nothing above -70
    d = O.analyse(O.quarter_rate_sine(fs), fs)
    print("fs / 4 sine: peak %.4f dB, true peak %.4f dBTP" % (d["peak_db"], d["true_peak_db"]))
    assert abs(d["peak_db"] + 3.0103) < 1e-3 and abs(d["true_peak_db"]) < 0.2


# ---- the kernel bodies compiled for the host ------------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "loudness_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libloudness_emu.so")
P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    return C.CDLL(EMU_SO)


def run_emu(lib, sigs, fs, blocks=True, gap=0):
    """-> (out [n, 6], [E of each signal] or None); gap: unused samples between the signals"""
    dt = sigs[0].dtype if sigs else np.float32
    ln = np.array([len(s) for s in sigs], np.int32)
    off = (np.cumsum(ln + gap) - ln).astype(np.int64)
    data = np.full(int((ln + gap).sum()) + 1, np.nan, dt)
    for o, s in zip(off, sigs):
        data[o:o + len(s)] = s
    out = np.full((len(sigs), 6), -123.0)
    S = ln // O.sub_len(fs)
    bo = (np.cumsum(S) - S).astype(np.int64)
    bl = np.full(int(S.sum()) + 1, -5.0)
    assert lib.loudness_emu(P(data), int(dt == np.float64), P(off), P(ln), len(sigs), fs, P(out), P(bo), P(bl) if blocks else None) == 0
    assert bl[-1] == -5.0
    return out, ([bl[o:o + s] for o, s in zip(bo, S)] if blocks else None)


@pytest.fixture(scope="module")
def inputs():
    """The input list, computed once: (rate, name) -> float64 signal."""
    got = {}
    for fs in O.RATES:
        got[fs, "levels"] = O.piecewise_noise(fs)
        got[fs, "silence"] = O.noise_with_silence(fs)
        got[fs, "sine"] = O.quarter_rate_sine(fs)
    return got


@pytest.mark.parametrize("fs", O.RATES)
def test_emulated_kernels_match_the_oracle_on_the_input_list(emu, inputs, fs):
    """Piecewise-level noise (both momentary gates remove blocks), noise around 4.6 s of silence (all four gates do), the fs / 4
    sine, as float64 and as float32 signals, in one batch per dtype."""
    names = ("levels", "silence", "sine")
    c = O.conditioning(inputs[fs, "levels"], fs)
    print(fs, "levels: removed", c[:4], "gate margin %.3g LU, rank gap %.3g LU" % c[4:])
    assert c[0] >= 1 and c[1] >= 1 and c[4] >= O.GATE_MARGIN and c[5] >= O.RANK_MARGIN
    c = O.assert_conditioned(inputs[fs, "silence"], fs, "silence")
    print(fs, "silence: removed", c[:4], "gate margin %.3g LU, rank gap %.3g LU" % c[4:])
    for dt in (np.float64, np.float32):
        sigs = [inputs[fs, k].astype(dt) for k in names]
        out, E = run_emu(emu, sigs, fs)
        for k, s, o, e in zip(names, sigs, out, E):
            worst = O.check(o, e, s, fs, k)
            print(fs, k, np.dtype(dt).name, "worst E %.3g, loudness %.3g LU, true peak %.3g dB, peak %.3g dB" % worst)
    assert abs(out[2, 4] + 3.0103) < 1e-3 and abs(out[2, 5]) < 0.2


@pytest.mark.parametrize("fs,dt", [(44100, np.float32), (44100, np.float64), (8000, np.float32), (48000, np.float64)],
                         ids=["44k1-f32", "44k1-f64", "8k-f32", "48k-f64"])
def test_emulated_geometry_shapes_and_bit_level_properties(emu, fs, dt):
    """The geometry cases in ONE batch (at 44.1 kHz the eight segments of a sub-block have two lengths, 551 and 552) against the
    oracle; then: a signal alone, in the reversed batch and with other gaps between the signals gives the bits it gives in the
    batch, and blocks_out = NULL changes no bit of out."""
    sigs = O.geometry_signals(fs, dt)
    out, E = run_emu(emu, sigs, fs)
    for i, s in enumerate(sigs):
        worst = O.check(out[i], E[i], s, fs, "signal %d (n = %d)" % (i, len(s)))
    print("last signal: worst E %.3g, loudness %.3g LU, true peak %.3g dB, peak %.3g dB" % worst)
    assert np.isnan(out[[0, 1], :4]).all() and np.isnan(out[7]).all() and np.isnan(out[10]).all() and np.isnan(out[11]).all()
    assert np.isfinite(out[2, [0, 2, 4, 5]]).all() and np.isnan(out[[2, 3, 4]][:, [1, 3]]).all() and np.isfinite(out[[5, 6, 12]]).all()
    assert np.isfinite(out[[8, 9], 4:]).all()
    for i in (2, 6, 9, 12):
        alone, Ea = run_emu(emu, [sigs[i]], fs)
        assert alone.tobytes() == out[i:i + 1].tobytes() and Ea[0].tobytes() == E[i].tobytes(), i
    back, Eb = run_emu(emu, sigs[::-1], fs, gap=3)
    assert back[::-1].tobytes() == out.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(Eb[::-1], E))
    assert run_emu(emu, sigs, fs, blocks=False, gap=1)[0].tobytes() == out.tobytes()


def test_emulated_exact_facts(emu, inputs):
    """Scaling by a power of two moves lufs, the two maxima and the two peaks by 20 log10 of it and leaves lra where it is: every
    operation before the logarithms is exact under the scaling, so two results differ by the roundings of log10, of its product
    with 10 or 20 and of the sum with -0.691 - four roundings of values below 128: 4 ulp(128) is the bar.  (The input holds no
    digital silence: a filter state that decays into the subnormal range does not scale exactly.)  All-zero input: NaN."""
    fs = 22050
    x = inputs[fs, "levels"] * 0.5
    bar = 4 * np.spacing(128.0)
    base, Eb = run_emu(emu, [x], fs)
    for k in (-3, 1, 4):
        got, E = run_emu(emu, [x * 2.0 ** k], fs)
        shift = 20.0 * np.log10(2.0) * k
        d = got[0] - base[0] - np.array([shift, 0.0, shift, shift, shift, shift])
        print(k, d)
        assert np.max(np.abs(d)) <= bar and np.array_equal(E[0], Eb[0] * 4.0 ** k)
    z, Ez = run_emu(emu, [np.zeros(3 * fs + 5, np.float32)], fs)
    assert np.isnan(z).all() and not np.any(Ez[0]) and len(Ez[0]) == 30


def test_emulated_tables_and_limits(emu):
    """The filter of the oversampled peak is scipy.signal.resample_poly's; the coefficients are the oracle's; a signal of more than
    6144 sub-blocks and a rate outside 8 .. 192 kHz are refused; 6000 sub-blocks (10 minutes) are taken."""
    from scipy.signal import firwin
    geo = np.zeros(7, np.int64)
    for fs in (8000, 44100, 48000, 192000):
        emu.loudness_geometry(fs, P(geo))
        tab = np.zeros(int(geo[4]))
        emu.loudness_tables(fs, P(tab))
        (b1, a1), (b2, a2) = O.k_weighting(fs)
        assert geo[0] == O.sub_len(fs) and np.max(np.abs(tab[:10] - np.concatenate((b1, a1[1:], b2, a2[1:])))) <= 1e-15
        taps = 4.0 * firwin(81, 0.25, window=("kaiser", 5.0))
        assert np.max(np.abs(tab[geo[6]:geo[6] + 81] - taps)) <= 1e-15
    assert geo[1] == 8 and geo[2] == 6144
    out = np.zeros(6)
    ln, off = np.array([800 * 6145], np.int32), np.zeros(1, np.int64)
    x = np.zeros(800 * 6145 + 1, np.float32)
    assert emu.loudness_emu(P(x), 0, P(off), P(ln), 1, 8000, P(out), None, None) == -2
    assert emu.loudness_emu(P(x), 0, P(off), P(ln), 1, 7999, P(out), None, None) == -2
    rng = np.random.default_rng(3)
    long = (0.05 * rng.standard_normal(800 * 6000 + 17)).astype(np.float32)
    long[800 * 2000:800 * 2500] *= 0.01
    got, E = run_emu(emu, [long], 8000)
    print("10 minutes at 8 kHz: worst", O.check(got[0], E[0], long, 8000, "10 minutes"))


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _call(lib, lens, rate=48000, n_sig=None, sig=_DUMMY, off=_DUMMY, out=_DUMMY, boff=None, blocks=None, ws=_DUMMY, ws_bytes=1 << 40,
          null_len=False):
    ln = np.ascontiguousarray(lens, np.int32)
    return lib.ssr_loudness(sig, 0, off, None if null_len else P(ln), len(ln) if n_sig is None else n_sig, rate, out, boff, blocks, ws,
                            ws_bytes, None)


def test_loudness_rejects_bad_arguments_before_launch():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E = _lib.ERR_INVALID_ARG
    for rate in (0, -48000, 7999, 192001, 1 << 30):
        assert _call(lib, [4000], rate=rate) == E and "rate" in err()
    assert _call(lib, [4000], n_sig=-1) == E and "n_sig" in err()
    assert _call(lib, [4000], null_len=True) == E and "null" in err()
    assert _call(lib, [4000, -1]) == E and "lengths" in err()
    assert _call(lib, [1 << 29]) == E and "lengths" in err()
    assert _call(lib, [4800 * 6145]) == _lib.ERR_UNSUPPORTED and "6144" in err()
    assert _call(lib, [4000], out=None) == E and "null" in err()
    assert _call(lib, [4000], off=None) == E and "null" in err()
    assert _call(lib, [4000], sig=None) == E and "null" in err()
    assert _call(lib, [4000], blocks=_DUMMY) == E and "null" in err()                        # blocks_out without blocks_off
    bo = np.array([0, -1], np.int64)
    assert _call(lib, [4000, 9000], boff=P(bo), blocks=_DUMMY) == E and "blocks_off" in err()
    ln = np.array([48000, 4800 * 6144, 0], np.int32)
    need = lib.ssr_loudness_workspace_bytes(P(ln), 3, 48000)
    assert need > 0 and lib.ssr_loudness_workspace_bytes(P(ln), 3, 8000) == 0                 # (more than 6144 sub-blocks at 8 kHz)
    assert _call(lib, ln, ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in err()
    assert _call(lib, ln, ws=None) == _lib.ERR_WORKSPACE
    assert lib.ssr_loudness_workspace_bytes(P(ln), 3, 7999) == 0 and lib.ssr_loudness_workspace_bytes(P(ln), -1, 48000) == 0
    assert lib.ssr_loudness_workspace_bytes(None, 1, 48000) == 0
    neg = np.array([5, -2], np.int32)
    assert lib.ssr_loudness_workspace_bytes(P(neg), 2, 48000) == 0
    assert _call(lib, [], n_sig=0, sig=None, off=None, out=None, ws=None, ws_bytes=0) == 0         # nothing to measure: nothing queued


def test_header_ctypes_table_and_library_agree():
    from ssr_eval_amd import _lib
    path = os.path.join(ROOT, "ssr_eval_amd", "csrc", "ssr_hip_loudness.h")
    header = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    declared = set(re.findall(r"\b(ssr_[a-z_0-9]+)\s*\(", header))
    assert declared == {"ssr_loudness", "ssr_loudness_workspace_bytes"} == set(_lib.LOUDNESS_SIGNATURES)
    assert not set(_lib.LOUDNESS_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.COHERENCE_SIGNATURES))
    lib = _lib.load()
    for name, (res, args) in _lib.LOUDNESS_SIGNATURES.items():
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    main = open(os.path.join(ROOT, "include", "ssr_hip.h")).read()
    inc = "#include \"../ssr_eval_amd/csrc/ssr_hip_loudness.h\""
    assert main.count(inc) == 1 and main.index(inc) > main.index("#include \"../ssr_eval_amd/csrc/ssr_hip_coherence.h\"")
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T ssr_loudness\n" in exported and " T ssr_loudness_workspace_bytes\n" in exported
    # the header is C99 on its own behind the main one
    src = "#include \"%s\"\nint main(void) { return ssr_loudness_workspace_bytes(0, 0, 48000) != 0; }\n" % os.path.join(ROOT, "include", "ssr_hip.h")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-"], input=src, text=True, check=True)


# ---- AudioMetrics / SSR_Eval_Helper options --------------------------------------------------------------------------------------
def test_audio_metrics_loudness_options():
    """Everything here is refused before any device is touched (this test runs without one)."""
    from ssr_eval_amd import AudioMetrics
    from ssr_eval_amd import backend as B
    assert B.check_loudness_rate(48000) == 48000 and B.check_loudness_rate(np.int64(8000)) == 8000 and B.check_loudness_rate(44100.0) == 44100
    for bad in (7999, 192001, 0, -44100, 44100.5, True, None, "48000", float("nan")):
        with pytest.raises(ValueError):
            B.check_loudness_rate(bad)
    assert [B.loudness_sub_len(fs) for fs in (8000, 11025, 44100)] == [800, 1103, 4410]
    x = np.zeros(3000, np.float32)
    for rate in (4000, 200000, 22050.5):
        with pytest.raises(ValueError):
            AudioMetrics(rate).loudness(x)
        with pytest.raises(ValueError):
            B.loudness_metrics([x], rate)
    am = AudioMetrics(16000)
    assert am._loudness_names(None, False) == ("lufs", "lra", "lufs_m_max", "lufs_s_max", "peak_db", "true_peak_db")
    assert am._loudness_names(None, True)[6:] == ("lufs_diff", "lra_diff", "true_peak_diff")
    assert am._loudness_names(["true_peak_db", "lufs"], False) == ("lufs", "true_peak_db")
    for kw in ({"names": ()}, {"names": "lufs"}, {"names": ("lufs_diff",)}, {"names": ("loud",)}, {"return_blocks": 1}, {"return_blocks": None}):
        with pytest.raises(ValueError):
            am.loudness_batch([x], **kw)
    with pytest.raises(ValueError):
        am.loudness_batch([x], [x], names=("lufs", "nope"))
    with pytest.raises(ValueError):
        am.loudness_multi([[x]], [x], return_blocks="yes")
    with pytest.raises(ValueError):
        am.loudness(np.zeros((2, 100), np.float32))


def test_helper_loudness_option_and_key_order():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd import eval as E
    mk = lambda sr=44100, **kw: SSR_Eval_Helper(BasicTestee(), sr, sr, evaluation_sr=sr, test_data_root=None, **kw)      # noqa: E731
    assert mk().loudness is None and mk(loudness=None).loudness is None and mk(loudness=True).loudness is True
    for bad in (False, 1, "all", "lufs", (), ("lufs",), {}, {"which": "lufs"}, [True]):
        with pytest.raises(ValueError):
            mk(loudness=bad)
    with pytest.raises(ValueError):
        mk(sr=4000, loudness=True)
    assert mk(sr=4000).loudness is None                                     # (the rate matters only where the option is on)
    # the family is a member of the open-ended tail and its four keys follow all_key_order(); nothing here says it is the only one
    tail = [f.option for f in E._TAIL_FAMILIES]
    assert "loudness" in tail
    fam = E._TAIL_FAMILIES[tail.index("loudness")]
    assert fam.keys == ("lufs", "lufs_diff", "true_peak_db", "true_peak_diff") and fam.per_key is False and "lra" not in fam.keys
    full = E.full_key_order()
    assert full[:len(E.all_key_order())] == E.all_key_order() and len(set(full)) == len(full)
    at = full.index("lufs")
    assert at >= len(E.all_key_order()) and full[at:at + 4] == fam.keys
    assert full[len(E.all_key_order()):] == tuple(k for f in E._TAIL_FAMILIES for k in f.keys)
    assert fam.arguments(mk(loudness=True), ["proc_fft_8000_44100"]) == ((), {"names": fam.keys})
    assert (fam.multi, fam.batch) == ("loudness_multi", "loudness_batch")
