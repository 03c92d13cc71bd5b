"""CPU tests of the DTW-aligned mel-cepstral distortion (mcd_dtw, dtw_dev, dtw_len): properties of the float64 oracle
(tests/mel_dtw_oracle.py), a g++ build of the kernel bodies (ssr_mel_dtw.h) against it - the warp alone on injected cepstra whose
arithmetic both sides do alike, so that ties fall alike, and the whole chain on oracle magnitude images - the C ABI's argument
checks (they return before anything touches a device) and SSR_Eval_Helper(mel_dtw=...) validation."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import mel_dtw_oracle as DO
import mel_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, N_FFT, HOP, N_MELS, N_CEP = 16000, 512, 128, 40, 13
SHIFTS = (0, 100, 256, 300, 700)
P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731


@pytest.fixture(scope="module")
def fb():
    from ssr_eval_amd.mel import mel_filterbank
    return np.ascontiguousarray(mel_filterbank(N_FFT // 2 + 1, 0.0, RATE / 2.0, N_MELS, RATE).numpy())


@pytest.fixture(scope="module")
def pairs(fb):
    """The shifted-harmonic pairs: [(name, estimate image, target image, c_E, c_G)], 1 s at 16 kHz."""
    x = DO.harmonic(RATE)
    St = MO.magnitudes(x.astype(np.float32), RATE, N_FFT, HOP)
    cG = DO.cepstra(St, fb, N_CEP)
    out = []
    for noise in (0.0, 0.003):
        for sh in SHIFTS:
            Se = MO.magnitudes(DO.shifted(x, sh, noise).astype(np.float32), RATE, N_FFT, HOP)
            out.append(("shift%d_noise%g" % (sh, noise), Se, St, DO.cepstra(Se, fb, N_CEP), cG))
    return out


# ---- oracle properties --------------------------------------------------------------------------------------------------------
def test_oracle_radius_zero_is_mcd(pairs, fb):
    for name, Se, St, cE, cG in pairs:
        want = MO.distances_from_images(Se, St, fb, N_CEP)["mcd"]
        got = DO.dtw(cE, cG, 0)
        assert abs(got["mcd_dtw"] - want) <= 1e-12 * max(1.0, want), name
        assert got["len"] == len(cE) and got["dev_sum"] == 0


def test_oracle_value_does_not_increase_with_the_radius(pairs):
    for name, _, _, cE, cG in pairs[3:8]:
        v = [DO.dtw(cE, cG, R)["D"] for R in (0, 1, 2, 5, 12, 31)]
        assert all(b <= a for a, b in zip(v, v[1:])), (name, v)


def test_oracle_single_frame_and_radius_beyond_the_matrix():
    rng = np.random.default_rng(3)
    cE, cG = rng.standard_normal((1, 5)), rng.standard_normal((1, 5))
    delta = DO.SCALE * np.sqrt(2.0 * np.sum((cE - cG) ** 2))
    for R in (0, 1, 31):
        got = DO.dtw(cE, cG, R)
        assert got["mcd_dtw"] == pytest.approx(delta, rel=1e-15) and got["len"] == 1 and got["dev_sum"] == 0
    cE, cG = rng.standard_normal((7, 5)), rng.standard_normal((7, 5))
    assert DO.dtw(cE, cG, 6) == DO.dtw(cE, cG, 7) == DO.dtw(cE, cG, 31)


@pytest.mark.parametrize("hops", [2, 3])
def test_oracle_follows_a_shift_of_whole_hops(fb, hops):
    x = DO.harmonic(RATE)
    St = MO.magnitudes(x.astype(np.float32), RATE, N_FFT, HOP)
    Se = MO.magnitudes(DO.shifted(x, hops * HOP).astype(np.float32), RATE, N_FFT, HOP)
    got = DO.from_images(Se, St, fb, 12, N_CEP)
    mcd = MO.distances_from_images(Se, St, fb, N_CEP)["mcd"]
    assert abs(got["dtw_dev"] - hops) <= 0.5
    assert got["mcd_dtw"] < 0.25 * mcd


# ---- the kernel bodies compiled for the host ---------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "mel_dtw_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libmel_dtw_emu.so")


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    return C.CDLL(EMU_SO)


def emu_warp(lib, ests, tgts, R):
    """ests: K lists of n [T_i, n_cep] cepstrum sequences, tgts: n sequences -> [n, K, 3]."""
    K, n, nc = len(ests), len(tgts), tgts[0].shape[1]
    rows = np.array([t.shape[0] for t in tgts], np.int32)
    off = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
    cep = np.ascontiguousarray(np.concatenate([np.concatenate(key) for key in ests] + [np.concatenate(tgts)]), np.float64)
    out = np.full((n, K, 3), -123.0)
    assert lib.mel_dtw_emu_warp(P(cep), C.c_int64(int(rows.sum())), P(off), P(rows), n, K, nc, R, P(out)) == 0
    return out


UNIT = np.log(10.0) / (10.0 * np.sqrt(2.0))          # delta of two frames whose one coefficient differs by k UNIT: k, up to rounding


def injected(T, seed):
    """Two [T, 3] sequences with one non-zero coefficient per frame, a small integer times UNIT, and a block of identical rows in
    both (all-zero costs: the tie rule decides)."""
    rng = np.random.default_rng(seed)
    cE, cG = np.zeros((T, 3)), np.zeros((T, 3))
    cE[:, 1] = rng.integers(0, 5, T) * UNIT
    cG[:, 1] = rng.integers(0, 5, T) * UNIT
    a, b = T // 3, T // 3 + max(1, T // 4)
    cE[a:b, 1] = cG[a:b, 1] = 2 * UNIT
    return cE, cG


def same(got, want):
    assert got[0] == want["mcd_dtw"] and got[1] == want["dtw_dev"] and got[2] == want["dtw_len"], (got, want)


@pytest.mark.parametrize("T", [1, 2, 3, 31, 32, 33, 64, 65, 200])
def test_emulated_warp_equals_the_oracle_on_injected_cepstra(emu, T):
    cE, cG = injected(T, T)
    for R in (0, 1, 2, 30, 31):
        want = DO.dtw(cE, cG, R)
        same(emu_warp(emu, [[cE]], [cG], R)[0, 0], want)
        assert want["len"] >= T and (R > 0 or want["dev_sum"] == 0)
    if T >= 31:          # the block of identical rows offers ties the rule has to break: warping through it is free
        assert DO.dtw(cE, cG, 2)["D"] < DO.dtw(cE, cG, 0)["D"]


def test_emulated_warp_ragged_batch_of_two_keys(emu):
    seqs = [injected(T, 100 + T) for T in (5, 1, 70, 33)]
    tg = [g for _, g in seqs]
    k0 = [e for e, _ in seqs]
    k1 = [np.roll(e, 1, axis=0) for e in k0]
    got = emu_warp(emu, [k0, k1], tg, 7)
    for i in range(len(tg)):
        same(got[i, 0], DO.dtw(k0[i], tg[i], 7))
        same(got[i, 1], DO.dtw(k1[i], tg[i], 7))
    np.testing.assert_array_equal(emu_warp(emu, [[k1[2]]], [tg[2]], 7)[0, 0], got[2, 1])          # a pair alone: its bits in the batch


def emu_chain(lib, ests, tgts, fb, n_cep, R, pitch=None):
    """ests: K lists of n [T_i, F] images, tgts: n images -> ([n, K, 3], cepstra [K + 1, total rows, n_cep])."""
    K, n, F = len(ests), len(tgts), tgts[0].shape[1]
    pitch = pitch or F
    rows = np.array([t.shape[0] for t in tgts], np.int32)
    off = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
    total = int(rows.sum())
    pad = lambda a: np.pad(a, ((0, 0), (0, pitch - F)))      # noqa: E731
    tp = np.ascontiguousarray(np.concatenate([pad(t) for t in tgts]), np.float32)
    ep = np.ascontiguousarray(np.concatenate([pad(e) for key in ests for e in key]), np.float32)
    out, cep = np.full((n, K, 3), -123.0), np.zeros((K + 1, total, n_cep))
    assert lib.mel_dtw_emu_chain(P(ep), C.c_int64(total * pitch), P(tp), P(off), P(rows), n, K, C.c_int64(total), F, pitch, P(fb), fb.shape[1],
                                 n_cep, R, P(out), P(cep)) == 0
    return out, cep


def test_emulated_chain_matches_the_oracle(emu, pairs, fb):
    R = 12
    St = pairs[0][2]
    got, cep = emu_chain(emu, [[Se] for _, Se, _, _, _ in pairs], [St], fb, N_CEP, R, pitch=(fb.shape[0] + 3) & ~3)
    np.testing.assert_allclose(cep[len(pairs)], pairs[0][4], rtol=0, atol=1e-11)
    for k, (name, _, _, cE, cG) in enumerate(pairs):
        assert DO.path_is_stable(cE, cG, R, rel=1e-4), name
        want = DO.dtw(cE, cG, R)
        print(name, got[0, k], want)
        assert abs(got[0, k, 0] - want["mcd_dtw"]) <= 1e-10 * abs(want["mcd_dtw"]), name
        assert got[0, k, 2] == want["dtw_len"] and got[0, k, 1] == want["dtw_dev"], name
    # the caller's unpadded pitch: the same bits
    one, _ = emu_chain(emu, [[pairs[3][1]]], [St], fb, N_CEP, R)
    np.testing.assert_array_equal(one[0, 0], got[0, 3])


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _spec_call(lib, fb, n_cep=13, radius=16, ws=_DUMMY, ws_bytes=1 << 30, n_images=2, max_rows=10, out=_DUMMY):
    fb = np.ascontiguousarray(fb, np.float32)
    return lib.ssr_spectrogram_mel_dtw(_DUMMY, _DUMMY, _DUMMY, _DUMMY, _DUMMY, n_images, max_rows, fb.shape[0], P(fb), fb.shape[1], n_cep,
                                       radius, out, ws, ws_bytes, None)


def test_dtw_abi_rejects_bad_arguments_before_launch(fb):
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E = _lib.ERR_INVALID_ARG
    F = fb.shape[0]
    for r in (-1, 32, 1000):
        assert _spec_call(lib, fb, radius=r) == E and "radius" in err()
    for nc in (0, -1, N_MELS, 200):
        assert _spec_call(lib, fb, n_cep=nc) == E and "n_cep" in err()
    bad = fb.copy(); bad[10, 3] = np.nan
    assert _spec_call(lib, bad) == E and "finite" in err()
    bad = fb.copy(); nz = np.nonzero(bad[:, 30])[0]; bad[nz[len(nz) // 2], 30] = 0.0
    assert _spec_call(lib, bad) == E and "contiguous" in err()
    bad = fb.copy(); bad[:, 7] = 0.0
    assert _spec_call(lib, bad) == E and "fewer mels" in err()
    assert _spec_call(lib, fb, out=None) == E and "null" in err()
    need = lib.ssr_spectrogram_mel_dtw_workspace_bytes(2, 10, F, N_MELS, 13, 16)
    assert need > 0
    assert _spec_call(lib, fb, ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in err()
    assert _spec_call(lib, fb, ws=None) == _lib.ERR_WORKSPACE
    assert _spec_call(lib, fb, n_images=0, ws=None, ws_bytes=0) == 0                  # nothing to score: nothing queued
    for args in ((2, 10, F, N_MELS, 13, -1), (2, 10, F, N_MELS, 13, 32), (2, 10, F, N_MELS, 0, 16), (2, 10, F, N_MELS, N_MELS, 16),
                 (2, 0, F, N_MELS, 13, 16), (2, 10, F, 257, 13, 16)):
        assert lib.ssr_spectrogram_mel_dtw_workspace_bytes(*args) == 0, args
    # the waveform level: no plan, then the family's checks
    for fn in (lib.ssr_pair_mel_dtw, lib.ssr_pair_mel_dtw_est64):
        assert fn(None, _DUMMY, _DUMMY, _DUMMY, _DUMMY, _DUMMY, _DUMMY, 1, 1, 100, 10, P(fb), N_MELS, 13, 16, _DUMMY, _DUMMY, 1 << 30,
                  None) == E and "null" in err()
    assert lib.ssr_pair_mel_dtw_workspace_bytes(None, 1, 1, 100, 10, N_MELS, 13, 16) == 0
    assert _lib.DTW_MAX_RADIUS == 31


def test_library_exports_the_dtw_symbols():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    for name in ("ssr_spectrogram_mel_dtw_workspace_bytes", "ssr_spectrogram_mel_dtw", "ssr_pair_mel_dtw_workspace_bytes", "ssr_pair_mel_dtw",
                 "ssr_pair_mel_dtw_est64"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


# ---- AudioMetrics / SSR_Eval_Helper --------------------------------------------------------------------------------------------
def test_radius_validation():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(16000)
    assert [am.dtw_radius(r) for r in (0, 16, 31, np.int64(5))] == [0, 16, 31, 5]
    for bad in (-1, 32, 1.0, True, None, "16"):
        with pytest.raises(ValueError, match="radius"):
            am.dtw_radius(bad)


def test_helper_mel_dtw_option():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.eval import _FAMILIES, _MEL_DTW_KEYS, _MEL_KEYS, _QUALITY_KEYS, result_key_order
    mk = lambda v: SSR_Eval_Helper(BasicTestee(), 44100, 44100, test_data_root=None, mel_dtw=v)      # noqa: E731
    for ok in (None, True, {}, {"radius": 0}, {"radius": 31, "n_mels": 80}, {"n_cep": 20, "norm": "slaney", "mel_scale": "slaney", "f_max": 8000}):
        assert mk(ok).mel_dtw == ok
    for bad in (False, "all", 1, 16, ("mcd_dtw",), {"radius": 32}, {"radius": -1}, {"radius": 2.0}, {"radius": True}, {"which": "mcd_dtw"},
                {"power": 2}, {"n_mels": 256}, {"n_cep": 128}, {"norm": "x"}):
        with pytest.raises(ValueError):
            mk(bad)
    assert _MEL_DTW_KEYS == ("mcd_dtw", "dtw_dev")
    names = [f[0] for f in _FAMILIES]
    assert names.index("mel_dtw") == names.index("mel") + 1
    order = result_key_order()
    assert order.index("mcd") + 1 == order.index("mcd_dtw") and order.index("dtw_dev") + 1 == order.index(_QUALITY_KEYS[0])
    assert _MEL_KEYS == ("mel_lsd", "mel_l1", "mcd") and "dtw_len" not in order
