"""CPU tests of the mel-spectrogram distances (mel_lsd, mel_l1, mcd): the host filterbank builder against the
reference's own MelScale tables (tests/golden/reference_mel.npz, make_golden_mel.py), properties of the float64 oracle
(tests/mel_oracle.py), the C ABI's argument checks (they return before anything touches a device), SSR_Eval_Helper(mel=...)
validation, and a g++ build of the kernel bodies (ssr_mel.h) against the oracle."""
import ctypes as C
import glob
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import mel_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_mel.npz")


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return g, json.loads(bytes(g["configs_json"]).decode())


def _fb(cfg):
    from ssr_eval_amd.mel import mel_filterbank
    sr, F, nm, f_min, f_max, norm, scale = cfg
    return mel_filterbank(F, f_min, float(sr // 2) if f_max is None else f_max, nm, sr, norm, scale).numpy()


# ---- the filterbank ---------------------------------------------------------------------------------------------------------
def test_filterbank_matches_the_references(golden):
    """Bit for bit on a host whose torch has the generating host's CPU capability (HTK; Slaney within the few weights next to a
    point torch.exp moved by an ulp - the GPU test host's case).  torch's float32 pow / exp are CPU-dispatched, so on a host with
    another capability a point f_m can move by an ulp and the weights of the bins next to it by up to ~1e-5."""
    g, cfgs = golden
    same = torch.backends.cpu.get_cpu_capability() == bytes(g["cpu_capability"]).decode()
    for name, cfg in cfgs.items():
        fb, ref = _fb(cfg), g["fb_" + name]
        assert fb.dtype == np.float32 and fb.shape == ref.shape
        if same and cfg[6] == "htk":
            np.testing.assert_array_equal(fb, ref, err_msg=name)
        np.testing.assert_allclose(fb, ref, rtol=0, atol=1e-7 if same else 2e-5, err_msg=name)
        assert np.count_nonzero(fb != ref) <= fb.size // (1000 if same else 100), name
    assert (g["fb_nvsr_44100"] != 0).sum() > 0


def test_projection_schedule_is_balanced_and_complete(emu, golden):
    """The schedule k_mel_schedule builds: every non-zero weight exactly once, C = ceil(nnz / 64) steps per lane, filter m's
    segments numbered seg_first[m] .. seg_first[m + 1] - 1, and the segmented sums give the dense product."""
    g, cfgs = golden
    for name in cfgs:
        fb = np.ascontiguousarray(g["fb_" + name])
        F, M = fb.shape
        nnz = int(np.count_nonzero(fb))
        cap = F * M + 64
        b, w, sf = np.zeros(cap, np.int32), np.zeros(cap, np.float32), np.zeros(M + 1, np.int32)
        steps = emu.mel_emu_schedule(P(fb), F, M, P(b), P(w), P(sf), cap)
        assert steps == -(-nnz // 64), name
        n = steps * 64
        b, w = b[:n], w[:n]
        assert (w[b >> 16 == 0] >= 0).all()
        assert np.count_nonzero(w) == nnz and sorted(w[w != 0].tolist()) == sorted(fb[fb != 0].tolist())
        wmax = int((fb != 0).sum(axis=0).max())
        assert sf[0] == 0 and (np.diff(sf) >= 1).all() and (np.diff(sf) <= 2 + (wmax - 1) // steps).all() and sf[M] <= M + 63
        # replay: lane l runs entries j * 64 + l, j = 0 .. steps - 1
        x = np.abs(np.random.default_rng(1).standard_normal(F))
        seg = np.zeros(sf[M])
        for l in range(64):
            acc = 0.0
            for j in range(steps):
                e = int(b[j * 64 + l])
                acc += x[e & 0xffff] * float(w[j * 64 + l])
                if e >> 16:
                    seg[(e >> 16) - 1] = acc
                    acc = 0.0
        mel = np.array([seg[sf[m]:sf[m + 1]].sum() for m in range(M)])
        np.testing.assert_allclose(mel, x @ fb.astype(np.float64), rtol=1e-13, err_msg=name)


def test_reference_tables_have_narrow_contiguous_filters(golden):
    """What the kernel's lanes-over-filters layout relies on: every filter one contiguous run of bins, every bin in <= 2 filters."""
    g, cfgs = golden
    for name in cfgs:
        fb = g["fb_" + name]
        for m in range(fb.shape[1]):
            nz = np.nonzero(fb[:, m])[0]
            assert len(nz) and nz[-1] - nz[0] + 1 == len(nz), (name, m)
        assert (np.count_nonzero(fb, axis=1) <= 2).all(), name


def test_audio_metrics_filterbank_defaults_are_nvsrs(golden):
    from ssr_eval_amd import AudioMetrics
    g, _ = golden
    fb, n_cep = AudioMetrics(44100).mel_filterbank()
    np.testing.assert_array_equal(fb.numpy(), g["fb_nvsr_44100"])
    assert n_cep == 13
    fb48, _ = AudioMetrics(48000, n_fft=2228).mel_filterbank()
    np.testing.assert_array_equal(fb48.numpy(), g["fb_htk_48000"])


def test_empty_filter_raises():
    from ssr_eval_amd import AudioMetrics
    from ssr_eval_amd.mel import mel_filterbank
    with pytest.raises(ValueError, match="fewer mels"):
        AudioMetrics(44100).mel_filterbank(n_mels=256)
    with pytest.raises(ValueError, match="fewer mels"):
        mel_filterbank(1025, 0.0, 22050.0, 256, 44100)
    assert mel_filterbank(1025, 0.0, 22050.0, 256, 44100, check_empty=False).shape == (1025, 256)


def test_option_validation():
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(16000)
    assert am.mel_options() == (128, 0.0, 8000.0, None, "htk", 13)
    assert am.mel_options(n_mels=80, norm="slaney", mel_scale="slaney", n_cep=20, f_min=20, f_max=7600) == (80, 20.0, 7600.0, "slaney", "slaney", 20)
    for bad in ({"n_mels": 1}, {"n_mels": 257}, {"n_mels": 80.0}, {"n_cep": 0}, {"n_mels": 40, "n_cep": 40}, {"norm": "htk"},
                {"mel_scale": "mel"}, {"f_min": -1}, {"f_min": 9000.0}, {"f_max": float("nan")}, {"power": 2}, {"which": "mcd"}):
        with pytest.raises(ValueError):
            am.mel_options(**bad)
    assert am._mel_which("all") == 7 and am._mel_which("mel_lsd") == 1 and am._mel_which(("mcd", "mel_l1")) == 6
    for bad in (None, True, 7, "MCD", (), ("mcd", "x")):
        with pytest.raises(ValueError):
            am._mel_which(bad)
    assert am._mel_dict(np.array([1.0, np.nan, 3.0]), 5) == {"mel_lsd": 1.0, "mcd": 3.0}


# ---- oracle properties --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sig():
    rng = np.random.default_rng(7)
    x = np.convolve(rng.standard_normal(16000), np.hanning(25), "same").astype(np.float32)
    return x, (x + 0.2 * np.std(x) * rng.standard_normal(x.shape)).astype(np.float32)


def test_oracle_identical_images_give_zero(sig, golden):
    g, _ = golden
    x, _ = sig
    d = O.distances(x, x, 16000, g["fb_slaney_slaney_16000"])
    assert d == {"mel_lsd": pytest.approx(0.0, abs=1e-9), "mel_l1": 0.0, "mcd": 0.0}


def test_oracle_mcd_is_gain_invariant_and_l1_symmetric(sig, golden):
    g, _ = golden
    x, y = sig
    W = g["fb_slaney_slaney_16000"]
    Sx, Sy = O.magnitudes(x, 16000), O.magnitudes(y, 16000)
    Ex, Ey = O.mel(Sx, W), O.mel(Sy, W)
    assert min(Ex.min(), Ey.min()) > 1e-5 * 4          # no mel value reaches the clamp, even at a quarter of the gain
    d = O.distances_from_mel(Ey, Ex)
    for gain in (0.25, 3.0):
        assert abs(O.distances_from_mel(gain * Ey, Ex)["mcd"] - d["mcd"]) < 1e-9
    assert O.distances_from_mel(3.0 * Ey, Ex)["mel_l1"] > d["mel_l1"]
    assert O.distances_from_mel(Ex, Ey)["mel_l1"] == pytest.approx(d["mel_l1"], rel=1e-15)
    assert d["mel_lsd"] > 0 and d["mcd"] > 0


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _spec_call(lib, fb, n_cep=13, which=7, ws=_DUMMY, ws_bytes=1 << 30, n_images=2, max_rows=10, out=_DUMMY):
    fb = np.ascontiguousarray(fb, np.float32)
    return lib.ssr_spectrogram_mel_metrics(_DUMMY, _DUMMY, _DUMMY, _DUMMY, _DUMMY, n_images, max_rows, fb.shape[0],
                                           fb.ctypes.data_as(C.c_void_p), fb.shape[1], n_cep, which, out, ws, ws_bytes, None)


def test_mel_abi_rejects_bad_arguments_before_launch(golden):
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E = _lib.ERR_INVALID_ARG
    fb = golden[0]["fb_slaney_slaney_16000"].copy()
    for w in (0, 8, -1):
        assert _spec_call(lib, fb, which=w) == E and "which" in err()
    for nc in (0, -1, 80, 200):
        assert _spec_call(lib, fb, n_cep=nc) == E and "n_cep" in err()
    bad = fb.copy(); bad[10, 3] = np.nan
    assert _spec_call(lib, bad) == E and "finite" in err()
    bad = fb.copy(); bad[10, 3] = -1e-3
    assert _spec_call(lib, bad) == E and ">= 0" in err()
    bad = fb.copy(); nz = np.nonzero(bad[:, 40])[0]; bad[nz[len(nz) // 2], 40] = 0.0
    assert _spec_call(lib, bad) == E and "contiguous" in err()
    bad = fb.copy(); bad[:, 7] = 0.0
    assert _spec_call(lib, bad) == E and "fewer mels" in err()
    assert _spec_call(lib, np.ones((372, 257), np.float32), n_cep=13) == E and "n_mels" in err()
    assert _spec_call(lib, fb, out=None) == E and "null" in err()
    need = lib.ssr_spectrogram_mel_metrics_workspace_bytes(2, 10, 372, 80, 13)
    assert need > 0
    assert _spec_call(lib, fb, ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in err()
    assert _spec_call(lib, fb, ws=None) == _lib.ERR_WORKSPACE
    assert _spec_call(lib, fb, n_images=0, ws=None, ws_bytes=0) == 0                  # nothing to score: nothing queued
    assert lib.ssr_spectrogram_mel_metrics_workspace_bytes(2, 10, 372, 80, 80) == 0
    assert lib.ssr_spectrogram_mel_workspace_bytes(372, 0) == 0
    # the projection: the same table checks, no n_cep
    bad = fb.copy(); bad[:, 0] = 0.0
    assert lib.ssr_spectrogram_mel(_DUMMY, _DUMMY, _DUMMY, 1, 10, 372, bad.ctypes.data_as(C.c_void_p), 80, _DUMMY, _DUMMY, 1 << 30,
                                   None) == E and "fewer mels" in err()
    # the waveform level: no plan
    assert lib.ssr_pair_mel_metrics(None, _DUMMY, _DUMMY, _DUMMY, _DUMMY, _DUMMY, _DUMMY, 1, 1, 100, 10, fb.ctypes.data_as(C.c_void_p),
                                    80, 13, 7, _DUMMY, _DUMMY, 1 << 30, None) == E and "null" in err()
    assert lib.ssr_pair_mel_metrics_workspace_bytes(None, 1, 1, 100, 10, 80, 13) == 0


# ---- SSR_Eval_Helper ---------------------------------------------------------------------------------------------------------
def test_helper_mel_option():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.eval import _MEL_KEYS
    mk = lambda v: SSR_Eval_Helper(BasicTestee(), 44100, 44100, test_data_root=None, mel=v)      # noqa: E731
    for ok in (None, True, {}, {"n_mels": 80}, {"which": "mcd", "n_cep": 20}, {"norm": "slaney", "mel_scale": "slaney", "f_max": 8000}):
        assert mk(ok).mel == ok
    for bad in (False, "all", 1, ("mcd",), {"power": 2}, {"which": "pesq"}, {"n_mels": 256}, {"n_cep": 128}, {"norm": "x"}):
        with pytest.raises(ValueError):
            mk(bad)
    assert _MEL_KEYS == ("mel_lsd", "mel_l1", "mcd")


# ---- the kernel bodies compiled for the host ---------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "mel_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libmel_emu.so")


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    return C.CDLL(EMU_SO)


P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731


def run_emu(lib, ests, tgts, fb, n_cep, which, kg=1, pitch=None):
    """ests: K lists of n [T_i, F] images, tgts: n [T_i, F] images -> [n, K, 3]."""
    K, n = len(ests), len(tgts)
    F = tgts[0].shape[1]
    pitch = pitch or F
    rows = np.array([t.shape[0] for t in tgts], np.int32)
    off = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
    total = int(rows.sum())
    pad = lambda a: np.pad(a, ((0, 0), (0, pitch - F)))      # noqa: E731
    tp = np.ascontiguousarray(np.concatenate([pad(t) for t in tgts]), np.float32)
    ep = np.ascontiguousarray(np.concatenate([pad(e) for key in ests for e in key]), np.float32)
    fb = np.ascontiguousarray(fb, np.float32)
    out = np.full((n, K, 3), -123.0)
    assert lib.mel_emu_metrics(P(ep), C.c_int64(total * pitch), P(tp), P(off), P(rows), n, K, kg, F, pitch, P(fb), fb.shape[1], n_cep,
                               which, P(out)) == 0
    return out


@pytest.mark.parametrize("cfg", ["nvsr_44100", "slaney_slaney_16000", "band_20_8000_44100"])
def test_emulated_kernels_match_the_oracle(emu, golden, cfg):
    g, cfgs = golden
    sr = cfgs[cfg][0]
    fb = g["fb_" + cfg]
    rng = np.random.default_rng(len(cfg))
    lens = [int(0.31 * sr), int(0.07 * sr) + 5, 700, int(0.2 * sr) + 1]
    tg = [np.convolve(rng.standard_normal(n), np.hanning(9), "same").astype(np.float32) for n in lens]
    ests = [[(t + s * rng.standard_normal(len(t))).astype(np.float32) for t in tg] for s in (0.05, 0.5, 0.0)]
    ests[1][2] = (0.3 * tg[2]).astype(np.float32)
    St = [O.magnitudes(t, sr) for t in tg]
    Se = [[O.magnitudes(e, sr) for e in key] for key in ests]
    for n_cep in (13, 40):
        got = run_emu(emu, Se, St, fb, n_cep, 7, kg=3, pitch=(fb.shape[0] + 3) & ~3)
        for i in range(len(tg)):
            for k in range(3):
                want = O.distances_from_images(Se[k][i], St[i], fb, n_cep)
                for j, m in enumerate(O.NAMES):
                    assert abs(got[i, k, j] - want[m]) <= 1e-10 * max(1.0, abs(want[m])), (cfg, n_cep, i, k, m, got[i, k, j], want[m])
        assert (got[:, 2, 1:] == 0).all() and (got[:, 2, 0] < 1e-9).all()            # estimate = target (mel_lsd: the 1e-12 terms)
    # one key per wave, the caller's unpadded pitch and subsets: the same bits
    one = run_emu(emu, Se, St, fb, 13, 7, kg=1)
    np.testing.assert_array_equal(one, run_emu(emu, Se, St, fb, 13, 7, kg=3, pitch=(fb.shape[0] + 3) & ~3))
    sub = run_emu(emu, Se, St, fb, 13, 5)
    np.testing.assert_array_equal(sub[..., [0, 2]], one[..., [0, 2]])
    assert np.isnan(sub[..., 1]).all()
    # a pair alone: its bits in the batch
    alone = run_emu(emu, [[Se[1][3]]], [St[3]], fb, 13, 7)
    np.testing.assert_array_equal(alone[0, 0], one[3, 1])


def test_emulated_projection_matches_the_golden_forward(emu, golden):
    g, cfgs = golden
    for name in ("nvsr_44100", "slaney_slaney_16000"):
        fb = g["fb_" + name]
        F = fb.shape[0]
        seed = int(g["fwd_seed_" + name])
        rng = np.random.default_rng(seed)
        x = np.abs(rng.standard_normal((60, F))) * np.exp(-np.arange(F) / (F / 4.0))[None, :]
        x = np.ascontiguousarray(x.astype(np.float32))
        out = np.zeros((60, fb.shape[1]), np.float32)
        rows, off = np.array([60], np.int32), np.zeros(1, np.int64)
        assert emu.mel_emu_project(P(x), P(off), P(rows), 1, F, P(np.ascontiguousarray(fb)), fb.shape[1], P(out)) == 0
        want = O.mel(x, fb)
        np.testing.assert_allclose(out, want, rtol=1e-7, atol=0)
        np.testing.assert_allclose(out, g["fwd_" + name], rtol=1e-6, atol=1e-30)
