"""CPU tests of the noise-to-mask family (nmr, nmr_seg, rdf, nmr_hf, nmr_lf): anchors of the float64 oracle
(tests/nmr_oracle.py: direct O(Nc^2) spreading with ** 0.4, an explicit frame loop), a g++ build of the kernel bodies (ssr_nmr.h)
against the oracle - rates, transform sizes, the shapes where the geometry can go wrong, the exact facts, the bit-level properties -,
the C ABI's argument checks (they return before anything touches a device), the header / ctypes table / library agreement, and
AudioMetrics / SSR_Eval_Helper(nmr=...) validation and the registry rules.

Tolerances: the mask M within 1e-9 relative; Pn within 1e-9 of the frame's largest G W2 |X|^2 in every frame of every pair (the
emulation writes R of every frame, Pn = R M; the mean ratio per band, which is all the device returns, is held to the sum of that
bound over the frames, over M); every dB column within 1e-6 dB, the bar of coh_sdr and mod_dist - the compared pairs' error is at least -80 dB relative to the
target, so Pn is no round-off; frames equal; rdf equal on inputs for which the oracle alone is first asserted to have no frame within
1e-4 dB of the 1.5 dB threshold.  Worst differences seen in emulation: M 2.5e-14 relative, Pn 7.5e-16 of the frame's peak, a dB
column 1.2e-8 dB (the cancellation in |X| - |Y| where the two spectra nearly agree)."""
import ctypes as C
import glob
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import nmr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FR = O.FR
DTYPES = [(np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64), (np.float64, np.float64)]
DTYPE_IDS = ["f32-f32", "f64-f32", "f32-f64", "f64-f64"]
_DESIGNS = {}


def B():
    from ssr_eval_amd import backend
    return backend


def design(fs, N=None, level_db=92.0):
    """The oracle's tables, made once per (fs, N, level) and shared (Bs is filled in at the first use)."""
    key = (fs, N, level_db)
    if key not in _DESIGNS:
        _DESIGNS[key] = O.design(fs, N, level_db)
    return _DESIGNS[key]


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------
def test_oracle_band_layout_and_default_nfft():
    assert [O.default_nfft(fs) for fs in (8000, 16000, 24000, 32000, 44100, 48000, 192000)] == [256, 512, 1024, 1024, 2048, 2048, 2048]
    for fs, Nc in ((8000, 65), (16000, 84), (44100, 109), (48000, 109)):
        d = design(fs)
        assert d["Nc"] == Nc == len(d["fc"]) and d["U"].shape == (Nc, d["N"] // 2 + 1)
        # the first centre lies an eighth of a Bark above 80 Hz, the last at the middle of the (cut) last band
        assert abs(d["fc"][0] - 650.0 * np.sinh((7.0 * np.arcsinh(80.0 / 650.0) + 0.125) / 7.0)) < 1e-9
        top = min(18000.0, 0.45 * fs)
        assert d["fl"][-1] < d["fc"][-1] < d["fu"][-1] and abs(d["fu"][-1] - top) < 1e-8 and abs(d["fl"][0] - 80.0) < 1e-10
        assert np.all(np.diff(d["fc"]) > 0)
        # every bin wholly inside the range is shared out with sum 1; no bin gets more
        width = fs / d["N"]
        k = np.arange(d["N"] // 2 + 1)
        inside = ((k - 0.5) * width >= 80.0) & ((k + 0.5) * width <= top)
        tot = d["U"].sum(axis=0)
        assert inside.sum() > 10 and np.max(np.abs(tot[inside] - 1.0)) < 1e-12 and np.all(tot <= 1.0 + 1e-12) and np.all(d["U"] >= 0.0)
        assert d["W2"][0] == 0.0 and np.all(d["W2"][1:] > 0.0) and np.all(d["Ein"] > 0.0)
        assert np.all(d["m_db"][:49] == 3.0) and d["m_db"][49] == 0.25 * 49 * 0.25 and np.all((d["a"] > 0.0) & (d["a"] < 1.0))


@pytest.mark.parametrize("fs,k0,amp", [(48000, 43, 0.25), (16000, 64, 1.0), (8000, 20, 0.5)])
def test_oracle_level_of_a_bin_centre_sine(fs, k0, amp):
    """A sine at the centre of bin k0: |X[k0]| = A N / 4, |X[k0 +- 1]| = A N / 8, nothing elsewhere, so the band energies above the
    internal noise add up to G sum_k W2 |X|^2 - and a full-scale one has a peak-bin power of 10^9.2 before the ear weighting."""
    d = design(fs)
    N = d["N"]
    x = amp * np.sin(2.0 * np.pi * k0 * np.arange(3 * N) / N + 0.3)
    X = np.abs(O.stft(x, N))
    assert np.max(np.abs(X[:, k0] - amp * N / 4.0)) < 1e-9 * N and np.max(np.abs(X[:, [k0 - 1, k0 + 1]] - amp * N / 8.0)) < 1e-9 * N
    assert abs(d["G"] * (N / 4.0) ** 2 - 10.0 ** 9.2) < 1e-3
    _, Eb, _ = O.excitation(x, d)
    want = d["G"] * (d["W2"][k0] * (amp * N / 4.0) ** 2 + (d["W2"][k0 - 1] + d["W2"][k0 + 1]) * (amp * N / 8.0) ** 2)
    got = (Eb - d["Ein"][None, :]).sum(axis=1)
    assert np.max(np.abs(got - want)) < 1e-9 * want


def test_oracle_spreading_of_unit_energy_and_step_response():
    for fs in (8000, 48000):
        d = design(fs)
        assert np.max(np.abs(O.spread(np.ones(d["Nc"]), d) - 1.0)) < 1e-14
        S = O.spread_matrix(np.full(d["Nc"], 1e6), d)
        assert np.max(np.abs(S.sum(axis=0) - 1.0)) < 1e-14 and abs(S[11, 10] / S[10, 10] - 10.0 ** ((d["c_up"][10] + 12.0) * 0.025)) < 1e-12
        assert abs(S[9, 10] / S[10, 10] - 10.0 ** -0.675) < 1e-14
        # a constant excitation switched on at frame 0: Ef[t] = E (1 - a^(t + 1)), and the maximum with Es is Es
        E = np.linspace(1.0, 5.0, d["Nc"])
        Ef, Et = O.time_spread(np.tile(E, (40, 1)), d)
        t = np.arange(40)[:, None]
        assert np.max(np.abs(Ef - E[None, :] * (1.0 - d["a"][None, :] ** (t + 1)))) < 1e-13 and np.max(np.abs(Et - E[None, :])) < 1e-14
        # switched off again: the smeared value decays by a per frame and is what the maximum keeps
        Ef, Et = O.time_spread(np.concatenate([np.tile(E, (40, 1)), np.zeros((5, d["Nc"]))]), d)
        assert np.max(np.abs(Et[44] - Ef[39] * d["a"] ** 5)) < 1e-13


def test_oracle_gain_step_and_near_against_far_masking():
    fs = 48000
    d = design(fs)
    n = fs // 2
    x = O.music_like(n, fs, 3)
    # an estimate that is a gain: |X| - |Y| = c |X|, so (1 + 2 c) x reads 20 log10 2 more than (1 + c) x in both dB columns (c a power
    # of two: the products are exact and what is left is the rounding of the two subtractions and logarithms)
    c = 1.0 / 64.0
    a, b = O.nmr(x, (1.0 + c) * x, fs, d=d)[0], O.nmr(x, (1.0 + 2.0 * c) * x, fs, d=d)[0]
    assert abs(b[0] - a[0] - 20.0 * np.log10(2.0)) < 1e-10 and abs(b[1] - a[1] - 20.0 * np.log10(2.0)) < 1e-10
    # the same noise power under a strong partial and in an empty band
    t = np.arange(fs) / fs
    tone = 0.25 * np.sin(2.0 * np.pi * 1000.0 * t)
    p = np.mean(tone ** 2) * 10.0 ** -3.0
    near = O.nmr(tone, tone + np.sqrt(p) * O.band_noise(fs, fs, 900.0, 1100.0, 1), fs, d=d)[0]
    far = O.nmr(tone, tone + np.sqrt(p) * O.band_noise(fs, fs, 6000.0, 7000.0, 1), fs, d=d)[0]
    print("30 dB SNR noise at 900-1100 Hz: nmr %.2f dB, rdf %.2f; at 6-7 kHz: nmr %.2f dB, rdf %.2f" % (near[0], near[2], far[0], far[2]))
    assert near[0] < -20.0 and far[0] > 20.0 and far[0] - near[0] > 40.0 and near[2] == 0.0 and far[2] == 1.0


def test_oracle_nan_floor_and_split_rules():
    fs = 16000
    d = design(fs)
    N = d["N"]
    x = O.music_like(3 * N, fs, 5)
    cols, bands, _, _, _ = O.nmr(x[:N - 1], x[:N - 1], fs, d=d)
    assert np.isnan(cols[:5]).all() and cols[5] == 0 and np.isnan(bands).all()
    cols = O.nmr(x, x, fs, d=d, split_hz=2000.0)[0]
    assert cols[0] == -200.0 and cols[1] == -200.0 and cols[2] == 0.0 and cols[3] == -200.0 and cols[4] == -200.0 and cols[5] == 5
    y = O.noisy(x, 30.0, 1)
    assert np.isnan(O.nmr(x, y, fs, d=d)[0][3:5]).all()
    assert np.isnan(O.nmr(x, y, fs, d=d, split_hz=1e9)[0][3]) and np.isnan(O.nmr(x, y, fs, d=d, split_hz=0.0)[0][4])
    cols = O.nmr(x, y, fs, d=d, split_hz=1e9)[0]
    assert cols[4] == cols[0] and np.isfinite(cols).sum() == 5


def test_backend_design_is_the_oracles():
    bk = B()
    for fs, N, level in ((8000, None, 92.0), (16000, None, 92.0), (44100, None, 92.0), (48000, None, 100.0), (48000, 256, 92.0), (192000, 256, 92.0),
                         (32000, 2048, 80.0)):
        d, q = O.design(fs, N, level), bk.nmr_design(fs, N, level)
        Nc, nb = d["Nc"], d["N"] // 2 + 1
        assert q["n_fft"] == d["N"] and q["bins"].shape == (Nc, 2) and q["bins"].dtype == np.int32 and q["table"].shape == (Nc, 8)
        assert q["weights"].shape == (nb,) and q["weights"].flags.c_contiguous and q["table"].flags.c_contiguous and q["bins"].flags.c_contiguous
        assert np.max(np.abs(q["fc"] - d["fc"])) < 1e-9 and np.max(np.abs(q["weights"] - d["G"] * d["W2"])) <= 1e-12 * np.max(q["weights"])
        U = np.zeros((Nc, nb))                                     # the compact (k_lo, k_hi, u_lo, u_hi) form is the dense U
        for i, ((lo, hi), row) in enumerate(zip(q["bins"], q["table"])):
            assert 0 <= lo <= hi <= nb - 1
            U[i, lo:hi + 1] = 1.0
            U[i, hi] = row[1]
            U[i, lo] = row[0]
        assert np.max(np.abs(U - d["U"])) < 1e-12
        O.spread(np.ones(Nc), d)
        rd = 10.0 ** -0.675
        assert np.max(np.abs(q["table"][:, 2] - d["Ein"])) < 1e-12 and np.max(np.abs(q["table"][:, 3] - d["c_up"])) < 1e-12
        assert np.max(np.abs(q["table"][:, 4] - np.array([sum(rd ** j for j in range(1, l + 1)) for l in range(Nc)]))) < 1e-13
        assert np.max(np.abs(q["table"][:, 5] * d["Bs"] - 1.0)) < 1e-13 and np.max(np.abs(q["table"][:, 6] - d["a"])) < 1e-15
        assert np.max(np.abs(q["table"][:, 7] * 10.0 ** (d["m_db"] / 10.0) - 1.0)) < 1e-14 and np.array_equal(q["mask_db"], d["m_db"])
    assert bk.nmr_design(48000) is bk.nmr_design(48000.0, 2048, 92)      # cached per (fs, N, level)


# ---- the kernel bodies compiled for the host ------------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "nmr_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libnmr_emu.so")


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    lib = C.CDLL(EMU_SO)
    lib.nmr_emu.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                            C.c_int, C.c_int] + [C.c_void_p] * 10
    return lib


def split_bands(fs, N, splits, n_est, level_db=92.0):
    """One split frequency per estimate (None: none) -> the int32 first band of the upper part, -1 for no split."""
    d = design(fs, N, level_db)
    if splits is None:
        return np.full(n_est, -1, np.int32)
    return np.array([O.split_band(d, s) for s in splits], np.int32)


class Emu:
    """What one emulated ssr_nmr call returns: out [n_est, 6], bands [n_est, Nc] or None, and per target M and Es [K, Nc], per pair
    its chunk rows [chunks, Nc + 2] and R of every frame [K, Nc]."""


def run_emu(lib, tgts, ests, idx, fs, N=None, splits=None, with_bands=True, with_mask=True, level_db=92.0):
    q = B().nmr_design(fs, N, level_db)
    N, Nc = q["n_fft"], q["fc"].shape[0]
    tdt, edt = tgts[0].dtype, (ests[0].dtype if ests else tgts[0].dtype)
    P = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None      # noqa: E731
    tl = np.array([len(t) for t in tgts], np.int32)
    el = np.array([len(e) for e in ests], np.int64)
    to = np.concatenate(([0], np.cumsum(tl)[:-1])).astype(np.int64)
    eo = np.concatenate(([0], np.cumsum(el)[:-1])).astype(np.int64)
    td = np.concatenate(list(tgts) + [np.zeros(1, tdt)])
    ed = np.concatenate(list(ests) + [np.zeros(1, edt)])
    idx = np.ascontiguousarray(idx, np.int32)
    sp = split_bands(fs, N, splits, len(ests), level_db)
    Ks = [O.frames(int(n), N) for n in tl]
    chunks = [-(-Ks[i] // FR) for i in idx]
    r = Emu()
    r.out = np.full((len(ests), 6), -123.0)
    r.bands = np.full((len(ests), Nc), -7.0) if with_bands else None
    M = np.full((sum(Ks) + 1, Nc), -5.0) if with_mask else None
    Es = np.full((sum(Ks) + 1, Nc), -5.0)
    part = np.full((sum(chunks) + 1, Nc + 2), -9.0)
    R = np.full((sum(Ks[i] for i in idx) + 1, Nc), -3.0)
    assert lib.nmr_emu(P(td), int(tdt == np.float64), P(to), P(tl), len(tgts), P(ed), int(edt == np.float64), P(eo), P(idx), len(ests), N, Nc,
                       P(q["weights"]), P(q["bins"]), P(q["table"]), P(sp), P(r.out), P(r.bands), P(M), P(Es), P(part), P(R)) == 0
    assert np.all(Es[-1] == -5.0) and np.all(part[-1] == -9.0) and np.all(R[-1] == -3.0) and np.all(R[:-1] >= 0.0) and (M is None or np.all(M[-1] == -5.0))
    fe, ce = np.concatenate(([0], np.cumsum(Ks))), np.concatenate(([0], np.cumsum(chunks))).astype(int)
    r.M = [M[fe[i]:fe[i + 1]] for i in range(len(tgts))] if with_mask else None
    r.Es = [Es[fe[i]:fe[i + 1]] for i in range(len(tgts))]
    r.part = [part[ce[e]:ce[e + 1]] for e in range(len(ests))]
    re = np.concatenate(([0], np.cumsum([Ks[i] for i in idx]))).astype(int)
    r.R = [R[re[e]:re[e + 1]] for e in range(len(ests))]
    return r


WORST = {"M": 0.0, "Pn": 0.0, "dB": 0.0}


def check(r, tgts, ests, idx, fs, N=None, splits=None, level_db=92.0, rdf=True, what=""):
    """Everything an emulated (or device) call returned against the oracle, pair by pair."""
    d = design(fs, N, level_db)
    Nc = d["Nc"]
    masks = {}
    for e, (y, ti) in enumerate(zip(ests, idx)):
        x = tgts[ti]
        cols, bands, frame_db, M, Pn = O.nmr(x, y, fs, d=d, split_hz=None if splits is None else splits[e])
        got = r.out[e]
        assert got[5] == cols[5], (what, e, got, cols)
        if cols[5] == 0:
            assert np.isnan(got[:5]).all() and (r.bands is None or np.isnan(r.bands[e]).all()), (what, e, got)
            continue
        if r.M is not None and ti not in masks:
            masks[ti] = float(np.max(np.abs(r.M[ti] - M) / M))
            assert r.M[ti].shape == M.shape and masks[ti] <= O.TOL_REL, (what, "mask of target", ti, masks[ti])
            WORST["M"] = max(WORST["M"], masks[ti])
        peak = (d["G"] * d["W2"][None, :] * np.abs(O.stft(x, d["N"])) ** 2).max(axis=1)              # per frame
        # (a digitally silent target frame has no scale of its own: there the estimate's largest weighted bin is the scale)
        peak = np.where(peak > 0.0, peak, (d["G"] * d["W2"][None, :] * np.abs(O.stft(y, d["N"])) ** 2).max(axis=1))
        if r.bands is not None:
            bound = (O.TOL_REL * peak[:, None] / M).mean(axis=0) + O.TOL_REL * bands
            assert np.all(np.abs(r.bands[e] - bands) <= bound), (what, e, np.max(np.abs(r.bands[e] - bands) / bound))
        if hasattr(r, "R") and r.M is not None:      # the emulation's row of every frame: Pn = R M, both slots of a packed transform
            diff = np.abs(r.R[e] * r.M[ti] - Pn)
            assert r.R[e].shape == Pn.shape and np.all(diff <= O.TOL_REL * peak[:, None]), (what, e, "Pn", diff.max(), peak)
            WORST["Pn"] = max(WORST["Pn"], float(np.max(diff[peak > 0] / peak[peak > 0, None], initial=0.0)))
            if cols[5] == 1:                          # one frame: the chunk row holds R of that frame
                assert r.part[e][0, :Nc].tobytes() == r.R[e][0].tobytes()
        if rdf:
            assert O.rdf_margin(frame_db) >= 1e-4, (what, e, "a frame of the oracle lies on the disturbed-frame threshold")
            assert got[2] == cols[2], (what, e, got[2], cols[2])
        for c in (0, 1, 3, 4):
            if np.isnan(cols[c]):
                assert np.isnan(got[c]), (what, e, c, got)
            else:
                assert abs(got[c] - cols[c]) <= O.TOL_DB, (what, e, c, got[c], cols[c])
                WORST["dB"] = max(WORST["dB"], abs(got[c] - cols[c]))
        assert np.isfinite(got).all() or splits is None or np.isnan(cols).any()
    return WORST


def _estimates(x, seed):
    """Errors of at least -80 dB relative to the target: noise at 30 dB SNR, clipping, a low-passed copy - and the target itself."""
    spec = np.fft.rfft(x)
    spec[len(spec) // 3:] = 0.0
    return [O.noisy(x, 30.0, seed), O.clipped(x), np.fft.irfft(spec, len(x)), x.copy()]


@pytest.mark.parametrize("fs,N,Nc", [(8000, 256, 65), (16000, 512, 84), (32000, 1024, 103), (44100, 2048, 109), (48000, 2048, 109), (48000, 256, 109)])
def test_emulated_kernels_match_the_oracle_at_every_rate(emu, fs, N, Nc):
    """Partials with slow envelopes over a noise floor at every default (rate, N), and N = 256 at 48 kHz - more bands than threads;
    four estimates of one target (the last the target itself), the four dtype mixes, a split at a quarter of the rate."""
    assert (O.default_nfft(fs) == N == B().nmr_default_nfft(fs) or N == 256) and design(fs, N)["Nc"] == Nc
    x = O.music_like(O.len_for_frames(11, N, 5), fs, fs // 1000)
    ys = _estimates(x, 7)
    splits = [fs / 8.0, None, fs / 8.0, fs / 8.0]
    for dt in DTYPES:
        tg, es = [x.astype(dt[0])], [y.astype(dt[1]) for y in ys]
        if dt == (np.float32, np.float64):
            es[3] = tg[0].astype(np.float64)               # (a float32 target widened is that target)
        r = run_emu(emu, tg, es, [0, 0, 0, 0], fs, N, splits)
        w = check(r, tg, es, [0, 0, 0, 0], fs, N, splits, what="rate %d %s" % (fs, dt))
        if dt != (np.float64, np.float32):                 # y == x bit for bit
            assert r.out[3].tolist() == [-200.0, -200.0, 0.0, -200.0, -200.0, 11.0] and np.all(r.bands[3] == 0.0)
        assert np.isnan(r.out[1, 3:5]).all() and np.isfinite(r.out[[0, 2]]).all() and r.out[0, 0] > -120.0
    print("worst so far: M %.3g relative, Pn %.3g of the frame's peak, a dB column %.3g dB" % (w["M"], w["Pn"], w["dB"]))


def _geometry_batch(dt, fs=8000, N=256):
    """n = N - 1 (K = 0), N (K = 1, twice: Pn is read directly there), K = 2, FR - 1, FR, FR + 1 (one frame behind the seam: the
    half-filled last transform), 33 N / 2 + N + 7 (K = 34: two frames behind the seam) with three estimates, K = 2 FR + 3."""
    lens = [N - 1, N, N + 9] + [O.len_for_frames(K, N, e) for K, e in ((2, 0), (FR - 1, 5), (FR, 63), (FR + 1, 0))] + [33 * N // 2 + N + 7] + \
        [O.len_for_frames(2 * FR + 3, N, 17)]
    xs = [O.music_like(n, fs, 40 + i) for i, n in enumerate(lens)]
    tg = [x.astype(dt[0]) for x in xs]
    ests, idx = [], []
    for i, x in enumerate(xs):
        for k in range(3 if i == 7 else 1):
            ests.append((O.noisy(x, 25.0 + 10.0 * k, 50 + i + k) if k != 1 else O.clipped(x)).astype(dt[1]))
            idx.append(i)
    return fs, N, tg, ests, idx


# one split per estimate of the geometry batch; 3600 Hz and 1e9 Hz lie above the last centre at 8 kHz (3592 Hz): the empty upper side,
# 50 Hz below the first: the empty lower side
GEOMETRY_SPLITS = [1000.0, 1500.0, 2000.0, 2500.0, 3000.0, 50.0, 3600.0, 500.0, None, 1e9, 700.0]


@pytest.mark.parametrize("dt", DTYPES, ids=DTYPE_IDS)
def test_emulated_geometry_shapes_and_bit_level_properties(emu, dt):
    """The ragged geometry batch; then: a pair alone and at another position gives the bits it gives in the batch, a target's mask
    is the same with one and with three estimates, bands_out = NULL and mask_out = NULL change no bit of out."""
    fs, N, tg, ests, idx = _geometry_batch(dt)
    splits = GEOMETRY_SPLITS
    assert len(splits) == len(ests) and split_bands(fs, N, splits, len(ests)).tolist() == [31, 41, 48, 54, 59, 0, 65, 16, -1, 65, 23]
    r = run_emu(emu, tg, ests, idx, fs, N, splits)
    w = check(r, tg, ests, idx, fs, N, splits, what="shapes")
    print("worst so far: M %.3g relative, Pn %.3g of the frame's peak, a dB column %.3g dB" % (w["M"], w["Pn"], w["dB"]))
    assert r.out[:, 5].tolist() == [0, 1, 1, 2, FR - 1, FR, FR + 1, 34, 34, 34, 2 * FR + 3] and np.isnan(r.out[0, :5]).all()
    assert np.isnan(r.out[5, 4]) and np.isfinite(r.out[5, 3]) and np.isnan(r.out[[6, 9], 3]).all() and np.isfinite(r.out[[6, 9], 4]).all()
    assert np.isnan(r.out[8, 3:5]).all() and np.isfinite(r.out[1:, :3]).all() and not np.isinf(r.out).any()
    for e in (1, 3, 6, 7, 8, 9, len(ests) - 1):
        a = run_emu(emu, [tg[idx[e]]], [ests[e]], [0], fs, N, [splits[e]])
        assert a.out.tobytes() == r.out[e:e + 1].tobytes() and a.bands.tobytes() == r.bands[e:e + 1].tobytes(), e
        assert a.M[0].tobytes() == r.M[idx[e]].tobytes()                           # one estimate or three: the same mask
    order = list(range(len(ests)))[::-1]
    b = run_emu(emu, tg, [ests[e] for e in order], [idx[e] for e in order], fs, N, [splits[e] for e in order])
    assert b.out[::-1].tobytes() == r.out.tobytes() and b.bands[::-1].tobytes() == r.bands.tobytes()
    assert run_emu(emu, tg, ests, idx, fs, N, splits, with_bands=False, with_mask=False).out.tobytes() == r.out.tobytes()
    none = run_emu(emu, tg, ests, idx, fs, N)
    assert none.out[:, :3].tobytes() == r.out[:, :3].tobytes() and np.isnan(none.out[:, 3:5]).all()      # the split moves no bit of the others


@pytest.mark.parametrize("fs,N,K", [(48000, 2048, 3), (44100, 1024, FR + 1), (16000, 512, 4), (96000, 2048, 2), (8000, 512, 2 * FR + 1)])
def test_emulated_other_transform_sizes(emu, fs, N, K):
    """Every n_fft, away from the rate's default too - float32 targets with float64 estimates, next to a pair one sample too short for
    a frame - and another level."""
    x = O.music_like(O.len_for_frames(K, N, 3), fs, 70 + N // 256)
    tg = [x.astype(np.float32), x[:N - 1].astype(np.float32)]
    ests = [O.noisy(x, 35.0, 3), O.clipped(x)[:N - 1]]
    r = run_emu(emu, tg, ests, [0, 1], fs, N, [1500.0, 1500.0], level_db=80.0)
    w = check(r, tg, ests, [0, 1], fs, N, [1500.0, 1500.0], level_db=80.0, what="sizes")
    print("worst so far: M %.3g relative, Pn %.3g of the frame's peak, a dB column %.3g dB" % (w["M"], w["Pn"], w["dB"]))
    assert np.isnan(r.out[1, :5]).all() and np.isfinite(r.out[0]).all() and r.out[:, 5].tolist() == [K, 0]


def test_emulated_exact_facts_silence_and_masking(emu):
    """y == x: -200 exactly and rdf 0, for a silent target too (the internal noise keeps M positive: no NaN, no infinity); a silent
    estimate; stretches of exact zeros inside a loud signal; and the near-against-far masking pair."""
    fs = 16000
    d = design(fs)
    N = d["N"]
    x = O.music_like(O.len_for_frames(9, N, 3), fs, 90)
    xf, z = x.astype(np.float32), np.zeros(len(x), np.float32)
    for same in (xf, xf.astype(np.float64)):
        r = run_emu(emu, [xf], [same], [0], fs, splits=[2000.0])
        assert r.out[0].tolist() == [-200.0, -200.0, 0.0, -200.0, -200.0, 9.0] and np.all(r.bands == 0.0)
    r = run_emu(emu, [z, z], [z, xf], [0, 1], fs, splits=[2000.0, 2000.0])
    check(r, [z, z], [z, xf], [0, 1], fs, splits=[2000.0, 2000.0], what="silent target")
    assert r.out[0].tolist() == [-200.0, -200.0, 0.0, -200.0, -200.0, 9.0] and np.isfinite(r.out[1]).all() and r.out[1, 0] > 30.0
    r = run_emu(emu, [xf], [z], [0], fs, splits=[2000.0])
    check(r, [xf], [z], [0], fs, splits=[2000.0], what="silent estimate")
    x2, y = x.copy(), O.noisy(x, 30.0, 91)
    y2 = y.copy()
    x2[1500:1500 + 2 * N] = 0.0
    y2[2500:2500 + N + 17] = 0.0
    tg, es, idx = [x2, x], [y, y2, y], [0, 1, 1]
    r = run_emu(emu, tg, es, idx, fs, splits=[2000.0] * 3)
    check(r, tg, es, idx, fs, splits=[2000.0] * 3, what="silent stretches")
    fs = 48000
    t = np.arange(fs // 2) / fs
    tone = 0.25 * np.sin(2.0 * np.pi * 1000.0 * t)
    p = np.mean(tone ** 2) * 10.0 ** -3.0
    es = [tone + np.sqrt(p) * O.band_noise(len(t), fs, 900.0, 1100.0, 1), tone + np.sqrt(p) * O.band_noise(len(t), fs, 6000.0, 7000.0, 1)]
    r = run_emu(emu, [tone], es, [0, 0], fs)
    check(r, [tone], es, [0, 0], fs, what="near and far")
    assert r.out[1, 0] - r.out[0, 0] > 40.0 and r.out[0, 2] == 0.0 and r.out[1, 2] == 1.0


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


def _call(lib, tl, idx, n_fft=256, n_bands=65, bins=None, table=None, split=None, n_est=None, ws=_DUMMY, ws_bytes=1 << 40, out=_DUMMY,
          weights=_DUMMY, null=()):
    tl, tp = _i32(tl)
    idx, ip = _i32(idx)
    q = B().nmr_design(8000, 256)
    nb = max(n_bands, 1)
    bins = np.ascontiguousarray(np.resize(q["bins"], (nb, 2)) if bins is None else bins, np.int32)
    table = np.ascontiguousarray(np.resize(q["table"], (nb, 8)) if table is None else table, np.float64)
    sp, spp = _i32(np.full(max(len(idx), 1), -1) if split is None else split)
    return lib.ssr_nmr(_DUMMY, 0, _DUMMY, tp, len(tl), _DUMMY, 0, _DUMMY, ip, len(idx) if n_est is None else n_est, n_fft, n_bands,
                       None if "weights" in null else weights, None if "bins" in null else bins.ctypes.data_as(C.c_void_p),
                       None if "table" in null else table.ctypes.data_as(C.c_void_p), None if "split" in null else spp, out, None, None, ws,
                       ws_bytes, None)


def test_nmr_rejects_bad_arguments_before_launch():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E = _lib.ERR_INVALID_ARG
    q = B().nmr_design(8000, 256)
    for n_fft in (0, 128, 255, 1000, 4096, -1024):
        assert _call(lib, [4000], [0], n_fft=n_fft) == E and "n_fft" in err()
    for n_bands in (0, -1, 129):
        assert _call(lib, [4000], [0], n_bands=n_bands) == E and "n_bands" in err()
    for lo, hi in ((-1, 3), (5, 4), (3, 129), (200, 200)):
        bins = q["bins"].copy()
        bins[7] = (lo, hi)
        assert _call(lib, [4000], [0], bins=bins) == E and "bins" in err()
    for col, bad in ((0, -0.1), (0, 1.5), (1, float("nan")), (2, 0.0), (2, float("inf")), (3, float("nan")), (4, -1.0), (5, 0.0), (5, float("inf")),
                     (6, 1.0), (6, -0.5), (6, float("nan")), (7, 0.0), (7, float("nan"))):
        table = q["table"].copy()
        table[11, col] = bad
        assert _call(lib, [4000], [0], table=table) == E and "table" in err(), (col, bad)
    for bad in (-2, 66):
        assert _call(lib, [4000], [0], split=[bad]) == E and "split" in err()
    assert _call(lib, [4000], [0], split=[65], ws_bytes=0) == _lib.ERR_WORKSPACE                 # (n_bands itself: no band above)
    assert _call(lib, [4000, 5000], [2]) == E and "tgt_index" in err()
    assert _call(lib, [4000, 5000], [0, -1]) == E and "tgt_index" in err()
    assert _call(lib, [-3], [0]) == E and "lengths" in err()
    assert _call(lib, [1 << 29], [0]) == E and "lengths" in err()
    assert _call(lib, [4000], [0], out=None) == E and "null" in err()
    for name in ("weights", "bins", "table", "split"):
        assert _call(lib, [4000], [0], null=(name,)) == E and "null" in err()
    tl, tp = _i32([4000, 9000])
    idx, ip = _i32([1, 1, 0])
    need = lib.ssr_nmr_workspace_bytes(tp, 2, ip, 3, 256, 65)
    assert need > 0 and lib.ssr_nmr_workspace_bytes(tp, 2, ip, 3, 256, 100) > need
    # one mask row of n_bands doubles per frame of a target, one row of n_bands + 2 doubles per chunk of 32 frames of a pair
    z, zp = _i32([0])
    a, ap = _i32([256 + 31 * 128])
    b, bp = _i32([256 + 32 * 128])
    more = lib.ssr_nmr_workspace_bytes(bp, 1, zp, 1, 256, 65) - lib.ssr_nmr_workspace_bytes(ap, 1, zp, 1, 256, 65)
    assert abs(more - (65 * 8 + 67 * 8)) < 512                                       # (areas are rounded to 256 bytes)
    assert _call(lib, [4000, 9000], [1, 1, 0], ws_bytes=need - 1) == _lib.ERR_WORKSPACE and "workspace" in err()
    assert _call(lib, [4000, 9000], [1, 1, 0], ws=None) == _lib.ERR_WORKSPACE
    bad, bdp = _i32([2])
    assert lib.ssr_nmr_workspace_bytes(tp, 2, bdp, 1, 256, 65) == 0
    assert lib.ssr_nmr_workspace_bytes(tp, 2, ip, 3, 1000, 65) == 0
    assert lib.ssr_nmr_workspace_bytes(tp, 2, ip, 3, 256, 0) == 0
    assert lib.ssr_nmr_workspace_bytes(tp, 2, ip, 3, 256, 129) == 0
    neg, ngp = _i32([4000, -1])
    assert lib.ssr_nmr_workspace_bytes(ngp, 2, ip, 3, 256, 65) == 0
    # one workgroup of n_fft / 8 threads per chunk of 32 frames: 2^32 threads are refused before anything is queued
    many, mp = _i32([(1 << 29) - 1])
    rep, rp = _i32([0] * 1100)
    assert lib.ssr_nmr_workspace_bytes(mp, 1, rp, 1100, 256, 1) > 0
    assert _call(lib, [(1 << 29) - 1], [0] * 1100, n_bands=1, ws_bytes=1 << 62) == _lib.ERR_UNSUPPORTED and "too large" in err()
    # a workgroup of 128 threads per target (mask) and per estimate (score): 2^25 of either are 2^32 threads
    assert _call(lib, np.zeros(1 << 25, np.int32), [0], ws_bytes=1 << 62) == _lib.ERR_UNSUPPORTED and "too large" in err()
    assert _call(lib, [4000], np.zeros(1 << 25, np.int32), ws_bytes=1 << 62) == _lib.ERR_UNSUPPORTED and "too large" in err()
    assert _call(lib, np.zeros((1 << 25) - 1, np.int32), [0], ws_bytes=0) == _lib.ERR_WORKSPACE
    assert _call(lib, [4000], [], n_est=0, ws=None, ws_bytes=0, out=None, null=("weights", "bins", "table", "split")) == 0      # nothing queued


def test_header_ctypes_table_and_library_agree():
    from ssr_eval_amd import _lib
    path = os.path.join(ROOT, "ssr_eval_amd", "csrc", "ssr_hip_nmr.h")
    header = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    declared = set(re.findall(r"\b(ssr_[a-z_0-9]+)\s*\(", header))
    assert declared == {"ssr_nmr", "ssr_nmr_workspace_bytes"} == set(_lib.NMR_SIGNATURES)
    others = set(_lib.SIGNATURES) | set(_lib.COHERENCE_SIGNATURES) | set(_lib.LOUDNESS_SIGNATURES) | set(_lib.SPECTRUM_SIGNATURES) | \
        set(_lib.AUDITORY_SIGNATURES) | set(_lib.MODULATION_SIGNATURES) | set(_lib.DISTRIBUTION_SIGNATURES) | set(_lib.CSII_SIGNATURES) | \
        set(_lib.ALIGN_SIGNATURES)
    assert not set(_lib.NMR_SIGNATURES) & others
    assert "#define SSR_NMR_BANDS 128" in header and "#define SSR_NMR_COLUMNS 6" in header and "#define SSR_NMR_TABLE 8" in header
    assert (_lib.NMR_BANDS, _lib.NMR_COLUMNS, _lib.NMR_TABLE) == (128, 6, 8)
    for name, n in (("ssr_nmr", 22), ("ssr_nmr_workspace_bytes", 6)):
        n_args = len(re.search(r"\b%s\((.*?)\);" % name, header, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.NMR_SIGNATURES[name][1]) == n, name
    lib = _lib.load()
    for name, (res, args) in _lib.NMR_SIGNATURES.items():
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    main = open(os.path.join(ROOT, "include", "ssr_hip.h")).read()
    assert main.count("#include \"../ssr_eval_amd/csrc/ssr_hip_nmr.h\"") == 1
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T ssr_nmr\n" in exported and " T ssr_nmr_workspace_bytes\n" in exported
    # the header is C99 on its own behind the main one
    src = "#include \"%s\"\nint main(void) { return ssr_nmr_workspace_bytes(0, 0, 0, 0, 256, 65) != 0 || SSR_NMR_BANDS != 128; }\n" % \
        os.path.join(ROOT, "include", "ssr_hip.h")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-"], input=src, text=True, check=True)


# ---- AudioMetrics / SSR_Eval_Helper options --------------------------------------------------------------------------------------
def test_audio_metrics_nmr_options():
    """Everything here is refused before any device is touched (this test runs without one)."""
    from ssr_eval_amd import AudioMetrics
    bk = B()
    assert [bk.nmr_default_nfft(fs) for fs in (8000, 16000, 16001, 24000, 32000, 44100, 48000, 192000)] == [256, 512, 1024, 1024, 1024, 2048, 2048, 2048]
    for bad in (7999, 192001, 0, -1, True, None, "16000", float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rate from 8000 to 192000 Hz"):
            bk.nmr_default_nfft(bad)
    for bad in ({"n_fft": 1000}, {"n_fft": 4096}, {"n_fft": 256.0}, {"level_db": -1}, {"level_db": 201}, {"level_db": "92"}, {"level_db": True},
                {"level_db": float("nan")}):
        with pytest.raises(ValueError):
            bk.nmr_design(16000, **bad)
    am = AudioMetrics(16000)
    fc = bk.nmr_design(16000)["fc"]
    names = ("nmr", "nmr_seg", "rdf", "nmr_hf", "nmr_lf")
    assert am._nmr_names(None) == names and am._nmr_names(["rdf", "nmr"]) == ("nmr", "rdf")
    assert am._nmr_splits(fc, None, 2) == [-1, -1] and am._nmr_splits(fc, 4000.0, 2) == [67, 67]
    assert am._nmr_splits(fc, [None, 1e9, 0.0, float(fc[10]), float(fc[10]) + 1e-6], 5) == [-1, 84, 0, 10, 11]
    x = np.zeros(3000, np.float32)
    for kw in ({"n_fft": 300}, {"n_fft": 1024.0}, {"level_db": -3}, {"level_db": None}, {"split_hz": -5}, {"split_hz": "x"}, {"split_hz": True},
               {"split_hz": float("inf")}, {"split_hz": [4000.0, 2000.0]}, {"names": ()}, {"names": "nmr"}, {"names": ("nope",)}, {"return_bands": 1}):
        with pytest.raises(ValueError):                                          # rejected before any device is touched
            am.nmr(x, x, **kw)
        with pytest.raises(ValueError):
            am.nmr_batch([x], [x], **kw)
        with pytest.raises(ValueError):
            am.nmr_multi([[x]], [x], **kw)
    with pytest.raises(ValueError):
        am.nmr_multi([[x], [x]], [x], split_hz=[1000.0])
    with pytest.raises(ValueError):
        am.nmr(np.zeros((2, 3000), np.float32), x)
    with pytest.raises(ValueError):
        am.masking_threshold(np.zeros((2, 3000), np.float32))
    with pytest.raises(ValueError, match="rate from 8000 to 192000 Hz"):
        AudioMetrics(4000).nmr(x, x)
    for kw in ({"split_bands": [-2]}, {"split_bands": [85]}, {"split_bands": [1, 2]}, {"n_fft": 100}, {"level_db": 500}, {"return_bands": "yes"},
               {"return_mask": 1}):
        with pytest.raises(ValueError):
            bk.nmr_metrics([x], [x], [0], 16000, **kw)
    with pytest.raises(ValueError, match="tgt_index out of range"):
        bk.nmr_metrics([x], [x], [1], 16000)
    with pytest.raises(ValueError, match="one target index per estimate"):
        bk.nmr_metrics([x], [x], [0, 0], 16000)


def test_helper_nmr_option_and_the_registry():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd import eval as E
    mk = lambda sr=44100, **kw: SSR_Eval_Helper(BasicTestee(), sr, sr, evaluation_sr=sr, test_data_root=None, **kw)      # noqa: E731
    assert mk().nmr is None and mk(nmr=None).nmr is None and mk(nmr=True).nmr is True
    ok = {"n_fft": 1024, "level_db": 96.0, "split": 4000.0}
    assert mk(nmr=ok).nmr == ok and mk(nmr={"split": 0}).nmr == {"split": 0}
    messages = {"nmr must be None, True or a dict": (False, 1, "all", "nmr", (), ("rdf",), {}, {"which": "rdf"}, [True], {"split_hz": 4000}, {"hop": 512}),
                "n_fft must be one of": ({"n_fft": 1000}, {"n_fft": 4096}, {"n_fft": 1024.0}, {"n_fft": None}),
                "level_db must be a number": ({"level_db": -1.0}, {"level_db": "92"}, {"level_db": None}),
                "split must be a frequency": ({"split": None}, {"split": "4000"}, {"split": [4000.0]}, {"split": True}),
                "a split frequency is a finite number": ({"split": -5.0}, {"split": float("inf")})}
    for message, values in messages.items():
        for bad in values:
            with pytest.raises(ValueError, match=message):
                mk(nmr=bad)
    with pytest.raises(ValueError, match="rate from 8000 to 192000 Hz"):
        mk(4000, nmr=True)
    params = inspect.signature(SSR_Eval_Helper.__init__).parameters
    assert params["nmr"].kind is inspect.Parameter.KEYWORD_ONLY and params["nmr"].default is None
    # the pinned tuples and their order functions are what they were; the open tuple is queued behind them
    assert [f.option for f in E._TAIL_FAMILIES] == ["loudness", "bandwidth", "modulation", "auditory"]
    assert [f.option for f in E._LATER_FAMILIES] == ["coherence"] and len(E._FAMILIES) == 10 and [f.option for f in E._NEWER_FAMILIES] == ["csii"]
    assert E._ALL_FAMILIES == E._FAMILIES + E._LATER_FAMILIES + E._TAIL_FAMILIES + E._NEWER_FAMILIES and len(E._ALL_FAMILIES) == 16
    assert len(E.every_key_order()) == 56 and E.every_key_order()[-4:] == ("csii", "csii_mid", "i3", "csii_hf")
    assert [f.option for f in E._OPEN_FAMILIES] == ["nmr"] and not set(E._OPEN_FAMILIES) & set(E._ALL_FAMILIES)
    fam = E._OPEN_FAMILIES[0]
    assert fam.keys == ("nmr", "rdf", "nmr_hf") and fam.per_key is True and (fam.multi, fam.batch) == ("nmr_multi", "nmr_batch")
    assert not set(fam.keys) & set(E.every_key_order()) and not set(fam.keys) & set(E.ALIGN_KEYS)
    assert E.open_key_order() == E.every_key_order() + fam.keys + E.ALIGN_KEYS and len(set(E.open_key_order())) == 61
    keys = ["proc_fft_8000_44100", "proc_mp3_32k_44100"]
    args, kw = fam.arguments(mk(nmr=True), keys)
    assert args == ([4000, None], None, 92.0) and kw == {"names": fam.keys}
    args, kw = fam.arguments(mk(nmr=ok), keys)
    assert args == ([4000.0, 4000.0], 1024, 96.0) and kw == {"names": fam.keys}
