"""CPU tests of k_stft_wave's fused windowed first pass (ssr_stft_wave.h: ssr_dft32_win), through a g++ build of the kernel bodies
(tests/emu/pass0_emu.cpp).

* One lane's radix-32 DFT of the windowed packed frame: ssr_dft32_win against the sequence it replaces (window, then ssr_dft32) and
  against the exact DFT in long double.
* The whole windowed 2048-point transform of one wave (table requests where k_stft_wave makes them, window values formed per lane as
  it forms them) against numpy's long-double FFT of the frame times the window values the pass multiplied by, at the inputs of
  tests/test_fft_fma_host.py: the transform's own error, as in that file.
* The window values themselves (ssr_window_from_lane) against the exact window, in ulps of 1/4: they are accurate in ABSOLUTE terms, as a
  sum of terms of size 1/4 is - an impulse on one of the window's smallest samples (0.5 hann[1] = 2.4e-6) sees 1 ulp of 1/4 as 1.2e-11
  of ITS weight in float64, which is 2.8e-17 of a frame's largest possible weight.

Bounds: no new tolerance.  The new pass may deviate from the long-double result by at most FACTOR = 2 (the margin of
tests/test_fft_fma_host.py for the same comparison) times what the parent's pass deviates on the same class of inputs; the whole transform
keeps that file's bounds, 4 eps for an impulse and 2 eps for Gaussian noise relative to the largest bin.  Measured ratios: see
profiles/stft_pass0_notes.md."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SRC = os.path.join(ROOT, "tests", "emu", "pass0_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libpass0_emu.so")
FACTOR = 2.0                     # tests/test_fft_fma_host.py: FACTOR
LD = np.longdouble
TWO_PI = 2 * np.arccos(LD(-1))
N = 2048


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    return C.CDLL(EMU_SO)


def _p(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def _ct(dt):
    return C.c_double if dt == np.float64 else C.c_float


def lane_window(lane, dt):
    """wl[r] = 0.5 * hann[lane + 64 r], r < 16, rounded to dt as the plan's table is."""
    m = (lane + 64 * np.arange(16)).astype(LD)
    return (LD(0.25) - LD(0.25) * np.cos(TWO_PI * m / N)).astype(dt)


def dft32(lib, which, pa, pb, wl, dt):
    pa, pb = np.ascontiguousarray(pa, np.float32), np.ascontiguousarray(pb, np.float32)
    wl = np.ascontiguousarray(wl, dt)
    o = np.full((32, 2), np.nan, dt)
    fn = lib.pass0_dft32_f64 if dt == np.float64 else lib.pass0_dft32_f32
    fn(which, _p(pa, C.c_float), _p(pb, C.c_float), _p(wl, _ct(dt)), _p(o, _ct(dt)))
    return o[:, 0].astype(LD) + 1j * o[:, 1].astype(LD)


def exact_dft32(pa, pb, wl):
    """DFT32 of (pa + i pb) w in long double: the samples as float32, the window's first half as the table holds it, the second half
    1/2 - w exactly."""
    w = np.concatenate([wl.astype(LD), LD(0.5) - wl.astype(LD)])
    x = (np.asarray(pa, np.float32).astype(LD) + 1j * np.asarray(pb, np.float32).astype(LD)) * w
    k = np.arange(32).astype(LD)
    e = np.outer(k, k) * (TWO_PI / 32)
    return (np.cos(e) - 1j * np.sin(e)) @ x


def _impulses():
    for r in range(32):
        pa, pb = np.zeros(32, np.float32), np.zeros(32, np.float32)
        pa[r], pb[r] = 1.0, -0.5
        yield (7 * r + 3) % 64, pa, pb


def _gaussians():
    for seed in range(8):
        rng = np.random.default_rng(100 + seed)
        yield (11 * seed + 5) % 64, rng.standard_normal(32).astype(np.float32), rng.standard_normal(32).astype(np.float32)


def _silent():
    rng = np.random.default_rng(7)
    yield 9, np.zeros(32, np.float32), rng.standard_normal(32).astype(np.float32)
    yield 40, rng.standard_normal(32).astype(np.float32), np.zeros(32, np.float32)


CLASSES = {"impulse": _impulses, "gaussian": _gaussians, "silent": _silent}


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("kind", sorted(CLASSES))
def test_windowed_dft32_is_as_close_to_the_exact_dft_as_window_then_dft32(emu, kind, dt):
    eps = np.finfo(dt).eps
    dev_new = dev_old = agree = 0.0
    for lane, pa, pb in CLASSES[kind]():
        wl = lane_window(lane, dt)
        want = exact_dft32(pa, pb, wl)
        new, old = dft32(emu, 0, pa, pb, wl, dt), dft32(emu, 1, pa, pb, wl, dt)
        scale = float(np.abs(want).max())
        assert scale > 0
        dev_new = max(dev_new, float(np.abs(new - want).max()) / scale)
        dev_old = max(dev_old, float(np.abs(old - want).max()) / scale)
        agree = max(agree, float(np.abs(new - old).max()) / scale)
    print("%s %s: largest deviation new %.3e old %.3e ratio %.2f; new - old %.3e"
          % (kind, np.dtype(dt).name, dev_new, dev_old, dev_new / dev_old, agree))
    assert 0 < dev_old <= 8 * eps
    assert dev_new <= FACTOR * dev_old
    assert agree <= 16 * eps


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_windowed_dft32_of_silence_is_zero(emu, dt):
    """All-zero samples give exact zeros (no fused step may turn 0 * w + 0 into anything else), and a silent signal leaves its own
    spectrum exactly Hermitian-zero: with pb = 0 the packed spectrum is the real signal's, X[32 - k] = conj(X[k]) to rounding."""
    z = np.zeros(32, np.float32)
    got = dft32(emu, 0, z, z, lane_window(17, dt), dt)
    assert (got == 0).all()
    rng = np.random.default_rng(3)
    pa = rng.standard_normal(32).astype(np.float32)
    got = dft32(emu, 0, pa, z, lane_window(17, dt), dt)
    k = np.arange(1, 32)
    assert float(np.abs(got[32 - k] - np.conj(got[k])).max()) <= 16 * np.finfo(dt).eps * float(np.abs(got).max())


def frame(lib, which, a, b, dt):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    o, win = np.full((N, 2), np.nan, dt), np.zeros(N, dt)
    fn = lib.pass0_frame_f64 if dt == np.float64 else lib.pass0_frame_f32
    assert fn(which, _p(a, C.c_float), _p(b, C.c_float), _p(o, _ct(dt)), _p(win, _ct(dt))) == 0
    w = win.astype(LD)                                              # the lower half as pass 0 had it (formed per lane, or the table's)
    w[N // 2:] = LD(0.5) - w[:N // 2]                               # the upper half exactly: rounding 1/2 - w is the pass's own
    want = np.fft.fft((a.astype(LD) + 1j * b.astype(LD)) * w)
    assert want.dtype == np.clongdouble
    return o[:, 0].astype(LD) + 1j * o[:, 1].astype(LD), want


def exact_half_window():
    return LD(0.25) - LD(0.25) * np.cos(TWO_PI * np.arange(N).astype(LD) / N)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_window_formed_per_lane_is_the_hann_window(emu, dt):
    """ssr_window_from_lane: 0.5 hann[l + 64 r] = 1/4 - (CA cos_r - SA sin_r) by two fused multiply-adds.  Bound: 3 ulp of 1/4 - two
    roundings of values below 1/2 (1/2 ulp of 1/4 each), CA and SA rounded below 1/4 (1/4 ulp each, times |cos_r|, |sin_r| <= 1), the
    constants cos_r, sin_r rounded (2^-p relative of a product below 1/4: 1/2 ulp each): 2.5 ulp.  The plan's table is each value rounded
    once.  The upper half is 1/2 - w in both forms."""
    z = np.zeros(N, np.float32)
    ulp = float(np.spacing(dt(0.25)))
    exact = exact_half_window()
    wins = []
    for which in (0, 1):
        win = np.zeros(N, dt)
        o = np.zeros((N, 2), dt)
        fn = emu.pass0_frame_f64 if dt == np.float64 else emu.pass0_frame_f32
        assert fn(which, _p(z, C.c_float), _p(z, C.c_float), _p(o, _ct(dt)), _p(win, _ct(dt))) == 0
        wins.append(win.astype(LD))
    d_new, d_tab = np.abs(wins[0] - exact)[:N // 2], np.abs(wins[1] - exact)[:N // 2]
    print("%s: formed per lane within %.2f ulp(1/4) of the exact window, the table within %.2f; %d of %d values differ from the table's"
          % (np.dtype(dt).name, float(d_new.max()) / ulp, float(d_tab.max()) / ulp, int((wins[0] != wins[1])[:N // 2].sum()), N // 2))
    assert float(d_tab.max()) <= 0.5 * ulp
    assert float(d_new.max()) <= 3 * ulp
    assert wins[0][0] == 0                                           # sample 0 carries weight exactly 0 (the silent-frame vote relies on it)


def rel_err(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_windowed_transform_of_an_impulse_at_every_in_lane_position(emu, dt):
    worst = worst_old = 0.0
    for r in range(N // 64):                                      # register r of lane (7 r + 3) mod 64
        a, b = np.zeros(N, np.float32), np.zeros(N, np.float32)
        a[(7 * r + 3) % 64 + 64 * r], b[(7 * r + 3) % 64 + 64 * r] = 1.0, -0.5
        worst = max(worst, rel_err(*frame(emu, 0, a, b, dt)))
        worst_old = max(worst_old, rel_err(*frame(emu, 1, a, b, dt)))
    print("impulse %s: new %.3e parent's pass 0 %.3e" % (np.dtype(dt).name, worst, worst_old))
    assert worst <= 4 * np.finfo(dt).eps


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_windowed_transform_of_a_random_pair(emu, dt):
    worst = worst_old = 0.0
    for seed in range(8):
        rng = np.random.default_rng(100 + seed)
        z = rng.standard_normal(N) + 1j * rng.standard_normal(N)
        worst = max(worst, rel_err(*frame(emu, 0, z.real, z.imag, dt)))
        worst_old = max(worst_old, rel_err(*frame(emu, 1, z.real, z.imag, dt)))
    print("random %s: new %.3e parent's pass 0 %.3e" % (np.dtype(dt).name, worst, worst_old))
    assert worst <= 2 * np.finfo(dt).eps


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_windowed_transform_of_silence(emu, dt):
    z = np.zeros(N, np.float32)
    a, b = np.ascontiguousarray(z), np.ascontiguousarray(z)
    o, win = np.full((N, 2), np.nan, dt), np.zeros(N, dt)
    fn = emu.pass0_frame_f64 if dt == np.float64 else emu.pass0_frame_f32
    assert fn(0, _p(a, C.c_float), _p(b, C.c_float), _p(o, _ct(dt)), _p(win, _ct(dt))) == 0
    assert (o == 0).all()
    rng = np.random.default_rng(11)
    got, want = frame(emu, 0, z, rng.standard_normal(N), dt)      # one silent signal: the other one's spectrum stays as accurate
    assert rel_err(got, want) <= 2 * np.finfo(dt).eps
