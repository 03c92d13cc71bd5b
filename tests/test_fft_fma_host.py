"""CPU tests of the wave engines' fused radix-8 passes (ssr_fft.h: ssr_bfly8_tw; ssr_stft_wave.h: SSR_W_FFT_TAIL_X), through a g++
build of the kernel bodies (tests/emu/fft_fma_emu.cpp).

* The butterfly alone against the exact twiddled DFT (long double) and against the sequence it replaces - seven complex multiplies,
  then ssr_bfly8, which the block engines keep (ssr_fft_compute_tw).
* The 2048-point tail (split, full and paired exchange) and the 1536-point tail as whole transforms against numpy's long-double FFT.

Bounds.  Butterfly: the new form may deviate from the exact DFT by at most FACTOR = 2 times what the old sequence deviates on the
same inputs.  Counting roundings per output, the old sequence has 5 (multiply 2, three addition layers) and the new one up to 9 (three
layers of: two chained fused multiply-adds, plus one more on the `2 a - p` output): sqrt(9 / 5) = 1.35 if they were independent and
equally large; 2 leaves room for the maximum over a batch.  Measured (float64 | float32), largest deviation new / old, 4000 butterflies per
class:  random twiddles 0.98 | 0.53,  t = 1  0.97 | 1.09,  multiples of 45 degrees 1.22 | 1.03  (old sequence's own deviation: 2.9e-16 to
3.5e-16 and 1.4e-7 to 3.3e-7 of the largest output).
Tails: relative to the spectrum's largest bin, 4 eps for an impulse and 2 eps for Gaussian noise - the bound the engine met BEFORE the
passes were fused (parent commit, the same inputs: float64 7.04e-16 = 3.2 eps and 3.54e-16 = 1.6 eps at 2048 points, 6.64e-16 and 3.08e-16
at 1536; float32 3.00e-7 = 2.5 eps and 1.77e-7 = 1.5 eps, 3.01e-7 and 1.78e-7).  The fused passes: float64 7.53e-16 and 3.34e-16, float32 3.23e-7
and 2.10e-7 at 2048 points (the 1536-point tail keeps its multiplies, see ssr_fft24.h)."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SRC = os.path.join(ROOT, "tests", "emu", "fft_fma_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libfft_fma_emu.so")
FACTOR = 2.0
LD = np.longdouble
TWO_PI = 2 * np.arccos(LD(-1))


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    return C.CDLL(EMU_SO)


def _ct(dt):
    return C.c_double if dt == np.float64 else C.c_float


def bfly(lib, which, x, tw, dt):
    """x: [8] complex, tw: [3] complex (t, t^2, t^4) -> [8] complex long double of the dt arithmetic's result."""
    a = np.ascontiguousarray(np.stack([x.real, x.imag], -1).astype(dt))
    w = np.ascontiguousarray(np.stack([tw.real, tw.imag], -1).astype(dt))
    o = np.zeros_like(a)
    fn = lib.fma_bfly8_f64 if dt == np.float64 else lib.fma_bfly8_f32
    fn(which, a.ctypes.data_as(C.POINTER(_ct(dt))), w.ctypes.data_as(C.POINTER(_ct(dt))), o.ctypes.data_as(C.POINTER(_ct(dt))))
    return o[:, 0].astype(LD) + 1j * o[:, 1].astype(LD)


def exact_bfly(x, theta, dt):
    """X_k = sum_q x_q exp(-i theta q) W8^(q k) in long double, x rounded to dt first (what the butterfly is given)."""
    xr = x.real.astype(dt).astype(LD) + 1j * x.imag.astype(dt).astype(LD)
    q = np.arange(8).astype(LD)
    tq = np.cos(theta * q) - 1j * np.sin(theta * q)
    return np.fft.fft(xr * tq)


def twiddles(theta):
    m = np.array([1, 2, 4]).astype(LD)
    return np.cos(theta * m) - 1j * np.sin(theta * m)            # each power rounded from its exact value, as the tables hold them


THETAS = {
    "random": lambda rng, i: TWO_PI * LD(rng.random()),
    "one": lambda rng, i: LD(0),                                  # lane 0 / butterfly 0: t = 1
    "octants": lambda rng, i: TWO_PI * LD(i % 8) / 8,             # t at multiples of 45 degrees
}


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("kind", sorted(THETAS))
def test_fused_butterfly_is_the_twiddled_dft_as_closely_as_the_multiply_form(emu, kind, dt):
    rng = np.random.default_rng(2024)
    eps = np.finfo(dt).eps
    dev_new = dev_old = 0.0
    for i in range(4000):
        theta = THETAS[kind](rng, i)
        x = rng.standard_normal(8) + 1j * rng.standard_normal(8)
        tw = twiddles(theta)
        want = exact_bfly(x, theta, dt)
        new, old = bfly(emu, 0, x, tw, dt), bfly(emu, 1, x, tw, dt)
        scale = float(np.abs(want).max())
        dev_new = max(dev_new, float(np.abs(new - want).max()) / scale)
        dev_old = max(dev_old, float(np.abs(old - want).max()) / scale)
        assert float(np.abs(new - old).max()) / scale <= 16 * eps      # the two forms agree output for output (v[k] = X_k)
    print("%s %s: largest deviation new %.3e old %.3e ratio %.2f" % (kind, np.dtype(dt).name, dev_new, dev_old, dev_new / dev_old))
    assert 0 < dev_old <= 8 * eps
    assert dev_new <= FACTOR * dev_old


def test_fused_butterfly_exact_cases(emu):
    """t = 1 and an impulse: every output is the input itself, bit for bit (1 * x + 0 and 2 x - x round nothing); a power-of-two
    scaling of the inputs scales every output exactly."""
    one = twiddles(LD(0))
    for q in range(8):
        x = np.zeros(8, complex)
        x[q] = 0.3 - 0.7j
        got = bfly(emu, 0, x, one, np.float64)
        want = (0.3 - 0.7j) * np.array([1, (1 - 1j) / np.sqrt(2), -1j, (-1 - 1j) / np.sqrt(2), -1, (-1 + 1j) / np.sqrt(2), 1j, (1 + 1j) / np.sqrt(2)]) ** q
        assert float(np.abs(got - want).max()) <= 4 * np.finfo(np.float64).eps
    got = bfly(emu, 0, np.array([0.3 - 0.7j] + [0] * 7), one, np.float64)
    assert (got == got[0]).all() and complex(got[0]) == 0.3 - 0.7j
    rng = np.random.default_rng(3)
    x = rng.standard_normal(8) + 1j * rng.standard_normal(8)
    tw = twiddles(LD(0.7))
    assert (bfly(emu, 0, 0.125 * x, tw, np.float64) == 0.125 * bfly(emu, 0, x, tw, np.float64)).all()


def tail(lib, n, mode, z, dt):
    a = np.ascontiguousarray(np.stack([z.real, z.imag], -1).astype(dt))
    o = np.full_like(a, np.nan)
    fn = lib.fma_tail_f64 if dt == np.float64 else lib.fma_tail_f32
    assert fn(n, mode, a.ctypes.data_as(C.POINTER(_ct(dt))), o.ctypes.data_as(C.POINTER(_ct(dt)))) == 0
    want = np.fft.fft(a[:, 0].astype(LD) + 1j * a[:, 1].astype(LD))
    assert want.dtype == np.clongdouble
    return o[:, 0].astype(LD) + 1j * o[:, 1].astype(LD), want


def rel_err(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


# (n, mode): 2048 points through the split, the full and the paired second exchange; 1536 points
TAILS = [(2048, 0), (2048, 1), (2048, 2), (1536, 0)]


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n,mode", TAILS)
def test_tail_spectrum_of_an_impulse_at_every_in_lane_position(emu, n, mode, dt):
    worst = 0.0
    for r in range(n // 64):                                      # register r of lane (7 r + 3) mod 64
        z = np.zeros(n, complex)
        z[(7 * r + 3) % 64 + 64 * r] = 1.0 - 0.5j
        worst = max(worst, rel_err(*tail(emu, n, mode, z, dt)))
    print("impulse %d mode %d %s: %.3e" % (n, mode, np.dtype(dt).name, worst))
    assert worst <= 4 * np.finfo(dt).eps


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n,mode", TAILS)
def test_tail_spectrum_of_a_random_pair(emu, n, mode, dt):
    worst = 0.0
    for seed in range(8):
        rng = np.random.default_rng(100 + seed)
        z = rng.standard_normal(n) + 1j * rng.standard_normal(n)  # two real signals packed as one complex frame
        worst = max(worst, rel_err(*tail(emu, n, mode, z, dt)))
    print("random %d mode %d %s: %.3e" % (n, mode, np.dtype(dt).name, worst))
    assert worst <= 2 * np.finfo(dt).eps


def test_exchange_variants_give_the_same_bits(emu):
    rng = np.random.default_rng(5)
    z = rng.standard_normal(2048) + 1j * rng.standard_normal(2048)
    for dt in (np.float64, np.float32):
        ref = tail(emu, 2048, 0, z, dt)[0]
        for mode in (1, 2):
            assert (tail(emu, 2048, mode, z, dt)[0] == ref).all()
