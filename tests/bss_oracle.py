"""Float64 oracle of the filter-invariant SDR: BSS Eval's SDR (Vincent, Gribonval & Févotte 2006) for one source with
a causal `taps`-tap FIR filter of the target as the allowed distortion - the definition of mir_eval.separation.bss_eval_sources
restated with NumPy and SciPy.  Test infrastructure only; nothing in ssr_eval_amd imports it."""
import numpy as np
import scipy.linalg
import scipy.signal

EPS = float(np.finfo(np.float64).eps)
MAX_TAPS = 512


def correlations(x, y, taps):
    """r[k] = Σ_{t<n-k} x[t] x[t+k], b[k] = Σ_{t<n-k} x[t] y[t+k], k < taps, by direct dot products (k >= n: no term exists)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = len(x)
    r, b = np.zeros(taps), np.zeros(taps)
    for k in range(min(taps, n)):
        r[k] = np.dot(x[:n - k], x[k:])
        b[k] = np.dot(x[:n - k], y[k:])
    return r, b


def projection_filter(x, y, taps=MAX_TAPS, levinson=False):
    """c with Toeplitz(r) c = b: the dense positive-definite solve, or SciPy's Levinson recursion."""
    r, b = correlations(x, y, taps)
    if levinson:
        return scipy.linalg.solve_toeplitz(r, b)
    return scipy.linalg.solve(scipy.linalg.toeplitz(r), b, assume_a="pos")


def sdr_of_filter(x, y, c):
    """10 log10((Σp² + EPS) / (Σe² + EPS)) with p = c * x over n + taps - 1 samples and e = y - p formed explicitly."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    p = np.convolve(x, c)
    e = np.concatenate([y, np.zeros(len(p) - len(y))]) - p
    return float(10.0 * np.log10((np.sum(p * p) + EPS) / (np.sum(e * e) + EPS)))


def bss_sdr(x, y, taps=MAX_TAPS, levinson=False):
    """-> (sdr, sdr_lag, c).  n = 0 or a digitally silent target: (NaN, NaN, zeros)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if len(x) != len(y):
        raise ValueError("the estimate must be as long as its target")
    if not 1 <= taps <= MAX_TAPS:
        raise ValueError("taps must be in [1, %d]" % MAX_TAPS)
    if len(x) == 0 or not np.any(x):
        return float("nan"), float("nan"), np.zeros(taps)
    c = projection_filter(x, y, taps, levinson)
    return sdr_of_filter(x, y, c), float(np.argmax(np.abs(c))), c


def closed_form_one_tap(x, y):
    """taps = 1: 10 log10(a² Σx² / Σ(y - a x)²), a = Σxy / Σx² - the non-zero-mean scale-invariant SDR - with EPS added to both sums
    as everywhere (at 100 dB the EPS in the denominator is worth 1e-7 dB on a short signal)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    a = np.dot(x, y) / np.dot(x, x)
    return float(10.0 * np.log10((a * a * np.dot(x, x) + EPS) / (np.sum((y - a * x) ** 2) + EPS)))


# ---- the inputs the host and the GPU tests share --------------------------------------------------------------------------------
FS, N = 48000, 24000


def targets(seed=0, n=N):
    """white, Butterworth-low-passed and FFT-brickwalled noise, a 440 Hz sine, a constant (float64)."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n)
    spec = np.fft.rfft(w)
    spec[np.fft.rfftfreq(n, 1.0 / FS) > 4000.0] = 0.0
    return {"white": 0.1 * w,
            "lowpass": 0.1 * scipy.signal.sosfilt(scipy.signal.butter(4, 4000.0, fs=FS, output="sos"), w),
            "brickwall": 0.1 * np.fft.irfft(spec, n),
            "sine": 0.5 * np.sin(2.0 * np.pi * 440.0 * np.arange(n) / FS),
            "constant": np.full(n, 0.25)}


def estimates(x, seed=1):
    """20 dB and 100 dB of added white noise, and the target delayed by 37 samples and scaled by 0.7."""
    rng = np.random.default_rng(seed)
    rms = float(np.sqrt(np.mean(x * x)))
    return {"20dB": x + rms * 10.0 ** (-20 / 20) * rng.standard_normal(len(x)),
            "100dB": x + rms * 10.0 ** (-100 / 20) * rng.standard_normal(len(x)),
            "delayed": 0.7 * np.concatenate([np.zeros(37), x[:-37]])}


def exact_fir_pair(L, n=4099, seed=5):
    """x with its last L - 1 samples zero, y = the first n samples of h * x for a random decaying h: y lies in the span exactly."""
    rng = np.random.default_rng(seed + L)
    x = 0.1 * rng.standard_normal(n)
    if L > 1:
        x[-(L - 1):] = 0.0
    h = rng.standard_normal(L) * np.exp(-np.arange(L) / (1.0 + L / 8.0))
    return x, np.convolve(x, h)[:n], h
