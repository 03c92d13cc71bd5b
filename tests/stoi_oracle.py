"""Float64 NumPy / SciPy restatement of STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) as pystoi 0.3.x computes them.

Test infrastructure: the yardstick of ssr_stoi, written from the algorithm's published description, not from a
pinned copy of pystoi.  Differences from pystoi, by design: ESTOI adds no EPS-scale random noise before its normalisations
and divides by (norm + EPS) instead (deterministic; a silent band or frame normalises to zeros); a signal with no frame at all
(<= 256 samples at 10 kHz) scores 1e-5 instead of raising.
"""
from math import gcd

import numpy as np
from scipy.signal import resample_poly

FS = 10000
N_FRAME = 256
NFFT = 512
NUMBAND = 15
MINFREQ = 150
N = 30
BETA = -15.0
DYN_RANGE = 40
EPS = np.finfo(float).eps
SHORT = 1e-5


def octave_window(p, q):
    """pystoi.utils.resample_oct's filter for resample_poly(x, p, q), p / q already reduced, normalised to unit sum."""
    stop = 1.0 / (2 * max(p, q))
    roll = stop / 10
    rej_db = 60.0
    L = int(np.ceil((rej_db - 8) / (28.714 * roll)))
    t = np.arange(-L, L + 1)
    ideal = 2 * p * stop * np.sinc(2 * stop * t)
    h = np.kaiser(2 * L + 1, 0.1102 * (rej_db - 8.7)) * ideal
    return h / np.sum(h)


def resample_to_fs(x, fs):
    x = np.asarray(x)
    if fs == FS:
        return x.astype(np.float64)
    g = gcd(FS, int(fs))
    p, q = FS // g, int(fs) // g
    return resample_poly(x, p, q, window=octave_window(p, q))


def thirdoct():
    """-> (OBM [15, 257], lo [15], hi [15]) of pystoi.utils.thirdoct(10000, 512, 15, 150)."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(NUMBAND, dtype=float)
    lo_f = MINFREQ * np.power(2.0, (2 * k - 1) / 6)
    hi_f = MINFREQ * np.power(2.0, (2 * k + 1) / 6)
    obm = np.zeros((NUMBAND, len(f)))
    lo, hi = np.zeros(NUMBAND, int), np.zeros(NUMBAND, int)
    for i in range(NUMBAND):
        lo[i] = np.argmin(np.square(f - lo_f[i]))
        hi[i] = np.argmin(np.square(f - hi_f[i]))
        obm[i, lo[i]:hi[i]] = 1
    return obm, lo, hi


def _window():
    return np.hanning(N_FRAME + 2)[1:-1]


def remove_silent_frames(x, y):
    """Frames of the target 40 dB below its loudest removed from both signals, the rest overlap-added (hop 128)."""
    w, hop = _window(), N_FRAME // 2
    starts = range(0, len(x) - N_FRAME, hop)
    xf = np.array([w * x[i:i + N_FRAME] for i in starts]).reshape(-1, N_FRAME)
    yf = np.array([w * y[i:i + N_FRAME] for i in starts]).reshape(-1, N_FRAME)
    if len(xf) == 0:
        return np.zeros(0), np.zeros(0)
    e = 20 * np.log10(np.linalg.norm(xf, axis=1) + EPS)
    mask = (np.max(e) - DYN_RANGE - e) < 0
    xf, yf = xf[mask], yf[mask]

    def ola(fr):
        out = np.zeros((len(fr) + 1) * hop)
        for j, f in enumerate(fr):
            out[j * hop:j * hop + N_FRAME] += f
        return out
    return ola(xf), ola(yf)


def band_image(x, obm):
    """[15, T] one-third-octave band magnitudes of the STFT (frames range(0, len - 256, 128), rfft n = 512)."""
    w = _window()
    spec = np.array([np.fft.rfft(w * x[i:i + N_FRAME], n=NFFT) for i in range(0, len(x) - N_FRAME, N_FRAME // 2)])
    spec = spec.reshape(-1, NFFT // 2 + 1)
    return np.sqrt(obm @ np.square(np.abs(spec)).T)


def _segments(a):
    return np.array([a[:, m - N:m] for m in range(N, a.shape[1] + 1)])


def _normalise(v, axis):
    v = v - np.mean(v, axis=axis, keepdims=True)
    return v / (np.linalg.norm(v, axis=axis, keepdims=True) + EPS)


def stoi_10k(x, y, extended=False):
    """STOI / ESTOI of 10 kHz float64 signals (x clean, y processed, equal lengths)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    assert x.shape == y.shape
    xs, ys = remove_silent_frames(x, y)
    obm = thirdoct()[0]
    xt, yt = band_image(xs, obm), band_image(ys, obm)
    if xt.shape[1] < N:
        return SHORT
    xseg, yseg = _segments(xt), _segments(yt)              # [J, 15, 30]
    J = xseg.shape[0]
    if extended:
        xn = _normalise(_normalise(xseg, 2), 1)
        yn = _normalise(_normalise(yseg, 2), 1)
        return float(np.sum(xn * yn / N) / J)
    alpha = np.linalg.norm(xseg, axis=2, keepdims=True) / (np.linalg.norm(yseg, axis=2, keepdims=True) + EPS)
    yp = np.minimum(yseg * alpha, xseg * (1 + 10 ** (-BETA / 20)))
    return float(np.sum(_normalise(yp, 2) * _normalise(xseg, 2)) / (J * NUMBAND))


def stoi(x, y, fs, extended=False):
    """pystoi.stoi(x, y, fs, extended) restated: x clean (target), y processed (estimate), both at fs."""
    return stoi_10k(resample_to_fs(x, fs), resample_to_fs(y, fs), extended)


def speech_like(rng, n, fs, silences=((0.3, 0.45), (0.7, 0.8))):
    """A test signal: a few modulated harmonic tones plus noise, with digital-silence stretches (fractions of the length) that
    the voice-activity mask removes from the middle of the signal."""
    t = np.arange(n) / fs
    f0 = 120 + 40 * rng.random()
    x = sum(np.sin(2 * np.pi * f0 * h * t + rng.random() * 6) / h for h in range(1, 12))
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * t)) + 0.05 * rng.standard_normal(n)
    for a, b in silences:
        x[int(a * n):int(b * n)] = 0.0
    return x.astype(np.float64)
