"""Float64 NumPy statement of the waveform metrics: SNR, zero-mean SI-SDR (Le Roux et al. 2019) and segmental SNR
(Loizou, Speech Enhancement: Theory and Practice, §11.1, comp_snr.m).

Test infrastructure: the yardstick of ssr_wave_metrics, written from the definitions, with every residual formed sample by
sample.  x is the target (clean), y the estimate; both are widened to float64 (exact for float32) whatever their dtype.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
SEG_LO, SEG_HI = -10.0, 35.0


def frame_geometry(fs, n):
    """-> (L, R, M): frame length (30 ms rounded half up), hop, and comp_snr.m's frame count max(0, (n - L) // R)."""
    L = (3 * int(fs) + 50) // 100
    R = L // 4
    M = max(0, (int(n) - L) // R) if R > 0 else 0
    return L, R, M


def _pair(x, y):
    x, y = np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64)
    assert x.shape == y.shape and x.ndim == 1
    return x, y


def snr(x, y):
    x, y = _pair(x, y)
    if len(x) == 0:
        return float("nan")
    d = x - y
    return float(10 * np.log10((np.sum(x * x) + EPS) / (np.sum(d * d) + EPS)))


def si_sdr(x, y):
    x, y = _pair(x, y)
    if len(x) == 0:
        return float("nan")
    x0, y0 = x - np.mean(x), y - np.mean(y)
    alpha = (np.sum(x0 * y0) + EPS) / (np.sum(x0 * x0) + EPS)
    s = alpha * x0
    r = s - y0
    return float(10 * np.log10((np.sum(s * s) + EPS) / (np.sum(r * r) + EPS)))


def seg_snr(x, y, fs):
    x, y = _pair(x, y)
    L, R, M = frame_geometry(fs, len(x))
    if M == 0:
        return float("nan")
    w = 0.5 * (1 - np.cos(2 * np.pi * np.arange(1, L + 1) / (L + 1)))
    seg = np.empty(M)
    for j in range(M):
        c = w * x[j * R:j * R + L]
        e = w * (x[j * R:j * R + L] - y[j * R:j * R + L])
        S, N = np.sum(c * c), np.sum(e * e)
        seg[j] = min(max(10 * np.log10(S / (N + EPS) + EPS), SEG_LO), SEG_HI)
    return float(np.mean(seg))


def waveform(x, y, fs):
    return {"snr": snr(x, y), "si_sdr": si_sdr(x, y), "seg_snr": seg_snr(x, y, fs)}
