"""NumPy float64 oracle of the multi-resolution STFT distance: spectral convergence and log-magnitude
distance of Parallel WaveGAN (Yamamoto et al. 2020) per resolution (n_fft, hop, win) and their means, written as the definition
reads: framing, np.fft.rfft, the clamp, the two norms.  Test infrastructure; nothing in ssr_eval_amd imports it."""
import numpy as np

NAMES = ("mrstft", "mrstft_sc", "mrstft_mag")
N_FFTS = (256, 512, 1024, 2048)
DEFAULT_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
EPS = 1e-7


def num_frames(n, n_fft, hop):
    """T = 1 + n // hop centred frames; 0 where the reflect padding of n_fft / 2 samples is undefined."""
    return 1 + n // hop if n > n_fft // 2 else 0


def window(n_fft, win):
    """The periodic Hann window of `win` samples at l = (n_fft - win) // 2 of an n_fft-point frame, zero elsewhere."""
    w = np.zeros(n_fft)
    l = (n_fft - win) // 2
    w[l:l + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    return w


def magnitudes(x, n_fft, hop, win, eps=EPS):
    """[T, n_fft / 2 + 1] float64: m = sqrt(max(|X|^2, eps)) of the centred, reflect-padded, windowed frames."""
    x = np.asarray(x, np.float64)
    T = num_frames(len(x), n_fft, hop)
    xp = np.pad(x, n_fft // 2, mode="reflect")
    idx = hop * np.arange(T)[:, None] + np.arange(n_fft)[None, :]
    X = np.fft.rfft(xp[idx] * window(n_fft, win), axis=-1)
    return np.sqrt(np.maximum(X.real ** 2 + X.imag ** 2, eps))


def resolution(x, y, n_fft, hop, win, band_bins=None, eps=EPS):
    """(sc, mag) of estimate y against target x (equal lengths) at one resolution; (nan, nan) without frames."""
    assert len(x) == len(y)
    lo, hi = (0, n_fft // 2) if band_bins is None else band_bins
    assert 0 <= lo <= hi <= n_fft // 2
    if num_frames(len(x), n_fft, hop) == 0:
        return float("nan"), float("nan")
    mx, my = (magnitudes(s, n_fft, hop, win, eps)[:, lo:hi + 1] for s in (x, y))
    sc = np.sqrt(np.sum((mx - my) ** 2) / np.sum(mx ** 2))
    return float(sc), float(np.mean(np.abs(np.log(mx) - np.log(my))))


def mrstft(x, y, resolutions=DEFAULT_RESOLUTIONS, bands=None, eps=EPS):
    """-> ({'mrstft', 'mrstft_sc', 'mrstft_mag'}, [(sc, mag) per resolution]); bands: None or one (k_lo, k_hi) or None per
    resolution.  The means add the resolutions in index order; NaN where any is NaN."""
    rows = [resolution(x, y, *res, None if bands is None else bands[r], eps) for r, res in enumerate(resolutions)]
    sc = mag = 0.0
    for s, m in rows:
        sc, mag = sc + s, mag + m
    sc, mag = sc / len(rows), mag / len(rows)
    return {"mrstft": sc + mag, "mrstft_sc": sc, "mrstft_mag": mag}, rows
