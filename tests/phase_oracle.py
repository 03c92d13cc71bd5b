"""NumPy float64 oracle of the anti-wrapping phase distances: instantaneous phase (IP), group delay (GD) and
instantaneous angular frequency (IAF) of an estimate against its target.  Restated from Ai & Ling 2023 and AP-BWE (Lu et al. 2024):
framing and np.fft.rfft, the explicit zero rule, the three means - in the product form the kernels use (phase_distance) and in the
papers' literal anti-wrapping form f(u) = |u - 2 pi round(u / 2 pi)| on phase differences (phase_distance_literal).  Test
infrastructure; nothing in ssr_eval_amd imports it."""
import numpy as np

NAMES = ("phase_ip", "phase_gd", "phase_iaf")
N_FFTS = (256, 512, 1024, 2048)


def num_frames(n, n_fft, hop):
    """T = 1 + n // hop centred frames; 0 where the reflect padding of n_fft / 2 samples is undefined."""
    return 1 + n // hop if n > n_fft // 2 else 0


def spectra(x, n_fft, hop):
    """[T, n_fft / 2 + 1] complex128: centred frames, reflect padding, periodic Hann window."""
    x = np.asarray(x, np.float64)
    T = num_frames(len(x), n_fft, hop)
    xp = np.pad(x, n_fft // 2, mode="reflect")
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    idx = hop * np.arange(T)[:, None] + np.arange(n_fft)[None, :]
    return np.fft.rfft(xp[idx] * w, axis=-1)


def _band(n_fft, band_bins):
    lo, hi = (0, n_fft // 2) if band_bins is None else band_bins
    assert 0 <= lo <= hi <= n_fft // 2
    return int(lo), int(hi)


def a(z):
    """|arg z| in [0, pi]; 0 where both parts are zero, whatever their signs (np.angle(-0.0 + 0j) is pi)."""
    z = np.asarray(z)
    return np.where((z.real == 0) & (z.imag == 0), 0.0, np.abs(np.arctan2(z.imag, z.real)))


def _mean(v):
    return float(np.mean(v)) if v.size else float("nan")


def _nan():
    return {m: float("nan") for m in NAMES}


def phase_distance(x, y, n_fft=1024, hop=None, band_bins=None):
    """{'phase_ip', 'phase_gd', 'phase_iaf'} in radians of estimate y against target x (equal lengths)."""
    hop = n_fft // 4 if hop is None else hop
    lo, hi = _band(n_fft, band_bins)
    assert len(x) == len(y)
    if num_frames(len(x), n_fft, hop) == 0:
        return _nan()
    C = spectra(y, n_fft, hop) * np.conj(spectra(x, n_fft, hop))
    return {"phase_ip": _mean(a(C[:, lo:hi + 1])),
            "phase_gd": _mean(a(C[:, lo + 1:hi + 1] * np.conj(C[:, lo:hi]))),
            "phase_iaf": _mean(a(C[1:, lo:hi + 1] * np.conj(C[:-1, lo:hi + 1])))}


def anti_wrap(u):
    return np.abs(u - 2.0 * np.pi * np.round(u / (2.0 * np.pi)))


def phase_distance_literal(x, y, n_fft=1024, hop=None, band_bins=None):
    """The same three means as the papers write them: f() of the difference of the two signals' phases (IP), of their phase
    differences along frequency (GD) and along time (IAF).  Only for spectra without zeros (no zero rule here)."""
    hop = n_fft // 4 if hop is None else hop
    lo, hi = _band(n_fft, band_bins)
    if num_frames(len(x), n_fft, hop) == 0:
        return _nan()
    px, py = np.angle(spectra(x, n_fft, hop)), np.angle(spectra(y, n_fft, hop))
    d = py - px
    return {"phase_ip": _mean(anti_wrap(d[:, lo:hi + 1])),
            "phase_gd": _mean(anti_wrap(d[:, lo + 1:hi + 1] - d[:, lo:hi])),
            "phase_iaf": _mean(anti_wrap(d[1:, lo:hi + 1] - d[:-1, lo:hi + 1]))}


def conditioning(x, y, n_fft=1024, hop=None, band_bins=None):
    """The smallest |X[t][k]| / max_k |X[t]| and |Y[t][k]| / max_k |Y[t]| over the scored cells (the frame's maximum over ALL its
    bins: the transform's rounding error is relative to it) -> (r_x, r_y); (inf, inf) without frames.  Frames in which either
    signal is digitally silent are left out: their C is zero exactly, in the oracle and in the kernels."""
    hop = n_fft // 4 if hop is None else hop
    lo, hi = _band(n_fft, band_bins)
    if num_frames(len(x), n_fft, hop) == 0:
        return float("inf"), float("inf")
    mags = [np.abs(spectra(s, n_fft, hop)) for s in (x, y)]
    loud = (np.max(mags[0], axis=-1) > 0) & (np.max(mags[1], axis=-1) > 0)
    return tuple(float(np.min(m[loud, lo:hi + 1] / np.max(m[loud], axis=-1, keepdims=True), initial=np.inf)) for m in mags)
