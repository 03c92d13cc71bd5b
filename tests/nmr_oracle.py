"""Float64 oracle of the noise-to-mask family (nmr, nmr_seg, rdf, nmr_hf, nmr_lf): NumPy, the spreading over
frequency in its direct O(Nc^2) form with `** 0.4`, an explicit loop over the frames for the spreading over time.  Test
infrastructure; nothing here is imported by the package."""
import math

import numpy as np

N_FFTS = (256, 512, 1024, 2048)
FR = 32                                  # frames per chunk of the kernels (the seam the tests aim at)
DZ = 0.25                                # band width in Bark
FLOOR = 1e-20
RDF_DB = 1.5


def default_nfft(fs):
    return next((n for n in N_FFTS if n >= 0.032 * float(fs)), N_FFTS[-1])


def frames(n, N):
    return 1 + (n - N) // (N // 2) if n >= N else 0


def len_for_frames(K, N, extra=0):
    return N + (K - 1) * (N // 2) + extra


def bark(f):
    return 7.0 * np.arcsinh(np.asarray(f, np.float64) / 650.0)


def bark_inv(z):
    return 650.0 * np.sinh(np.asarray(z, np.float64) / 7.0)


def ear_weight_db(f_hz):
    f = np.asarray(f_hz, np.float64) / 1000.0
    with np.errstate(divide="ignore"):
        return -2.184 * f ** -0.8 + 6.5 * np.exp(-0.6 * (f - 3.3) ** 2) - 0.001 * f ** 3.6


def design(fs, N=None, level_db=92.0):
    """Every table of the definition as a dict: N, Nc, G, W2 [N/2+1], fl, fu, fc [Nc], U [Nc, N/2+1] dense, Ein, m_db, a (time),
    c_up = -24 - 230 / fc."""
    fs = float(fs)
    N = default_nfft(fs) if N is None else int(N)
    G = 10.0 ** (level_db / 10.0) / (N / 4.0) ** 2
    k = np.arange(N // 2 + 1, dtype=np.float64)
    W2 = np.zeros(N // 2 + 1)
    W2[1:] = 10.0 ** (ear_weight_db(k[1:] * fs / N) / 10.0)
    zL, zU = float(bark(80.0)), float(bark(min(18000.0, 0.45 * fs)))
    Nc = int(math.ceil((zU - zL) / DZ))
    lo = zL + DZ * np.arange(Nc)
    hi = np.minimum(lo + DZ, zU)
    fl, fu, fc = bark_inv(lo), bark_inv(hi), bark_inv(0.5 * (lo + hi))
    U = np.zeros((Nc, N // 2 + 1))
    width = fs / N
    for i in range(Nc):
        a = np.maximum((k - 0.5) * width, fl[i])
        b = np.minimum((k + 0.5) * width, fu[i])
        U[i] = np.maximum(b - a, 0.0) / width
    Ein = 10.0 ** (0.1456 * (fc / 1000.0) ** -0.8)
    idx = np.arange(Nc)
    m_db = np.where(idx <= 12.0 / DZ, 3.0, 0.25 * idx * DZ)
    tau = 0.008 + (100.0 / fc) * 0.022
    a_t = np.exp(-((N // 2) / fs) / tau)
    return dict(fs=fs, N=N, Nc=Nc, G=G, W2=W2, fl=fl, fu=fu, fc=fc, U=U, Ein=Ein, m_db=m_db, a=a_t, c_up=-24.0 - 230.0 / fc,
                level_db=float(level_db))


def stft(x, N):
    """[K, N/2+1] complex: periodic Hann, hop N/2, no padding."""
    x = np.asarray(x, np.float64)
    K = frames(len(x), N)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)
    H = N // 2
    return np.array([np.fft.rfft(w * x[t * H:t * H + N]) for t in range(K)]).reshape(K, N // 2 + 1)


def spread_matrix(Eb, d):
    """S [i, l] of one frame's band energies, every column divided by its own sum."""
    Nc = d["Nc"]
    L = 10.0 * np.log10(Eb)
    s_u = d["c_up"] + 0.2 * L
    i, l = np.arange(Nc)[:, None], np.arange(Nc)[None, :]
    with np.errstate(over="ignore"):
        S = np.where(i >= l, 10.0 ** (s_u[None, :] * (i - l) * DZ / 10.0), 10.0 ** (-2.7 * (l - i) * DZ))
    return S / S.sum(axis=0, keepdims=True)


def spread_raw(Eb, d):
    return ((Eb[None, :] * spread_matrix(Eb, d)) ** 0.4).sum(axis=1) ** 2.5


def spread(Eb, d):
    """Es of one frame."""
    if "Bs" not in d:
        d["Bs"] = spread_raw(np.ones(d["Nc"]), d)
    return spread_raw(Eb, d) / d["Bs"]


def time_spread(Es, d):
    """(Ef, E~) [K, Nc] of Es [K, Nc]: the explicit frame loop."""
    Ef = np.zeros_like(Es)
    prev = np.zeros(Es.shape[1])
    for t in range(Es.shape[0]):
        prev = d["a"] * prev + (1.0 - d["a"]) * Es[t]
        Ef[t] = prev
    return Ef, np.maximum(Ef, Es)


def excitation(x, d):
    """(Px [K, bins], Eb [K, Nc], Es [K, Nc]) of a target."""
    X = stft(x, d["N"])
    Px = d["G"] * d["W2"][None, :] * np.abs(X) ** 2
    Eb = Px @ d["U"].T + d["Ein"][None, :]
    Es = np.array([spread(e, d) for e in Eb]).reshape(len(Eb), d["Nc"])
    return Px, Eb, Es


def mask(x, d):
    """M [K, Nc] of a target."""
    _, _, Es = excitation(x, d)
    _, Et = time_spread(Es, d)
    return Et / 10.0 ** (d["m_db"][None, :] / 10.0)


def noise(x, y, d):
    """Pn [K, Nc]."""
    X, Y = stft(x, d["N"]), stft(y, d["N"])
    Pd = d["G"] * d["W2"][None, :] * (np.abs(X) - np.abs(Y)) ** 2
    return Pd @ d["U"].T


def _db(v):
    return 10.0 * np.log10(np.maximum(v, FLOOR))


def split_band(d, split_hz):
    return -1 if split_hz is None else int(np.searchsorted(d["fc"], float(split_hz), side="left"))


def nmr(x, y, fs, N=None, level_db=92.0, split_hz=None, d=None):
    """-> (columns [6]: nmr, nmr_seg, rdf, nmr_hf, nmr_lf, frames; bands [Nc] = mean_t R; frame_db [K] = 10 log10 max_i R; M; Pn)."""
    d = design(fs, N, level_db) if d is None else d
    n = min(len(x), len(y))
    x, y = np.asarray(x, np.float64)[:n], np.asarray(y, np.float64)[:n]
    K, Nc = frames(n, d["N"]), d["Nc"]
    if K == 0:
        return np.array([np.nan] * 5 + [0.0]), np.full(Nc, np.nan), np.zeros(0), np.zeros((0, Nc)), np.zeros((0, Nc))
    M, Pn = mask(x, d), noise(x, y, d)
    R = Pn / M
    s = split_band(d, split_hz)
    with np.errstate(divide="ignore"):
        frame_db = 10.0 * np.log10(R.max(axis=1))
    hf = float(_db(R[:, s:].mean())) if 0 <= s < Nc else np.nan
    lf = float(_db(R[:, :s].mean())) if s > 0 else np.nan
    cols = np.array([float(_db(R.mean())), float(np.mean(_db(R.mean(axis=1)))), float(np.mean(frame_db >= RDF_DB)), hf, lf, float(K)])
    return cols, R.mean(axis=0), frame_db, M, Pn


# ---- test signals -------------------------------------------------------------------------------------------------------------------
def music_like(n, fs, seed):
    """Partials of a few notes with slow envelopes over a noise floor 50 dB down: tonal maskers and gaps between them."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(fs)
    x = np.zeros(n)
    for _ in range(4):
        f0 = rng.uniform(110.0, 880.0)
        env = 0.5 + 0.5 * np.sin(2.0 * np.pi * rng.uniform(0.5, 3.0) * t + rng.uniform(0, 6.28))
        for h in range(1, 9):
            if f0 * h < 0.45 * fs:
                x += env * np.sin(2.0 * np.pi * f0 * h * t + rng.uniform(0, 6.28)) / h
    x = 0.1 * x / max(np.max(np.abs(x)), 1e-12)
    return x + 0.1 * 10.0 ** (-50.0 / 20.0) * rng.standard_normal(n)


def noisy(x, snr_db, seed):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(len(x))
    e *= math.sqrt(np.mean(np.asarray(x, np.float64) ** 2) / np.mean(e ** 2)) * 10.0 ** (-snr_db / 20.0)
    return np.asarray(x, np.float64) + e


def clipped(x, seed=0):
    x = np.asarray(x, np.float64)
    return np.clip(x, -0.6 * np.max(np.abs(x)), 0.6 * np.max(np.abs(x)))


def band_noise(n, fs, f_lo, f_hi, seed):
    """White noise limited to [f_lo, f_hi] by zeroing the bins of one long transform, unit mean square."""
    rng = np.random.default_rng(seed)
    E = np.fft.rfft(rng.standard_normal(n))
    f = np.arange(len(E)) * fs / n
    E[(f < f_lo) | (f > f_hi)] = 0.0
    e = np.fft.irfft(E, n)
    return e / math.sqrt(np.mean(e ** 2))


def rdf_margin(frame_db):
    """The smallest distance in dB of a frame's peak ratio from the disturbed-frame threshold."""
    f = frame_db[np.isfinite(frame_db)]
    return float(np.min(np.abs(f - RDF_DB))) if len(f) else np.inf


TOL_DB = 1e-6
TOL_REL = 1e-9
