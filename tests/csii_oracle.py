"""NumPy float64 oracle of the coherence speech intelligibility index (Kates & Arehart 2005): section 20's
framing, the level class of every target segment, the spectra of the four segment sets, the critical-band weights and importances
of ANSI S3.5-1997, the per-band signal-to-distortion ratio mapped to [0, 1], CSII per set, I3 and the values above a split - with
explicit loops over the sets and the bands.  Also the seeded inputs the CPU and the GPU tests share.  Test infrastructure; nothing
in ssr_eval_amd imports it."""
import math

import numpy as np

import coherence_oracle as CO

NAMES = ("csii", "csii_low", "csii_mid", "csii_high", "i3", "csii_hf", "csii_low_hf", "csii_mid_hf", "csii_high_hf")
COUNT_NAMES = ("n_all", "n_low", "n_mid", "n_high")
SETS = ("all", "low", "mid", "high")
N_FFTS = (256, 512, 1024, 2048)
FR = CO.FR                                 # segments per chunk
CENTRES = (150., 250., 350., 450., 570., 700., 840., 1000., 1170., 1370., 1600., 1850., 2150., 2500., 2900., 3400., 4000., 4800.,
           5800., 7000., 8500.)
IMPORTANCE = (.0103, .0261, .0419) + (.0577,) * 14 + (.0460, .0343, .0226, .0110)
TOL, TOL_I3 = 1e-7, 3e-7                   # the five CSII values and the _hf values; i3
LEVEL_MARGIN = 1e-6                        # dB: no segment level may lie closer to a class threshold in a compared case
THRESHOLDS = (0.0, -10.0, -30.0)


def default_nfft(fs):
    """The smallest allowed power of two >= 0.016 fs, capped at 2048."""
    for n in N_FFTS:
        if n >= 0.016 * fs:
            return n
    return N_FFTS[-1]


def design(fs, n_fft, band=None):
    """-> (f_c [J], importance [J] renormalised to sum 1, W [J, n_fft / 2 + 1]): the critical bands with f_c <= fs / 2 (inside
    `band` = (lo_hz, hi_hz), if any); W_j[k] = (1 + p g) exp(-p g), g = |k fs / N - f_c| / f_c, p = 4 f_c / ERB(f_c), ERB = 24.7 (4.37
    f_c / 1000 + 1); W_j[0] = 0."""
    keep = [j for j, f in enumerate(CENTRES) if f <= fs / 2.0 and (band is None or band[0] <= f <= band[1])]
    assert keep
    fc = np.array([CENTRES[j] for j in keep])
    imp = np.array([IMPORTANCE[j] for j in keep])
    imp = imp / np.sum(imp)
    W = np.zeros((len(keep), n_fft // 2 + 1))
    for j, f in enumerate(fc):
        p = 4.0 * f / (24.7 * (4.37 * f / 1000.0 + 1.0))
        for k in range(1, n_fft // 2 + 1):
            g = abs(k * fs / n_fft - f) / f
            W[j, k] = (1.0 + p * g) * math.exp(-p * g)
    return fc, imp, W


def levels(x, n_fft, hop):
    """L_t = 10 log10(ms_t / ms_all) of every segment of the target (-inf where ms_t == 0; all NaN where ms_all == 0)."""
    x = np.asarray(x, np.float64)
    K = CO.segments(len(x), n_fft, hop)
    if K == 0:
        return np.zeros(0)
    ms_all = float(np.mean(x * x))
    ms = np.array([np.mean(x[t * hop:t * hop + n_fft] ** 2) for t in range(K)])
    if ms_all == 0.0:
        return np.full(K, np.nan)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(ms / ms_all)


def classes(x, n_fft, hop):
    """int8 [K]: 3 high, 2 mid, 1 low, 0 dropped; -1 everywhere for a digitally silent target."""
    L = levels(x, n_fft, hop)
    c = np.zeros(len(L), np.int8)
    if len(L) and np.isnan(L).all():
        return c - 1
    c[L >= -30.0] = 1
    c[L >= -10.0] = 2
    c[L >= 0.0] = 3
    return c


def level_margin(x, n_fft, hop):
    """The smallest distance in dB of a segment level from a class threshold (inf without a finite level)."""
    L = levels(x, n_fft, hop)
    L = L[np.isfinite(L)]
    return float(min((np.min(np.abs(L - th)) for th in THRESHOLDS), default=np.inf)) if len(L) else float("inf")


def set_spectra(x, y, n_fft, hop):
    """-> (Sxx, Syy, Sxy) [4, n_fft / 2 + 1] of the sets all, low, mid, high, and the four segment counts."""
    X, Y = CO.spectra(x, n_fft, hop), CO.spectra(y, n_fft, hop)
    c = classes(x, n_fft, hop)
    nb = n_fft // 2 + 1
    sxx, syy, sxy, cnt = np.zeros((4, nb)), np.zeros((4, nb)), np.zeros((4, nb), complex), np.zeros(4, int)
    for s in range(4):
        for t in range(len(c)):
            if s == 0 or c[t] == s:
                sxx[s] += np.abs(X[t]) ** 2
                syy[s] += np.abs(Y[t]) ** 2
                sxy[s] += Y[t] * np.conj(X[t])
                cnt[s] += 1
    return sxx, syy, sxy, cnt


def band_values(sxx, syy, sxy, W):
    """T_j [J] of one set from its spectra."""
    den = sxx * syy
    g2 = np.zeros_like(den)
    nz = den != 0.0
    g2[nz] = (sxy.real[nz] ** 2 + sxy.imag[nz] ** 2) / den[nz]
    g2 = np.minimum(g2, 1.0)
    T = np.zeros(W.shape[0])
    for j in range(W.shape[0]):
        num = float(np.sum(W[j] * g2 * syy))
        dis = float(np.sum(W[j] * (1.0 - g2) * syy))
        if num + dis == 0.0 or num == 0.0:
            T[j] = 0.0
        elif dis == 0.0:
            T[j] = 1.0
        else:
            T[j] = (min(max(10.0 * math.log10(num / dis), -15.0), 15.0) + 15.0) / 30.0
    return T


def csii(x, y, fs, n_fft=None, hop=None, band=None, split_hz=None):
    """-> (values [9] in NAMES order, counts [4], T [4, J]) of one pair.  NaN: a set of fewer than 2 segments, a digitally silent
    target, i3 where csii_low or csii_mid is, the _hf values without a split or without a band at or above it."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    assert len(x) == len(y)
    n_fft = default_nfft(fs) if n_fft is None else n_fft
    hop = n_fft // 2 if hop is None else hop
    fc, imp, W = design(fs, n_fft, band)
    sxx, syy, sxy, cnt = set_spectra(x, y, n_fft, hop)
    silent = len(x) > 0 and not np.any(x)
    vals, T = np.full(9, np.nan), np.full((4, len(fc)), np.nan)
    first = None if split_hz is None else int(np.searchsorted(fc, float(split_hz), side="left"))
    for s in range(4):
        if cnt[s] < 2 or silent:
            continue
        T[s] = band_values(sxx[s], syy[s], sxy[s], W)
        vals[s] = float(np.sum(imp * T[s]) / np.sum(imp))          # (over the importance sum: band values of 1 give 1 exactly)
        if first is not None and first < len(fc):
            vals[5 + s] = float(np.sum(imp[first:] * T[s, first:]) / np.sum(imp[first:]))
    vals[4] = 1.0 / (1.0 + math.exp(-(-3.47 + 1.84 * vals[1] + 9.99 * vals[2]))) if not np.isnan(vals[1] + vals[2]) else np.nan
    return vals, cnt, T


# ---- the seeded inputs the CPU and the GPU tests share ---------------------------------------------------------------------------
def speech_like(n, fs, seed=0, f0=140.0):
    """A synthetic voiced signal with pauses: harmonics of a slowly moving f0 under a spectral tilt plus a little noise, in stretches
    of 30 to 90 ms at 0, -4, -9, -16, -24 and -60 dB (the last: a pause), so that segments fall into every class and are dropped."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    f = f0 * (1.0 + 0.1 * np.sin(2 * np.pi * 1.7 * t + rng.uniform(0, 6.28)))
    ph = 2 * np.pi * np.cumsum(f) / fs
    x = np.zeros(n)
    for h in range(1, int(0.45 * fs / (1.1 * f0)) + 1):
        x += np.sin(h * ph + rng.uniform(0, 6.28)) / h ** 0.8
    x = x / (np.std(x) + 1e-30) + 0.05 * rng.standard_normal(n)
    gains = 10.0 ** (np.array([0.0, -4.0, -9.0, -16.0, -24.0, -60.0]) / 20.0)
    env, i = np.zeros(n), 0
    while i < n:
        m = int(rng.uniform(0.03, 0.09) * fs)
        env[i:i + m] = gains[rng.integers(len(gains))]
        i += m
    return 0.3 * x * env


def noisy(x, snr_db, seed=0):
    """x plus white noise at snr_db relative to the whole signal's power."""
    rng = np.random.default_rng(seed)
    p = float(np.mean(np.asarray(x, np.float64) ** 2))
    return x + rng.standard_normal(len(x)) * math.sqrt(p / 10.0 ** (snr_db / 10.0))


def distorted(x, seed=0):
    """A non-linear estimate: a soft clipper at twice the signal's RMS plus noise 25 dB below the signal."""
    r = 2.0 * math.sqrt(float(np.mean(np.asarray(x, np.float64) ** 2))) + 1e-30
    return noisy(r * np.tanh(np.asarray(x, np.float64) / r), 25.0, seed)


def check_rows(out, tgts, ests, idx, fs, n_fft, hop, band=None, splits=None, bands_out=None, what=""):
    """Every row of out [n_est, 13] (and bands_out [n_est, 4, J]) against the oracle: the eight CSII values within TOL, i3 within
    TOL_I3, counts equal, NaN where the oracle has NaN; no segment level of a compared target within LEVEL_MARGIN of a threshold ->
    the worst (CSII, i3, T_j) differences."""
    worst = [0.0, 0.0, 0.0]
    # (a target of exactly one segment's length has its one level at 0 dB by definition, on the threshold between mid and high:
    # every value is NaN there, and the counts must be one segment in all, none low, one in mid or in high)
    for t in set(idx):
        m = level_margin(tgts[t], n_fft, hop)
        assert m >= LEVEL_MARGIN or len(tgts[t]) == n_fft, (what, "target", t, "level margin", m)
    for e, (y, i) in enumerate(zip(ests, idx)):
        want, cnt, T = csii(tgts[i], y, fs, n_fft, hop, band, None if splits is None else splits[e])
        got = out[e]
        print(what, "pair", e, "n", len(y), "got", got[:9], "want", want, "counts", got[9:], cnt)
        if len(y) == n_fft:              # one segment, mid or high
            assert got[9] == cnt[0] == 1 and got[10] == 0.0 and sorted(got[11:].tolist()) == [0.0, 1.0], (what, e, got[9:], cnt)
        else:
            assert got[9:].tolist() == [float(c) for c in cnt], (what, e, got[9:], cnt)
        assert np.array_equal(np.isnan(got[:9]), np.isnan(want)), (what, e, got[:9], want)
        for c in range(9):
            if not np.isnan(want[c]):
                d = abs(got[c] - want[c])
                assert d <= (TOL_I3 if c == 4 else TOL), (what, e, NAMES[c], got[c], want[c])
                worst[1 if c == 4 else 0] = max(worst[1 if c == 4 else 0], d)
        if bands_out is not None:
            assert np.array_equal(np.isnan(bands_out[e]), np.isnan(T)), (what, e)
            if not np.isnan(T).all():
                worst[2] = max(worst[2], float(np.nanmax(np.abs(bands_out[e] - T))))
                assert np.nanmax(np.abs(bands_out[e] - T)) <= TOL, (what, e)
    return worst
