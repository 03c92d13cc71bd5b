"""NumPy float64 oracle of the magnitude-squared coherence family: Welch framing without padding, centring or
detrending, the per-bin spectra Sxx, Syy, Sxy, the coherence g2 with its zero rule and clamp, and per band msc, coh_sdr and coh_bins.
Also the seeded input list the CPU and the GPU tests share.  Test infrastructure; nothing in ssr_eval_amd imports it."""
import numpy as np

NAMES = ("msc", "coh_sdr", "coh_bins")
N_FFTS = (256, 512, 1024, 2048)
EPS = float(np.finfo(np.float64).eps)
FR = 32                                   # segments per chunk (SSR_COH_FR)
TOL, TOL_DB = 1e-9, 1e-6                  # msc and the per-bin coherence; coh_sdr in dB
R_MIN, THR_MARGIN = 1e-4, 1e-6            # what conditioning() must show for a compared pair
CASES = ((4000, 256, 128), (8411, 512, 128), (9001, 1024, 512), (2048, 256, 256))      # (n, N, H) at 16 kHz


def segments(n, n_fft, hop):
    """K = 1 + (n - N) // H segments for n >= N, else 0."""
    return 1 + (n - n_fft) // hop if n >= n_fft else 0


def spectra(x, n_fft, hop):
    """[K, n_fft / 2 + 1] complex128: segment t is samples [t H, t H + N) times the periodic Hann window."""
    x = np.asarray(x, np.float64)
    K = segments(len(x), n_fft, hop)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    idx = hop * np.arange(K)[:, None] + np.arange(n_fft)[None, :]
    return np.fft.rfft(x[idx] * w, axis=-1)


def auto_cross(x, y, n_fft, hop):
    """(Sxx, Syy, Sxy) per bin: sums over the segments, every bin once."""
    assert len(x) == len(y)
    X, Y = spectra(x, n_fft, hop), spectra(y, n_fft, hop)
    return np.sum(np.abs(X) ** 2, axis=0), np.sum(np.abs(Y) ** 2, axis=0), np.sum(Y * np.conj(X), axis=0)


def gamma2(x, y, n_fft, hop):
    """g2[k] = min(1, |Sxy|^2 / (Sxx Syy)), 0 where Sxx Syy == 0 (K = 0: all zero)."""
    sxx, syy, sxy = auto_cross(x, y, n_fft, hop)
    den = sxx * syy
    with np.errstate(divide="ignore", invalid="ignore"):
        g2 = np.where(den == 0.0, 0.0, (sxy.real ** 2 + sxy.imag ** 2) / np.where(den == 0.0, 1.0, den))
    return np.minimum(g2, 1.0), syy


def coherence(x, y, n_fft=1024, hop=None, bands=None, thr=0.5):
    """-> (rows [n_bands, 3] = msc, coh_sdr, coh_bins per inclusive (lo, hi) band, g2 [n_fft / 2 + 1]).  bands None: the full band.
    K < 2 and an empty band (lo > hi): NaN; K < 2: g2 all NaN."""
    hop = n_fft // 2 if hop is None else hop
    bands = [(0, n_fft // 2)] if bands is None else bands
    K = segments(len(x), n_fft, hop)
    rows = np.full((len(bands), 3), np.nan)
    if K < 2:
        return rows, np.full(n_fft // 2 + 1, np.nan)
    g2, syy = gamma2(x, y, n_fft, hop)
    for b, (lo, hi) in enumerate(bands):
        if lo > hi:
            continue
        assert 0 <= lo <= hi <= n_fft // 2
        g, s = g2[lo:hi + 1], syy[lo:hi + 1]
        rows[b] = (np.mean(g), 10.0 * np.log10((np.sum(g * s) + EPS) / (np.sum((1.0 - g) * s) + EPS)), np.sum(g >= thr))
    return rows, g2


def conditioning(x, y, n_fft, hop, thr=0.5):
    """(the smallest |g2 - thr| over the bins, the smallest Sxx / max Sxx, the smallest Syy / max Syy): what the tolerances of the
    kernel comparisons rest on."""
    sxx, syy, _ = auto_cross(x, y, n_fft, hop)
    g2, _ = gamma2(x, y, n_fft, hop)
    return float(np.min(np.abs(g2 - thr))), float(np.min(sxx) / np.max(sxx)), float(np.min(syy) / np.max(syy))


def input_pair(n, seed=0):
    """The seeded test pair: x white noise; y = 0.8 roll(lowpass(x), 3) + 0.05 noise + 0.5 highpass(noise2), the two filters
    order-8 Butterworth at half Nyquist - coherent below, incoherent above."""
    from scipy.signal import butter, sosfilt
    rng = np.random.default_rng(seed)
    x, n1, n2 = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    lp, hp = butter(8, 0.5, "low", output="sos"), butter(8, 0.5, "high", output="sos")
    y = 0.8 * np.roll(sosfilt(lp, x), 3) + 0.05 * n1 + 0.5 * sosfilt(hp, n2)
    return x, y


def input_bands(n_fft):
    """The bands every input case is scored on: full, lower half, upper half, an interior odd-sized one."""
    h = n_fft // 2
    return [(0, h), (0, h // 2), (h // 2 + 1, h), (h // 8 + 1, h // 4 + 2)]


# ---- what the CPU and the GPU tests share: band tables, the comparison, shapes ---------------------------------------------------
def band_table(bands, n_est):
    """One list of (lo, hi) for every estimate, or one list per estimate -> int32 [n_est][n_bands][2]."""
    b = np.asarray(bands, np.int32)
    if b.ndim == 2:
        b = np.broadcast_to(b, (n_est,) + b.shape)
    assert b.shape[0] == n_est and b.shape[2] == 2
    return np.ascontiguousarray(b)


def check_rows(out, g2, tgts, ests, idx, n_fft, hop, bands, thr=0.5, what=""):
    """Every row against the oracle: msc and the per-bin coherence within TOL, coh_sdr within TOL_DB, coh_bins equal, NaN where the
    oracle has NaN; every compared pair well conditioned -> the worst (msc, per-bin, coh_sdr) differences."""
    worst = [0.0, 0.0, 0.0]
    tab = band_table(bands, len(ests))
    for e, (y, i) in enumerate(zip(ests, idx)):
        want, wg = coherence(tgts[i], y, n_fft, hop, [tuple(b) for b in tab[e]], thr)
        if segments(len(y), n_fft, hop) >= 2:
            margin, rx, ry = conditioning(tgts[i], y, n_fft, hop, thr)
            assert margin >= THR_MARGIN and rx >= R_MIN and ry >= R_MIN, (what, e, margin, rx, ry)
        if g2 is not None:
            assert np.array_equal(np.isnan(g2[e]), np.isnan(wg)), (what, e)
            if not np.isnan(wg).any():
                worst[1] = max(worst[1], float(np.max(np.abs(g2[e] - wg))))
                assert np.max(np.abs(g2[e] - wg)) <= TOL, (what, e, np.max(np.abs(g2[e] - wg)))
        for b in range(tab.shape[1]):
            print(what, "pair", e, "n", len(y), "band", tuple(tab[e, b]), "got", out[e, b], "want", want[b])
            if np.isnan(want[b]).any():
                assert np.isnan(out[e, b]).all() and np.isnan(want[b]).all(), (what, e, b, out[e, b])
                continue
            assert abs(out[e, b, 0] - want[b, 0]) <= TOL, (what, e, b, out[e, b, 0], want[b, 0])
            assert abs(out[e, b, 1] - want[b, 1]) <= TOL_DB, (what, e, b, out[e, b, 1], want[b, 1])
            assert out[e, b, 2] == want[b, 2], (what, e, b, out[e, b, 2], want[b, 2])
            worst[0] = max(worst[0], abs(out[e, b, 0] - want[b, 0]))
            worst[2] = max(worst[2], abs(out[e, b, 1] - want[b, 1]))
    return worst


def len_for_segments(K, n_fft, hop, extra=0):
    n = n_fft + (K - 1) * hop + extra
    assert segments(n, n_fft, hop) == K and 0 <= extra < hop
    return n
