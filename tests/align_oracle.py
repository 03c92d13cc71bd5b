"""NumPy float64 oracle of the delay stage: the bounded two-sided cross-correlation by explicit sums, the
tie-ruled peak, the parabola, the 33 windowed-sinc taps and the shift.  Test infrastructure; nothing in the package imports it."""
import numpy as np

HALF, TAPS, MAX_LAG = 16, 33, 4096


def xcorr(x, y, L):
    """c[d + L] = sum_t x[t] y[t + d] over the t with 0 <= t < n_x and 0 <= t + d < n_y, d = -L .. L (no such t: 0)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    nx, ny = len(x), len(y)
    c = np.zeros(2 * L + 1)
    for d in range(-L, L + 1):
        t0, t1 = max(0, -d), min(nx, ny - d)
        if t1 > t0:
            c[d + L] = np.dot(x[t0:t1], y[t0 + d:t1 + d])
    return c


def scan_order(L):
    """The lags in the order 0, +1, -1, +2, -2, ..."""
    return [0] + [s * k for k in range(1, L + 1) for s in (1, -1)]


def peak(c, L):
    """-> (d*, the margin of c[d*] over the largest value at any other lag): strict > in scan order."""
    best, d_star = c[L], 0
    for d in scan_order(L)[1:]:
        if c[d + L] > best:
            best, d_star = c[d + L], d
    others = np.delete(c, d_star + L)
    return d_star, float(best - others.max()) if len(others) else np.inf


def parabola(c, d, L):
    """-> (delta, denominator) at a peak that is not on the edge."""
    cm, c0, cp = c[d - 1 + L], c[d + L], c[d + 1 + L]
    den = (cm - 2.0 * c0) + cp
    if den == 0.0 or not np.isfinite(den):
        return 0.0, den
    v = 0.5 * (cm - cp) / den
    return (float(min(0.5, max(-0.5, v))) if v == v else 0.0), den


def estimate(x, y, L):
    """-> dict: delay, frac, corr, edge, c, margin (of the peak over its runner-up), den (the parabola's denominator, NaN on an edge
    or a degenerate pair), scale = sqrt(Ex Ey)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    c = xcorr(x, y, L)
    ex, ey = float(np.dot(x, x)), float(np.dot(y, y))
    d, margin = peak(c, L)
    out = {"c": c, "margin": margin, "scale": float(np.sqrt(ex * ey)), "den": np.nan}
    if len(x) == 0 or len(y) == 0 or ex == 0.0 or ey == 0.0 or not c[d + L] > 0.0:
        out.update(delay=0, frac=0.0, corr=np.nan, edge=0, degenerate=True)
        return out
    edge = int(abs(d) == L)
    frac = 0.0
    if not edge:
        frac, out["den"] = parabola(c, d, L)
    out.update(delay=d, frac=frac, corr=c[d + L] / np.sqrt(ex * ey), edge=edge, degenerate=False)
    return out


def taps(delta):
    """h[m + 16], m = -16 .. 16, of the fractional shift by delta != 0."""
    m = np.arange(-HALF, HALF + 1)
    u = m - delta
    s = np.where(m % 2 != 0, 1.0, -1.0) * np.sin(np.pi * delta) / (np.pi * u)
    w = 0.5 * (1.0 + np.cos(np.pi * u / (HALF + 1)))
    h = s * w
    total = 0.0
    for v in h:
        total += v
    return h / total


def shift(y, d, delta=0.0):
    """z[t] = y[t + d] with zero fill (delta = 0: a copy in y's dtype), else the 33-tap filter in float64 rounded once to y's dtype."""
    y = np.asarray(y)
    n = len(y)
    if delta == 0.0:
        z = np.zeros_like(y)
        lo, hi = max(0, -d), min(n, n - d)
        if hi > lo:
            z[lo:hi] = y[lo + d:hi + d]
        return z
    h = taps(delta)
    pad = abs(d) + HALF + 1
    yp = np.concatenate((np.zeros(pad), y.astype(np.float64), np.zeros(pad)))
    z = np.zeros(n)
    for mm in range(TAPS):                       # ascending m, as the kernel adds them
        start = pad + d + mm - HALF
        z += h[mm] * yp[start:start + n]
    return z.astype(y.dtype)


def align(x, y, L, subsample=False):
    """-> (z, the estimate() dict)."""
    r = estimate(x, y, L)
    return shift(y, r["delay"], r["frac"] if subsample else 0.0), r


# ---- seeded signals ----------------------------------------------------------------------------------------------------------------
def noise(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


def lowpassed(n, seed, width=9):
    """Seeded noise through a short raised-cosine FIR: a smooth correlation peak (a parabola that is well conditioned)."""
    v = np.random.default_rng(seed).standard_normal(n + width - 1)
    k = 0.5 * (1.0 - np.cos(2.0 * np.pi * (np.arange(width) + 1) / (width + 1)))
    return np.convolve(v, k / k.sum(), mode="valid") if n else np.zeros(0)


def delayed(x, d, n=None):
    """y[t] = x[t - d] (zero where x has no sample), n samples (None: len(x)): an estimate that is d samples late."""
    n = len(x) if n is None else n
    y = np.zeros(n, dtype=np.asarray(x).dtype)
    lo, hi = max(0, d), min(n, len(x) + d)
    if hi > lo:
        y[lo:hi] = x[lo - d:hi - d]
    return y


# ---- the shapes at which the geometry can go wrong (tests/test_align_host.py on the emulated kernels, tests/test_gpu_align.py) ------
TILE = 16384                                     # SSR_ALIGN_TILE
LAGS = (1, 8, 9, 64, 1024, 2047, 2049, 4096)     # around a lane's 8 lags and a block's 2048


def geometry_lengths(L):
    """Target lengths: one sample, a few, around L, one below / at / one above a tile, several tiles."""
    return sorted({n for n in (1, 7, L - 1, L + 1, TILE - 1, TILE, TILE + 1, 40000) if n > 0})


def geometry_delays(L):
    """True delays: none, one sample, a few, the last lag inside the search, the edge, beyond the search."""
    return [0, 1, -1, 37, -37, L - 1, -(L - 1), L, -L, L + 5]


def geometry_batch(L, tgt_dtype, est_dtype):
    """-> (targets, estimates, tgt_index): every length of geometry_lengths(L) as a target (seeded noise and low-passed noise in
    turn), two estimates per target with delays taken in turn from geometry_delays(L) - so every delay occurs and every target is
    named twice -, the second estimate of a target longer or shorter than it in turn, and a faint independent noise on every
    estimate (no two lags tie)."""
    delays = geometry_delays(L)
    tgts, ests, idx = [], [], []
    for i, n in enumerate(geometry_lengths(L)):
        x = (noise(n, 100 * L + i) if i % 2 else lowpassed(n, 100 * L + i)).astype(tgt_dtype)
        tgts.append(x)
        for j in range(2):
            d = delays[(2 * i + j) % len(delays)]
            m = n if j == 0 else max(1, n + (13 if i % 2 else -5))
            y = delayed(x.astype(np.float64), d, m) + 1e-3 * noise(m, 100 * L + 50 + 2 * i + j)
            ests.append(y.astype(est_dtype)); idx.append(i)
    return tgts, ests, idx
