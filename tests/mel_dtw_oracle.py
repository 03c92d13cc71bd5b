"""Float64 oracle of the DTW-aligned mel-cepstral distortion, written from the definition (test infrastructure).

  c[t, d]  = orthonormal DCT-II over m of ln+((S W)[t, m]),  d = 1 .. n_cep           (every image on its own)
  delta(i, j) = (10 / ln 10) sqrt(2 sum_d (c_E[i, d] - c_G[j, d])^2)   for |i - j| <= R, +inf outside
  D[0][0]  = 2 delta(0, 0);  D[i][j] = min(D[i-1][j-1] + 2 delta, D[i-1][j] + delta, D[i][j-1] + delta), formed in that order, a later
  candidate replacing an earlier one only when strictly smaller;  mcd_dtw = D[T-1][T-1] / (2 T);  len / dev_sum: the cells of the
  chosen path and the sum of |i - j| over them;  dtw_len = len, dtw_dev = dev_sum / len.

The recurrence is the plain double loop.  The local costs are summed over d in ascending order, one term after another, so that on
inputs whose arithmetic is exact - and on any input whose costs are formed by the same IEEE operations - ties fall as in the kernel.
"""
import math

import numpy as np

import mel_oracle as MO

NAMES = ("mcd_dtw", "dtw_dev", "dtw_len")
SCALE = 10.0 / math.log(10.0)


def cepstra(S, W, n_cep=13):
    """[T, n_cep] float64 cepstra of a [T, F] magnitude image."""
    return MO.ln_plus(MO.mel(S, W)) @ MO.dct_matrix(np.asarray(W).shape[1], n_cep).T


def band_costs(cE, cG, R):
    """{o: delta(i, i - o) for every i with both indices inside the matrix}, o = -R .. R: array o holds i = max(o, 0) .. T - 1 + min(o, 0)."""
    cE, cG = np.asarray(cE, np.float64), np.asarray(cG, np.float64)
    T = cE.shape[0]
    out = {}
    for o in range(-min(R, T - 1), min(R, T - 1) + 1):
        i0, i1 = max(o, 0), T + min(o, 0)
        diff = cE[i0:i1] - cG[i0 - o:i1 - o]
        acc = np.zeros(i1 - i0)
        for d in range(cE.shape[1]):
            acc = acc + diff[:, d] * diff[:, d]
        out[o] = SCALE * np.sqrt(2.0 * acc)
    return out


def warp(costs, T, R):
    """The recurrence on band_costs' table -> (D[T-1][T-1], len, dev_sum)."""
    INF = math.inf
    R = min(R, T - 1)
    W = 2 * R + 1
    # rows of the band: prev[o + R] = (D, len, dev) of cell (i - 1, i - 1 - o), cur the same for row i
    prev = None
    for i in range(T):
        cur = [(INF, 0, 0)] * W
        for o in range(R, -R - 1, -1):                     # j = i - o ascending
            j = i - o
            if j < 0 or j >= T:
                continue
            dl = float(costs[o][i - max(o, 0)])
            if i == 0 and j == 0:
                cur[o + R] = (2.0 * dl, 1, 0)
                continue
            best = (INF, 0, 0)
            if prev is not None:                           # (i - 1, j - 1): offset o
                p = prev[o + R]
                best = (p[0] + 2.0 * dl, p[1], p[2])
                if o - 1 >= -R:                            # (i - 1, j): offset o - 1
                    p = prev[o - 1 + R]
                    c = p[0] + dl
                    if c < best[0]:
                        best = (c, p[1], p[2])
            if o + 1 <= R:                                 # (i, j - 1): offset o + 1
                p = cur[o + 1 + R]
                c = p[0] + dl
                if c < best[0]:
                    best = (c, p[1], p[2])
            cur[o + R] = (best[0], best[1] + 1, best[2] + abs(o))
        prev = cur
    return prev[R]


def result(D, ln, dev, T):
    return {"D": D, "len": ln, "dev_sum": dev, "mcd_dtw": D / (2.0 * T), "dtw_dev": dev / ln, "dtw_len": float(ln)}


def dtw(cE, cG, R):
    """The measure of two [T, n_cep] cepstrum sequences at radius R: {D, len, dev_sum, mcd_dtw, dtw_dev, dtw_len}."""
    T = np.asarray(cE).shape[0]
    assert np.asarray(cG).shape[0] == T and T >= 1 and R >= 0
    return result(*warp(band_costs(cE, cG, R), T, R), T)


def perturbed(cE, cG, R, rel=1e-4, trials=6, seed=0):
    """[(D, len, dev_sum)]: the unperturbed warp, then `trials` warps with every local cost scaled by a random 1 +- rel."""
    T = np.asarray(cE).shape[0]
    costs = band_costs(cE, cG, R)
    rng = np.random.default_rng(seed)
    out = [warp(costs, T, R)]
    for _ in range(trials):
        out.append(warp({o: c * (1.0 + rel * rng.uniform(-1.0, 1.0, c.shape)) for o, c in costs.items()}, T, R))
    return out


def path_is_stable(cE, cG, R, rel=1e-4, trials=6, seed=0):
    """True where the chosen path's integers do not depend on the last digits of the local costs: len and dev_sum stay what they are
    under `trials` random relative perturbations of every local cost within +-rel (and the value moves by no more than rel, as it
    must: D is a minimum of sums of costs with positive weights).  Tests compare path integers with a kernel only for inputs this
    accepts."""
    (D, ln, dev), *rest = perturbed(cE, cG, R, rel, trials, seed)
    return all((l2, d2) == (ln, dev) and abs(D2 - D) <= rel * abs(D) * (1 + 1e-9) for D2, l2, d2 in rest)


def from_images(Se, St, W, R, n_cep=13):
    return dtw(cepstra(Se, W, n_cep), cepstra(St, W, n_cep), R)


def from_waves(est, tgt, rate, W, R, n_cep=13, n_fft=None, hop=None):
    """The measure of two waveforms (truncated to the common length, as AudioMetrics does)."""
    m = min(len(est), len(tgt))
    return from_images(MO.magnitudes(est[:m], rate, n_fft, hop), MO.magnitudes(tgt[:m], rate, n_fft, hop), W, R, n_cep)


def harmonic(n, rate=16000, seed=0):
    """The test signal: a harmonic carrier (every harmonic below 7.8 kHz, amplitudes 1 / sqrt(h): no mel band is left to the noise
    floor) with a slow F0 wobble and an amplitude envelope, with a 1500-sample stretch of digital silence (float64; callers cast)."""
    t = np.arange(n) / rate
    f0 = 140.0 + 25.0 * np.sin(2 * np.pi * 1.3 * t) + 10.0 * np.sin(2 * np.pi * 0.37 * t + seed)
    ph = 2 * np.pi * np.cumsum(f0) / rate
    x = sum(np.where(h * f0 < 7800.0, np.sin(h * ph + 0.3 * h), 0.0) / np.sqrt(h) for h in range(1, 76))
    x = x * (0.4 + 0.3 * (1.0 + np.sin(2 * np.pi * 2.1 * t + 0.5 * seed))) * 0.12
    a = min(n // 2, 6000)
    x[a:a + 1500] = 0.0
    return x


def shifted(x, shift, noise=0.0, seed=1):
    """x delayed by `shift` samples (zeros in front, the same length), plus white noise of that standard deviation."""
    y = np.concatenate((np.zeros(shift), x[:len(x) - shift])) if shift else x.copy()
    if noise:
        y = y + noise * np.random.default_rng(seed).standard_normal(len(x))
    return y
