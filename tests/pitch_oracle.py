"""Float64 NumPy oracle of the pitch metrics: YIN F0 tracking (de Cheveigné & Kawahara, JASA 2002) and the pair
statistics F0 RMSE, F0 correlation, GPE, VDE (Nakatani et al. 2008) and FFE (Chu & Alwan 2009), written from the definition in the
direct form.  SciPy does the resampling to 16 kHz.  Test infrastructure: it restates the definition, it is not pinned against
any pitch tracker package.

Besides the values, every track carries a per-frame `stable` mask: the frame's tau*, and its voicing, stay the same when every d'
and every E is multiplied by 1 + 1e-9 u (u uniform in [-1, 1], 8 seeds).  The d' = 1 of an all-zero prefix is exact and is not
perturbed (a digitally silent frame ties every lag exactly, and its tau* is tau_lo everywhere).  The pair statistics add the gross-error test, with each
ratio perturbed the same way.  GPU and oracle are compared on stable frames only: elsewhere a last-bit difference in a sum may
legitimately flip a discrete decision."""
import math

import numpy as np
from scipy.signal import resample_poly

FS, H, W = 16000, 160, 400
TROUGH, VOICED, SILENCE, GROSS = 0.1, 0.2, 1e-4, 0.2
NAMES = ("f0_rmse", "f0_corr", "gpe", "vde", "ffe")
SEEDS, REL = 8, 1e-9


def lag_range(fmin=50.0, fmax=500.0):
    return int(math.floor(FS / fmax)), int(math.ceil(FS / fmin))


def valid_range(fmin, fmax):
    if not (40.0 <= fmin < fmax <= 1000.0):
        return False
    lo, hi = lag_range(fmin, fmax)
    return hi - lo >= 2


def to_16k(x, fs):
    """scipy.signal.resample_poly(x64, 16000 // g, fs // g), g = gcd(16000, fs) (the identity at 16 kHz)."""
    x64 = np.asarray(x, np.float64)
    g = math.gcd(FS, int(fs))
    up, down = FS // g, int(fs) // g
    return resample_poly(x64, up, down)


def n_frames(n16):
    return n16 // H + 1 if n16 > 0 else 0


def _diff(x16, tau_hi):
    """d [T, tau_hi] (column tau - 1) and E [T], direct form."""
    n = len(x16)
    T = n_frames(n)
    xp = np.concatenate((np.zeros(W // 2), x16, np.zeros(W + tau_hi)))
    d = np.zeros((T, tau_hi))
    E = np.zeros(T)
    lag = np.arange(W)[None, :] + np.arange(1, tau_hi + 1)[:, None]
    for t in range(T):
        seg = xp[t * H:t * H + W + tau_hi]
        base = seg[:W]
        d[t] = np.sum((base[None, :] - seg[lag]) ** 2, axis=1)
        E[t] = np.sum(base * base)
    return d, E


def _cmnd(d):
    """(d', exact): d' [T, tau_hi], and where it is the exact 1 of an all-zero prefix (no rounding there to perturb)."""
    tau = np.arange(1, d.shape[1] + 1, dtype=np.float64)
    cum = np.cumsum(d, axis=1)
    out = np.ones_like(d)
    np.divide(tau * d, cum, out=out, where=cum > 0)
    return out, cum == 0


def _pick(v):
    """v = d'(tau_lo .. tau_hi) of one frame -> index of tau* in v."""
    trough = np.zeros(len(v), bool)
    trough[1:-1] = (v[1:-1] < v[:-2]) & (v[1:-1] <= v[2:])
    trough[0] = v[0] < v[1]
    trough[-1] = v[-1] < v[-2]
    c = np.nonzero(trough & (v < TROUGH))[0]
    return int(c[0]) if len(c) else int(np.argmin(v))


def _voicing(E, a):
    return (E > 0) & (E >= SILENCE * (E.max() if len(E) else 0.0)) & (a < VOICED)


def track16(x16, fmin=50.0, fmax=500.0):
    """YIN on a 16 kHz float64 signal -> dict f0, aperiodicity, energy, voiced, tau (tau*), stable (per frame)."""
    tau_lo, tau_hi = lag_range(fmin, fmax)
    d, E = _diff(np.asarray(x16, np.float64), tau_hi)
    dp, exact = _cmnd(d)
    T = len(E)
    f0, ap, tau = np.full(T, np.nan), np.zeros(T), np.zeros(T, np.int64)
    for t in range(T):
        v = dp[t, tau_lo - 1:tau_hi]
        k = _pick(v)
        ts = tau_lo + k
        delta = 0.0
        if tau_lo < ts < tau_hi:
            den = 2.0 * (v[k - 1] - 2.0 * v[k] + v[k + 1])
            if den > 0:
                dl = (v[k - 1] - v[k + 1]) / den
                if abs(dl) <= 1.0:
                    delta = dl
        ap[t], tau[t] = v[k], ts
        if E[t] > 0:
            f0[t] = FS / (ts + delta)
    voiced = _voicing(E, ap)
    stable = np.ones(T, bool)
    for s in range(SEEDS):
        rng = np.random.default_rng(1000 + s)
        u = np.where(exact[:, tau_lo - 1:tau_hi], 0.0, rng.uniform(-1, 1, (T, tau_hi - tau_lo + 1)))
        dq = dp[:, tau_lo - 1:tau_hi] * (1 + REL * u)
        Eq = E * (1 + REL * rng.uniform(-1, 1, T))
        kq = np.array([_pick(dq[t]) for t in range(T)], np.int64)
        aq = dq[np.arange(T), kq]
        stable &= (tau_lo + kq == tau) & (_voicing(Eq, aq) == voiced)
    return {"f0": f0, "aperiodicity": ap, "energy": E, "voiced": voiced, "tau": tau, "stable": stable}


def track(x, fs, fmin=50.0, fmax=500.0):
    return track16(to_16k(x, fs), fmin, fmax)


def pair_stats(tx, ty):
    """The five metrics of the estimate's track ty against the target's tx, and whether every frame is stable."""
    fx, fy, vx, vy = tx["f0"], ty["f0"], tx["voiced"], ty["voiced"]
    T = len(fx)
    both = vx & vy
    nv = int(np.sum(vx != vy))
    nb = int(both.sum())
    r = fy[both] / fx[both]
    gross = np.abs(r - 1.0) > GROSS
    ng = int(gross.sum())
    stable = bool(tx["stable"].all() and ty["stable"].all())
    for s in range(SEEDS):
        rq = r * (1 + REL * np.random.default_rng(2000 + s).uniform(-1, 1, len(r)))
        stable &= bool(np.array_equal(np.abs(rq - 1.0) > GROSS, gross))
    nan = float("nan")
    out = {"f0_rmse": math.sqrt(np.mean((1200.0 * np.log2(r)) ** 2)) if nb else nan,
           "gpe": ng / nb if nb else nan, "vde": nv / T if T else nan, "ffe": (nv + ng) / T if T else nan}
    a, b = fx[both], fy[both]
    if nb >= 2 and a.min() < a.max() and b.min() < b.max():
        a, b = a - a.mean(), b - b.mean()
        out["f0_corr"] = float(np.sum(a * b) / math.sqrt(np.sum(a * a) * np.sum(b * b)))
    else:
        out["f0_corr"] = nan
    return {k: out[k] for k in NAMES}, stable


def pitch(x, y, fs, fmin=50.0, fmax=500.0):
    """(metrics dict, all frames stable) of estimate y against target x, both at fs (truncated to their common length)."""
    n = min(len(x), len(y))
    return pair_stats(track(x[:n], fs, fmin, fmax), track(y[:n], fs, fmin, fmax))
