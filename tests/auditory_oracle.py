"""NumPy / SciPy float64 oracle of the auditory family: Hohmann's complex all-pole gammatone filterbank of order
4, the 10 ms / 20 ms power image, level matching, the dB image on the target's floor and the neurogram similarity index (NSIM, Hines &
Harte 2012) in its centred form.  The definition restated, line by line; nothing here knows how the kernels cut a signal.

The cascade is the recursion itself, sample by sample, vectorised over the bands; tests/test_auditory_host.py pins it to four
scipy.signal.lfilter passes and to the |H(f_c)| = 2 anchor."""
import math

import numpy as np

A_GAMMA = math.pi * 720.0 * 2.0 ** -6 / 36.0        # pi 6! 2^-6 / (3!)^2 = 0.98174770...
MIN_BANDS, MAX_BANDS = 3, 64
TOL_P = 1e-9            # P re the target's largest cell
TOL_NSIM = 1e-9         # worst emulated difference 1.1e-14 <= 1e-11: the project's customary bar (see test_auditory_host's docstring)
LEVEL_MARGIN = 1e-12    # match_level: sum P_estimate at least this share of sum P_target, or exactly 0


# ---- design ----------------------------------------------------------------------------------------------------------------------
def erbn(f):
    return 24.7 * (1.0 + 0.00437 * f)


def erb_scale(f):
    return 21.4 * np.log10(1.0 + 0.00437 * np.asarray(f, np.float64))


def centres(fs, n_bands=32, band=None):
    lo, hi = (50.0, 0.45 * fs) if band is None else (float(band[0]), float(band[1]))
    e = np.linspace(erb_scale(lo), erb_scale(hi), n_bands)
    return (10.0 ** (e / 21.4) - 1.0) / 0.00437


def design(fs, n_bands=32, band=None):
    """-> (f_c [C], coef [C, 3] = Re a, Im a, g)"""
    fc = centres(fs, n_bands, band)
    lam = np.exp(-2.0 * np.pi * (erbn(fc) / A_GAMMA) / fs)
    a = lam * np.exp(2j * np.pi * fc / fs)
    return fc, np.ascontiguousarray(np.stack([a.real, a.imag, 2.0 * (1.0 - lam) ** 4], axis=1))


def split_band(fc, split_hz):
    """The first interior band at or above split_hz (C - 1: none), or -1 for no split."""
    if split_hz is None:
        return -1
    inner = np.asarray(fc)[1:-1]
    return 1 + int(np.searchsorted(inner, float(split_hz), side="left"))


# ---- filterbank and images ---------------------------------------------------------------------------------------------------------
def filterbank(x, coef):
    """z [C, n] complex: y_0 = g x, y_s[n] = y_{s-1}[n] + a y_s[n - 1], s = 1 .. 4, from the zero state."""
    x = np.asarray(x, np.float64)
    coef = np.asarray(coef, np.float64)
    a, g = coef[:, 0] + 1j * coef[:, 1], coef[:, 2]
    z = np.empty((len(a), len(x)), np.complex128)
    y = np.zeros((4, len(a)), np.complex128)
    for n in range(len(x)):
        u = g * x[n]
        for s in range(4):
            u = u + a * y[s]
            y[s] = u
        z[:, n] = u
    return z


def rows(n, hop):
    return 1 + (n - 2 * hop) // hop if n >= 2 * hop else 0


def power_image(x, coef, hop):
    """P [T, C]"""
    C, T = len(coef), rows(len(x), hop)
    if T == 0:
        return np.zeros((0, C))
    e = np.abs(filterbank(np.asarray(x, np.float64)[:(T + 1) * hop], coef)) ** 2
    B = np.array([[math.fsum(e[c, j * hop:(j + 1) * hop]) for c in range(C)] for j in range(T + 1)])
    return (B[:-1] + B[1:]) / (2.0 * (2 * hop))


def db_images(Pr, Pd, range_db=60.0, match_level=True):
    """-> (D_r, D_d, floor_db, f): the clamped dB images of target and estimate on the target's floor and the level factor (None,
    None, nan, nan where the target is silent or has no row; D_d all NaN where the factor is not finite - sum P_estimate denormal).
    G = D - floor_db."""
    if Pr.size == 0 or not np.max(Pr) > 0.0:
        return None, None, math.nan, math.nan
    f = 1.0
    if match_level and Pd is not None:
        sd = math.fsum(Pd.ravel())
        with np.errstate(over="ignore"):
            f = float(np.float64(math.fsum(Pr.ravel())) / np.float64(sd)) if sd != 0.0 else 1.0
    floor_db = 10.0 * math.log10(float(np.max(Pr))) - range_db
    with np.errstate(divide="ignore"):
        Dr = np.maximum(10.0 * np.log10(Pr), floor_db)
        if Pd is None:
            Dd = None
        elif not math.isfinite(f):
            Dd = np.full(Pd.shape, np.nan)
        else:
            Dd = np.maximum(10.0 * np.log10(Pd * f), floor_db)
    return Dr, Dd, floor_db, f


def nsim_map(Gr, Gd, range_db=60.0):
    """[T - 2, C - 2]: the valid 3 x 3 neighbourhoods, centred form"""
    g3 = np.array([math.exp(-2.0), 1.0, math.exp(-2.0)]) / (1.0 + 2.0 * math.exp(-2.0))
    w = np.outer(g3, g3)
    c1, c3 = (0.01 * range_db) ** 2, (0.03 * range_db) ** 2 / 2.0
    T, C = Gr.shape
    out = np.empty((T - 2, C - 2))
    for t in range(T - 2):
        for c in range(C - 2):
            r, d = Gr[t:t + 3, c:c + 3], Gd[t:t + 3, c:c + 3]
            mr, md = float(np.sum(w * r)), float(np.sum(w * d))
            vr, vd = float(np.sum(w * (r - mr) ** 2)), float(np.sum(w * (d - md) ** 2))
            cov = float(np.sum(w * (r - mr) * (d - md)))
            out[t, c] = (2.0 * mr * md + c1) / (mr * mr + md * md + c1) * (cov + c3) / (math.sqrt(vr * vd) + c3)
    return out


def analyse(target, est, coef, hop, range_db=60.0, match_level=True, split=-1, Pr=None, Pd=None):
    """-> {"pair": [nsim, nsim_hf, nsim_lf], "bands": fvnsim [C] (NaN in the edge bands), "Pr", "Pd", "Dr", "Dd", "f" (the level
    factor), "floor_db"}; Pr / Pd: the power images where the caller has them already"""
    C = len(coef)
    Pr = power_image(target, coef, hop) if Pr is None else Pr
    Pd = power_image(est, coef, hop) if Pd is None else Pd
    Dr, Dd, floor_db, f = db_images(Pr, Pd, range_db, match_level)
    out = {"Pr": Pr, "Pd": Pd, "Dr": Dr, "Dd": Dd, "f": f, "floor_db": floor_db, "pair": np.full(3, np.nan), "bands": np.full(C, np.nan)}
    if Dr is None or Pr.shape[0] < 3 or not math.isfinite(f):
        return out
    m = nsim_map(Dr - floor_db, Dd - floor_db, range_db)
    out["map"] = m
    out["bands"][1:-1] = np.mean(m, axis=0)
    out["pair"][0] = float(np.mean(m))
    if split >= 1:
        if split <= C - 2:
            out["pair"][1] = float(np.mean(m[:, split - 1:]))
        if split >= 2:
            out["pair"][2] = float(np.mean(m[:, :split - 1]))
    return out


def assert_conditioned(target, est, coef, hop, range_db=60.0, match_level=True, name="", d=None):
    """An input of the comparison keeps every scored value finite and its level factor away from rounding: at least 3 rows, a target
    with energy, and - with level matching - an estimate whose image holds LEVEL_MARGIN of the target's power or none at all.
    d: analyse()'s result where the caller has it already."""
    d = analyse(target, est, coef, hop, range_db, match_level, 1) if d is None else d
    assert d["Pr"].shape[0] >= 3 and np.max(d["Pr"]) > 0.0, name
    sr, sd = float(np.sum(d["Pr"])), float(np.sum(d["Pd"]))
    assert not match_level or sd == 0.0 or sd >= LEVEL_MARGIN * sr, (name, sr, sd)
    assert np.isfinite(d["map"]).all() and np.isfinite(d["pair"][0]), name
    return float(np.min(d["map"])), sd / sr


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def harmonic(n, fs, seed=0, f0=150.0, amp=0.2):
    """a harmonic f0 tone with a 3 Hz envelope over a faint noise floor"""
    t = np.arange(n) / fs
    k = np.arange(1, int(0.45 * fs / f0))
    x = np.sum(np.sin(2.0 * np.pi * f0 * k[:, None] * t[None, :]) / k[:, None], axis=0)
    return amp * (0.55 + 0.45 * np.sin(2.0 * np.pi * 3.0 * t)) * x + 1e-4 * np.random.default_rng(seed).standard_normal(n)


def noise(n, seed, amp=0.1):
    return amp * np.random.default_rng(seed).standard_normal(n)


def lowpassed(x, cutoff):
    """8th-order zero-phase Butterworth low-pass, cutoff as a fraction of Nyquist"""
    from scipy.signal import butter, sosfiltfilt
    return sosfiltfilt(butter(4, cutoff, output="sos"), x)


def geometry_case(fs, hop, n_bands, ks, tdt=np.float64, edt=np.float32, **kw):
    """The lengths where the geometry can go wrong in ONE batch: win - 1 (no row), win, win + hop (T = 2: NaN), win + 2 hop (T = 3: one
    valid column), then one sample short of and one past k hop-blocks for every k of ks (segment and workgroup boundaries).  Every
    target has one estimate (itself plus noise), the last one two more (low-passed; unrelated noise); the splits run through -1, 1,
    n_bands - 1 (above every interior band) and the middle band."""
    fc, coef = design(fs, n_bands)
    win = 2 * hop
    lens = [win - 1, win, win + hop, win + 2 * hop] + [k * hop + d for k in ks for d in (-1, 1)]
    tgts = [harmonic(n, fs, 100 + i) for i, n in enumerate(lens)]
    ests = [t + noise(len(t), 200 + i, 0.02) for i, t in enumerate(tgts)] + [lowpassed(tgts[-1], 0.25), noise(lens[-1], 300)]
    index = list(range(len(lens))) + [len(lens) - 1] * 2
    cycle = [-1, 1, n_bands - 1, max(1, n_bands // 2)]
    return Case(tgts, ests, index, coef, hop, splits=[cycle[e % 4] for e in range(len(ests))], tdt=tdt, edt=edt, fs=fs, **kw)


def pack(sigs, gap, dt):
    """-> (buffer with NaN in the unused samples, offsets, lengths)"""
    ln = np.array([len(s) for s in sigs], np.int64)
    off = (np.cumsum(ln + gap) - ln).astype(np.int64)
    data = np.full(int((ln + gap).sum()) + 1, np.nan, dt)
    for o, s in zip(off, sigs):
        data[o:o + len(s)] = s
    return data, off, ln.astype(np.int32)


class Case:
    """One call of ssr_auditory: targets, estimates, the pair -> target map and the options; check() compares (pair_out, band_out,
    image_out rows per signal, power rows per signal or None) with the oracle."""

    def __init__(self, tgts, ests, index, coef, hop, range_db=60.0, match=True, splits=None, tdt=np.float64, edt=np.float64, power=None, fs=16000):
        self.fs = fs                # the rate the coefficients were designed for (a device call designs them again)
        self.power = power          # the oracle's power images of tgts + ests where a caller has them (check() fills it)
        self.tgts, self.ests = [np.asarray(t, tdt) for t in tgts], [np.asarray(e, edt) for e in ests]
        self.index, self.coef, self.hop, self.range_db, self.match = list(index), np.ascontiguousarray(coef, np.float64), hop, range_db, match
        self.splits = [-1] * len(ests) if splits is None else list(splits)
        self.tdt, self.edt = tdt, edt

    def rows(self):
        return [rows(len(s), self.hop) for s in self.tgts] + [rows(len(self.tgts[i]), self.hop) for i in self.index]

    def check(self, pair, bands, images, powers=None, name="", conditioned=True):
        """-> worst (P re the target's largest cell, NSIM value, dB image)"""
        n_t = len(self.tgts)
        w_p = w_n = w_d = 0.0
        if self.power is None:                   # (the oracle's filterbank is a Python loop: once per signal of a case)
            self.power = [power_image(s, self.coef, self.hop) for s in self.tgts + self.ests]
        for e, (est, ti) in enumerate(zip(self.ests, self.index)):
            tgt = self.tgts[ti]
            d = analyse(tgt, est, self.coef, self.hop, self.range_db, self.match, self.splits[e], self.power[ti], self.power[n_t + e])
            tag = "%s pair %d" % (name, e)
            ok = not np.isnan(d["pair"][0])
            if ok and conditioned:
                assert_conditioned(tgt, est, self.coef, self.hop, self.range_db, self.match, tag, d)
            assert np.array_equal(np.isnan(pair[e]), np.isnan(d["pair"])) and not np.isinf(pair[e]).any(), (tag, pair[e], d["pair"])
            assert np.array_equal(np.isnan(bands[e]), np.isnan(d["bands"])) and not np.isinf(bands[e]).any(), (tag, bands[e])
            if ok:
                w_n = max(w_n, float(np.nanmax(np.abs(pair[e] - d["pair"]))), float(np.nanmax(np.abs(bands[e] - d["bands"]))))
            top = float(np.max(d["Pr"])) if d["Pr"].size else 0.0
            if powers is not None and top > 0.0:
                w_p = max(w_p, float(np.max(np.abs(powers[ti] - d["Pr"]))) / top, float(np.max(np.abs(powers[n_t + e] - d["Pd"]))) / top)
            if images is not None and d["Dr"] is not None:
                # the dB images, and through their unclamped cells the power images themselves: 10^(D / 10) against P (the estimate's
                # against f P) re the target's largest cell - the bar for P where only the images leave the library
                for img, D, Pw in ((images[ti], d["Dr"], d["Pr"]), (images[n_t + e], d["Dd"], d["Pd"] * (d["f"] if math.isfinite(d["f"]) else 1.0))):
                    if np.isnan(D).all() and D.size:             # (the level factor's NaN rule)
                        assert np.isnan(img).all(), tag
                        continue
                    assert not np.isinf(img).any(), tag
                    w_d = max(w_d, float(np.max(np.abs(img - D))))
                    free = D > d["floor_db"]
                    if free.any():
                        w_p = max(w_p, float(np.max(np.abs(10.0 ** (img[free] / 10.0) - Pw[free]))) / top)
            elif images is not None:
                assert np.isnan(images[ti]).all() and np.isnan(images[n_t + e]).all(), tag
        assert w_p <= TOL_P and w_n <= TOL_NSIM and w_d <= 1e-6, (name, w_p, w_n, w_d)
        return w_p, w_n, w_d
