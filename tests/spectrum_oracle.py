"""Float64 oracle of the spectrum family: plain NumPy, np.fft.rfft per segment, restating the definitions.

Framing: N = n_fft, hop H, periodic Hann window, no padding / centring / detrending, K = 1 + (n - N) // H segments for n >= N else 0.
Per signal, X_t[k] the unscaled DFT of windowed segment t, 0 <= k <= N / 2: P[k] = sum_t |X_t[k]|^2, A[k] = sum_t |X_t[k]|; c[k] = 1 at
k = 0 and N / 2, else 2; band lo .. hi; E_tot = sum c P over it;
  rolloff  the smallest r in the band with sum_{lo..r} A >= rho sum_{lo..hi} A
  edge     the highest e in the band with P[e] >= max_band(P) 10^(-drop_db / 10)
  centroid sum k c P / sum c P over the band (bins)
  hf_db    10 log10(max(E_hi / E_tot, DBL_EPSILON)), E_hi over the band's bins >= split
  L_b      10 log10(max(E_b / E_tot, DBL_EPSILON)) per analysis band; ltas_dist = sqrt(mean d_b^2), ltas_max = max |d_b|
K == 0, the empty band and E_tot == 0 give NaN.  Bars: P and A within 1e-9 of the signal's largest bin, rolloff and edge bins equal,
the centroid within 1e-9 N bins (1e-9 fs in Hz), every dB value within 1e-6 dB."""
import fractions
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
TOL_SPEC, TOL_CENTROID, TOL_DB = 1e-9, 1e-9, 1e-6
ROLL_MARGIN, EDGE_MARGIN, LEVEL_FLOOR_DB = 1e-9, 1e-9, -120.0
MAX_BANDS = 40
CASES = ((48000, 2048, 1024), (16000, 512, 128), (8000, 256, 256), (44100, 1024, 512))      # (rate, n_fft, hop) of the input list


def segments(n, N, H):
    return 1 + (n - N) // H if n >= N else 0


def window(N):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)


def weights(N):
    c = np.full(N // 2 + 1, 2.0)
    c[0] = c[-1] = 1.0
    return c


def spectra(x, N, H):
    """-> (P, A, K): the sums over the K segments, in segment order."""
    x = np.asarray(x, np.float64)
    K = segments(len(x), N, H)
    P, A, w = np.zeros(N // 2 + 1), np.zeros(N // 2 + 1), window(N)
    for t in range(K):
        m = np.abs(np.fft.rfft(w * x[t * H:t * H + N]))
        P += m * m
        A += m
    return P, A, K


def hz_to_bins(fs, N, band):
    """AudioMetrics._phase_bins' rule: (ceil(lo N / fs), floor(hi N / fs)) clamped to [0, N / 2]; None: every bin."""
    if band is None:
        return 0, N // 2
    lo, hi = (fractions.Fraction(float(v)) * N / fractions.Fraction(float(fs)) for v in band)
    return max(0, math.ceil(lo)), min(N // 2, math.floor(hi))


def split_bin(fs, N, split_hz):
    """coherence's split_hz rule: the first bin of the upper part is ceil(split N / fs); None: -1 (no split)."""
    return -1 if split_hz is None else math.ceil(fractions.Fraction(float(split_hz)) * N / fractions.Fraction(float(fs)))


def third_octave_bands(fs, N, band=None):
    """The default analysis bands: base-2 third-octave bands, centres 1000 2^(i / 3) Hz, edges 2^(+-1/6) around them; a band's bins
    are those with f_lo <= k fs / N < f_hi; the table starts at the lowest band with f_lo >= lo_hz that holds at least 2 bins, the
    top band is clipped at the scored band's last bin and kept if it still holds at least 2; at most 40 bands (the lowest 40)."""
    lo_bin, hi_bin = hz_to_bins(fs, N, band)
    lo_hz = 0.0 if band is None else float(band[0])
    edge = lambda j: 1000.0 * 2.0 ** ((2 * j - 1) / 6.0)      # noqa: E731  (the lower edge of band j = the upper edge of band j - 1)
    out = []
    for i in range(-60, 40):
        f_lo, f_hi = edge(i), edge(i + 1)
        k0, k1 = math.ceil(f_lo * N / fs), math.ceil(f_hi * N / fs) - 1
        if f_lo < lo_hz or k0 < lo_bin or k0 > hi_bin:
            continue
        clipped = k1 > hi_bin
        k1 = min(k1, hi_bin)
        count = k1 - k0 + 1
        if (not out or clipped) and count < 2:
            continue
        if count >= 1 and len(out) < MAX_BANDS:
            out.append((k0, k1))
    return out


def analyse(x, N, H, lo=0, hi=None, rho=0.97, drop_db=60.0, bands=None):
    """-> dict(K, P, A, cp, roll, edge, centroid (bins), e_tot, levels); the values NaN by the NaN rules."""
    hi = N // 2 if hi is None else hi
    P, A, K = spectra(x, N, H)
    cp = weights(N) * P
    bands = [(0, N // 2)] if bands is None else bands
    d = dict(K=K, P=P, A=A, cp=cp, roll=math.nan, edge=math.nan, centroid=math.nan, e_tot=math.nan, levels=np.full(len(bands), math.nan))
    if K == 0 or lo > hi:
        return d
    e_tot = float(np.sum(cp[lo:hi + 1]))
    if not e_tot > 0.0:
        return d
    cum = np.cumsum(A[lo:hi + 1])
    want = rho * cum[-1]
    r = lo + int(np.argmax(cum >= want))
    thr = np.max(P[lo:hi + 1]) * 10.0 ** (-drop_db / 10.0)
    e = lo + int(np.nonzero(P[lo:hi + 1] >= thr)[0][-1])
    k = np.arange(lo, hi + 1)
    lev = np.array([10.0 * np.log10(max(float(np.sum(cp[a:b + 1])) / e_tot, EPS)) for a, b in bands])
    d.update(roll=float(r), edge=float(e), centroid=float(np.sum(k * cp[lo:hi + 1]) / e_tot), e_tot=e_tot, levels=lev)
    return d


def hf_db(d, split, lo, hi):
    """hf_db of an analyse() result at the first upper bin `split` (-1: none)."""
    k0 = max(split, lo)
    if split < 0 or k0 > hi or math.isnan(d["e_tot"]):
        return math.nan
    return 10.0 * math.log10(max(float(np.sum(d["cp"][k0:hi + 1])) / d["e_tot"], EPS))


def sig_row(d):
    return np.array([d["roll"], d["edge"], d["centroid"]])


def pair_row(dy, dx, split, lo, hi):
    """The eight columns of ssr_spectrum's pair_out."""
    hy, hx = hf_db(dy, split, lo, hi), hf_db(dx, split, lo, hi)
    diff = dy["levels"] - dx["levels"]
    ok = not (math.isnan(dy["e_tot"]) or math.isnan(dx["e_tot"]))
    return np.array([hy, hx, dy["roll"] - dx["roll"], dy["edge"] - dx["edge"], dy["centroid"] - dx["centroid"], hy - hx,
                     math.sqrt(float(np.mean(diff * diff))) if ok else math.nan, float(np.max(np.abs(diff))) if ok else math.nan])


# ---- conditioning: an input on which the two bin decisions and the band levels are not decided by rounding ---------------------------
def conditioning(x, N, H, lo=0, hi=None, rho=0.97, drop_db=60.0, bands=None):
    """-> (rolloff margin re the total magnitude, edge margin relative to the threshold, lowest band level in dB)."""
    hi = N // 2 if hi is None else hi
    d = analyse(x, N, H, lo, hi, rho, drop_db, bands)
    assert not math.isnan(d["e_tot"]), "the input has no energy in the band"
    cum = np.cumsum(d["A"][lo:hi + 1])
    want, r = rho * cum[-1], int(d["roll"]) - lo
    below = cum[r - 1] if r > 0 else 0.0
    roll = min(cum[r] - want, want - below) / cum[-1]
    thr = np.max(d["P"][lo:hi + 1]) * 10.0 ** (-drop_db / 10.0)
    edge = float(np.min(np.abs(d["P"][lo:hi + 1] / thr - 1.0)))
    return float(roll), edge, float(np.min(d["levels"]))


def assert_conditioned(x, N, H, lo=0, hi=None, rho=0.97, drop_db=60.0, bands=None, name=""):
    c = conditioning(x, N, H, lo, hi, rho, drop_db, bands)
    assert c[0] >= ROLL_MARGIN and c[1] >= EDGE_MARGIN and c[2] >= LEVEL_FLOOR_DB, (name, c)
    return c


# ---- the comparison every test of the kernels uses -------------------------------------------------------------------------------
def check_signal(row, d, N, name="", ltas=None, pa=None):
    """A sig_out row (and the signal's ltas_out row / emulation debug row) against analyse()'s d -> worst (spectrum re the largest
    bin, centroid in bins)."""
    if math.isnan(d["e_tot"]):
        assert np.isnan(row).all(), (name, row)
        w_c = 0.0
    else:
        assert row[0] == d["roll"] and row[1] == d["edge"], (name, row, d["roll"], d["edge"])
        w_c = abs(row[2] - d["centroid"])
        assert w_c <= TOL_CENTROID * N, (name, w_c)
    w_s = 0.0
    if ltas is not None:
        if d["K"] == 0:
            assert np.isnan(ltas).all(), name
        else:
            top = max(float(np.max(d["cp"])), np.finfo(np.float64).tiny)
            w_s = float(np.max(np.abs(ltas * d["K"] - d["cp"]))) / top
    if pa is not None and d["K"] > 0:
        top_p, top_a = (max(float(np.max(d[k])), np.finfo(np.float64).tiny) for k in ("P", "A"))
        w_s = max(w_s, float(np.max(np.abs(pa[:, 0] - d["P"]))) / top_p, float(np.max(np.abs(pa[:, 1] - d["A"]))) / top_a)
    assert w_s <= TOL_SPEC, (name, w_s)
    return w_s, w_c


def check_pair(row, want, name=""):
    """A pair_out row against pair_row() -> worst dB difference (columns 0, 1, 5, 6, 7); the bin differences are exact but for the
    centroid's."""
    assert np.array_equal(np.isnan(row), np.isnan(want)) and not np.isinf(row).any(), (name, row, want)
    assert np.array_equal(row[2:4], want[2:4], equal_nan=True), (name, row, want)
    db = [abs(row[j] - want[j]) for j in (0, 1, 5, 6, 7) if not math.isnan(want[j])]
    worst = max(db) if db else 0.0
    assert worst <= TOL_DB, (name, worst, row, want)
    return worst


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def white(n, seed, amp=0.1):
    return amp * np.random.default_rng(seed).standard_normal(n)


def lowpassed(n, seed, cutoff=0.5, floor_db=-90.0):
    """8th-order Butterworth low-passed noise (cutoff as a fraction of Nyquist) over a white floor floor_db below it: the floor keeps
    the band levels above the -120 dB of assert_conditioned."""
    from scipy.signal import butter, sosfilt
    rng = np.random.default_rng(seed)
    x = sosfilt(butter(8, cutoff, output="sos"), 0.1 * rng.standard_normal(n))
    return x + 0.1 * 10.0 ** (floor_db / 20.0) * rng.standard_normal(n)


def coloured(n, seed, pole=0.9):
    """one-pole coloured noise: y[i] = pole y[i - 1] + e[i]"""
    from scipy.signal import lfilter
    return 0.02 * lfilter([1.0], [1.0, -pole], np.random.default_rng(seed).standard_normal(n))


def sine(n, N, k0):
    """a full-scale sine centred on bin k0 of an N-point transform"""
    return np.sin(2.0 * np.pi * k0 * np.arange(n) / N)


def make(kind, n, seed):
    return {"white": white, "lowpassed": lowpassed, "coloured": coloured}[kind](n, seed)


# ---- a call and its comparison -----------------------------------------------------------------------------------------------------
def pack(sigs, gap, dt):
    """-> (buffer with NaN in the unused samples, offsets, lengths)"""
    ln = np.array([len(s) for s in sigs], np.int64)
    off = (np.cumsum(ln + gap) - ln).astype(np.int64)
    data = np.full(int((ln + gap).sum()) + 1, np.nan, dt)
    for o, s in zip(off, sigs):
        data[o:o + len(s)] = s
    return data, off, ln.astype(np.int32)


class Case:
    """One call of ssr_spectrum: targets, estimates, the pair -> target map and the options; check() compares (sig_out, pair_out, ltas_out, debug
    rows or None) with the oracle."""

    def __init__(self, tgts, ests, index, N, H, lo=0, hi=None, rho=0.97, drop=60.0, bands=None, splits=None, tdt=np.float64, edt=np.float64):
        self.tgts, self.ests = [np.asarray(t, tdt) for t in tgts], [np.asarray(e, edt) for e in ests]
        self.index, self.N, self.H, self.lo, self.hi = list(index), N, H, lo, N // 2 if hi is None else hi
        self.rho, self.drop, self.bands = rho, drop, [(0, N // 2)] if bands is None else bands
        self.splits = [-1] * len(ests) if splits is None else splits
        self.tdt, self.edt = tdt, edt

    def signals(self):
        return self.tgts + self.ests

    def analyses(self):
        return [analyse(s.astype(np.float64), self.N, self.H, self.lo, self.hi, self.rho, self.drop, self.bands) for s in self.signals()]

    def check(self, got, name="", conditioned=None):
        """got = run()'s tuple against the oracle -> worst (spectrum, centroid in bins, dB); conditioned: the signals (None: all
        with energy) that must pass assert_conditioned - and do, or the input is wrong."""
        sig, pair, lt, pa = got
        ds = self.analyses()
        worst = [0.0, 0.0, 0.0]
        for i, (s, d) in enumerate(zip(self.signals(), ds)):
            if (conditioned is None and not math.isnan(d["e_tot"])) or (conditioned is not None and i in conditioned):
                assert_conditioned(s.astype(np.float64), self.N, self.H, self.lo, self.hi, self.rho, self.drop, self.bands, "%s signal %d" % (name, i))
            w = check_signal(sig[i], d, self.N, "%s signal %d" % (name, i), None if lt is None else lt[i], None if pa is None else pa[i])
            worst[0], worst[1] = max(worst[0], w[0]), max(worst[1], w[1])
        n_t = len(self.tgts)
        for e, t in enumerate(self.index):
            want = pair_row(ds[n_t + e], ds[t], self.splits[e], self.lo, self.hi)
            worst[2] = max(worst[2], check_pair(pair[e], want, "%s pair %d" % (name, e)))
        return tuple(worst)


GEOMETRY_K = (0, 1, 2, 3, 31, 32, 33, 64, 65)


def geometry_case(N, H, tdt=np.float64, edt=np.float32, **kw):
    """Signals of K = 0 .. 65 segments (the chunk is 32 segments, a transform two), one with digital silence longer than a segment
    from an odd segment on, one from an even one, an all-zero one and an empty one, as targets; estimates: K = 1 and K = 3 per target."""
    rng = np.random.default_rng(N + H)
    tgts = [0.1 * rng.standard_normal(max(0, N + (K - 1) * H + min(K % 3, H - 1))) if K else 0.1 * rng.standard_normal(N - 1) for K in GEOMETRY_K]
    span = N // H + 2                                             # segments a silent run must cover to empty at least one
    for first in (3, 6):
        x = 0.1 * rng.standard_normal(N + 40 * H)
        x[first * H:(first + span) * H + N] = 0.0
        tgts.append(x)
    tgts += [np.zeros(N + 5 * H), np.zeros(0)]
    index = [4, 8, 8, 8, 9, 10, 11, 0, 12]
    ests = [0.1 * rng.standard_normal(len(tgts[t])) if t != 11 else np.zeros(len(tgts[t])) for t in index]
    ests[4][:N + 2 * H] = 0.0                                      # silence from the start: the first transform's halves are both empty
    return Case(tgts, ests, index, N, H, tdt=tdt, edt=edt, **kw)
