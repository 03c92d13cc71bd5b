"""NumPy / SciPy float64 oracle of the modulation family: the envelopes of section 23's gammatone bands
(auditory_oracle.filterbank) as block RMS values, eight second-order modulation band-passes (scipy.signal.lfilter), 256 ms Hamming
frames in explicit loops, SRMR's adaptive ratio and the modulation-spectrum distance.  The definition restated, line by line;
nothing here knows how the kernels cut a signal.  full_rate_srmr() is the variant the family is measured against: |z| at the
signal's own rate through the same bank designed at that rate.

The analyses are kept per input (analyses_of): the gammatone cascade is a Python loop over the samples, and the host and the device
tests of one session score the same cases."""
import math

import numpy as np

import auditory_oracle as A

K = 8                   # modulation bands
Q = 2.0
TOL_E = 1e-9            # Ebar re the signal's largest cell
TOL_SRMR = 1e-9         # times max(1, |srmr|)
TOL_DIFF = 2e-9         # srmr_diff, times max(1, |srmr|) (of the two values the one nearer to 0)
TOL_DIST = 1e-6         # dB
C90_MARGIN = 1e-6       # the cumulative shares at c90 and c90 - 1 stay this far from 0.9
LEVEL_MARGIN = 1e-12    # sum Ebar_estimate at least this share of sum Ebar_target, or exactly 0


# ---- design ----------------------------------------------------------------------------------------------------------------------
def hop_e(fs, env_rate=1600):
    return max(1, int(fs // env_rate))


def frame_step(fe):
    return int(math.floor(0.064 * fe + 0.5))


def mod_centres():
    return 4.0 * 32.0 ** (np.arange(K) / 7.0)


def mod_design(fe):
    """[8, 5] = (b0, b1, b2, a1, a2): the bilinear (RBJ) band-pass of unit peak gain, Q = 2, at the envelope rate fe."""
    out = np.empty((K, 5))
    for k, f in enumerate(mod_centres()):
        w0 = 2.0 * math.pi * f / fe
        alpha = math.sin(w0) / (2.0 * Q)
        out[k] = (alpha / (1.0 + alpha), 0.0, -alpha / (1.0 + alpha), -2.0 * math.cos(w0) / (1.0 + alpha), (1.0 - alpha) / (1.0 + alpha))
    return out


def kstar_table(fc, kstar=None):
    if kstar is not None:
        return np.full(len(fc), int(kstar), np.int32)
    edge = mod_centres()[4:] * (math.sqrt(1.0 + 1.0 / (4.0 * Q * Q)) - 1.0 / (2.0 * Q))
    return np.array([max(5, 4 + sum(1 for e in edge if e < A.erbn(f))) for f in fc], np.int32)


def split_band(fc, split_hz):
    """The first band with f_c >= split_hz in [0, C], or -1 for no split."""
    return -1 if split_hz is None else int(np.searchsorted(np.asarray(fc), float(split_hz), side="left"))


def hamming(W):
    return np.array([0.54 - 0.46 * math.cos(2.0 * math.pi * i / (W - 1)) for i in range(W)])


# ---- one signal ------------------------------------------------------------------------------------------------------------------
def blocks(n, hop):
    return n // hop if n >= 2 * hop else 0


def frames(nb, S):
    return 1 + (nb - 4 * S) // S if nb >= 4 * S else 0


def envelopes(signals, coef, hop, budget=1 << 27):
    """env [NB, C] = sqrt(B / hop) of every signal, B the block sums of |z|^2.  auditory_oracle.filterbank runs one Python loop over
    the samples with the bands as a vector: signals of about one length go through it together, each with its own copy of the
    bands (a sample row holds every signal's sample once per band; the shorter ones end in zeros, which a causal filter never
    sees before their end) - element by element the arithmetic of a call per signal."""
    C = len(coef)
    out = [None] * len(signals)
    todo = sorted((i for i in range(len(signals)) if blocks(len(signals[i]), hop) > 0), key=lambda i: -len(signals[i]))
    for i in range(len(signals)):
        if out[i] is None and i not in todo:
            out[i] = np.zeros((0, C))
    while todo:
        n = len(signals[todo[0]])
        group = [i for i in todo if 4 * len(signals[i]) >= 3 * n][:max(1, budget // (16 * C * n))]
        todo = [i for i in todo if i not in group]
        X = np.zeros((n, len(group) * C))
        for j, i in enumerate(group):
            X[:len(signals[i]), j * C:(j + 1) * C] = np.asarray(signals[i], np.float64)[:, None]
        e = np.abs(A.filterbank(X, np.tile(coef, (len(group), 1)))) ** 2
        for j, i in enumerate(group):
            nb = blocks(len(signals[i]), hop)
            B = np.array([[math.fsum(e[j * C + c, m * hop:(m + 1) * hop]) for c in range(C)] for m in range(nb)])
            out[i] = np.sqrt(B / hop)
    return out


def envelope(x, coef, hop):
    return envelopes([x], coef, hop)[0]


def spectrum(env, mod, S):
    """Ebar [C, 8] from the envelope [NB, C] at its own rate (all NaN where no frame fits), and F"""
    from scipy.signal import lfilter
    nb, C = env.shape
    W, F = 4 * S, frames(env.shape[0], S)
    if F == 0:
        return np.full((C, K), np.nan), 0
    w = hamming(W)
    out = np.zeros((C, K))
    for c in range(C):
        for k in range(K):
            v = lfilter(mod[k, :3], np.concatenate(([1.0], mod[k, 3:])), env[:, c])
            total = 0.0
            for f in range(F):
                total += math.fsum((w * v[f * S:f * S + W]) ** 2)
            out[c, k] = total / F
    return out, F


def srmr_of(E, kstar):
    """-> (srmr, K*, c90, sum Ebar, the cumulative shares at c90 - 1 and c90): NaN / -1 by the NaN rules"""
    if np.isnan(E).any():
        return math.nan, -1, -1, math.nan, (math.nan, math.nan)
    e = np.sum(E, axis=1)
    total = float(np.sum(e))
    if not total > 0.0:
        return math.nan, -1, -1, total, (math.nan, math.nan)
    share = np.cumsum(e) / total
    c90 = int(np.argmax(np.cumsum(e) > 0.9 * total))
    ks = int(kstar[c90])
    den = float(np.sum(E[:, 4:ks]))
    val = float(np.sum(E[:, :4])) / den if den > 0.0 else math.nan
    return val, ks, c90, total, (float(share[c90 - 1]) if c90 else 0.0, float(share[c90]))


def analyse_signal(x, fs, hop, n_bands=32, band=None, kstar=None):
    """-> {"E": Ebar [C, 8], "F", "srmr", "kstar", "c90", "total", "shares"}"""
    fc, coef = A.design(fs, n_bands, band)
    fe = fs / hop
    E, F = spectrum(envelope(x, coef, hop), mod_design(fe), frame_step(fe))
    val, ks, c90, total, shares = srmr_of(E, kstar_table(fc, kstar))
    return {"E": E, "F": F, "srmr": val, "kstar": ks, "c90": c90, "total": total, "shares": shares}


def full_rate_srmr(x, fs, n_bands=32, band=None, kstar=None):
    """SRMR with |z| at fs as the envelope and the modulation bank designed at fs"""
    fc, coef = A.design(fs, n_bands, band)
    env = np.abs(A.filterbank(np.asarray(x, np.float64), coef)).T
    E, _ = spectrum(np.ascontiguousarray(env), mod_design(float(fs)), frame_step(float(fs)))
    return srmr_of(E, kstar_table(fc, kstar))[0]


_KEPT = {}


def analyses_of(signals, fs, hop, n_bands, kstar=None):
    """analyse_signal() of float64 arrays, computed once per distinct input (those not seen yet filtered together: envelopes())"""
    sigs = [np.ascontiguousarray(x, np.float64) for x in signals]
    keys = [(x.tobytes(), fs, hop, n_bands, kstar) for x in sigs]
    new = [i for i, k in enumerate(keys) if k not in _KEPT and keys.index(k) == i]
    if new:
        fc, coef = A.design(fs, n_bands)
        fe = fs / hop
        for i, env in zip(new, envelopes([sigs[i] for i in new], coef, hop)):
            E, F = spectrum(env, mod_design(fe), frame_step(fe))
            val, ks, c90, total, shares = srmr_of(E, kstar_table(fc, kstar))
            _KEPT[keys[i]] = {"E": E, "F": F, "srmr": val, "kstar": ks, "c90": c90, "total": total, "shares": shares}
    return [_KEPT[k] for k in keys]


# ---- a pair ----------------------------------------------------------------------------------------------------------------------
def pair_of(t, e, split=-1, range_db=60.0):
    """(srmr_diff, mod_dist, mod_dist_hf, mod_dist_lf) from two analyse_signal() results, and the level factor"""
    nan4 = np.full(4, np.nan)
    if t["F"] == 0 or not t["total"] > 0.0:
        return nan4, math.nan
    with np.errstate(divide="ignore", over="ignore"):
        f = float(np.float64(t["total"]) / np.float64(e["total"]))
    if not (math.isfinite(f) and f > 0.0):
        return nan4, f
    floor = 10.0 * math.log10(float(np.max(t["E"]))) - range_db
    with np.errstate(divide="ignore"):
        Dt = np.maximum(10.0 * np.log10(t["E"]), floor)
        De = np.maximum(10.0 * np.log10(e["E"] * f), floor)
    d2 = (De - Dt) ** 2
    C = d2.shape[0]
    out = np.array([e["srmr"] - t["srmr"], math.sqrt(float(np.mean(d2))), math.nan, math.nan])
    if 0 <= split < C:
        out[2] = math.sqrt(float(np.mean(d2[split:])))
    if split > 0:
        out[3] = math.sqrt(float(np.mean(d2[:split])))
    return out, f


def assert_conditioned(d, name="", target=None):
    """An input of the comparison keeps its discrete decision away from rounding: the cumulative shares at c90 and c90 - 1 stay
    C90_MARGIN from 0.9; as the estimate of a pair with finite values its sum Ebar is LEVEL_MARGIN of the target's.  -> the margin"""
    if d["F"] == 0 or not d["total"] > 0.0:
        return math.inf
    margin = min(abs(s - 0.9) for s in d["shares"])
    assert margin >= C90_MARGIN, (name, d["shares"])
    if target is not None and target["F"] > 0 and target["total"] > 0.0:
        assert d["total"] == 0.0 or d["total"] >= LEVEL_MARGIN * target["total"], (name, d["total"], target["total"])
    return margin


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def voiced(n, fs, seed=0, f0=120.0, rate=4.0):
    """a harmonic tone whose level moves at the syllable rate (and a little faster), over a faint noise floor"""
    t = np.arange(n) / fs
    rng = np.random.default_rng(seed)
    k = np.arange(1, int(0.4 * fs / f0))
    x = np.sum(np.sin(2.0 * np.pi * f0 * k[:, None] * t[None, :] + rng.uniform(0, 2 * np.pi, len(k))[:, None]) / k[:, None], axis=0)
    env = (0.5 + 0.5 * np.sin(2.0 * np.pi * rate * t + rng.uniform(0, 2 * np.pi))) ** 2 * (0.8 + 0.2 * np.sin(2.0 * np.pi * 11.0 * t))
    return 0.2 * env * x + 1e-3 * rng.standard_normal(n)


def reverberated(x, fs, seed, t60=0.4):
    """x through an exponentially decaying noise tail"""
    rng = np.random.default_rng(seed)
    n = int(t60 * fs)
    h = rng.standard_normal(n) * np.exp(-6.9 * np.arange(n) / n)
    h[0] = 1.0
    return np.convolve(x, h / np.sqrt(np.sum(h * h)))[:len(x)]


def geometry_lengths(fs, hop, S, n_bands, tile):
    """The lengths where the geometry can go wrong, in samples: no frame, one, one short of two, two; one sample short of and one past
    a multiple of a segment (8 blocks), of a sweep workgroup ((256 / CP) 8 blocks) and of the bank's staging tile (`tile` blocks) -
    each the first multiple that holds a frame and is not taken yet -; a length that is no multiple of hop; 2 s"""
    W = 4 * S
    cp = 4
    while cp < n_bands:
        cp <<= 1
    lens, taken = [W * hop - 1, W * hop, (W + S) * hop - 1, (W + S) * hop], set()
    for q in (8, 256 // cp * 8, tile):
        m = -(-(W + 1) // q) * q
        while m in taken:
            m += q
        taken.add(m)
        lens += [m * hop - 1, m * hop + 1]
    # (the frames of W + 12 S blocks end on a tile boundary where S = 102: 1632 = 51 * 32)
    return lens + [(W + 12 * S) * hop + hop // 2 + 1, 2 * int(fs)]


class Case:
    """One call of ssr_modulation: targets, estimates, the pair -> target map and the options; check() compares (signal_out,
    pair_out, spectrum_out or None) with the oracle."""

    def __init__(self, tgts, ests, index, fs, hop, n_bands=32, splits=None, range_db=60.0, kstar=None, tdt=np.float64, edt=np.float64):
        self.tgts, self.ests = [np.asarray(t, tdt) for t in tgts], [np.asarray(e, edt) for e in ests]
        self.index, self.fs, self.hop, self.n_bands, self.range_db, self.kstar = list(index), fs, hop, n_bands, range_db, kstar
        self.splits = [-1] * len(ests) if splits is None else list(splits)
        self.tdt, self.edt = tdt, edt
        self.fc, self.coef = A.design(fs, n_bands)
        fe = fs / hop
        self.mod, self.S, self.ktab = mod_design(fe), frame_step(fe), kstar_table(self.fc, kstar)

    def check(self, signal, pair, spectrum=None, name=""):
        """-> worst (Ebar re the signal's largest cell, srmr re max(1, |srmr|), mod_dist* in dB, srmr_diff re max(1, |srmr|))"""
        n_t = len(self.tgts)
        an = analyses_of(self.tgts + self.ests, self.fs, self.hop, self.n_bands, self.kstar)
        w_e = w_s = w_d = w_f = 0.0
        assert not np.isinf(signal).any() and not np.isinf(pair).any() and (spectrum is None or not np.isinf(spectrum).any()), name
        for i, d in enumerate(an):
            tag = "%s signal %d" % (name, i)
            assert_conditioned(d, tag)
            got = signal[i]
            if math.isnan(d["srmr"]):
                assert math.isnan(got[0]), (tag, got)
            else:
                w_s = max(w_s, abs(got[0] - d["srmr"]) / max(1.0, abs(d["srmr"])))
            if d["c90"] < 0:
                assert np.isnan(got[1:3]).all(), (tag, got)
                assert (math.isnan(got[3]) and math.isnan(d["total"])) or got[3] == d["total"] == 0.0, (tag, got)
            else:
                assert got[1] == d["kstar"] and got[2] == d["c90"], (tag, got, d["kstar"], d["c90"], d["shares"])
                assert abs(got[3] - d["total"]) <= TOL_E * K * self.n_bands * float(np.max(d["E"])), (tag, got)
            if spectrum is not None:
                assert np.array_equal(np.isnan(spectrum[i]), np.isnan(d["E"])), tag
                if d["F"] > 0 and np.max(d["E"]) > 0.0:
                    w_e = max(w_e, float(np.max(np.abs(spectrum[i] - d["E"]))) / float(np.max(d["E"])))
                elif d["F"] > 0:
                    assert not np.any(spectrum[i]), tag
        for e, ti in enumerate(self.index):
            tag = "%s pair %d" % (name, e)
            want, _ = pair_of(an[ti], an[n_t + e], self.splits[e], self.range_db)
            assert np.array_equal(np.isnan(pair[e]), np.isnan(want)), (tag, pair[e], want)
            if not math.isnan(want[1]):
                assert_conditioned(an[n_t + e], tag, an[ti])
                w_d = max(w_d, float(np.nanmax(np.abs(pair[e, 1:] - want[1:]))))
            if not math.isnan(want[0]):
                w_f = max(w_f, abs(pair[e, 0] - want[0]) / max(1.0, min(abs(an[ti]["srmr"]), abs(an[n_t + e]["srmr"]))))
        assert w_e <= TOL_E and w_s <= TOL_SRMR and w_d <= TOL_DIST and w_f <= TOL_DIFF, (name, w_e, w_s, w_d, w_f)
        return w_e, w_s, w_d, w_f


def geometry_case(fs, n_bands, env_rate=1600, tile=32, tdt=np.float64, edt=np.float32, short=False):
    """The geometry lengths as the targets of ONE ragged batch.  Estimates: the no-frame and the one-frame target one each (itself plus
    noise), the first segment-boundary target three (reverberated; plus noise; unrelated noise), the last target (2 s; `short`: the
    tile-boundary one) one (reverberated); the splits run through -1, 0, n_bands and the middle band."""
    hop = hop_e(fs, env_rate)
    S = frame_step(fs / hop)
    lens = geometry_lengths(fs, hop, S, n_bands, tile)
    if short:
        lens = lens[:4] + lens[-2:-1]
    tgts = [voiced(n, fs, 100 + i) for i, n in enumerate(lens)]
    last = len(lens) - 1
    pick = [0, 1, 4, 4, 4, last] if not short else [0, 1, 3, 3, 3, last]
    ests = [tgts[0] + A.noise(lens[0], 200, 0.02), tgts[1] + A.noise(lens[1], 201, 0.02), reverberated(tgts[pick[2]], fs, 202),
            tgts[pick[2]] + A.noise(lens[pick[2]], 203, 0.02), A.noise(lens[pick[2]], 204), reverberated(tgts[last], fs, 205)]
    cycle = [-1, 0, n_bands, max(1, n_bands // 2)]
    return Case(tgts, ests, pick, fs, hop, n_bands, splits=[cycle[e % 4] for e in range(len(ests))], tdt=tdt, edt=edt)


# (fs, bands, env_rate): the shapes of the family's tests, then one case at each end of env_rate (hop_e = 1 among them)
SHAPES = [(8000, 3, 1600), (8000, 32, 1600), (8000, 40, 1600), (44100, 32, 1600), (48000, 32, 1600), (16000, 32, 800), (8000, 32, 6400)]
SHAPE_IDS = ["8k-3", "8k-32", "8k-40", "44k1-32", "48k-32", "16k-env800", "8k-env6400"]


def same_bits(a, b):
    return all((x is None and y is None) or np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def sub_case(c, targets, pairs):
    """The Case of some targets and pairs of c, in that order"""
    return Case([c.tgts[t] for t in targets], [c.ests[e] for e in pairs], [targets.index(c.index[e]) for e in pairs], c.fs, c.hop, c.n_bands,
                splits=[c.splits[e] for e in pairs], range_db=c.range_db, kstar=c.kstar, tdt=c.tdt, edt=c.edt)
