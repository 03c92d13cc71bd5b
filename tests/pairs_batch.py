"""The large batch of the per-pair families that were added after tests/test_gpu_pairs_batch.py was written - bss, coherence, spectrum,
auditory, modulation, csii and loudness - and the checks both its users run on it: tests/test_gpu_pairs_batch.py on the device and
tests/test_pairs_batch_host.py on the kernel bodies compiled for the host (tests/emu/*_emu.cpp).  Test infrastructure; nothing in
ssr_eval_amd imports it.

The batch: N_EST = 2 NT + 3 pairs (NT = SSR_PAIRS_NT, the threads of the geometry workgroup: every thread owns three pairs, the
trailing threads none), run k holding k % 5 + 1 pairs of target k, except run 3, which names target 1 again; float32 signals.
Target t has the length LENGTHS[t % 4] of its family:

  family      settings                        0   no item            shortest finite         two grid items
  bss         8 taps                          0   -  (1: see below)  1 (5: fewer than taps)  16384 + 5: two tiles of 16384 samples
  coherence   n_fft 256, hop 128              0   255: K = 0         384: K = 2              4355: K = 33, two chunks of 32 segments
  spectrum    n_fft 256, hop 128              0   255: K = 0         256: K = 1              4355: K = 33, two chunks of 32 segments
  auditory    16 kHz, hop 8, 5 bands          0   15: no row         32: T = 3 rows          4133: three staging tiles of 2048 samples
  modulation  8 kHz, hop_e 5, 3 bands         0   9: no block        2040: one frame         2553: two frames, 16 tiles of 32 rows
  csii        16 kHz, n_fft 256, hop 128      0   255: K = 0         384: K = 2              4355: K = 33, two chunks of 32 segments
  loudness    8 kHz (sub-blocks of 800)       0   799: no sub-block  3200: one 400 ms block  4807: six sub-blocks, three peak tiles

bss has no length above 0 without an item - a tile is any 1 .. 16384 samples, and a pair shorter than the filter is scored on the terms
that exist -, so its second class is 1 sample, the shortest length with a value, and its third 5 samples, fewer than the 8 taps; its
rows without a value are those of length 0 alone.  Its tile is a constant of the kernels: the longest class cannot be shorter.

The families that take a value per pair get one from a cycle of period 7 (coprime to the run lengths 1 .. 5 and to their period of
15 pairs), the "none" value among them: coherence its band table (the empty band lo > hi), spectrum split_bins (-1), auditory and
modulation split_bands (-1), csii a split frequency (None: -1).  Batch.pick() slices them with the pairs."""
import numpy as np

NT = 256                                   # SSR_PAIRS_NT
N_EST = 2 * NT + 3
SUB = 64
PERIOD = 7
NAMES = ("bss", "coherence", "spectrum", "auditory", "modulation", "csii", "loudness")
ORACLE_PAIRS = (0, NT - 1, NT, NT + 1, 2 * NT + 2)


def run_index(n_est=N_EST):
    """(tgt_index [n_est], the number of targets): run k has k % 5 + 1 pairs and names target k, except run 3, which names target 1."""
    idx, k = [], 0
    while len(idx) < n_est:
        idx += [1 if k == 3 else k] * (k % 5 + 1)
        k += 1
    return np.array(idx[:n_est], np.int32), k


def sub_batches(idx, n=None):
    """[a, b) pair ranges of at most SUB pairs that end where a run ends (idx None: n signals in ranges of SUB)."""
    if idx is None:
        return [(a, min(a + SUB, n)) for a in range(0, n, SUB)]
    ends = list(1 + np.flatnonzero(np.diff(idx))) + [len(idx)]
    out, a, last = [], 0, 0
    for e in ends:
        if e - a > SUB:
            out.append((a, last))
            a = last
        last = e
    out.append((a, len(idx)))
    assert all(0 < b - a <= SUB for a, b in out) and out[0][0] == 0 and all(x[1] == y[0] for x, y in zip(out, out[1:]))
    return out


class Batch:
    """Targets, estimates, the pair -> target map (None: signals only, in `ests`), the per-pair parameters and the family's settings."""

    def __init__(self, name, tgts, ests, idx, par, cfg):
        self.name, self.tgts, self.ests, self.idx, self.par, self.cfg = name, list(tgts), list(ests), idx, par, cfg

    def pick(self, pairs):
        """(the batch of these pairs with its targets renumbered from 0 in order of appearance, the targets' numbers in self)"""
        pairs = list(pairs)
        par = {k: [v[e] for e in pairs] for k, v in self.par.items()}
        if self.idx is None:
            return Batch(self.name, [], [self.ests[e] for e in pairs], None, par, self.cfg), []
        used = list(dict.fromkeys(int(self.idx[e]) for e in pairs))
        local = np.array([used.index(int(self.idx[e])) for e in pairs], np.int32)
        return Batch(self.name, [self.tgts[t] for t in used], [self.ests[e] for e in pairs], local, par, self.cfg), used

    def lengths(self):
        return np.array([len(e) for e in self.ests])


def _cycle(values, n=N_EST):
    assert len(values) == PERIOD
    return [values[e % PERIOD] for e in range(n)]


def _f32(x):
    return np.ascontiguousarray(x, np.float32)


def _build(name, lengths, cfg, target, estimate, par):
    """target(n, t) -> the float64 target t of n samples, estimate(x, e, t) -> pair e's estimate of x = target t"""
    idx, n_tgt = run_index()
    tgts = [_f32(target(lengths[t % 4], t)) if lengths[t % 4] else np.zeros(0, np.float32) for t in range(n_tgt)]
    ests = [_f32(estimate(tgts[t].astype(np.float64), e, int(t))) if len(tgts[t]) else np.zeros(0, np.float32) for e, t in enumerate(idx)]
    b = Batch(name, tgts, ests, idx, par, dict(cfg, lengths=tuple(lengths)))
    assert len(b.ests) == N_EST and all(len(e) == len(b.tgts[t]) for e, t in zip(b.ests, idx))
    return b


def _noise(n, seed, amp=0.1):
    return amp * np.random.default_rng(seed).standard_normal(n)


# ---- the seven families: build(), outputs(raw result) and check(sub-batch, its outputs) -----------------------------------------------
# outputs: {name: (kind, rows)}; kind "pair": a row per estimate; kind "sig": a row per target, then a row per estimate.  "main" is
# what the call returns without its optional outputs.
def build_bss():
    return _build("bss", (0, 1, 5, 16384 + 5), dict(taps=8), lambda n, t: _noise(n, 1000 + t),
                  lambda x, e, t: 0.7 * np.concatenate([np.zeros(min(1, len(x))), x[:len(x) - min(1, len(x))]]) + _noise(len(x), 5000 + e, 0.02), {})


def outputs_bss(raw, opt):
    out, filt = raw if isinstance(raw, tuple) else (raw, None)
    return {"main": ("pair", out)} if filt is None else {"main": ("pair", out), "filter": ("pair", filt)}


def check_bss(b, o, check_rows):
    check_rows(o["main"], b.tgts, b.ests, b.idx, b.cfg["taps"], "batch")


def build_coherence():
    import coherence_oracle as O
    N = 256
    slot = [(10, N // 2), (5, 4), (64, N // 2), (0, 0), (17, 40), (N // 2, N // 2), (33, 100)]          # (5, 4): the empty band
    bands = [[(0, N // 2), slot[e % PERIOD], slot[(e + 3) % PERIOD]] for e in range(N_EST)]
    pairs = {}

    def target(n, t):
        pairs[t] = O.input_pair(n, 2000 + t)
        return pairs[t][0]
    return _build("coherence", (0, 255, O.len_for_segments(2, N, 128), O.len_for_segments(O.FR + 1, N, 128, 3)), dict(N=N, H=128, thr=0.5), target,
                  lambda x, e, t: pairs[t][1] + _noise(len(x), 6000 + e, 0.05), {"bands": bands})


def outputs_coherence(raw, opt):
    out, g2 = raw if isinstance(raw, tuple) else (raw, None)
    return {"main": ("pair", out)} if g2 is None else {"main": ("pair", out), "spectrum": ("pair", g2)}


def check_coherence(b, o):
    import coherence_oracle as O
    O.check_rows(o["main"], o.get("spectrum"), b.tgts, b.ests, b.idx, b.cfg["N"], b.cfg["H"], b.par["bands"], b.cfg["thr"], what="batch")


def build_spectrum():
    import spectrum_oracle as O
    N = 256
    return _build("spectrum", (0, 255, 256, N + 32 * 128 + 3), dict(N=N, H=128, bands=[(2, 9), (10, 40), (41, N // 2)]),
                  lambda n, t: O.white(n, 3000 + t), lambda x, e, t: 0.7 * x + O.coloured(len(x), 7000 + e),
                  {"splits": _cycle([-1, 32, 64, 3, N // 2, 17, 100])})


def case_spectrum(b):
    import spectrum_oracle as O
    return O.Case(b.tgts, b.ests, b.idx, b.cfg["N"], b.cfg["H"], bands=b.cfg["bands"], splits=b.par["splits"], tdt=np.float32, edt=np.float32)


def outputs_spectrum(raw, opt):
    o = {"sig": ("sig", raw[0]), "main": ("pair", raw[1])}
    if opt:
        o["ltas"] = ("sig", raw[2])
    return o


def check_spectrum(b, o):
    case_spectrum(b).check((o["sig"], o["main"], o.get("ltas"), None), "batch")


def build_auditory():
    import auditory_oracle as O
    fs, hop, C = 16000, 8, 5
    return _build("auditory", (0, 2 * hop - 1, 4 * hop, 2 * 2048 + 37), dict(fs=fs, hop=hop, n_bands=C, coef=O.design(fs, C)[1]),
                  lambda n, t: O.harmonic(n, fs, 4000 + t), lambda x, e, t: x + O.noise(len(x), 8000 + e, 0.02),
                  {"splits": _cycle([-1, 1, C - 1, C // 2, 3, -1, 1])})


def case_auditory(b):
    import auditory_oracle as O
    return O.Case(b.tgts, b.ests, b.idx, b.cfg["coef"], b.cfg["hop"], splits=b.par["splits"], tdt=np.float32, edt=np.float32, fs=b.cfg["fs"])


def outputs_auditory(raw, opt):
    o = {"main": ("pair", raw[0])}
    if opt:
        o["bands"], o["images"] = ("pair", raw[1]), ("sig", raw[2])
    return o


def check_auditory(b, o):
    case_auditory(b).check(o["main"], o["bands"], o["images"], name="batch")


def build_modulation():
    import auditory_oracle as A
    import modulation_oracle as O
    fs, C = 8000, 3
    hop = O.hop_e(fs)
    S = O.frame_step(fs / hop)
    return _build("modulation", (0, 2 * hop - 1, 4 * S * hop, 5 * S * hop + 3), dict(fs=fs, hop=hop, n_bands=C),
                  lambda n, t: O.voiced(n, fs, 5000 + t), lambda x, e, t: x + A.noise(len(x), 9000 + e, 0.02),
                  {"splits": _cycle([-1, 0, C, 1, 2, -1, 1])})


def case_modulation(b):
    import modulation_oracle as O
    return O.Case(b.tgts, b.ests, b.idx, b.cfg["fs"], b.cfg["hop"], b.cfg["n_bands"], splits=b.par["splits"], tdt=np.float32, edt=np.float32)


def outputs_modulation(raw, opt):
    o = {"signal": ("sig", raw[0]), "main": ("pair", raw[1])}
    if opt:
        o["spectrum"] = ("sig", raw[2])
    return o


def check_modulation(b, o):
    case_modulation(b).check(o["signal"], o["main"], o.get("spectrum"), name="batch")


def build_csii():
    import coherence_oracle as CO
    import csii_oracle as O
    fs, N, H = 16000, 256, 128
    return _build("csii", (0, 255, CO.len_for_segments(2, N, H), CO.len_for_segments(CO.FR + 1, N, H, 3)), dict(fs=fs, N=N, H=H),
                  lambda n, t: O.speech_like(n, fs, 6000 + t), lambda x, e, t: O.noisy(x, 3.0 + 4.0 * (e % 3), 10000 + e),
                  {"splits": _cycle([None, 2000.0, 3000.0, 7500.0, 1000.0, 4500.0, 150.0])})      # 7500 Hz: above the last centre


def outputs_csii(raw, opt):
    return {"main": ("pair", raw[0]), "bands": ("pair", raw[1])} if opt else {"main": ("pair", raw[0])}


def check_csii(b, o):
    import csii_oracle as O
    O.check_rows(o["main"], b.tgts, b.ests, b.idx, b.cfg["fs"], b.cfg["N"], b.cfg["H"], None, b.par["splits"], o.get("bands"), what="batch")


def build_loudness():
    fs, h = 8000, 800
    lengths = (0, h - 1, 4 * h, 6 * h + 7)
    sigs = [_f32(_noise(lengths[i % 4], 7000 + i, 0.2)) for i in range(N_EST)]
    return Batch("loudness", [], sigs, None, {}, dict(fs=fs, lengths=lengths))


def outputs_loudness(raw, opt):
    out, E = raw if isinstance(raw, tuple) else (raw, None)
    return {"main": ("pair", out)} if E is None else {"main": ("pair", out), "blocks": ("pair", E)}


def check_loudness(b, o):
    import loudness_oracle as O
    for i, s in enumerate(b.ests):
        O.check(o["main"][i], o["blocks"][i] if "blocks" in o else None, s, b.cfg["fs"], "signal %d (n = %d)" % (i, len(s)))


BUILD = {"bss": build_bss, "coherence": build_coherence, "spectrum": build_spectrum, "auditory": build_auditory,
         "modulation": build_modulation, "csii": build_csii, "loudness": build_loudness}
OUTPUTS = {"bss": outputs_bss, "coherence": outputs_coherence, "spectrum": outputs_spectrum, "auditory": outputs_auditory,
           "modulation": outputs_modulation, "csii": outputs_csii, "loudness": outputs_loudness}
CHECK = {"coherence": check_coherence, "spectrum": check_spectrum, "auditory": check_auditory, "modulation": check_modulation,
         "csii": check_csii, "loudness": check_loudness}      # (bss: check_bss with the check_rows of the caller's side)
# the column of "main" that holds a value wherever the pair has one, and the columns that are NaN where it has none
VALUE = {"bss": (0,), "coherence": (0, 0), "spectrum": (6,), "auditory": (0,), "modulation": (1,), "csii": (0,), "loudness": (0,)}
NO_VALUE = {"bss": np.s_[:], "coherence": np.s_[:], "spectrum": np.s_[:], "auditory": np.s_[:], "modulation": np.s_[:], "csii": np.s_[:9],
            "loudness": np.s_[:4]}
_BATCHES = {}


def batch(name):
    """The family's batch, built once per session."""
    if name not in _BATCHES:
        _BATCHES[name] = BUILD[name]()
    return _BATCHES[name]


# ---- the checks ------------------------------------------------------------------------------------------------------------------------
def _bits(rows):
    """One bytes object per row: the float64 bit patterns (NaN rows compare by their bits)."""
    return [np.ascontiguousarray(r, np.float64).view(np.uint64).tobytes() for r in rows]


def _slice(o, n_t, used, pairs):
    """The outputs of the sub-batch Batch.pick(pairs) cut out of the whole batch's"""
    take = lambda rows, ii: [rows[i] for i in ii] if isinstance(rows, list) else rows[list(ii)]      # noqa: E731
    return {k: take(rows, pairs) if kind == "pair" else take(rows, list(used) + [n_t + e for e in pairs]) for k, (kind, rows) in o.items()}


def whole_and_parts(b, run, opt):
    """-> the outputs of the whole batch; asserts that they are, bit for bit, those of its consecutive sub-batches"""
    n_t = len(b.tgts)
    whole = OUTPUTS[b.name](run(b, opt), opt)
    ranges = sub_batches(b.idx, len(b.ests))
    assert len(ranges) >= N_EST // SUB
    for a, z in ranges:
        sub, used = b.pick(range(a, z))
        part = OUTPUTS[b.name](run(sub, opt), opt)
        assert list(part) == list(whole)
        cut = _slice(whole, n_t, used, range(a, z))
        for k, (kind, rows) in part.items():
            want = cut[k]
            assert len(rows) == len(want) == (z - a if kind == "pair" else len(used) + z - a), (b.name, k, a, z, len(rows))
            diff = [i for i, (x, y) in enumerate(zip(_bits(rows), _bits(want))) if x != y]
            assert not diff, (b.name, k, "opt" if opt else "plain", (a, z), diff[:8], rows[diff[0]], want[diff[0]])
    return whole


def value_column(name, main):
    v = np.asarray(main, np.float64)
    for c in VALUE[name]:
        v = v[:, c]
    return v


def oracle_pairs(b, finite):
    """ORACLE_PAIRS and the first pair of the target that two runs name, each moved to the nearest pair with a finite value"""
    want = list(ORACLE_PAIRS) + ([int(np.flatnonzero(b.idx == 1)[0])] if b.idx is not None else [])
    ok = np.flatnonzero(finite)
    return sorted({int(ok[np.argmin(np.abs(ok - e))]) for e in want})


def check_family(name, run, check):
    """Everything the two test files assert on the family's batch; run(batch, opt) -> what the family's entry point returns with
    (opt) or without its optional outputs; check(sub-batch, outputs): the family's comparison with its float64 oracle.  Prints and
    returns the pairs it compared with the oracle."""
    b = batch(name)
    lens, L = b.lengths(), b.cfg["lengths"]
    assert len(b.ests) == N_EST and sorted(set(lens.tolist())) == sorted(L) and len(set(L)) == 4 and L[0] == 0     # all four classes occur
    for k, v in b.par.items():
        assert len(v) == N_EST and len({repr(x) for x in v}) >= 3, (name, k)                 # at least three values per parameter
    if b.idx is not None:
        runs = np.flatnonzero(np.diff(b.idx)) + 1
        assert len(np.flatnonzero(b.idx == 1)) == 2 + 4 and not np.all(np.diff(np.flatnonzero(b.idx == 1)) == 1)      # two runs name target 1
        assert set(np.diff(np.concatenate(([0], runs))).tolist()) == {1, 2, 3, 4, 5}
    # 1. the whole batch is its sub-batches, with and without the optional outputs; the outputs both runs have agree
    full = whole_and_parts(b, run, True)
    plain = whole_and_parts(b, run, False)
    assert set(plain) < set(full) and "main" in plain, (name, list(plain), list(full))
    for k in plain:
        assert _bits(plain[k][1]) == _bits(full[k][1]), (name, k)
    # 2. a repeated call repeats the bits
    again = OUTPUTS[name](run(b, True), True)
    for k in full:
        assert _bits(again[k][1]) == _bits(full[k][1]), (name, k)
    # 4. no value where there is no item, values on the longest class
    main = np.asarray(full["main"][1], np.float64)
    value = value_column(name, main)
    empty = L[:1] if name == "bss" else L[:2]
    rows = main.reshape(N_EST, -1) if name != "coherence" else main[:, 0]                    # (coherence: the full band's row)
    assert np.isnan(rows[np.isin(lens, empty)][:, NO_VALUE[name]]).all(), name
    assert np.isfinite(value[lens == L[3]]).all() and np.isfinite(value[lens == L[2]]).all(), name
    assert not np.isfinite(value[np.isin(lens, empty)]).any()
    # 3. the oracle at the seams of the geometry
    pairs = oracle_pairs(b, np.isfinite(value))
    sub, used = b.pick(pairs)
    print(name, "oracle pairs", pairs, "lengths", [int(lens[e]) for e in pairs])
    assert len(pairs) >= 4 and np.isfinite(value[pairs]).all()
    check(sub, _slice(full, len(b.tgts), used, pairs))
    return pairs
