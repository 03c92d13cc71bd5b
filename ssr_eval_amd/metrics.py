"""AudioMetrics - drop-in for ssr_eval.metrics.AudioMetrics (ssr_eval/metrics.py:15-132) on MI355X.

Same constructor, method names, argument order (estimate first, target second) and result keys as the
reference.  All arithmetic runs in libssrhip.so (HIP, gfx950):

* ``evaluation`` -> one ``ssr_pair_metrics`` call: STFT of both signals (two-for-one complex FFT),
  fused LSD + SISpec + log-SISpec epilogue, SSIM kernel, finalisation.
* ``wav_to_spectrogram`` -> ``ssr_stft``;  ``lsd`` / ``sispec`` / ``ssim`` on tensors ->
  ``ssr_spectrogram_metrics``.

Extras (keyword-only, not in the reference): ``precision`` ("f64" parity mode / "f32"), ``device``,
``n_fft`` / ``hop_length`` overrides, and ``evaluation_batch`` for lists of pairs.
"""
import fractions
import functools
import math

import numpy as np
import torch

from . import backend as B
from . import mel as M

EPS = 1e-12
_KEYS = ("lsd", "log_sispec", "sispec", "ssim")
_WAVE_NAMES = ("snr", "si_sdr", "seg_snr")        # SSR_WAVE_SNR, SSR_WAVE_SI_SDR, SSR_WAVE_SEG_SNR: bits 0, 1, 2
_MEL_NAMES = ("mel_lsd", "mel_l1", "mcd")         # SSR_MEL_LSD, SSR_MEL_L1, SSR_MEL_MCD: bits 0, 1, 2
_MEL_DTW_NAMES = ("mcd_dtw", "dtw_dev", "dtw_len")      # the columns of ssr_pair_mel_dtw
_QUALITY_NAMES = ("llr", "cep_dist", "wss", "fwseg_snr")   # SSR_QUAL_LLR, SSR_QUAL_CEP, SSR_QUAL_WSS, SSR_QUAL_FWSEG: bits 0 .. 3
_PITCH_NAMES = ("f0_rmse", "f0_corr", "gpe", "vde", "ffe")  # SSR_PITCH_F0_RMSE, _F0_CORR, _GPE, _VDE, _FFE: bits 0 .. 4
_PHASE_NAMES = ("phase_ip", "phase_gd", "phase_iaf")       # SSR_PHASE_IP, SSR_PHASE_GD, SSR_PHASE_IAF: bits 0, 1, 2
_MRSTFT_NAMES = ("mrstft_sc", "mrstft_mag", "mrstft")     # the means over the resolutions of ssr_mrstft_metrics, and their sum
_BSS_NAMES = ("sdr", "sdr_lag")                           # the columns of ssr_bss_sdr
_COH_NAMES = ("msc", "coh_sdr", "coh_bw")                 # a band's columns of ssr_coherence (coh_bw: coh_bins in Hz)
_COH_HF_NAMES = ("msc_hf", "coh_sdr_hf")                  # the same above a split frequency
_LOUD_NAMES = ("lufs", "lra", "lufs_m_max", "lufs_s_max", "peak_db", "true_peak_db")     # the columns of ssr_loudness
_LOUD_DIFF_NAMES = ("lufs_diff", "lra_diff", "true_peak_diff")                           # estimate minus target
_SPEC_NAMES = ("bw_hz", "edge_hz", "centroid_hz", "hf_db")                                # of one signal (ssr_spectrum)
_SPEC_PAIR_NAMES = ("bw_diff", "edge_diff", "centroid_diff", "hf_diff", "ltas_dist", "ltas_max")     # estimate against target
_NSIM_NAMES = ("nsim", "nsim_hf", "nsim_lf")                                              # the columns of ssr_auditory
_MOD_NAMES = ("srmr", "srmr_diff", "mod_dist", "mod_dist_hf", "mod_dist_lf")              # the estimate's srmr, then ssr_modulation's pair columns
_CSII_NAMES = ("csii", "csii_low", "csii_mid", "csii_high", "i3", "csii_hf", "csii_mid_hf")      # columns 0 .. 5 and 7 of ssr_csii
_CSII_COLUMNS = (0, 1, 2, 3, 4, 5, 7)
_ALIGN_NAMES = ("delay", "delay_frac", "align_corr", "align_edge")                        # the columns of ssr_align
_CSII_COUNT_NAMES = ("n_segments", "n_low", "n_mid", "n_high")                            # columns 9 .. 12
_NMR_NAMES = ("nmr", "nmr_seg", "rdf", "nmr_hf", "nmr_lf")                                # columns 0 .. 4 of ssr_nmr (column 5: frames)


def which_mask(which, names):
    """"all", one of `names` or a tuple / list of them -> the C ABI's bit mask (bit j asks for names[j])."""
    asked = names if (isinstance(which, str) and which == "all") else ((which,) if isinstance(which, str) else which)
    if not isinstance(asked, (tuple, list)) or not asked or not all(isinstance(m, str) and m in names for m in asked):
        raise ValueError("which must be 'all', one of %s or a tuple of them" % (names,))
    return sum(1 << names.index(m) for m in set(asked))


def rows_dicts(vals, mask, names, packed=True):
    """Result rows -> one {name: float} per row with the names `mask` asks for.  packed: a row holds one column per name asked
    for, in bit order; otherwise one column per name of `names` (NaN where not asked)."""
    cols = [(j, m) for j, m in enumerate(names) if mask & (1 << j)]
    return [{m: float(row[c if packed else j]) for c, (j, m) in enumerate(cols)} for row in vals]


def _item_major(by_key, n, K):
    """by_key[k][i] -> the flat list with the K entries of item i next to each other."""
    return [by_key[k][i] for i in range(n) for k in range(K)]


def _flat_pairs(ests_by_key, targets):
    """K lists of n estimates, n targets -> (n * K estimates, n * K targets, n, K), the K pairs of a target next to each other."""
    K, n = len(ests_by_key), len(targets)
    return _item_major(ests_by_key, n, K), [t for t in targets for _ in range(K)], n, K


def _regroup(flat, n, K, deferred):
    """flat: a function that returns n * K item-major rows -> the n lists of K (deferred: the function that returns them)."""
    def finish():
        rows = flat()
        return [rows[i * K:(i + 1) * K] for i in range(n)]
    return finish if deferred else finish()


def _by_dtype(j, wide):
    """The keyed drivers' group of a family whose estimates of one dtype share a call."""
    return wide


def _shared_targets(targets):
    """-> (the distinct target objects, the index of every entry among them): a target object passed for several pairs (at one
    length) is analysed once."""
    tgts, index, seen = [], [], {}
    for t in targets:
        key = (id(t), int(t.shape[0]))
        if key not in seen:
            seen[key] = len(tgts)
            tgts.append(t)
        index.append(seen[key])
    return tgts, index


def _names_asked(names, allowed):
    """The result keys asked for, in result order, or ValueError: None = all of `allowed`, or a non-empty tuple / list of them."""
    if names is None:
        return allowed
    if not isinstance(names, (tuple, list)) or not names or not all(isinstance(k, str) and k in allowed for k in names):
        raise ValueError("names must be None or a tuple of %s" % (allowed,))
    return tuple(k for k in allowed if k in names)


def _split_indices(split, n, to_index):
    """The split index of n pairs: split = None (no split: -1 for every pair), one frequency in Hz for every pair, or a list of one
    per pair (None: -1 for that pair).  to_index(the frequency as a float) is the family's own mapping."""
    if split is None:
        return [-1] * n
    splits = split if isinstance(split, list) else [split] * n
    if len(splits) != n:
        raise ValueError("one split frequency per pair")
    message = "a split frequency is a finite number >= 0 in Hz"
    return [-1 if s is None else to_index(float(B._number_in(s, 0.0, math.inf, False, True, message))) for s in splits]


def _tile_key_splits(split_hz, K, n):
    """The split of a *_multi call for its n * K item-major pairs: a list holds one frequency per key and is tiled n times; None
    or one frequency is for every pair as it is."""
    if not isinstance(split_hz, list):
        return split_hz
    if len(split_hz) != K:
        raise ValueError("one split frequency per key")
    return list(split_hz) * n


def _check_1d(signals):
    """ValueError for a signal in memory that is not 1-D (a path is read later)."""
    for w in signals:
        if not isinstance(w, str) and len(w.shape) != 1:
            raise ValueError("expected a 1-D signal, got shape %s" % (tuple(w.shape),))


def _group_by_dtype(signals):
    """The positions of the float32 and of the float64 signals, the group met first in front: one library call per dtype."""
    groups = {}
    for i, w in enumerate(signals):
        groups.setdefault(bool(B._is_f64(w)), []).append(i)
    return list(groups.values())


class AudioMetrics:
    def __init__(self, rate, *, precision="f64", device=None, n_fft=None, hop_length=None):
        self.rate = rate
        # integer table of ssr_eval/metrics.py:18-19 (bit-exact): 48000 -> (2229, 480), 44100 -> (2048, 441)
        self.hop_length = int(rate / 100) if hop_length is None else int(hop_length)
        self.n_fft = int(2048 / (44100 / rate)) if n_fft is None else int(n_fft)
        self.precision = precision
        self._device = device

    # ---- plumbing
    def _plan(self):
        return B.get_plan(self.n_fft, self.hop_length, self.precision, self._device)

    def read(self, est, target):
        """ssr_eval/metrics.py:21-24 (file decode + resample is host I/O)."""
        from .io import load_audio
        return load_audio(est, self.rate), load_audio(target, self.rate)

    # ---- reference API
    def wav_to_spectrogram(self, wav, *, keep_on_device=False):
        """[n] waveform -> magnitude spectrogram tensor [1, 1, T, F] float32 (metrics.py:26-30)."""
        plan = self._plan()
        sp = B.stft(plan, [np.asarray(wav) if not isinstance(wav, torch.Tensor) else wav])[0][None, None]
        return sp if keep_on_device else sp.cpu()

    def _prepare_pair(self, est, target, resident=False):
        # resident (internal callers): the signals may be device tensors the previous stage left in HBM, next to ndarrays
        if type(est) != type(target) and not (resident and not isinstance(est, str) and not isinstance(target, str)):
            raise ValueError("The input value should either both be numpy array or strings")
        if isinstance(est, str):
            est, target = self.read(est, target)
        if est.shape == target.shape and len(est.shape) == 1:        # the common case (every key of a file): nothing to check or cut
            return est, target
        assert len(est.shape) == 1 and len(target.shape) == 1, (
            "The input numpy array shape should be [samples,]. Got input shape %s and %s. " % (est.shape, target.shape))
        assert abs(target.shape[0] - est.shape[0]) < 100, (
            "Error: Shape mismatch between target and estimation %s and %s" % (str(target.shape), str(est.shape)))
        m = min(target.shape[0], est.shape[0])           # metrics.py:89-90
        return est[:m], target[:m]

    def evaluation(self, est, target, file=None):
        """{lsd, log_sispec, sispec, ssim} for one (estimate, target) pair (metrics.py:51-107)."""
        return self.evaluation_batch([est], [target])[0]

    def evaluation_batch(self, ests, targets, mask=B.M_ALL, resident=False, deferred=False):
        """The same four metrics for lists of pairs, one fused launch sequence for the whole batch.
        deferred: the launches are queued and a function is returned that waits for the values and builds the list (the caller
        queues its next batch in between)."""
        pairs = [self._prepare_pair(e, t, resident) for e, t in zip(ests, targets)]
        # A float64 estimate (IIR-degraded input passed through a testee, eval.py:138-150) makes the reference's est
        # spectrogram - and with it every metric - float64; float64 targets (arrays decoded as float64 by the caller)
        # likewise.  Pairs are grouped by dtype combination and each group runs its own launch sequence:
        # 0 = both float32, 1 = float64 estimate / float32 target, 2 = float64 target (estimate widened if needed).
        kind = [2 if B._is_f64(p[1]) else (1 if B._is_f64(p[0]) else 0) for p in pairs]
        groups = []
        for want in (0, 1, 2):
            idx = [i for i, f in enumerate(kind) if f == want]
            if idx:
                groups.append((want, idx, B.pair_metrics(self._plan(), [pairs[i][0] for i in idx], [pairs[i][1] for i in idx], mask,
                                                         deferred=True)))

        def finish():
            out = [None] * len(pairs)
            for want, idx, pending in groups:
                for i, row in zip(idx, pending()):
                    # float32 pairs: lsd / sispec are float32 tensors in the reference (float() of fp32), ssim float64
                    out[i] = self._row_dict(row, mask, bool(want))
            return out
        return finish if deferred else finish()

    @staticmethod
    def _row_dict(row, mask, wide):
        d = {}
        for k, v in zip(_KEYS, row):
            if not np.isnan(v) or (mask & (1 << _KEYS.index(k))):
                d[k] = float(v) if (k == "ssim" or wide) else float(np.float32(v))
        return d

    def evaluation_multi(self, ests_by_key, targets, mask=B.M_ALL, resident=False, deferred=False):
        """K estimates per target (the degradation keys of a file, ssr_eval/eval.py:136-154): ests_by_key = K lists of n
        waveforms, targets = n waveforms -> n lists of K dicts.  Every target is transformed once per GROUP of keys: the float32 keys
        of the files (FFT low-pass, subsampling, mp3) through one ssr_pair_metrics_multi launch sequence, the float64 keys (every IIR
        design: sosfiltfilt returns float64 and the reference keeps it, eval.py:138-150) through one ssr_pair_metrics_multi_est64.
        Needs float32 targets and, per item, one truncated length for all keys (metrics.py:89-90) - otherwise (and for a group of a
        single key) the pairs go through evaluation_batch.  deferred: as evaluation_batch."""
        K, n = len(ests_by_key), len(targets)
        pairs = [[self._prepare_pair(ests_by_key[k][i], targets[i], resident) for i in range(n)] for k in range(K)]
        same_len = all(len({pairs[k][i][0].shape[0] for k in range(K)}) == 1 for i in range(n))
        tgt32 = not any(B._is_f64(pairs[k][i][1]) for k in range(K) for i in range(n))
        # a key is float64 / float32 if ALL its estimates are; a key with both kinds sends everything through evaluation_batch
        kinds = [{bool(B._is_f64(pairs[k][i][0])) for i in range(n)} for k in range(K)]
        if K < 2 or n == 0 or not same_len or not tgt32 or any(len(kd) != 1 for kd in kinds):
            ests, tgts_, _, _ = _flat_pairs(ests_by_key, targets)
            return _regroup(self.evaluation_batch(ests, tgts_, mask, resident, deferred=True), n, K, deferred)
        tgts = [pairs[0][i][1] for i in range(n)]

        def one_key(k):                                              # a group of ONE key: the plain pair path -> [n][1] dicts
            flat = self.evaluation_batch([pairs[k][i][0] for i in range(n)], tgts, mask, True, deferred=True)
            return lambda: [[row] for row in flat()]

        def many_keys(keys, wide):                                   # one multi launch sequence -> [n][len(keys)] dicts
            pending = B.pair_metrics_multi(self._plan(), [[pairs[k][i][0] for i in range(n)] for k in keys], tgts, mask, deferred=True)

            def collect():
                vals = pending()
                return [[self._row_dict(vals[i, j], mask, wide) for j in range(len(keys))] for i in range(n)]
            return collect

        parts = []                                                   # (key indices, collector)
        for wide in (False, True):
            keys = [k for k in range(K) if next(iter(kinds[k])) == wide]
            if keys:
                parts.append((keys, one_key(keys[0]) if len(keys) == 1 else many_keys(keys, wide)))

        def finish():
            out = [[None] * K for _ in range(n)]
            for keys, collect in parts:
                rows = collect()
                for i in range(n):
                    for j, k in enumerate(keys):
                        out[i][k] = rows[i][j]
            return out
        return finish if deferred else finish()

    # ---- band-split LSD (not in the reference): lsd() over the bins on either side of a degradation's cutoff
    def split_bin(self, cutoff_hz):
        """c = int(F * (cutoff_hz / (rate / 2))), F = n_fft // 2 + 1: lowpass.cut_bin's expression at this rate's STFT size."""
        return int((self.n_fft // 2 + 1) * (cutoff_hz / (self.rate / 2)))

    def _split_edges(self, cutoff_hz):
        """-> (edges, (lf band index or None, hf band index or None)); None for no cutoff: both NaN.  A side that comes out empty
        (c <= 0 or c >= F) is NaN and the other side is the whole band."""
        F = self.n_fft // 2 + 1
        if cutoff_hz is None:
            return None, (None, None)
        c = self.split_bin(cutoff_hz)
        if c <= 0:
            return (0, F), (None, 0)
        if c >= F:
            return (0, F), (0, None)
        return (0, c, F), (0, 1)

    @staticmethod
    def _split_dict(vals, which):
        return {name: (float(vals[j]) if j is not None else float("nan")) for name, j in zip(("lsd_lf", "lsd_hf"), which)}

    def lsd_bands(self, est, target, edges):
        """[B, C, T, F] magnitude tensors x2 -> [B, C, n_bands] float64: lsd() over the bins [edges[j], edges[j + 1]) of each band.
        edges: n_bands + 1 strictly ascending bins in [0, F] for every image, or [B, C, n_bands + 1] per image."""
        if est.shape != target.shape or est.dim() != 4:
            raise ValueError("expected two [B, C, T, F] tensors of one shape, got %s and %s" % (tuple(est.shape), tuple(target.shape)))
        Bn, Cn, T, F = (int(v) for v in est.shape)
        e = np.asarray(edges, dtype=np.int64)
        e = np.broadcast_to(e, (Bn, Cn, e.shape[-1])) if e.ndim == 1 else e
        if e.shape[:2] != (Bn, Cn):
            raise ValueError("edges must be [n_bands + 1] or [B, C, n_bands + 1]")
        v = B.spectrogram_lsd_bands(est.reshape(Bn * Cn, T, F), target.reshape(Bn * Cn, T, F), e.reshape(Bn * Cn, -1))
        return v.to(est.device).reshape(Bn, Cn, -1)

    # The image families (band-split LSD, the mel distances, mel_dtw) hold K + 1 magnitude images per item: estimates that may share
    # a launch sequence form a group.  group(j, float64 estimates) -> the group of pair / key j, None: no call, the entry is
    # `default`; run(est_lists, tgt_list, members) -> Pending of [n, K, cols] for the group's members; to_dict(row, j) -> the dict.
    def _keyed_batch(self, group, run, to_dict, default, ests, targets, resident, deferred):
        """Lists of pairs with evaluation_batch's input rules: one call of one key per group of pairs."""
        pairs = [self._prepare_pair(e, t, resident) for e, t in zip(ests, targets)]
        groups = {}
        for i, (e, _) in enumerate(pairs):
            g = group(i, bool(B._is_f64(e)))
            if g is not None:
                groups.setdefault(g, []).append(i)
        pending = [(idx, run([[pairs[i][0] for i in idx]], [pairs[i][1] for i in idx], idx)) for idx in groups.values()]

        def finish():
            out = [default if default is None else dict(default) for _ in pairs]
            for idx, p in pending:
                vals = p()
                for r, i in enumerate(idx):
                    out[i] = to_dict(vals[r, 0], i)
            return out
        return finish if deferred else finish()

    def _keyed_multi(self, group, run, to_dict, default, batch, ests_by_key, targets, resident, deferred):
        """K estimates per target: the keys of a group share one multi-key launch sequence (the target transformed once per chunk of
        keys); lengths that differ between keys, or a key with both dtypes, send the pairs through batch(ests, targets) (deferred,
        resident)."""
        K, n = len(ests_by_key), len(targets)
        pairs = [[self._prepare_pair(ests_by_key[k][i], targets[i], resident) for i in range(n)] for k in range(K)]
        same_len = all(len({pairs[k][i][0].shape[0] for k in range(K)}) == 1 for i in range(n))
        kinds = [{bool(B._is_f64(pairs[k][i][0])) for i in range(n)} for k in range(K)]
        if n == 0 or not same_len or any(len(kd) != 1 for kd in kinds):
            flat = _item_major(pairs, n, K)
            return _regroup(batch([e for e, _ in flat], [t for _, t in flat]), n, K, deferred)
        tgts = [pairs[0][i][1] for i in range(n)]
        groups = {}
        for k in range(K):
            g = group(k, next(iter(kinds[k])))
            if g is not None:
                groups.setdefault(g, []).append(k)
        pending = [(keys, run([[pairs[k][i][0] for i in range(n)] for k in keys], tgts, keys)) for keys in groups.values()]

        def finish():
            out = [[default if default is None else dict(default) for _ in range(K)] for _ in range(n)]
            for keys, p in pending:
                vals = p()
                for i in range(n):
                    for j, k in enumerate(keys):
                        out[i][k] = to_dict(vals[i, j], k)
            return out
        return finish if deferred else finish()

    def lsd_split(self, est, target, cutoff_hz):
        """{'lsd_lf', 'lsd_hf'} of one (estimate, target) pair split at cutoff_hz."""
        return self.lsd_split_batch([est], [target], [cutoff_hz])[0]

    def _split_family(self, cutoffs_hz):
        """-> (group, to_dict, default) of the keyed drivers, and the band edges per cutoff: estimates of one dtype and band count
        share a call, a cutoff of None has none."""
        split = [self._split_edges(c) for c in cutoffs_hz]
        return (lambda j, wide: None if split[j][0] is None else (wide, len(split[j][0]) - 1),
                lambda row, j: self._split_dict(row, split[j][1]), self._split_dict((), (None, None))), [edges for edges, _ in split]

    def lsd_split_batch(self, ests, targets, cutoffs_hz, resident=False, deferred=False):
        """lsd_split for lists of pairs (the input rules of evaluation_batch: metrics.py:89-90 truncation, float64 estimates kept
        float64; float32 targets).  cutoffs_hz: one value for every pair, or one per pair (None: both values NaN)."""
        n = min(len(ests), len(targets))
        cuts = list(cutoffs_hz) if isinstance(cutoffs_hz, (list, tuple)) else [cutoffs_hz] * n
        if len(cuts) != n:
            raise ValueError("one cutoff per pair")
        (group, to_dict, default), edges = self._split_family(cuts)
        return self._keyed_batch(group, lambda e, t, idx: B.pair_lsd_bands(self._plan(), e, t, [[edges[i] for i in idx]], deferred=True),
                                 to_dict, default, ests, targets, resident, deferred)

    def lsd_split_multi(self, ests_by_key, targets, cutoffs_hz, resident=False, deferred=False, keys_per_chunk=None):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms, cutoffs_hz = one
        split frequency per key (None: NaN) -> n lists of K {'lsd_lf', 'lsd_hf'}.  Keys with the same estimate dtype and band count
        share one multi-key launch sequence (the target transformed once per chunk of keys); otherwise - lengths that differ between
        keys, a key with both dtypes - the pairs go through lsd_split_batch."""
        n = len(targets)
        if len(cutoffs_hz) != len(ests_by_key):
            raise ValueError("one cutoff per key")
        (group, to_dict, default), edges = self._split_family(cutoffs_hz)
        return self._keyed_multi(group, lambda e, t, keys: B.pair_lsd_bands(self._plan(), e, t, [[edges[k]] * n for k in keys], deferred=True,
                                                                           keys_per_chunk=keys_per_chunk),
                                 to_dict, default, lambda e, t: self.lsd_split_batch(e, t, list(cutoffs_hz) * n, True, deferred=True),
                                 ests_by_key, targets, resident, deferred)

    # ---- the per-pair metric families (not in the reference): estimate e against target index[e].  A family is two functions -
    # call(tgts, ests, index) queues its backend call and returns the Pending, dicts(rows) names the columns - and the drivers
    # below are the same for all of them
    def _pairs(self, family, ests, targets, resident, deferred, by_dtype, per_pair=False):
        """Lists of pairs with evaluation_batch's input rules (metrics.py:89-90 truncation; float32 or float64 signals).  by_dtype:
        one call per (target dtype, estimate dtype) group - the family reads the signals in their own dtype; otherwise one call
        (it widens them itself).  A target object passed for several pairs of a call appears once in it.  per_pair: the family's
        arguments hold one value per pair - call() also gets the positions of its pairs in the lists."""
        call, dicts = family
        pairs = [self._prepare_pair(e, t, resident) for e, t in zip(ests, targets)]
        groups = {}
        for i, (e, t) in enumerate(pairs):
            groups.setdefault((bool(B._is_f64(t)), bool(B._is_f64(e))) if by_dtype else None, []).append(i)
        pending = []
        for idx in groups.values():
            tgts, index = _shared_targets([pairs[i][1] for i in idx])
            pending.append((idx, call(tgts, [pairs[i][0] for i in idx], index, *((idx,) if per_pair else ()))))

        def finish():
            out = [None] * len(pairs)
            for idx, p in pending:
                for i, d in zip(idx, dicts(p())):
                    out[i] = d
            return out
        return finish if deferred else finish()

    def _multi_flat(self, family, ests_by_key, targets, resident, deferred):
        """K estimates per target, as evaluation_multi, through _pairs: the K pairs of a target next to each other in one call per
        dtype group."""
        ests, tgts, n, K = _flat_pairs(ests_by_key, targets)
        return _regroup(self._pairs(family, ests, tgts, resident, True, by_dtype=True), n, K, deferred)

    def _multi_shared(self, family, ests_by_key, targets, resident, deferred):
        """K estimates per target, as evaluation_multi, in ONE call that names each target once for its K estimates."""
        call, dicts = family
        K, n = len(ests_by_key), len(targets)
        pairs = [self._prepare_pair(ests_by_key[k][i], targets[i], resident) for i in range(n) for k in range(K)]
        ests, tgts = [e for e, _ in pairs], [t for _, t in pairs]
        if not all(len({t.shape[0] for t in tgts[i * K:(i + 1) * K]}) == 1 for i in range(n)):
            # truncation cut a target differently per key: one target copy per length
            return _regroup(self._pairs(family, ests, tgts, True, True, by_dtype=False), n, K, deferred)
        pending = call(tgts[::K] if K else [], ests, np.repeat(np.arange(n), K))
        return _regroup(lambda: dicts(pending()), n, K, deferred)

    # ---- STOI / ESTOI: intelligibility as pystoi computes it, at self.rate
    @staticmethod
    def _stoi_which(extended):
        if extended is False or extended is True:
            return B._lib.ESTOI if extended else B._lib.STOI
        if isinstance(extended, str) and extended == "both":
            return B._lib.STOI_BOTH
        raise ValueError("extended must be False (STOI), True (ESTOI) or 'both'")

    def _stoi_family(self, extended):
        which = self._stoi_which(extended)
        names = {B._lib.STOI: ("stoi",), B._lib.ESTOI: ("estoi",), B._lib.STOI_BOTH: ("stoi", "estoi")}[which]
        return (lambda tgts, ests, index: B.stoi(tgts, ests, index, self.rate, which, self._device, deferred=True),
                lambda vals: [{k: float(v) for k, v in zip(names, row)} for row in vals])

    def stoi(self, est, target, extended=False):
        """STOI (extended=False), ESTOI (True) of one (estimate, target) pair at self.rate; 'both': {'stoi', 'estoi'}."""
        d = self.stoi_batch([est], [target], extended)[0]
        return d if extended == "both" else next(iter(d.values()))

    def stoi_batch(self, ests, targets, extended=False, resident=False, deferred=False):
        """{'stoi'} / {'estoi'} / both for lists of pairs, with evaluation_batch's input rules (metrics.py:89-90 truncation; float32
        or float64 signals - resampled to 10 kHz in float64 either way).  A target object passed for several pairs is analysed once.
        deferred: as evaluation_batch."""
        return self._pairs(self._stoi_family(extended), ests, targets, resident, deferred, by_dtype=False)

    def stoi_multi(self, ests_by_key, targets, extended=False, resident=False, deferred=False):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> n lists of K
        dicts.  Each target is resampled, masked and transformed once for its K estimates."""
        return self._multi_shared(self._stoi_family(extended), ests_by_key, targets, resident, deferred)

    # ---- waveform metrics: SNR, SI-SDR, segmental SNR, at self.rate
    _wave_which = staticmethod(functools.partial(which_mask, names=_WAVE_NAMES))
    _wave_dicts = staticmethod(functools.partial(rows_dicts, names=_WAVE_NAMES))

    def _wave_family(self, which):
        mask = self._wave_which(which)
        return (lambda tgts, ests, index: B.wave_metrics(tgts, ests, index, self.rate, mask, self._device, deferred=True),
                lambda vals: self._wave_dicts(vals, mask))

    def waveform(self, est, target, which="all"):
        """{'snr', 'si_sdr', 'seg_snr'} (or the subset `which` names) of one (estimate, target) pair, in dB."""
        return self.waveform_batch([est], [target], which)[0]

    def snr(self, est, target):
        return self.waveform(est, target, "snr")["snr"]

    def si_sdr(self, est, target):
        return self.waveform(est, target, "si_sdr")["si_sdr"]

    def seg_snr(self, est, target):
        return self.waveform(est, target, "seg_snr")["seg_snr"]

    def waveform_batch(self, ests, targets, which="all", resident=False, deferred=False):
        """waveform() for lists of pairs, with stoi_batch's input rules (metrics.py:89-90 truncation; float32 or float64 signals, read
        in their own dtype: one ssr_wave_metrics call per (target dtype, estimate dtype) group).  A target object passed for several
        pairs is read once for all of them.  deferred: as evaluation_batch."""
        return self._pairs(self._wave_family(which), ests, targets, resident, deferred, by_dtype=True)

    def waveform_multi(self, ests_by_key, targets, which="all", resident=False, deferred=False):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> n lists of K
        dicts.  The K pairs of a target sit next to each other in one call: each tile of the target is read once for all of them."""
        return self._multi_flat(self._wave_family(which), ests_by_key, targets, resident, deferred)

    # ---- objective quality measures: Loizou's LLR, LPC cepstral distance, WSS and fwSNRseg at self.rate.  WSS and
    # fwSNRseg look at Loizou's 25 critical bands only, 50 Hz to about 3.9 kHz at every rate: they score the band a model was
    # given, not the band it restored.
    _quality_which = staticmethod(functools.partial(which_mask, names=_QUALITY_NAMES))
    _quality_dicts = staticmethod(functools.partial(rows_dicts, names=_QUALITY_NAMES))

    @staticmethod
    def _quality_order(lpc_order):
        """None (10 below 10 kHz, else 16) or an int in [1, 32] -> the C ABI's lpc_order (0 = default)."""
        if lpc_order is None:
            return 0
        if isinstance(lpc_order, bool) or not isinstance(lpc_order, (int, np.integer)) or not 1 <= int(lpc_order) <= 32:
            raise ValueError("lpc_order must be None or an integer in [1, 32]")
        return int(lpc_order)

    def _quality_family(self, which, lpc_order):
        mask, order = self._quality_which(which), self._quality_order(lpc_order)
        if not 8000 <= self.rate <= 48000:
            raise ValueError("the quality measures need 8000 <= rate <= 48000")
        return (lambda tgts, ests, index: B.quality_metrics(tgts, ests, index, self.rate, mask, order, self._device, deferred=True),
                lambda vals: self._quality_dicts(vals, mask))

    def quality(self, est, target, which="all", lpc_order=None):
        """{'llr', 'cep_dist', 'wss', 'fwseg_snr'} (or the subset `which` names) of one (estimate, target) pair."""
        return self.quality_batch([est], [target], which, lpc_order)[0]

    def llr(self, est, target, lpc_order=None):
        return self.quality(est, target, "llr", lpc_order)["llr"]

    def cep_dist(self, est, target, lpc_order=None):
        return self.quality(est, target, "cep_dist", lpc_order)["cep_dist"]

    def wss(self, est, target):
        return self.quality(est, target, "wss")["wss"]

    def fwseg_snr(self, est, target):
        return self.quality(est, target, "fwseg_snr")["fwseg_snr"]

    def quality_batch(self, ests, targets, which="all", lpc_order=None, resident=False, deferred=False):
        """quality() for lists of pairs, with waveform_batch's input rules (metrics.py:89-90 truncation; float32 or float64 signals,
        read in their own dtype: one ssr_quality_metrics call per (target dtype, estimate dtype) group).  A target object passed for
        several pairs is analysed once for all of them.  deferred: as evaluation_batch."""
        return self._pairs(self._quality_family(which, lpc_order), ests, targets, resident, deferred, by_dtype=True)

    def quality_multi(self, ests_by_key, targets, which="all", lpc_order=None, resident=False, deferred=False):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> n lists of K
        dicts.  The K pairs of a target sit next to each other in one call: the target's frames are analysed once for all of them."""
        return self._multi_flat(self._quality_family(which, lpc_order), ests_by_key, targets, resident, deferred)

    # ---- pitch: YIN F0 tracks on 16 kHz float64 signals, 10 ms frames, and the pair statistics F0 RMSE (cents), F0
    # correlation, GPE, VDE and FFE of an estimate's track against its target's
    _pitch_which = staticmethod(functools.partial(which_mask, names=_PITCH_NAMES))
    _pitch_dicts = staticmethod(functools.partial(rows_dicts, names=_PITCH_NAMES))

    @staticmethod
    def _pitch_range(fmin, fmax):
        """(fmin, fmax) in Hz as floats, or ValueError (40 <= fmin < fmax <= 1000, at least three lags)."""
        for v in (fmin, fmax):
            if not B._is_number(v):
                raise ValueError("fmin and fmax must be numbers (Hz)")
        return B.check_pitch_range(fmin, fmax)

    def _pitch_rate(self):
        if not 8000 <= self.rate <= 48000:
            raise ValueError("the pitch metrics need 8000 <= rate <= 48000")

    def _pitch_family(self, which, fmin, fmax):
        mask = self._pitch_which(which)
        fmin, fmax = self._pitch_range(fmin, fmax)
        self._pitch_rate()
        return (lambda tgts, ests, index: B.pitch_metrics(tgts, ests, index, self.rate, mask, fmin, fmax, self._device, deferred=True),
                lambda vals: self._pitch_dicts(vals, mask))

    def f0(self, wav, fmin=50.0, fmax=500.0):
        """YIN F0 track of one waveform at self.rate: {'f0' (Hz, NaN where the frame is digitally silent), 'voiced' (bool),
        'aperiodicity'}, one value per 10 ms frame of the signal resampled to 16 kHz."""
        fmin, fmax = self._pitch_range(fmin, fmax)
        self._pitch_rate()
        f0, voiced, ap, _ = B.f0_track([wav], self.rate, fmin, fmax, self._device)[0]
        return {"f0": f0, "voiced": voiced, "aperiodicity": ap}

    def pitch(self, est, target, which="all", fmin=50.0, fmax=500.0):
        """{'f0_rmse', 'f0_corr', 'gpe', 'vde', 'ffe'} (or the subset `which` names) of one (estimate, target) pair."""
        return self.pitch_batch([est], [target], which, fmin, fmax)[0]

    def pitch_batch(self, ests, targets, which="all", fmin=50.0, fmax=500.0, resident=False, deferred=False):
        """pitch() for lists of pairs, with stoi_batch's input rules (metrics.py:89-90 truncation; float32 or float64 signals -
        resampled to 16 kHz in float64 either way).  A target object passed for several pairs is tracked once.  deferred: as
        evaluation_batch."""
        return self._pairs(self._pitch_family(which, fmin, fmax), ests, targets, resident, deferred, by_dtype=False)

    def pitch_multi(self, ests_by_key, targets, which="all", fmin=50.0, fmax=500.0, resident=False, deferred=False):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> n lists of K
        dicts.  Each target is resampled and tracked once for its K estimates."""
        return self._multi_shared(self._pitch_family(which, fmin, fmax), ests_by_key, targets, resident, deferred)

    # ---- anti-wrapping phase distances: instantaneous phase, group delay and instantaneous angular frequency of the
    # estimate's spectrum against the target's, in radians (0 .. pi), on centred n_fft-point Hann frames of the signals at self.rate
    _phase_which = staticmethod(functools.partial(which_mask, names=_PHASE_NAMES))
    _phase_dicts = staticmethod(functools.partial(rows_dicts, names=_PHASE_NAMES))

    @staticmethod
    def _phase_bins(rate, n_fft, band):
        """band None -> None (every bin); (lo_hz, hi_hz) -> the bins (ceil(lo n_fft / rate), floor(hi n_fft / rate)) clamped to
        [0, n_fft // 2]; ValueError where that leaves no bin."""
        if band is None:
            return None
        ok = isinstance(band, (tuple, list)) and len(band) == 2 and all(B._is_number(v) and np.isfinite(v) for v in band)
        if not ok:
            raise ValueError("band must be None or (lo_hz, hi_hz)")
        lo, hi = (fractions.Fraction(float(v)) * n_fft / fractions.Fraction(float(rate)) for v in band)
        k_lo, k_hi = max(0, math.ceil(lo)), min(n_fft // 2, math.floor(hi))
        if k_lo > k_hi:
            raise ValueError("band %r holds no bin of a %d-point transform at %r Hz" % (tuple(band), n_fft, rate))
        return k_lo, k_hi

    def _phase_family(self, which, n_fft, hop, band):
        mask = self._phase_which(which)
        n_fft, hop = B.check_phase_frames(n_fft, hop)
        bins = self._phase_bins(self.rate, n_fft, band)
        return (lambda tgts, ests, index: B.phase_metrics(tgts, ests, index, n_fft, hop, bins, mask, self._device, deferred=True),
                lambda vals: self._phase_dicts(vals, mask))

    def phase_distance(self, est, target, which="all", n_fft=1024, hop=None, band=None):
        """{'phase_ip', 'phase_gd', 'phase_iaf'} (or the subset `which` names) of one (estimate, target) pair, in radians.  n_fft:
        256, 512, 1024 or 2048; hop: None = n_fft // 4; band: None = every bin, or (lo_hz, hi_hz), the band scored."""
        return self.phase_distance_batch([est], [target], which, n_fft, hop, band)[0]

    def phase_distance_batch(self, ests, targets, which="all", n_fft=1024, hop=None, band=None, resident=False, deferred=False):
        """phase_distance() for lists of pairs, with waveform_batch's input rules (metrics.py:89-90 truncation; float32 or float64
        signals, read in their own dtype: one ssr_phase_metrics call per (target dtype, estimate dtype) group).  deferred: as
        evaluation_batch."""
        return self._pairs(self._phase_family(which, n_fft, hop, band), ests, targets, resident, deferred, by_dtype=True)

    def phase_distance_multi(self, ests_by_key, targets, which="all", n_fft=1024, hop=None, band=None, resident=False, deferred=False):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> n lists of K
        dicts.  The K pairs of a target sit next to each other in one call."""
        return self._multi_flat(self._phase_family(which, n_fft, hop, band), ests_by_key, targets, resident, deferred)

    # ---- multi-resolution STFT distance: Parallel WaveGAN's spectral convergence and log-magnitude distance, averaged
    # over several (n_fft, hop, win) - in SAMPLES whatever self.rate is; the defaults are the paper's, chosen at 24 kHz
    @staticmethod
    def _mrstft_bins(rate, resolutions, band):
        """band None -> None (every bin); (lo_hz, hi_hz) -> its bins per resolution by _phase_bins' rule; ValueError where a
        resolution has no bin inside."""
        return None if band is None else [AudioMetrics._phase_bins(rate, n_fft, band) for n_fft, _, _ in resolutions]

    def _mrstft_family(self, resolutions, band, eps, per_resolution):
        res = B.check_mrstft_resolutions(resolutions)
        eps = B.check_mrstft_eps(eps)
        bins = self._mrstft_bins(self.rate, res, band)

        def dicts(vals):
            out = []
            for row in vals:
                sc, mag = float(row[-1, 0]), float(row[-1, 1])
                d = {"mrstft_sc": sc, "mrstft_mag": mag, "mrstft": sc + mag}
                if per_resolution:
                    d["resolutions"] = [{"n_fft": n, "hop": h, "win": w, "sc": float(r[0]), "mag": float(r[1])}
                                        for (n, h, w), r in zip(res, row)]
                out.append(d)
            return out
        return (lambda tgts, ests, index: B.mrstft_metrics(tgts, ests, index, res, bins, eps, self._device, deferred=True)), dicts

    def mrstft(self, est, target, resolutions=None, band=None, eps=B.MRSTFT_EPS, per_resolution=False):
        """{'mrstft_sc', 'mrstft_mag', 'mrstft'} of one (estimate, target) pair: the spectral convergence and the mean absolute
        log-magnitude difference averaged over the resolutions, and their sum.  resolutions: None = ((1024, 120, 600),
        (2048, 240, 1200), (512, 50, 240)), or up to 8 (n_fft, hop, win) in samples with n_fft 256, 512, 1024 or 2048; band: None =
        every bin, or (lo_hz, hi_hz), mapped to bins per resolution as phase_distance maps it (ValueError where a resolution has no
        bin inside); eps: the floor of the squared magnitudes; per_resolution: also 'resolutions', a list of {'n_fft', 'hop', 'win',
        'sc', 'mag'}.  A resolution the signal is too short for (n <= n_fft / 2) is NaN, and so are the three values."""
        return self.mrstft_batch([est], [target], resolutions, band, eps, per_resolution)[0]

    def mrstft_batch(self, ests, targets, resolutions=None, band=None, eps=B.MRSTFT_EPS, per_resolution=False, resident=False,
                     deferred=False):
        """mrstft() for lists of pairs, with waveform_batch's input rules (metrics.py:89-90 truncation; float32 or float64 signals,
        read in their own dtype: one ssr_mrstft_metrics call per (target dtype, estimate dtype) group).  deferred: as
        evaluation_batch."""
        return self._pairs(self._mrstft_family(resolutions, band, eps, per_resolution), ests, targets, resident, deferred, by_dtype=True)

    def mrstft_multi(self, ests_by_key, targets, resolutions=None, band=None, eps=B.MRSTFT_EPS, per_resolution=False, resident=False,
                     deferred=False):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> n lists of K
        dicts.  The K pairs of a target sit next to each other in one call."""
        return self._multi_flat(self._mrstft_family(resolutions, band, eps, per_resolution), ests_by_key, targets, resident, deferred)

    # ---- filter-invariant SDR: BSS Eval's SDR, the estimate projected on the target's `taps` causal shifts - a delay or
    # a colouring of up to taps - 1 samples costs nothing, where snr and si_sdr collapse
    def _bss_family(self, taps, return_filter):
        taps = B.check_bss_taps(taps)

        def call(tgts, ests, index):
            got = B.bss_sdr(tgts, ests, index, taps, return_filter, self._device, deferred=True)
            return (lambda: (got[0](), got[1]())) if return_filter else (lambda: (got(), None))

        def dicts(vals):
            rows, filt = vals
            out = [{"sdr": float(r[0]), "sdr_lag": float(r[1])} for r in rows]
            if filt is not None:
                for d, c in zip(out, filt):
                    d["filter"] = np.array(c)
            return out
        return call, dicts

    def bss_sdr(self, est, target, taps=B.BSS_TAPS, return_filter=False):
        """{'sdr', 'sdr_lag'} of one (estimate, target) pair: BSS Eval's SDR in dB with a causal `taps`-tap FIR filter of the target
        as the allowed distortion (1 <= taps <= 512; 512 is mir_eval's), and the tap of the largest filter coefficient - the
        estimate's latency in samples.  return_filter: also 'filter', the float64 [taps] least-squares filter.  An empty or digitally
        silent target: NaN for both."""
        return self.bss_sdr_batch([est], [target], taps, return_filter)[0]

    def bss_sdr_batch(self, ests, targets, taps=B.BSS_TAPS, return_filter=False, resident=False, deferred=False):
        """bss_sdr() for lists of pairs, with waveform_batch's input rules (metrics.py:89-90 truncation; float32 or float64 signals,
        read in their own dtype: one ssr_bss_sdr call per (target dtype, estimate dtype) group).  A target object passed for several
        pairs next to each other is correlated with itself once.  deferred: as evaluation_batch."""
        return self._pairs(self._bss_family(taps, return_filter), ests, targets, resident, deferred, by_dtype=True)

    def bss_sdr_multi(self, ests_by_key, targets, taps=B.BSS_TAPS, return_filter=False, resident=False, deferred=False):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> n lists of K
        dicts.  The K pairs of a target sit next to each other in one call: K + 1 correlations per target, not 2 K."""
        return self._multi_flat(self._bss_family(taps, return_filter), ests_by_key, targets, resident, deferred)

    # ---- magnitude-squared coherence: is the estimate's band a linear function of the target's, or texture unrelated
    # to it?  Welch-averaged MSC per bin on n_fft-point periodic-Hann segments of the signals at self.rate (no padding); per band
    # its mean (msc), the coherence SDR in dB (coh_sdr) and the width of the coherent bins in Hz (coh_bw)
    def _coh_bands(self, n_fft, band, split, n):
        """The (lo, hi) bin pairs of n pairs: the band by _phase_bins' rule (None: every bin) and, with a split, the band from bin
        ceil(split n_fft / rate) to the band's hi.  split: None, one frequency in Hz for every pair, or a list of one per pair
        (None: no split for that pair - the empty band, NaN).  A split above the band leaves the empty band too."""
        lo, hi = self._phase_bins(self.rate, n_fft, band) or (0, n_fft // 2)
        if split is None:
            return [[(lo, hi)]] * n
        return [[(lo, hi), (k, hi) if 0 <= k <= hi else (1, 0)] for k in _split_indices(split, n, self._ceil_bin(n_fft))]

    def _ceil_bin(self, n_fft):
        """-> the function f in Hz -> ceil(f n_fft / rate), in exact arithmetic: the first bin at or above f."""
        return lambda f: math.ceil(fractions.Fraction(f) * n_fft / fractions.Fraction(float(self.rate)))

    def _coh_dicts(self, n_fft, split, spectrum):
        """(rows [n, n_bands, 3], spectra [n, n_fft / 2 + 1] or None) -> one dict per pair."""
        hz = float(self.rate) / n_fft

        def dicts(vals):
            rows, spec = vals
            out = []
            for i, r in enumerate(rows):
                d = {"msc": float(r[0, 0]), "coh_sdr": float(r[0, 1]), "coh_bw": float(r[0, 2]) * hz}
                if split:
                    d.update({"msc_hf": float(r[1, 0]), "coh_sdr_hf": float(r[1, 1])})
                if spectrum:
                    d["msc_spectrum"] = np.array(spec[i])
                out.append(d)
            return out
        return dicts

    def _coh_family(self, n_fft, hop, band, split, threshold, spectrum, n):
        n_fft, hop = B.check_coherence_frames(n_fft, hop)
        thr = B.check_coherence_threshold(threshold)
        bands = self._coh_bands(n_fft, band, split, n)

        def call(tgts, ests, index, idx):
            got = B.coherence_metrics(tgts, ests, index, n_fft, hop, [bands[i] for i in idx], thr, spectrum, self._device, deferred=True)
            return (lambda: (got[0](), got[1]())) if spectrum else (lambda: (got(), None))
        return call, self._coh_dicts(n_fft, split is not None, spectrum)

    def coherence(self, est, target, n_fft=1024, hop=None, band=None, split_hz=None, threshold=0.5, return_spectrum=False):
        """{'msc', 'coh_sdr', 'coh_bw'} of one (estimate, target) pair on `band`: the mean magnitude-squared coherence, the power of
        the estimate that is a linear function of the target over the power that is not, in dB, and the width in Hz of the bins whose
        coherence is >= threshold.  Invariant to any linear filtering of the estimate.  n_fft: 256, 512, 1024 or 2048; hop: None =
        n_fft // 2; band: None = every bin, or (lo_hz, hi_hz), mapped to bins as phase_distance maps it; split_hz: also 'msc_hf' and
        'coh_sdr_hf', on the bins from ceil(split_hz n_fft / rate) to the band's upper edge (NaN where that leaves none);
        return_spectrum: also 'msc_spectrum', the float64 [n_fft // 2 + 1] coherence per bin.  Fewer than two segments (n < n_fft +
        hop): NaN.  For unrelated signals the estimator's mean is about 1 / K at K segments, not 0."""
        return self.coherence_batch([est], [target], n_fft, hop, band, split_hz, threshold, return_spectrum)[0]

    def coherence_batch(self, ests, targets, n_fft=1024, hop=None, band=None, split_hz=None, threshold=0.5, return_spectrum=False,
                        resident=False, deferred=False):
        """coherence() for lists of pairs, with waveform_batch's input rules (metrics.py:89-90 truncation; float32 or float64 signals,
        read in their own dtype: one ssr_coherence call per (target dtype, estimate dtype) group).  split_hz: None, one frequency for
        every pair, or a list of one per pair (None: that pair's two _hf values are NaN).  deferred: as evaluation_batch."""
        n = min(len(ests), len(targets))
        return self._pairs(self._coh_family(n_fft, hop, band, split_hz, threshold, return_spectrum, n), ests, targets, resident, deferred,
                           by_dtype=True, per_pair=True)

    def coherence_multi(self, ests_by_key, targets, n_fft=1024, hop=None, band=None, split_hz=None, threshold=0.5, return_spectrum=False,
                        resident=False, deferred=False):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> n lists of K
        dicts.  split_hz: None, one frequency for every key, or a list of one per key (None: NaN).  The K pairs of a target sit next
        to each other in one call."""
        ests, tgts, n, K = _flat_pairs(ests_by_key, targets)
        split_hz = _tile_key_splits(split_hz, K, n)
        family = self._coh_family(n_fft, hop, band, split_hz, threshold, return_spectrum, n * K)
        return _regroup(self._pairs(family, ests, tgts, resident, True, by_dtype=True, per_pair=True), n, K, deferred)

    # ---- loudness: the EBU R128 meter quantities of ONE signal at self.rate - BS.1770-4 integrated loudness with gating,
    # the largest momentary and short-term loudness, the loudness range, the sample peak and the 4x oversampled peak - and, with a
    # target, the estimate's values minus the target's: is a difference between two testees content, or gain and clipping?
    @staticmethod
    def _loudness_names(names, with_target):
        """The result keys asked for, in result order, or ValueError: None = all, or a non-empty tuple / list of them."""
        return _names_asked(names, _LOUD_NAMES + (_LOUD_DIFF_NAMES if with_target else ()))

    def _loudness_signal(self, wav):
        if isinstance(wav, str):
            from .io import load_audio
            wav = load_audio(wav, self.rate)
        _check_1d([wav])
        return wav

    def loudness(self, est, target=None, return_blocks=False):
        """{'lufs', 'lra', 'lufs_m_max', 'lufs_s_max', 'peak_db', 'true_peak_db'} of one signal at self.rate (an integer in 8000 ..
        192000 Hz; mono, channel weight 1): the gated integrated loudness of ITU-R BS.1770-4 in LUFS, the loudness range of EBU Tech
        3342 in LU, the largest momentary (400 ms) and short-term (3 s) loudness, the sample peak in dBFS and the 4x oversampled
        peak in dBTP.  With a target also 'lufs_diff', 'lra_diff' and 'true_peak_diff', the estimate's value minus the target's.
        return_blocks: also 'blocks' (and 'target_blocks'), the K-weighted energies of the 100 ms sub-blocks.  A value whose block
        set is empty - shorter than 400 ms / 3 s, or nothing above -70 LUFS - is NaN, and so are both peaks of digital silence."""
        return self.loudness_batch([est], None if target is None else [target], return_blocks)[0]

    def loudness_batch(self, ests, targets=None, return_blocks=False, names=None, resident=False, deferred=False):
        """loudness() for lists of signals or, with targets, of pairs (waveform_batch's input rules: metrics.py:89-90 truncation;
        float32 or float64 signals, read in their own dtype: one ssr_loudness call per dtype).  A target object passed for several
        pairs is measured once.  names: None, or the result keys wanted.  deferred: as evaluation_batch."""
        rate = B.check_loudness_rate(self.rate)
        if not isinstance(return_blocks, bool):
            raise ValueError("return_blocks must be True or False")
        with_t = targets is not None
        keys = self._loudness_names(names, with_t)
        if with_t:
            pairs = [self._prepare_pair(e, t, resident) for e, t in zip(ests, targets)]
            sigs = [self._loudness_signal(e) for e, _ in pairs]
            tgts, index = _shared_targets([self._loudness_signal(t) for _, t in pairs])
        else:
            sigs, tgts, index = [self._loudness_signal(e) for e in ests], [], []
        n_e = len(sigs)
        every = sigs + tgts
        pending = [(idx, B.loudness_metrics([every[i] for i in idx], rate, return_blocks, self._device, deferred=True))
                   for idx in _group_by_dtype(every)]

        def finish():
            rows, blocks = np.empty((len(every), len(_LOUD_NAMES))), [None] * len(every)
            for idx, p in pending:
                got = p if return_blocks else (p, None)
                vals, blk = got[0](), (got[1]() if return_blocks else None)
                for j, i in enumerate(idx):
                    rows[i] = vals[j]
                    if return_blocks:
                        blocks[i] = blk[j]
            out = []
            for j in range(n_e):
                d = dict(zip(_LOUD_NAMES, (float(v) for v in rows[j])))
                if with_t:
                    t = rows[n_e + index[j]]
                    d.update(lufs_diff=float(rows[j][0] - t[0]), lra_diff=float(rows[j][1] - t[1]), true_peak_diff=float(rows[j][5] - t[5]))
                d = {k: d[k] for k in keys}
                if return_blocks:
                    d["blocks"] = blocks[j]
                    if with_t:
                        d["target_blocks"] = blocks[n_e + index[j]]
                out.append(d)
            return out
        return finish if deferred else finish()

    def loudness_multi(self, ests_by_key, targets, return_blocks=False, names=None, resident=False, deferred=False):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> n lists of K
        dicts.  Each target is measured once for its K estimates."""
        ests, tgts, n, K = _flat_pairs(ests_by_key, targets)
        return _regroup(self.loudness_batch(ests, tgts, return_blocks, names, resident, True), n, K, deferred)

    # ---- spectrum: what bandwidth did a signal come out with?  From its long-term average spectrum on n_fft-point
    # periodic-Hann segments at self.rate (no padding): the rolloff (the reference's BasicTestee._find_cutoff as a metric), the
    # spectral edge, the centroid, the level above a split frequency - and, with a target, their differences and the distance of the
    # two spectra in third-octave bands.  Every value is invariant to gain
    @staticmethod
    def _bandwidth_names(names, with_target):
        """The result keys asked for, in result order, or ValueError: None = all, or a non-empty tuple / list of them."""
        return _names_asked(names, _SPEC_NAMES + (_SPEC_PAIR_NAMES if with_target else ()))

    @staticmethod
    def _ltas_bands(rate, n_fft, band):
        """The analysis bands of ltas_dist / ltas_max as inclusive bin pairs: base-2 third-octave bands, centres 1000 2^(i / 3) Hz,
        edges 2^(+-1/6) around them, a band's bins those with f_lo <= k rate / n_fft < f_hi.  The table starts at the lowest band
        with f_lo >= lo_hz that holds at least 2 bins; the top band is clipped at the scored band's last bin and kept if it still
        holds at least 2; at most 40 bands (the lowest 40)."""
        lo_bin, hi_bin = AudioMetrics._phase_bins(rate, n_fft, band) or (0, n_fft // 2)
        lo_hz = 0.0 if band is None else float(band[0])
        edge = lambda j: 1000.0 * 2.0 ** ((2 * j - 1) / 6.0)      # noqa: E731  (the lower edge of band j, the upper edge of band j - 1)
        out = []
        for i in range(-60, 40):
            f_lo, f_hi = edge(i), edge(i + 1)
            k0, k1 = math.ceil(f_lo * n_fft / rate), math.ceil(f_hi * n_fft / rate) - 1
            if f_lo < lo_hz or k0 < lo_bin or k0 > hi_bin:
                continue
            clipped = k1 > hi_bin
            k1 = min(k1, hi_bin)
            if (not out or clipped) and k1 - k0 + 1 < 2:
                continue
            if k1 >= k0 and len(out) < B.SPECTRUM_MAX_BANDS:
                out.append((k0, k1))
        if not out:
            raise ValueError("band %r holds no third-octave band of 2 bins of a %d-point transform at %r Hz" % (band, n_fft, rate))
        return out

    def _bandwidth_splits(self, n_fft, split, n):
        """None, or the first upper bin of n pairs by coherence's rule, ceil(split n_fft / rate): split = one frequency in Hz for every
        pair, or a list of one per pair (None: no split for that pair, -1)."""
        if split is None:
            return None
        return [min(k, n_fft // 2 + 1) for k in _split_indices(split, n, self._ceil_bin(n_fft))]

    def bandwidth(self, est, target=None, n_fft=2048, hop=None, band=None, split_hz=None, rolloff=B.SPECTRUM_ROLLOFF,
                  drop_db=B.SPECTRUM_DROP_DB, names=None, return_ltas=False):
        """{'bw_hz', 'edge_hz', 'centroid_hz', 'hf_db'} of one signal at self.rate, from its long-term average spectrum: the rolloff -
        the frequency below which `rolloff` of the summed magnitudes lies (0.97: the reference's BasicTestee cutoff) -, the highest
        frequency whose power is within drop_db of the largest bin's, the power centroid, and the power at and above split_hz
        relative to the whole band's, in dB (NaN without split_hz or where no bin lies above it).  With a target also 'bw_diff',
        'edge_diff', 'centroid_diff', 'hf_diff' - the estimate's value minus the target's - and 'ltas_dist' / 'ltas_max', the RMS and
        the largest difference in dB of the two spectra's third-octave band levels, each relative to its signal's own total.  Every
        value is invariant to gain.  n_fft: 256, 512, 1024 or 2048; hop: None = n_fft // 2; band: None = every bin, or (lo_hz, hi_hz),
        mapped to bins as phase_distance maps it; names: None, or the result keys wanted; return_ltas: also 'ltas' (and
        'target_ltas'), the float64 [n_fft // 2 + 1] one-sided power per bin averaged over the segments.  Shorter than n_fft, or
        digitally silent in the band: NaN."""
        return self.bandwidth_batch([est], None if target is None else [target], n_fft, hop, band, split_hz, rolloff, drop_db, names,
                                    return_ltas)[0]

    def bandwidth_batch(self, ests, targets=None, n_fft=2048, hop=None, band=None, split_hz=None, rolloff=B.SPECTRUM_ROLLOFF,
                        drop_db=B.SPECTRUM_DROP_DB, names=None, return_ltas=False, resident=False, deferred=False):
        """bandwidth() for lists of signals or, with targets, of pairs (waveform_batch's input rules: metrics.py:89-90 truncation;
        float32 or float64 signals, read in their own dtype: one ssr_spectrum call per dtype group).  A target object passed for
        several pairs is transformed once.  split_hz: None, one frequency for every signal, or a list of one per signal (None:
        that signal's hf values are NaN).  deferred: as evaluation_batch."""
        n_fft, hop = B.check_coherence_frames(n_fft, hop)                   # (§20's framing)
        rho, drop = B.check_spectrum_rolloff(rolloff), B.check_spectrum_drop(drop_db)
        if not isinstance(return_ltas, bool):
            raise ValueError("return_ltas must be True or False")
        with_t = targets is not None
        keys = self._bandwidth_names(names, with_t)
        bins = self._phase_bins(self.rate, n_fft, band)
        table = self._ltas_bands(self.rate, n_fft, band)
        n = min(len(ests), len(targets)) if with_t else len(ests)
        splits = self._bandwidth_splits(n_fft, split_hz, n)
        hz = float(self.rate) / n_fft

        def row_dict(sig, pair, ltas, t_ltas):
            d = dict(zip(_SPEC_NAMES, (float(sig[0]) * hz, float(sig[1]) * hz, float(sig[2]) * hz, float(pair[0]) if pair is not None else math.nan)))
            if with_t:
                d.update(zip(_SPEC_PAIR_NAMES, (float(pair[2]) * hz, float(pair[3]) * hz, float(pair[4]) * hz, float(pair[5]), float(pair[6]),
                                                float(pair[7]))))
            d = {k: d[k] for k in keys}
            if return_ltas:
                d["ltas"] = np.array(ltas)
                if with_t:
                    d["target_ltas"] = np.array(t_ltas)
            return d

        if not with_t and splits is None:          # signals alone: they are the call's targets, there is no estimate
            sigs = [self._loudness_signal(e) for e in ests]
            pending = [(idx, B.spectrum_metrics([sigs[i] for i in idx], [], [], n_fft, hop, bins, rho, drop, table, None, return_ltas,
                                                self._device, deferred=True)) for idx in _group_by_dtype(sigs)]

            def finish():
                out = [None] * len(sigs)
                for idx, p in pending:
                    got = p()
                    for j, i in enumerate(idx):
                        out[i] = row_dict(got[0][j], None, got[2][j] if return_ltas else None, None)
                return out
            return finish if deferred else finish()

        # pairs - or signals alone with a split: the level above it is a pair's value, so each signal is paired with itself
        sigs = [self._loudness_signal(e) for e in ests[:n]]
        tgts = [self._loudness_signal(t) for t in targets[:n]] if with_t else sigs

        def call(tg, es, index, idx):
            got = B.spectrum_metrics(tg, es, index, n_fft, hop, bins, rho, drop, table, None if splits is None else [splits[i] for i in idx],
                                     return_ltas, self._device, deferred=True)
            return lambda: (got(), len(tg), list(index))

        def dicts(vals):
            got, n_t, index = vals
            return [row_dict(got[0][n_t + j], got[1][j], got[2][n_t + j] if return_ltas else None, got[2][index[j]] if return_ltas else None)
                    for j in range(len(index))]
        return self._pairs((call, dicts), sigs, tgts, resident, deferred, by_dtype=True, per_pair=True)

    def bandwidth_multi(self, ests_by_key, targets, n_fft=2048, hop=None, band=None, split_hz=None, rolloff=B.SPECTRUM_ROLLOFF,
                        drop_db=B.SPECTRUM_DROP_DB, names=None, return_ltas=False, resident=False, deferred=False):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> n lists of K
        dicts.  split_hz: None, one frequency for every key, or a list of one per key (None: NaN).  The K pairs of a target sit next
        to each other in one call and the target is transformed once."""
        ests, tgts, n, K = _flat_pairs(ests_by_key, targets)
        split_hz = _tile_key_splits(split_hz, K, n)
        return _regroup(self.bandwidth_batch(ests, tgts, n_fft, hop, band, split_hz, rolloff, drop_db, names, return_ltas, resident, True),
                        n, K, deferred)

    # ---- auditory: how alike do estimate and target look to the ear's filterbank?  The neurogram similarity index (NSIM,
    # Hines & Harte 2012; the core of ViSQOL) of their gammatone spectrograms at self.rate: a 4th-order complex gammatone filterbank on
    # the ERB scale, 20 ms power frames every 10 ms, dB over a range below the target's largest cell, a 3 x 3 SSIM-like index
    @staticmethod
    def _nsim_names(names):
        """The result keys asked for, in result order, or ValueError: None = all, or a non-empty tuple / list of them."""
        return _names_asked(names, _NSIM_NAMES)

    @staticmethod
    def _nsim_splits(fc, split, n):
        """The first interior band at or above the split of n pairs (len(fc) - 1: the split lies above every interior band): split = None
        (no split: -1 for every pair), one frequency in Hz for every pair, or a list of one per pair (None: -1 for that pair)."""
        return _split_indices(split, n, lambda f: 1 + int(np.searchsorted(fc[1:-1], f, side="left")))

    def nsim(self, est, target, split_hz=None, n_bands=B.AUDITORY_N_BANDS, band=None, range_db=B.AUDITORY_RANGE_DB, match_level=True,
             return_bands=False):
        """{'nsim', 'nsim_hf', 'nsim_lf'} of one (estimate, target) pair at self.rate: the neurogram similarity index of their
        gammatone spectrograms - 1 for identical images, lower the less the estimate's time-frequency pattern resembles the
        target's - over all interior bands, and over the interior bands whose centre frequency is at / above and below split_hz (NaN
        without split_hz or where no such band exists).  n_bands: 3 to 64 bands with centres equally spaced on the ERB scale over
        band = (lo_hz, hi_hz) (None: 50 Hz to 0.45 rate); range_db: the dB range below the target's largest cell that is scored;
        match_level: the estimate's image is scaled to the target's total power first, so that the value is invariant to the
        estimate's gain.  return_bands: also 'fvnsim', the mean over time of every band (NaN in the two edge bands), and
        'centre_hz'.  Shorter than 40 ms (fewer than 3 image rows), or a digitally silent target: NaN."""
        return self.nsim_batch([est], [target], split_hz, n_bands, band, range_db, match_level, return_bands)[0]

    def nsim_batch(self, ests, targets, split_hz=None, n_bands=B.AUDITORY_N_BANDS, band=None, range_db=B.AUDITORY_RANGE_DB, match_level=True,
                   return_bands=False, names=None, resident=False, deferred=False):
        """nsim() for lists of pairs, with waveform_batch's input rules (metrics.py:89-90 truncation; float32 or float64 signals, read
        in their own dtype: one ssr_auditory call per (target dtype, estimate dtype) group).  A target object passed for several pairs
        is filtered once.  split_hz: None, one frequency for every pair, or a list of one per pair (None: that pair's nsim_hf and
        nsim_lf are NaN).  names: None, or the result keys wanted.  deferred: as evaluation_batch."""
        fc, _ = B.gammatone_design(self.rate, n_bands, band)
        rng_db = B.check_auditory_range(range_db)
        if not isinstance(match_level, bool) or not isinstance(return_bands, bool):
            raise ValueError("match_level and return_bands must be True or False")
        keys = self._nsim_names(names)
        n = min(len(ests), len(targets))
        splits = self._nsim_splits(fc, split_hz, n)

        def call(tgts, es, index, idx):
            return B.auditory_metrics(tgts, es, index, self.rate, n_bands, band, rng_db, match_level, [splits[i] for i in idx], return_bands,
                                      False, None, self._device, deferred=True)

        def dicts(vals):
            pair, bands, _ = vals
            out = []
            for j, row in enumerate(pair):
                d = {k: float(v) for k, v in zip(_NSIM_NAMES, row) if k in keys}
                if return_bands:
                    d["fvnsim"], d["centre_hz"] = np.array(bands[j]), np.array(fc)
                out.append(d)
            return out
        _check_1d(list(ests[:n]) + list(targets[:n]))
        return self._pairs((call, dicts), ests[:n], targets[:n], resident, deferred, by_dtype=True, per_pair=True)

    def nsim_multi(self, ests_by_key, targets, split_hz=None, n_bands=B.AUDITORY_N_BANDS, band=None, range_db=B.AUDITORY_RANGE_DB,
                   match_level=True, return_bands=False, names=None, resident=False, deferred=False):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> n lists of K
        dicts.  split_hz: None, one frequency for every key, or a list of one per key (None: NaN).  The K pairs of a target sit next
        to each other in one call and the target is filtered once."""
        ests, tgts, n, K = _flat_pairs(ests_by_key, targets)
        split_hz = _tile_key_splits(split_hz, K, n)
        return _regroup(self.nsim_batch(ests, tgts, split_hz, n_bands, band, range_db, match_level, return_bands, names, resident, True),
                        n, K, deferred)

    def gammatone_spectrogram(self, wav, n_bands=B.AUDITORY_N_BANDS, band=None, range_db=B.AUDITORY_RANGE_DB):
        """(image [T, n_bands] float64, centre_hz [n_bands]): the gammatone power spectrogram of one signal at self.rate in dB re
        full-scale power - 20 ms frames every 10 ms, no padding (T = 1 + (len - win) // hop), clamped range_db below its largest
        cell; NaN for a digitally silent signal."""
        fc, _ = B.gammatone_design(self.rate, n_bands, band)
        _, _, images = B.auditory_metrics([self._loudness_signal(wav)], [], [], self.rate, n_bands, band, range_db, True, None, False, True,
                                          None, self._device)
        return images[0], np.array(fc)

    # ---- modulation: does a signal move like speech?  The envelopes of §23's gammatone bands, at about env_rate Hz,
    # through eight modulation band-passes from 4 to 128 Hz; 256 ms Hamming frames every 64 ms; the mean frame energy per (band,
    # modulation band) is the modulation spectrum.  SRMR (Falk, Zheng & Chan 2010) is its energy below 20 Hz over that above, and it
    # needs no target; mod_dist is the RMS difference in dB of two such spectra
    @staticmethod
    def _modulation_names(names):
        """The result keys asked for, in result order, or ValueError: None = all, or a non-empty tuple / list of them."""
        return _names_asked(names, _MOD_NAMES)

    @staticmethod
    def _modulation_splits(fc, split, n):
        """The first band whose centre frequency is at or above the split of n pairs, in [0, len(fc)]: split = None (no split: -1 for
        every pair), one frequency in Hz for every pair, or a list of one per pair (None: -1 for that pair)."""
        return _split_indices(split, n, lambda f: int(np.searchsorted(fc, f, side="left")))

    def _modulation_design(self, n_bands, band, env_rate, range_db, kstar):
        """-> (f_c, the modulation centres in Hz, range_db as a float): every option checked, nothing queued."""
        fc = B.modulation_design(self.rate, B.modulation_hop(self.rate, env_rate), n_bands, band, kstar)[0]
        return fc, 4.0 * 32.0 ** (np.arange(B.MODULATION_BANDS) / (B.MODULATION_BANDS - 1.0)), B.check_modulation_range(range_db)

    def srmr(self, wav, n_bands=B.AUDITORY_N_BANDS, band=None, env_rate=B.MODULATION_ENV_RATE, kstar=None, return_spectrum=False):
        """{'srmr', 'kstar', 'c90'} of one signal at self.rate, without a target: the speech-to-reverberation modulation energy ratio
        (Falk, Zheng & Chan 2010) - the energy of the sub-band envelopes in the four modulation bands from 4 to about 18 Hz over
        that in the bands from about 29 Hz up to the K*-th, K* = 5 .. 8 chosen from the gammatone band c90 below which 90 % of the
        modulation energy lies (or the constant `kstar`).  Clean, dry speech scores high; reverberation and stationary texture
        score low.  n_bands, band: the gammatone filterbank of nsim(); env_rate: the envelope is sampled at about this rate
        (self.rate / (self.rate // env_rate)), 800 to 6400 Hz.  return_spectrum: also 'mod_spectrum' [n_bands, 8], the mean frame
        energy per (band, modulation band), 'centre_hz' and 'mod_hz'.  Shorter than one 256 ms frame, digitally silent, or no
        energy above 20 Hz: NaN (kstar and c90: -1)."""
        fc, fk, _ = self._modulation_design(n_bands, band, env_rate, B.MODULATION_RANGE_DB, kstar)
        if not isinstance(return_spectrum, bool):
            raise ValueError("return_spectrum must be True or False")
        sig, _, spec = B.modulation_metrics([self._loudness_signal(wav)], [], [], self.rate, n_bands, band, env_rate, B.MODULATION_RANGE_DB,
                                            kstar, None, return_spectrum, None, self._device)
        whole = lambda v: -1 if math.isnan(v) else int(v)      # noqa: E731
        d = {"srmr": float(sig[0, 0]), "kstar": whole(sig[0, 1]), "c90": whole(sig[0, 2])}
        if return_spectrum:
            d["mod_spectrum"], d["centre_hz"], d["mod_hz"] = np.array(spec[0]), np.array(fc), fk
        return d

    def modulation(self, est, target, split_hz=None, n_bands=B.AUDITORY_N_BANDS, band=None, env_rate=B.MODULATION_ENV_RATE,
                   range_db=B.MODULATION_RANGE_DB, kstar=None, names=None, return_spectrum=False):
        """{'srmr', 'srmr_diff', 'mod_dist', 'mod_dist_hf', 'mod_dist_lf'} of one (estimate, target) pair at self.rate: the estimate's
        srmr(), that minus the target's, and the RMS difference in dB of the two modulation spectra - the estimate's scaled to the
        target's total first, so that the value is invariant to gain, both clamped range_db below the target's largest cell - over
        all cells, and over the gammatone bands whose centre frequency is at / above and below split_hz (NaN without split_hz or
        where no such band exists).  n_bands, band, env_rate, kstar: as srmr().  names: None, or the result keys wanted.
        return_spectrum: also 'mod_spectrum' and 'target_mod_spectrum' [n_bands, 8], 'centre_hz' and 'mod_hz'.  A target shorter
        than one 256 ms frame or digitally silent, or a silent estimate: NaN."""
        return self.modulation_batch([est], [target], split_hz, n_bands, band, env_rate, range_db, kstar, names, return_spectrum)[0]

    def modulation_batch(self, ests, targets, split_hz=None, n_bands=B.AUDITORY_N_BANDS, band=None, env_rate=B.MODULATION_ENV_RATE,
                         range_db=B.MODULATION_RANGE_DB, kstar=None, names=None, return_spectrum=False, resident=False, deferred=False):
        """modulation() for lists of pairs, with waveform_batch's input rules (metrics.py:89-90 truncation; float32 or float64 signals,
        read in their own dtype: one ssr_modulation call per (target dtype, estimate dtype) group, split further where its workspace
        would pass backend.MODULATION_WORKSPACE_CAP).  A target object passed for several pairs is filtered once.  split_hz: None,
        one frequency for every pair, or a list of one per pair (None: that pair's mod_dist_hf and mod_dist_lf are NaN).
        deferred: as evaluation_batch."""
        fc, fk, rng_db = self._modulation_design(n_bands, band, env_rate, range_db, kstar)
        if not isinstance(return_spectrum, bool):
            raise ValueError("return_spectrum must be True or False")
        keys = self._modulation_names(names)
        n = min(len(ests), len(targets))
        splits = self._modulation_splits(fc, split_hz, n)

        def call(tgts, es, index, idx):
            got = B.modulation_metrics(tgts, es, index, self.rate, n_bands, band, env_rate, rng_db, kstar, [splits[i] for i in idx],
                                       return_spectrum, None, self._device, deferred=True)
            return lambda: got() + (len(tgts), index)

        def dicts(vals):
            sig, pair, spec, n_t, index = vals
            out = []
            for j, row in enumerate(pair):
                d = {k: float(v) for k, v in zip(_MOD_NAMES, (sig[n_t + j, 0],) + tuple(row)) if k in keys}
                if return_spectrum:
                    d["mod_spectrum"], d["target_mod_spectrum"] = np.array(spec[n_t + j]), np.array(spec[index[j]])
                    d["centre_hz"], d["mod_hz"] = np.array(fc), np.array(fk)
                out.append(d)
            return out
        _check_1d(list(ests[:n]) + list(targets[:n]))
        return self._pairs((call, dicts), ests[:n], targets[:n], resident, deferred, by_dtype=True, per_pair=True)

    def modulation_multi(self, ests_by_key, targets, split_hz=None, n_bands=B.AUDITORY_N_BANDS, band=None, env_rate=B.MODULATION_ENV_RATE,
                         range_db=B.MODULATION_RANGE_DB, kstar=None, names=None, return_spectrum=False, resident=False, deferred=False):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> n lists of K
        dicts.  split_hz: None, one frequency for every key, or a list of one per key (None: NaN).  The K pairs of a target sit next
        to each other in one call and the target is filtered once."""
        ests, tgts, n, K = _flat_pairs(ests_by_key, targets)
        split_hz = _tile_key_splits(split_hz, K, n)
        return _regroup(self.modulation_batch(ests, tgts, split_hz, n_bands, band, env_rate, range_db, kstar, names, return_spectrum, resident,
                                              True), n, K, deferred)

    # ---- csii: how much of the estimate would a listener understand?  The coherence speech intelligibility index of
    # Kates & Arehart (2005): §20's magnitude-squared coherence as a signal-to-distortion ratio per critical band up to 8.5 kHz,
    # weighted with the band importance of ANSI S3.5-1997, taken separately over the target's high-, mid- and low-level segments (the
    # low-level ones carry the consonants), and the fitted three-level index I3
    @staticmethod
    def _csii_names(names):
        """The result keys asked for, in result order, or ValueError: None = all, or a non-empty tuple / list of them."""
        return _names_asked(names, _CSII_NAMES)

    @staticmethod
    def _csii_splits(fc, split, n):
        """The first band whose centre frequency is at or above the split of n pairs, in [0, len(fc)]: split = None (no split: -1 for
        every pair), one frequency in Hz for every pair, or a list of one per pair (None: -1 for that pair)."""
        return _split_indices(split, n, lambda f: int(np.searchsorted(fc, f, side="left")))

    def _csii_design(self, n_fft, hop, band):
        """-> (n_fft, hop, f_c): every option checked, nothing queued."""
        n_fft, hop = B.check_csii_frames(self.rate, n_fft, hop)
        return n_fft, hop, B.csii_design(self.rate, n_fft, band)[0]

    def csii(self, est, target, split_hz=None, n_fft=None, hop=None, band=None, names=None, return_bands=False, return_counts=False):
        """{'csii', 'csii_low', 'csii_mid', 'csii_high', 'i3', 'csii_hf', 'csii_mid_hf'} of one (estimate, target) pair at self.rate:
        the coherence speech intelligibility index over all segments and over the target's low- (-30 .. -10 dB re its overall level),
        mid- (-10 .. 0 dB) and high-level (>= 0 dB) segments, each in [0, 1] with 1 for an estimate that is a linear function of the
        target; i3 = 1 / (1 + exp(-(-3.47 + 1.84 csii_low + 9.99 csii_mid))), the fitted intelligibility; csii_hf / csii_mid_hf: csii
        and csii_mid over the critical bands whose centre is at or above split_hz (NaN without split_hz or where no such band
        exists).  Invariant to the estimate's gain.  n_fft: None = 16 ms (backend.csii_default_nfft), or 256, 512, 1024 or 2048;
        hop: None = n_fft // 2; band: None or (lo_hz, hi_hz), the band centres kept; names: None, or the result keys wanted.
        return_bands: also 'band_values' [4, n_bands], the band values of the sets all, low, mid, high, and 'centre_hz';
        return_counts: also 'n_segments', 'n_low', 'n_mid', 'n_high'.  A set of fewer than two segments and a digitally silent
        target: NaN (i3: NaN where csii_low or csii_mid is)."""
        return self.csii_batch([est], [target], split_hz, n_fft, hop, band, names, return_bands, return_counts)[0]

    def csii_batch(self, ests, targets, split_hz=None, n_fft=None, hop=None, band=None, names=None, return_bands=False, return_counts=False,
                   resident=False, deferred=False):
        """csii() for lists of pairs, with waveform_batch's input rules (metrics.py:89-90 truncation; float32 or float64 signals, read
        in their own dtype: one ssr_csii call per (target dtype, estimate dtype) group).  A target object passed for several pairs is
        classified once.  split_hz: None, one frequency for every pair, or a list of one per pair (None: that pair's two _hf values
        are NaN).  deferred: as evaluation_batch."""
        n_fft, hop, fc = self._csii_design(n_fft, hop, band)
        if not isinstance(return_bands, bool) or not isinstance(return_counts, bool):
            raise ValueError("return_bands and return_counts must be True or False")
        keys = self._csii_names(names)
        n = min(len(ests), len(targets))
        splits = self._csii_splits(fc, split_hz, n)

        def call(tgts, es, index, idx):
            return B.csii_metrics(tgts, es, index, self.rate, n_fft, hop, band, [splits[i] for i in idx], return_bands, self._device, deferred=True)

        def dicts(vals):
            rows, bands = vals
            out = []
            for j, row in enumerate(rows):
                d = {k: float(row[c]) for k, c in zip(_CSII_NAMES, _CSII_COLUMNS) if k in keys}
                if return_bands:
                    d["band_values"], d["centre_hz"] = np.array(bands[j]), np.array(fc)
                if return_counts:
                    d.update({k: int(row[9 + c]) for c, k in enumerate(_CSII_COUNT_NAMES)})
                out.append(d)
            return out
        _check_1d(list(ests[:n]) + list(targets[:n]))
        return self._pairs((call, dicts), ests[:n], targets[:n], resident, deferred, by_dtype=True, per_pair=True)

    def csii_multi(self, ests_by_key, targets, split_hz=None, n_fft=None, hop=None, band=None, names=None, return_bands=False,
                   return_counts=False, resident=False, deferred=False):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> n lists of K
        dicts.  split_hz: None, one frequency for every key, or a list of one per key (None: NaN).  The K pairs of a target sit next
        to each other in one call and the target is classified once."""
        ests, tgts, n, K = _flat_pairs(ests_by_key, targets)
        split_hz = _tile_key_splits(split_hz, K, n)
        return _regroup(self.csii_batch(ests, tgts, split_hz, n_fft, hop, band, names, return_bands, return_counts, resident, True), n, K, deferred)

    # ---- nmr: is the difference audible?  The noise-to-mask ratio: the error spectrum per quarter-Bark band over the
    # masking threshold the target itself produces (the FFT ear model of ITU-R BS.1387 after Kabal 2002, restated; no conformance
    # is claimed, the ODG network is not built).  Negative: the error lies under the threshold
    @staticmethod
    def _nmr_names(names):
        """The result keys asked for, in result order, or ValueError: None = all, or a non-empty tuple / list of them."""
        return _names_asked(names, _NMR_NAMES)

    @staticmethod
    def _nmr_splits(fc, split, n):
        """The first band whose centre frequency is at or above the split of n pairs, in [0, len(fc)]: split = None (no split: -1 for
        every pair), one frequency in Hz for every pair, or a list of one per pair (None: -1 for that pair)."""
        return _split_indices(split, n, lambda f: int(np.searchsorted(fc, f, side="left")))

    def _nmr_design(self, n_fft, level_db):
        """-> backend.nmr_design's dict: every option checked, nothing queued."""
        return B.nmr_design(self.rate, n_fft, level_db)

    def nmr(self, est, target, split_hz=None, n_fft=None, level_db=B.NMR_LEVEL_DB, names=None, return_bands=False):
        """{'nmr', 'nmr_seg', 'rdf', 'nmr_hf', 'nmr_lf'} of one (estimate, target) pair at self.rate (8 to 192 kHz): nmr, the total
        noise-to-mask ratio in dB - the mean over frames and quarter-Bark bands of the error power (the difference of the two
        magnitude spectra) over the target's masking threshold, negative where the error is masked; nmr_seg, the mean over frames of
        the frame's ratio in dB; rdf, the share of frames in which some band's ratio reaches 1.5 dB; nmr_hf / nmr_lf: nmr over the
        bands whose centre is at or above / below split_hz (NaN without split_hz or where no such band exists).  n_fft: None = 32 ms
        (backend.nmr_default_nfft), or 256, 512, 1024 or 2048, hop n_fft / 2; level_db: the level of a full-scale sine in dB SPL;
        names: None, or the result keys wanted.  return_bands: also 'band_ratio' [Nc], the mean ratio per band over the frames
        (linear), 'centre_hz' and 'frames'.  Shorter than one frame: NaN.  An estimate equal to the target: -200 and rdf 0."""
        return self.nmr_batch([est], [target], split_hz, n_fft, level_db, names, return_bands)[0]

    def nmr_batch(self, ests, targets, split_hz=None, n_fft=None, level_db=B.NMR_LEVEL_DB, names=None, return_bands=False, resident=False,
                  deferred=False):
        """nmr() for lists of pairs, with waveform_batch's input rules (metrics.py:89-90 truncation; float32 or float64 signals, read
        in their own dtype: one ssr_nmr call per (target dtype, estimate dtype) group).  The masking threshold of a target object
        passed for several pairs is made once.  split_hz: None, one frequency for every pair, or a list of one per pair (None: that
        pair's nmr_hf and nmr_lf are NaN).  deferred: as evaluation_batch."""
        d = self._nmr_design(n_fft, level_db)
        fc = d["fc"]
        if not isinstance(return_bands, bool):
            raise ValueError("return_bands must be True or False")
        keys = self._nmr_names(names)
        n = min(len(ests), len(targets))
        splits = self._nmr_splits(fc, split_hz, n)

        def call(tgts, es, index, idx):
            return B.nmr_metrics(tgts, es, index, self.rate, d["n_fft"], d["level_db"], [splits[i] for i in idx], return_bands, False, self._device,
                                 deferred=True)

        def dicts(vals):
            rows, bands, _ = vals
            out = []
            for j, row in enumerate(rows):
                q = {k: float(row[c]) for c, k in enumerate(_NMR_NAMES) if k in keys}
                if return_bands:
                    q["band_ratio"], q["centre_hz"], q["frames"] = np.array(bands[j]), np.array(fc), int(row[5])
                out.append(q)
            return out
        _check_1d(list(ests[:n]) + list(targets[:n]))
        return self._pairs((call, dicts), ests[:n], targets[:n], resident, deferred, by_dtype=True, per_pair=True)

    def nmr_multi(self, ests_by_key, targets, split_hz=None, n_fft=None, level_db=B.NMR_LEVEL_DB, names=None, return_bands=False,
                  resident=False, deferred=False):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> n lists of K
        dicts.  split_hz: None, one frequency for every key, or a list of one per key (None: NaN).  The K pairs of a target sit next
        to each other in one call and the target's masking threshold is made once."""
        ests, tgts, n, K = _flat_pairs(ests_by_key, targets)
        split_hz = _tile_key_splits(split_hz, K, n)
        return _regroup(self.nmr_batch(ests, tgts, split_hz, n_fft, level_db, names, return_bands, resident, True), n, K, deferred)

    def masking_threshold(self, wav, n_fft=None, level_db=B.NMR_LEVEL_DB):
        """(mask [T, Nc] float64, centre_hz [Nc]): the masking threshold of one signal at self.rate in dB (the level scale of
        level_db), per frame of n_fft samples every n_fft / 2 (T = 1 + (len - n_fft) // (n_fft // 2), no padding) and quarter-Bark
        band.  The call scores the signal against itself: ssr_nmr queues nothing without an estimate, so the noise and score kernels run
        too - about 60 % on top of the excitation and mask kernels' time - and their result is dropped."""
        d = self._nmr_design(n_fft, level_db)
        wav = self._loudness_signal(wav)
        _, _, mask = B.nmr_metrics([wav], [wav], [0], self.rate, d["n_fft"], d["level_db"], None, False, True, self._device)
        return 10.0 * np.log10(mask), np.array(d["fc"])

    # ---- delay estimation and compensation (not in the reference): a stage in front of the metrics, no metric family.
    # The estimate's delay against the target within +- max_lag samples by a float64 cross-correlation, and the estimate with that
    # delay taken out (zero-filled at the edge it is shifted away from); the two signals need not be equally long
    @staticmethod
    def _align_dicts(rows):
        return [{_ALIGN_NAMES[0]: float(r[0]), _ALIGN_NAMES[1]: float(r[1]), _ALIGN_NAMES[2]: float(r[2]), _ALIGN_NAMES[3]: float(r[3])} for r in rows]

    def align(self, est, target, max_lag=B.ALIGN_LAG, subsample=False):
        """-> (the estimate with its delay against `target` taken out, an ndarray of the estimate's dtype and length; {'delay': d*
        in samples, positive where the estimate is late, 'delay_frac': the parabola's sub-sample estimate in [-0.5, 0.5],
        'align_corr': the normalised correlation at d*, 'align_edge': 1.0 where |d*| = max_lag}).  subsample: the shift is by d* +
        delay_frac through a 33-tap windowed sinc; otherwise by d*, a copy.  Digital silence on either side: delay 0, NaN
        align_corr, the estimate as it is."""
        aligned, dicts = self.align_batch([est], [target], max_lag, subsample)
        return aligned[0], dicts[0]

    def delay(self, est, target, max_lag=B.ALIGN_LAG):
        """The dict of align() alone: nothing is shifted."""
        _check_1d([est, target])
        tgts, index = _shared_targets([target])
        rows, _, _ = B.align(tgts, [est], index, max_lag, False, False, self._device, shift=False)
        return self._align_dicts(rows)[0]

    def align_batch(self, ests, targets, max_lag=B.ALIGN_LAG, subsample=False, resident=False, deferred=False):
        """align() for lists of pairs in one ssr_align call per estimate dtype -> (the aligned estimates, the dicts).  A target object
        passed for several pairs appears once in the call.  resident: the aligned estimates stay device tensors, views of one buffer
        per dtype (otherwise ndarrays).  deferred: the dicts are a function that returns them; nothing waits for the delays - the
        shift reads them from device memory."""
        n = min(len(ests), len(targets))
        ests, targets = list(ests[:n]), list(targets[:n])
        _check_1d(ests + targets)
        tgts, index = _shared_targets(targets)
        rows, shifted, _ = B.align(tgts, ests, index, max_lag, subsample, False, self._device, deferred=True)
        if not resident:
            shifted = [z.cpu().numpy() for z in shifted]
        dicts = lambda: self._align_dicts(rows())      # noqa: E731
        return shifted, (dicts if deferred else dicts())

    def align_multi(self, ests_by_key, targets, max_lag=B.ALIGN_LAG, subsample=False, resident=False, deferred=False):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> (K lists of n
        aligned estimates, n lists of K dicts).  Only the estimates are shifted; a target is named once for its K estimates and is
        never cropped."""
        ests, tgts, n, K = _flat_pairs(ests_by_key, targets)
        shifted, dicts = self.align_batch(ests, tgts, max_lag, subsample, resident, True)
        return [[shifted[i * K + k] for i in range(n)] for k in range(K)], _regroup(dicts, n, K, deferred)

    # ---- mel-spectrogram distances (not in the reference): on this rate's magnitude image, NVSR's 128-band HTK mel
    # front end by default.  **mel: n_mels, f_min, f_max, norm, mel_scale (torchaudio's melscale_fbanks), n_cep (mcd).
    _fb_cache = {}

    def mel_options(self, **mel):
        """-> (n_mels, f_min, f_max, norm, mel_scale, n_cep) with the defaults filled in; ValueError for an unknown name or value."""
        bad = sorted(set(mel) - set(M.MEL_OPTIONS))
        if bad:
            raise ValueError("unknown mel option(s) %s (known: %s)" % (bad, M.MEL_OPTIONS))
        return M.check_options(self.rate, **mel)

    def mel_filterbank(self, **mel):
        """(float32 [F, n_mels] host tensor, n_cep): a copy of the filterbank at this rate's F = n_fft // 2 + 1."""
        fb, n_cep = self._mel_fb(**mel)
        return fb.clone(), n_cep

    def _mel_fb(self, **mel):
        """mel_filterbank's table itself: page-locked, cached per (rate, F, options, device) and never written again (the library
        copies it asynchronously).  Internal: callers outside this class get copies."""
        n_mels, f_min, f_max, norm, scale, n_cep = self.mel_options(**mel)
        F = self.n_fft // 2 + 1
        key = (self.rate, F, n_mels, f_min, f_max, norm, scale, str(self._device))
        fb = AudioMetrics._fb_cache.get(key)
        if fb is None:
            fb = M.mel_filterbank(F, f_min, f_max, n_mels, self.rate, norm, scale).contiguous()
            if torch.cuda.is_available():
                fb = fb.pin_memory()
            AudioMetrics._fb_cache[key] = fb
        return fb, n_cep

    _mel_which = staticmethod(functools.partial(which_mask, names=_MEL_NAMES))

    @staticmethod
    def _mel_dict(row, mask):
        return rows_dicts([row], mask, _MEL_NAMES, packed=False)[0]      # the library writes all three columns, NaN where not asked

    def mel_spectrogram(self, wav, keep_on_device=False, **mel):
        """[n] waveform -> mel spectrogram [1, 1, T, n_mels] float32: wav_to_spectrogram's magnitude image times the filterbank."""
        fb, _ = self._mel_fb(**mel)
        sp = self.wav_to_spectrogram(wav, keep_on_device=True)
        out = B.spectrogram_mel(sp[0], fb)[None]
        return out if keep_on_device else out.cpu()

    def mel_distance(self, est, target, which="all", **mel):
        """{'mel_lsd', 'mel_l1', 'mcd'} (or the subset `which` names) of one (estimate, target) pair."""
        return self.mel_distance_batch([est], [target], which, **mel)[0]

    def mel_distance_batch(self, ests, targets, which="all", resident=False, deferred=False, **mel):
        """mel_distance for lists of pairs, with evaluation_batch's input rules (metrics.py:89-90 truncation, float64 estimates kept
        float64; float32 targets): one ssr_pair_mel_metrics call per estimate dtype.  deferred: as evaluation_batch."""
        mask = self._mel_which(which)
        fb, n_cep = self._mel_fb(**mel)
        return self._keyed_batch(_by_dtype, lambda e, t, idx: B.pair_mel_metrics(self._plan(), e, t, fb, n_cep, mask, deferred=True),
                                 lambda row, i: self._mel_dict(row, mask), None, ests, targets, resident, deferred)

    def mel_distance_multi(self, ests_by_key, targets, which="all", resident=False, deferred=False, keys_per_chunk=None, **mel):
        """K estimates per target, as evaluation_multi: ests_by_key = K lists of n waveforms, targets = n waveforms -> n lists of K
        dicts.  Keys of one estimate dtype share one multi-key launch sequence (each target transformed once per chunk of keys);
        lengths that differ between keys, or a key with both dtypes, send the pairs through mel_distance_batch."""
        mask = self._mel_which(which)
        fb, n_cep = self._mel_fb(**mel)
        return self._keyed_multi(_by_dtype, lambda e, t, keys: B.pair_mel_metrics(self._plan(), e, t, fb, n_cep, mask, deferred=True,
                                                                                  keys_per_chunk=keys_per_chunk),
                                 lambda row, k: self._mel_dict(row, mask), None,
                                 lambda e, t: self.mel_distance_batch(e, t, which, True, deferred=True, **mel),
                                 ests_by_key, targets, resident, deferred)

    def mel_distance_spectrogram(self, est_sp, tgt_sp, which="all", **mel):
        """[B, C, T, F] magnitude tensors x2 (F = n_fft // 2 + 1) -> {name: [B, C] float64 tensor} for the names `which` asks for."""
        if est_sp.shape != tgt_sp.shape or est_sp.dim() != 4:
            raise ValueError("expected two [B, C, T, F] tensors of one shape, got %s and %s" % (tuple(est_sp.shape), tuple(tgt_sp.shape)))
        mask = self._mel_which(which)
        fb, n_cep = self._mel_fb(**mel)
        Bn, Cn, T, F = (int(v) for v in est_sp.shape)
        v = B.spectrogram_mel_metrics(est_sp.reshape(Bn * Cn, T, F), tgt_sp.reshape(Bn * Cn, T, F), fb, n_cep, mask)
        v = v.to(est_sp.device).reshape(Bn, Cn, 3)
        return {m: v[..., j] for j, m in enumerate(_MEL_NAMES) if mask & (1 << j)}

    # ---- DTW-aligned mel-cepstral distortion (not in the reference): the mel front end above, every image's own
    # cepstra, and a band-limited warp of the estimate's frames onto the target's.  radius: the band's half width in frames.
    @staticmethod
    def dtw_radius(radius):
        """-> the radius as an int; ValueError unless it is an integer in 0..31."""
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= B._lib.DTW_MAX_RADIUS:
            raise ValueError("radius must be an integer in 0..%d (frames)" % B._lib.DTW_MAX_RADIUS)
        return int(radius)

    @staticmethod
    def _dtw_dict(row, lengths=True):
        return {m: float(row[j]) for j, m in enumerate(_MEL_DTW_NAMES) if lengths or m != "dtw_len"}

    def mel_dtw(self, est, target, radius=16, **mel):
        """{'mcd_dtw', 'dtw_dev', 'dtw_len'} of one (estimate, target) pair: the mel-cepstral distortion along the best warp inside
        |i - j| <= radius frames, that path's mean drift in frames and its number of cells.  radius = 0: mcd."""
        return self.mel_dtw_batch([est], [target], radius, **mel)[0]

    def mel_dtw_batch(self, ests, targets, radius=16, resident=False, deferred=False, lengths=True, **mel):
        """mel_dtw for lists of pairs, with mel_distance_batch's input rules.  lengths=False: the dicts carry no dtw_len."""
        radius = self.dtw_radius(radius)
        fb, n_cep = self._mel_fb(**mel)
        return self._keyed_batch(_by_dtype, lambda e, t, idx: B.pair_mel_dtw(self._plan(), e, t, fb, n_cep, radius, deferred=True),
                                 lambda row, i: self._dtw_dict(row, lengths), None, ests, targets, resident, deferred)

    def mel_dtw_multi(self, ests_by_key, targets, radius=16, resident=False, deferred=False, keys_per_chunk=None, lengths=True, **mel):
        """K estimates per target, as mel_distance_multi -> n lists of K dicts."""
        radius = self.dtw_radius(radius)
        fb, n_cep = self._mel_fb(**mel)
        return self._keyed_multi(_by_dtype, lambda e, t, keys: B.pair_mel_dtw(self._plan(), e, t, fb, n_cep, radius, deferred=True,
                                                                              keys_per_chunk=keys_per_chunk),
                                 lambda row, k: self._dtw_dict(row, lengths), None,
                                 lambda e, t: self.mel_dtw_batch(e, t, radius, True, deferred=True, lengths=lengths, **mel),
                                 ests_by_key, targets, resident, deferred)

    def mel_dtw_spectrogram(self, est_sp, tgt_sp, radius=16, **mel):
        """[B, C, T, F] magnitude tensors x2 (F = n_fft // 2 + 1) -> {'mcd_dtw', 'dtw_dev', 'dtw_len'}: [B, C] float64 tensors."""
        if est_sp.shape != tgt_sp.shape or est_sp.dim() != 4:
            raise ValueError("expected two [B, C, T, F] tensors of one shape, got %s and %s" % (tuple(est_sp.shape), tuple(tgt_sp.shape)))
        radius = self.dtw_radius(radius)
        fb, n_cep = self._mel_fb(**mel)
        Bn, Cn, T, F = (int(v) for v in est_sp.shape)
        v = B.spectrogram_mel_dtw(est_sp.reshape(Bn * Cn, T, F), tgt_sp.reshape(Bn * Cn, T, F), fb, n_cep, radius)
        v = v.to(est_sp.device).reshape(Bn, Cn, 3)
        return {m: v[..., j] for j, m in enumerate(_MEL_DTW_NAMES)}

    # ---- reductions on [B, C, T, F] tensors (est first)
    @staticmethod
    def _images(x):
        """The B*C [T, F] images of a [B, C, T, F] tensor, batch-major (the reference loops b, then c: metrics.py:128-131)."""
        if x.dim() != 4:
            raise ValueError("expected a [B, C, T, F] tensor, got %s" % (tuple(x.shape),))
        return [x[b, c] for b in range(x.shape[0]) for c in range(x.shape[1])]

    def _reduce(self, est, target, mask):
        if est.shape != target.shape:
            raise ValueError("spectrogram shape mismatch: %s vs %s" % (tuple(est.shape), tuple(target.shape)))
        return B.spectrogram_metrics(self._images(est), self._images(target), mask)

    def lsd(self, est, target):
        """[B, C, T, F] x2 -> [B, C, 1, 1] float32 (metrics.py:109-112; one value per image)."""
        v = self._reduce(est, target, B.M_LSD)[:, 0]
        return v.to(torch.float32).to(est.device).reshape(est.shape[0], est.shape[1], 1, 1)

    def _sispec_multichannel(self, est, target, log_domain):
        """metrics.py:114-121 for C > 1 (one ratio per batch item over an all-channel target energy): ssr_sispec_multichannel."""
        if est.shape != target.shape:
            raise ValueError("spectrogram shape mismatch: %s vs %s" % (tuple(est.shape), tuple(target.shape)))
        return B.sispec_multichannel(est, target, log_domain).to(torch.float32).to(est.device)

    def sispec(self, est, target):
        """Scale-invariant spectrogram-to-noise ratio, mean over the batch, 0-dim float32 (metrics.py:114-121)."""
        if est.dim() == 4 and est.shape[1] != 1:
            return self._sispec_multichannel(est, target, False)
        v = self._reduce(est, target, B.M_SISPEC)[:, 2]
        return (v.sum() / v.shape[0]).to(torch.float32).to(est.device)

    def log_sispec(self, est, target):
        """sispec(to_log(est), to_log(target)) of metrics.py:99-101 with the log10(x + 1e-12) fused in-kernel."""
        if est.dim() == 4 and est.shape[1] != 1:
            return self._sispec_multichannel(est, target, True)
        v = self._reduce(est, target, B.M_LOG_SISPEC)[:, 1]
        return (v.sum() / v.shape[0]).to(torch.float32).to(est.device)

    def ssim(self, est, target):
        """[B, C, T, F] x2 -> [B, C, 1, 1] float64 (metrics.py:123-132; one skimage call per image)."""
        v = self._reduce(est, target, B.M_SSIM)[:, 3]
        return v.to(est.device).reshape(est.shape[0], est.shape[1], 1, 1)

    def center_crop(self, x, y):
        """Crop the longer of two [B, C, T, F] tensors around its centre (metrics.py:32-49; unused there)."""
        d = x.size(2) - y.size(2)
        if d == 0:
            return x, y
        assert abs(d) < 10, "Error: the offset %s is too large, check the code please" % (abs(d))
        a = abs(d) // 2
        b = abs(d) - a
        if d > 0:
            return x[:, :, a:x.size(2) - b, :], y
        return x, y[:, :, a:y.size(2) - b, :]
