"""SSR_Eval_Helper / BasicTestee - drop-in for ssr_eval.eval (ssr_eval/eval.py:17-421) on MI355X.

Constructor arguments, method names, degradation keys (``proc_fft_<2*cutoff>_<sr>`` ...), the in-place
doubling of the caller's ``cutoff_freq`` lists, the mean-of-speaker-means aggregation and the result JSON
schema follow the reference.  What changes is the execution model: instead of a serial loop that calls
librosa / skimage once per (utterance, degradation), the helper gathers every (processed, target) pair of
a speaker and dispatches ONE batched, ragged HIP launch sequence for each of
degradation (K6 / K7) -> user ``infer`` -> resample to the evaluation rate (K7) -> four metrics (K1-K5),
and shards utterances across ranks when torch.distributed is initialised (ssr_eval_amd.dist).

File decoding / sox resampling are host I/O (ssr_eval_amd.io).  For data already in
memory use ``evaluate_arrays``.
"""
import collections
import numbers
import os

import numpy as np
import torch

from . import backend as B
from . import dist as D
from .lowpass import lowpass, lowpass_batch, lowpass_iir_multi, stft_hard_lowpass_multi
from .metrics import AudioMetrics, which_mask, _BSS_NAMES, _COH_HF_NAMES, _COH_NAMES, _CSII_NAMES, _LOUD_DIFF_NAMES, _LOUD_NAMES, _MEL_DTW_NAMES, _MEL_NAMES, _MRSTFT_NAMES, \
    _MOD_NAMES, _NMR_NAMES, _NSIM_NAMES, _PHASE_NAMES, _PITCH_NAMES, _QUALITY_NAMES, _SPEC_NAMES, _SPEC_PAIR_NAMES, _WAVE_NAMES
from .distribution import check_option as check_distribution_option, embed_waves, result_block as distribution_block
from .stats import bootstrap_ci, bootstrap_option
from .utils import dict_mean, write_json

# the reference's four, then the band-split LSD of SSR_Eval_Helper(lsd_split=...) and the intelligibility of
# SSR_Eval_Helper(stoi=...) (only present in runs that ask for them)
_METRIC_KEYS = ("lsd", "log_sispec", "sispec", "ssim", "lsd_lf", "lsd_hf", "stoi", "estoi")
# SSR_Eval_Helper(stoi=...) -> AudioMetrics.stoi_* `extended`
_STOI_OPTIONS = {"stoi": False, "estoi": True, "both": "both"}
# the keys of the other families (only present in runs that ask for them).  dtw_len, a count of path cells, is not a per-key
# result: its mean over files of different lengths says nothing
_WAVEFORM_KEYS, _MEL_KEYS, _MEL_DTW_KEYS, _QUALITY_KEYS, _PITCH_KEYS = _WAVE_NAMES, _MEL_NAMES, _MEL_DTW_NAMES[:2], _QUALITY_NAMES, _PITCH_NAMES
_PHASE_KEYS, _MRSTFT_KEYS, _BSS_KEYS = _PHASE_NAMES, _MRSTFT_NAMES, _BSS_NAMES
_COH_KEYS = _COH_NAMES + _COH_HF_NAMES
# the loudness range stays out of a key's result: it is NaN for files under 3 s and the aggregate is a plain mean
_LOUD_KEYS = (_LOUD_NAMES[0], _LOUD_DIFF_NAMES[0], _LOUD_NAMES[5], _LOUD_DIFF_NAMES[2])
# of the spectrum family a key's result keeps the output's bandwidth, its difference to the target's, the HF level difference and the
# third-octave LTAS distance
_BW_KEYS = (_SPEC_NAMES[0], _SPEC_PAIR_NAMES[0], _SPEC_PAIR_NAMES[3], _SPEC_PAIR_NAMES[4])
# of the auditory family a key's result keeps the similarity over all bands and over the bands above the key's cutoff
_AUD_KEYS = _NSIM_NAMES[:2]
# of the modulation family a key's result keeps the output's SRMR, its difference to the target's and the modulation-spectrum
# distance over all bands and over the bands above the key's cutoff
_MOD_KEYS = _MOD_NAMES[:4]
# of the csii family a key's result keeps the index over all segments, over the mid-level ones, the fitted I3 and the index over the
# critical bands at or above the key's cutoff
_CSII_KEYS = (_CSII_NAMES[0], _CSII_NAMES[2], _CSII_NAMES[4], _CSII_NAMES[5])
# of the nmr family a key's result keeps the total noise-to-mask ratio, the share of disturbed frames and the ratio over the bands at
# or above the key's cutoff
_NMR_KEYS = (_NMR_NAMES[0], _NMR_NAMES[2], _NMR_NAMES[3])


def _option_dict(value):
    """The dict form of a family option: True -> every metric, a name or a tuple of names -> those, a dict -> itself."""
    return value if isinstance(value, dict) else {"which": "all" if value is True else value}


def _which_option(option, value, names, entries):
    """ValueError unless `value` is one of `names`, "all", a non-empty tuple of names, or a non-empty dict of 'which' and / or
    `entries`."""
    if isinstance(value, dict) and (not value or set(value) - {"which", *entries}):
        takes = ["'%s'" % k for k in ("which",) + tuple(entries)]
        raise ValueError("a %s dict takes %s and / or %s" % (option, ", ".join(takes[:-1]), takes[-1]))
    w = _option_dict(value).get("which", "all")
    if not (isinstance(w, str) or (isinstance(w, tuple) and w and all(isinstance(m, str) for m in w))):
        raise ValueError("%s must be None, True, one of %s, a tuple of them or a dict" % (option, names))
    which_mask(w, names)


# What a family's check refuses as the `split` of its option dict, beyond what its AudioMetrics._*_splits refuses (with a message of
# its own) when the check passes the value on.  The rules differ and are behaviour: each family keeps its own.
_SPLIT_REFUSED = {
    "coherence": lambda s: s is None,
    "bandwidth": lambda s: s is None or isinstance(s, (bool, str, list, tuple, dict)),
    "auditory": lambda s: not B._is_number(s),
    "modulation": lambda s: not B._is_number(s),
    "csii": lambda s: not B._is_number(s),
    "nmr": lambda s: not B._is_number(s),
}


def _dict_option(option, v, names):
    """ValueError unless `v`, the value of `option`, is True or a non-empty dict of `names` with a `split`, if any, the family takes."""
    if v is not True and (not isinstance(v, dict) or not v or set(v) - set(names)):
        takes = ["'%s'" % k for k in names]
        raise ValueError("%s must be None, True or a dict of %s and / or %s" % (option, ", ".join(takes[:-1]), takes[-1]))
    if v is not True and "split" in v and _SPLIT_REFUSED[option](v["split"]):
        raise ValueError("split must be a frequency in Hz (leave it out to split every key at its own cutoff)")


def _key_splits(q, keys):
    """One split frequency per degradation key: `split` Hz of the option dict q for every key where it names one, else the key's
    own cutoff (key_cutoff_hz; None for mp3 keys)."""
    return [float(q["split"])] * len(keys) if "split" in q else [key_cutoff_hz(k) for k in keys]


# A family's two functions: check(helper, value) raises ValueError for a value of the option the family does not take (it sees
# every value but None: None is "off"), arguments(helper, degradation keys of the call) -> the (positional, keyword) arguments of
# the family's AudioMetrics methods after the signals.  Where both need an option's defaults, *_args spells them out once.
def _lsd_split_check(h, v):
    if not (v is True or (isinstance(v, numbers.Real) and not isinstance(v, bool))):
        raise ValueError("lsd_split must be None, True or a split frequency in Hz")


def _stoi_check(h, v):
    if not (isinstance(v, str) and v in _STOI_OPTIONS):
        raise ValueError("stoi must be None, 'stoi', 'estoi' or 'both'")


def _waveform_check(h, v):
    try:                                       # True, a name or a tuple of names: no "all", no list, no dict
        ok = v is True or (isinstance(v, (str, tuple)) and v != "all" and which_mask(v, _WAVEFORM_KEYS) > 0)
    except ValueError:
        ok = False
    if not ok:
        raise ValueError("waveform must be None, True, one of %s or a tuple of them" % (_WAVEFORM_KEYS,))


def _mel_args(v):
    q = _option_dict(v)
    return (q.get("which", "all"),), {k: o for k, o in q.items() if k != "which"}


def _mel_check(h, v):
    if not (v is True or isinstance(v, dict)):
        raise ValueError("mel must be None, True or a dict of mel options")
    if isinstance(v, dict):                        # every option checked here, not at the first batch
        (which,), opts = _mel_args(v)
        which_mask(which, _MEL_KEYS)
        h.audio_metrics._mel_fb(**opts)


def _mel_dtw_args(v, **more):
    q = dict(v) if isinstance(v, dict) else {}
    return (q.pop("radius", 16),), dict(q, **more)


def _mel_dtw_check(h, v):
    if not (v is True or isinstance(v, dict)):
        raise ValueError("mel_dtw must be None, True or a dict of `radius` and mel options")
    (radius,), opts = _mel_dtw_args(v)             # every option checked here, not at the first batch
    AudioMetrics.dtw_radius(radius)
    h.audio_metrics._mel_fb(**opts)


def _quality_args(v):
    q = _option_dict(v)
    return q.get("which", "all"), q.get("lpc_order")


def _quality_check(h, v):
    if v is not True:
        _which_option("quality", v, _QUALITY_KEYS, ("lpc_order",))
        AudioMetrics._quality_order(_quality_args(v)[1])
        if h.evaluationset_sr < 8000:
            raise ValueError("the quality measures need evaluation_sr >= 8000")


def _pitch_args(v):
    q = _option_dict(v)
    return q.get("which", "all"), q.get("fmin", 50.0), q.get("fmax", 500.0)


def _pitch_check(h, v):
    if v is not True:
        _which_option("pitch", v, _PITCH_KEYS, ("fmin", "fmax"))
        AudioMetrics._pitch_range(*_pitch_args(v)[1:])
    if not 8000 <= h.evaluationset_sr <= 48000:
        raise ValueError("the pitch metrics need 8000 <= evaluation_sr <= 48000")


def _phase_args(v):
    q = _option_dict(v)
    return q.get("which", "all"), q.get("n_fft", 1024), q.get("hop"), q.get("band")


def _phase_check(h, v):
    if v is not True:
        _which_option("phase", v, _PHASE_KEYS, ("n_fft", "hop", "band"))
        _, n_fft, hop, band = _phase_args(v)
        AudioMetrics._phase_bins(h.evaluationset_sr, B.check_phase_frames(n_fft, hop)[0], band)


def _mrstft_args(v):
    q = v if isinstance(v, dict) else {}
    return q.get("resolutions"), q.get("band"), q.get("eps", B.MRSTFT_EPS)


def _mrstft_check(h, v):
    _dict_option("mrstft", v, ("resolutions", "band", "eps"))
    if v is not True:
        resolutions, band, eps = _mrstft_args(v)
        B.check_mrstft_eps(eps)
        AudioMetrics._mrstft_bins(h.evaluationset_sr, B.check_mrstft_resolutions(resolutions), band)


def _bss_taps(h, v):
    """ValueError unless `v` is True or {"taps": an integer in [1, 512]}; -> the tap count."""
    if v is True:
        return B.BSS_TAPS
    if not isinstance(v, dict) or set(v) != {"taps"}:
        raise ValueError("bss_sdr must be None, True or a dict of 'taps'")
    return B.check_bss_taps(v["taps"])


# The optional metric families in the order they are queued on the stream and their keys appear in a result.  option: the
# SSR_Eval_Helper argument; multi / batch: the AudioMetrics methods for K keys per file / for a flat list of pairs; keys: what the
# family adds to a key's result; check, arguments: above; per_key: the arguments hold one value per degradation key - such a family
# takes the multi path only when every file has the same keys.
_Family = collections.namedtuple("_Family", "option multi batch keys check arguments per_key")
_FAMILIES = (
    _Family("lsd_split", "lsd_split_multi", "lsd_split_batch", _METRIC_KEYS[4:6], _lsd_split_check,
            lambda h, keys: (([h.split_cutoff_hz(k) for k in keys],), {}), True),
    _Family("stoi", "stoi_multi", "stoi_batch", _METRIC_KEYS[6:8], _stoi_check, lambda h, keys: ((_STOI_OPTIONS[h.stoi],), {}), False),
    _Family("waveform", "waveform_multi", "waveform_batch", _WAVEFORM_KEYS, _waveform_check,
            lambda h, keys: ((_option_dict(h.waveform)["which"],), {}), False),
    _Family("mel", "mel_distance_multi", "mel_distance_batch", _MEL_KEYS, _mel_check, lambda h, keys: _mel_args(h.mel), False),
    _Family("mel_dtw", "mel_dtw_multi", "mel_dtw_batch", _MEL_DTW_KEYS, _mel_dtw_check,
            lambda h, keys: _mel_dtw_args(h.mel_dtw, lengths=False), False),
    _Family("quality", "quality_multi", "quality_batch", _QUALITY_KEYS, _quality_check, lambda h, keys: (_quality_args(h.quality), {}), False),
    _Family("pitch", "pitch_multi", "pitch_batch", _PITCH_KEYS, _pitch_check, lambda h, keys: (_pitch_args(h.pitch), {}), False),
    _Family("phase", "phase_distance_multi", "phase_distance_batch", _PHASE_KEYS, _phase_check, lambda h, keys: (_phase_args(h.phase), {}), False),
    _Family("mrstft", "mrstft_multi", "mrstft_batch", _MRSTFT_KEYS, _mrstft_check, lambda h, keys: (_mrstft_args(h.mrstft), {}), False),
    _Family("bss_sdr", "bss_sdr_multi", "bss_sdr_batch", _BSS_KEYS, _bss_taps, lambda h, keys: ((_bss_taps(h, h.bss_sdr),), {}), False),
)


def result_key_order():
    """Every built-in metric key in the order a result lists them: the reference's four, then each family's."""
    return _METRIC_KEYS[:4] + tuple(k for f in _FAMILIES for k in f.keys)


def _coherence_args(h, v, keys):
    """-> (n_fft, hop, band, one split frequency per degradation key (_key_splits; None: NaN values), threshold)."""
    q = v if isinstance(v, dict) else {}
    return q.get("n_fft", 1024), q.get("hop"), q.get("band"), _key_splits(q, keys), q.get("threshold", B.COHERENCE_THRESHOLD)


def _coherence_check(h, v):
    _dict_option("coherence", v, ("n_fft", "hop", "band", "threshold", "split"))
    if v is not True:
        n_fft, hop, band, split, thr = _coherence_args(h, {k: o for k, o in v.items() if k != "split"}, ["k"])
        B.check_coherence_threshold(thr)
        h.audio_metrics._coh_bands(B.check_coherence_frames(n_fft, hop)[0], band, v.get("split"), 1)


# The families added after the registry above was pinned by its tests: queued after _FAMILIES, their keys behind its keys.
_LATER_FAMILIES = (
    _Family("coherence", "coherence_multi", "coherence_batch", _COH_KEYS, _coherence_check,
            lambda h, keys: (_coherence_args(h, h.coherence, keys), {}), True),
)


def all_key_order():
    """result_key_order() and the keys of the later families behind it (full_key_order() adds the tail families')."""
    return result_key_order() + tuple(k for f in _LATER_FAMILIES for k in f.keys)


def _loudness_check(h, v):
    if v is not True:
        raise ValueError("loudness must be None or True")
    B.check_loudness_rate(h.evaluationset_sr)


def _bandwidth_args(h, v, keys):
    """-> ((n_fft, hop, band, one split frequency per degradation key (_key_splits; None: NaN hf_diff), rolloff, drop_db), {"names":
    the family's keys})."""
    q = v if isinstance(v, dict) else {}
    return ((q.get("n_fft", 2048), q.get("hop"), q.get("band"), _key_splits(q, keys), q.get("rolloff", B.SPECTRUM_ROLLOFF), q.get("drop_db", B.SPECTRUM_DROP_DB)),
            {"names": _BW_KEYS})


def _bandwidth_check(h, v):
    _dict_option("bandwidth", v, ("n_fft", "hop", "band", "split", "rolloff", "drop_db"))
    (n_fft, hop, band, split, rho, drop), _ = _bandwidth_args(h, v, ["k"])
    n_fft, hop = B.check_coherence_frames(n_fft, hop)
    B.check_spectrum_rolloff(rho)
    B.check_spectrum_drop(drop)
    h.audio_metrics._ltas_bands(h.evaluationset_sr, n_fft, band)
    h.audio_metrics._bandwidth_splits(n_fft, split, 1)


def _auditory_args(h, v, keys):
    """-> ((one split frequency per degradation key (_key_splits; None: NaN nsim_hf), n_bands, band, range_db, match_level), {"names":
    the family's keys})."""
    q = v if isinstance(v, dict) else {}
    return ((_key_splits(q, keys), q.get("n_bands", B.AUDITORY_N_BANDS), q.get("band"), q.get("range_db", B.AUDITORY_RANGE_DB), q.get("match_level", True)),
            {"names": _AUD_KEYS})


def _auditory_check(h, v):
    _dict_option("auditory", v, ("n_bands", "band", "range_db", "split", "match_level"))
    (split, n_bands, band, range_db, match), _ = _auditory_args(h, v, ["k"])
    fc, _ = B.gammatone_design(h.evaluationset_sr, n_bands, band)
    B.check_auditory_range(range_db)
    if not isinstance(match, bool):
        raise ValueError("match_level must be True or False")
    h.audio_metrics._nsim_splits(fc, split, 1)


def _modulation_args(h, v, keys):
    """-> ((one split frequency per degradation key (_key_splits; None: NaN mod_dist_hf), n_bands, band, env_rate, range_db, kstar),
    {"names": the family's keys})."""
    q = v if isinstance(v, dict) else {}
    return ((_key_splits(q, keys), q.get("n_bands", B.AUDITORY_N_BANDS), q.get("band"), q.get("env_rate", B.MODULATION_ENV_RATE),
             q.get("range_db", B.MODULATION_RANGE_DB), q.get("kstar")), {"names": _MOD_KEYS})


def _modulation_check(h, v):
    _dict_option("modulation", v, ("n_bands", "band", "env_rate", "range_db", "kstar", "split"))
    if v is not True and "kstar" in v and v["kstar"] is None:
        raise ValueError("kstar must be an integer in [5, 8] (leave it out for the adaptive table)")
    (split, n_bands, band, env_rate, range_db, kstar), _ = _modulation_args(h, v, ["k"])
    fc, _, _ = h.audio_metrics._modulation_design(n_bands, band, env_rate, range_db, kstar)
    h.audio_metrics._modulation_splits(fc, split, 1)


# The third tuple of the registry: queued after the two tuples above, its keys behind theirs.  It is closed - the tests of its
# families pin its four rows, and those of the auditory family its two keys as the end of full_key_order(); a new family's row goes
# into _NEWER_FAMILIES below.
_TAIL_FAMILIES = (
    _Family("loudness", "loudness_multi", "loudness_batch", _LOUD_KEYS, _loudness_check, lambda h, keys: ((), {"names": _LOUD_KEYS}), False),
    _Family("bandwidth", "bandwidth_multi", "bandwidth_batch", _BW_KEYS, _bandwidth_check,
            lambda h, keys: _bandwidth_args(h, h.bandwidth, keys), True),
    _Family("modulation", "modulation_multi", "modulation_batch", _MOD_KEYS, _modulation_check,
            lambda h, keys: _modulation_args(h, h.modulation, keys), True),
    _Family("auditory", "nsim_multi", "nsim_batch", _AUD_KEYS, _auditory_check, lambda h, keys: _auditory_args(h, h.auditory, keys), True),
)


def full_key_order():
    """all_key_order() and the keys of the tail families behind it: the order a result lists its metrics in."""
    return all_key_order() + tuple(k for f in _TAIL_FAMILIES for k in f.keys)


def _csii_args(h, v, keys):
    """-> ((one split frequency per degradation key (_key_splits; None: NaN csii_hf), n_fft, hop, band), {"names": the family's keys})."""
    q = v if isinstance(v, dict) else {}
    return (_key_splits(q, keys), q.get("n_fft"), q.get("hop"), q.get("band")), {"names": _CSII_KEYS}


def _csii_check(h, v):
    _dict_option("csii", v, ("n_fft", "hop", "band", "split"))
    if v is not True and "n_fft" in v and v["n_fft"] is None:
        raise ValueError("n_fft must be one of %s (leave it out for 16 ms segments)" % (B.PHASE_N_FFTS,))
    (split, n_fft, hop, band), _ = _csii_args(h, v, ["k"])
    _, _, fc = h.audio_metrics._csii_design(n_fft, hop, band)
    h.audio_metrics._csii_splits(fc, split, 1)


# The open end of the registry: the families added after _TAIL_FAMILIES was pinned, queued after it, their keys behind its keys.  A
# new family's row goes at the end.
_NEWER_FAMILIES = (
    _Family("csii", "csii_multi", "csii_batch", _CSII_KEYS, _csii_check, lambda h, keys: _csii_args(h, h.csii, keys), True),
)
_ALL_FAMILIES = _FAMILIES + _LATER_FAMILIES + _TAIL_FAMILIES + _NEWER_FAMILIES


def every_key_order():
    """full_key_order() and the keys of the newer families behind it: the order a result lists its metrics in."""
    return full_key_order() + tuple(k for f in _NEWER_FAMILIES for k in f.keys)


def _nmr_args(h, v, keys):
    """-> ((one split frequency per degradation key (_key_splits; None: NaN nmr_hf), n_fft, level_db), {"names": the family's keys})."""
    q = v if isinstance(v, dict) else {}
    return (_key_splits(q, keys), q.get("n_fft"), q.get("level_db", B.NMR_LEVEL_DB)), {"names": _NMR_KEYS}


def _nmr_check(h, v):
    _dict_option("nmr", v, ("n_fft", "level_db", "split"))
    if v is not True and "n_fft" in v and v["n_fft"] is None:
        raise ValueError("n_fft must be one of %s (leave it out for 32 ms frames)" % (B.PHASE_N_FFTS,))
    (split, n_fft, level_db), _ = _nmr_args(h, v, ["k"])
    h.audio_metrics._nmr_splits(h.audio_metrics._nmr_design(n_fft, level_db)["fc"], split, 1)


# The families behind the 16 of _ALL_FAMILIES, whose count and 56 keys the tests pin: queued after them, their keys behind
# every_key_order() and in front of ALIGN_KEYS.  A new family's row goes at the end.
_OPEN_FAMILIES = (
    _Family("nmr", "nmr_multi", "nmr_batch", _NMR_KEYS, _nmr_check, lambda h, keys: _nmr_args(h, h.nmr, keys), True),
)


def open_key_order():
    """every_key_order(), the keys of the open families and ALIGN_KEYS behind it: the order a result lists its metrics in."""
    return every_key_order() + tuple(k for f in _OPEN_FAMILIES for k in f.keys) + ALIGN_KEYS


# The delay stage of SSR_Eval_Helper(align=...) is no registry family: it runs in front of the metrics and changes what they see.  What
# it adds to a key's result sits behind the families' keys: the delay taken out, in samples at evaluation_sr, and the normalised
# correlation at that delay.
ALIGN_KEYS = ("delay", "align_corr")


def _align_option(v):
    """(max_lag, subsample) of the `align` option, or ValueError: True, or a non-empty dict of 'max_lag' and / or 'subsample'."""
    if v is not True and (not isinstance(v, dict) or not v or set(v) - {"max_lag", "subsample"}):
        raise ValueError("align must be None, True or a dict of 'max_lag' and / or 'subsample'")
    q = v if isinstance(v, dict) else {}
    return B.check_align_lag(q.get("max_lag", B.ALIGN_LAG)), B.check_align_subsample(q.get("subsample", False))


def key_cutoff_hz(key):
    """Cutoff in Hz of a degradation key: the integer after the tag, floor-divided by 2 - what preprocess passed to lowpass()
    (proc_bw_8000_4_44100 -> 4000, proc_fft_44099_44100 -> 22049: the sr - 1 quirk).  proc_mp3_* carries none: None."""
    parts = key.split("_")
    if len(parts) < 4 or parts[0] != "proc" or parts[1] == "mp3":
        return None
    return int(parts[2]) // 2


def pipeline_batches(paths, step):
    """The file batches of one evaluate() pass: `step` files per launch sequence, except that the first two batches hold a quarter
    and a half of `step` (pipeline fill: the GPU has work after a quarter of a batch's file reads and bus transfer).  Per-file
    results do not depend on how the files are batched."""
    batches, b = [], 0
    for size in (max(1, step // 4), max(1, step // 2)):
        if len(paths) - b > step:
            batches.append(paths[b:b + size]); b += size
    return batches + [paths[c:c + step] for c in range(b, len(paths), step)]


class BasicTestee:
    """Plugin base class (ssr_eval/eval.py:17-52): subclass and override ``infer``."""

    def __init__(self) -> None:
        pass

    def _find_cutoff(self, x, threshold=0.95):
        """Largest index (scanning from the top) whose cumulative energy is below threshold * total;
        integer, bit-exact with eval.py:21-26."""
        limit = x[-1] * threshold
        n = x.shape[0]
        below = np.nonzero(np.asarray(x[1:][::-1]) < limit)[0]     # x[-1], x[-2], ..., x[1]
        return n - (int(below[0]) + 1) if below.size else 0

    def _stft_mag_complex(self, x):
        plan = B.get_plan(2048, 512)                               # librosa.stft defaults (eval.py:29,37-38)
        re, im = B.stft(plan, [np.asarray(x, np.float32)], kind="complex")
        return re[0], im[0]                                        # [T, F] device tensors

    def _get_cutoff_index(self, x):
        """eval.py:28-31: np.cumsum(np.sum(np.abs(librosa.stft(x)), axis=-1)) -> _find_cutoff(., 0.97).  The magnitudes are the
        metric path's (ssr_stft, MAG: abs of the complex64 spectrum, float32); the 1,025 x T floats are summed ON THE HOST by the
        reference's own NumPy calls on the reference's [F, T] layout - np.sum's pairwise float32 summation over the frames of a bin,
        np.cumsum's sequential one over the bins - so that a threshold crossing cannot move by a bin because a GPU reduction added
        the same numbers in another order (N3 is not a hot path)."""
        plan = B.get_plan(2048, 512)                               # librosa.stft defaults
        mag = B.stft(plan, [np.asarray(x, np.float32)], kind="mag")[0]          # [T, F] float32 on the device
        stft_x = np.ascontiguousarray(mag.cpu().numpy().T)         # [F, T], as np.abs(librosa.stft(x))
        energy = np.cumsum(np.sum(stft_x, axis=-1))
        return self._find_cutoff(energy, 0.97)

    def postprocessing(self, x, out):
        """Replace the bins below the detected cutoff of `out` with those of `x` (eval.py:33-41)."""
        length = out.shape[0]
        k = self._get_cutoff_index(x)
        re_x, im_x = self._stft_mag_complex(x)
        re_o, im_o = self._stft_mag_complex(out)
        if re_x.shape != re_o.shape:
            raise ValueError("postprocessing needs x and out of equal length (the reference assigns whole bin rows)")
        re_o[:, :k], im_o[:, :k] = re_x[:, :k], im_x[:, :k]
        # librosa.istft(length=length): hop 512 synthesis, sum-of-squared-window normalisation
        return B.istft(B.get_plan(2048, 512), [re_o], [im_o], [length])[0].cpu().numpy()

    def tensor2numpy(self, tensor):
        return tensor.detach().cpu().numpy()                       # device.type check instead of a string match

    def infer(self, x):
        return x


class SSR_Eval_Helper:
    def __init__(self, testee, input_sr, output_sr, evaluation_sr=44100, test_name="test",
                 test_data_root="./datasets/vctk_test", setting_lowpass_filtering=None, setting_subsampling=None,
                 setting_fft=None, setting_mp3_compression=None, save_processed_result=False, *,
                 precision="f64", device=None, download=False, lsd_split=None, stoi=None, waveform=None, mel=None,
                 quality=None, pitch=None, iir_exact=True, bootstrap=None, mel_dtw=None, phase=None, mrstft=None, bss_sdr=None,
                 distribution=None, coherence=None, align=None, nmr=None, csii=None, auditory=None, modulation=None, loudness=None, bandwidth=None):
        """lsd_split (not in the reference): None = off; True = every key also gets lsd_lf / lsd_hf, the LSD below / above its own
        cutoff (key_cutoff_hz; mp3 keys: NaN); a number = the same split frequency in Hz for every key, mp3 included.
        stoi (not in the reference): None = off; "stoi", "estoi" or "both" = every key also gets that intelligibility score
        (AudioMetrics.stoi_multi / stoi_batch at evaluation_sr).
        waveform (not in the reference): None = off; True = every key also gets snr / si_sdr / seg_snr; one of those names or a
        tuple of them = those (AudioMetrics.waveform_multi / waveform_batch at evaluation_sr).
        mel (not in the reference): None = off; True = every key also gets mel_lsd / mel_l1 / mcd (AudioMetrics.mel_distance_multi /
        mel_distance_batch at evaluation_sr, NVSR's 128-band HTK front end); a dict = front-end options (n_mels, f_min, f_max, norm,
        mel_scale, n_cep) and optionally `which` ("all", one of those names or a tuple of them).
        mel_dtw (not in the reference): None = off; True = every key also gets mcd_dtw / dtw_dev, the mel-cepstral distortion along
        the best warp of the estimate's frames onto the target's inside a band of 16 frames and that warp's mean drift in frames
        (AudioMetrics.mel_dtw_multi / mel_dtw_batch at evaluation_sr); a dict = `radius` (0..31 frames) and / or
        the mel front-end options (n_mels, f_min, f_max, norm, mel_scale, n_cep).
        quality (not in the reference): None = off; True = every key also gets llr / cep_dist / wss / fwseg_snr
        (AudioMetrics.quality_multi / quality_batch at evaluation_sr; wss and fwseg_snr look at the band below about 3.9 kHz only);
        one of those names or a tuple of them = those; a dict = `which` ("all", a name or a tuple) and / or `lpc_order`.
        pitch (not in the reference): None = off; True = every key also gets f0_rmse / f0_corr / gpe / vde / ffe of the estimate's
        YIN F0 track against the target's (AudioMetrics.pitch_multi / pitch_batch at evaluation_sr, tracked at 16 kHz); one of those
        names or a tuple of them = those; a dict = `which` ("all", a name or a tuple) and / or the search range `fmin`, `fmax` (Hz,
        default 50 and 500).
        phase (not in the reference): None = off; True = every key also gets phase_ip / phase_gd / phase_iaf, the anti-wrapping
        instantaneous-phase, group-delay and instantaneous-angular-frequency distances in radians (AudioMetrics.phase_distance_multi /
        phase_distance_batch at evaluation_sr); one of those names or a tuple of them = those; a dict = `which`
        ("all", a name or a tuple) and / or `n_fft` (256, 512, 1024 or 2048; default 1024), `hop` (default n_fft // 4) and `band`
        ((lo_hz, hi_hz), the band scored; default every bin).
        mrstft (not in the reference): None = off; True = every key also gets mrstft_sc / mrstft_mag / mrstft, the spectral
        convergence and the log-magnitude distance of Parallel WaveGAN's multi-resolution STFT loss averaged over its three
        resolutions, and their sum (AudioMetrics.mrstft_multi / mrstft_batch at evaluation_sr); a dict =
        `resolutions` (up to 8 (n_fft, hop, win) in samples), `band` ((lo_hz, hi_hz), the band scored) and / or `eps`.
        bss_sdr (not in the reference): None = off; True = every key also gets sdr / sdr_lag, BSS Eval's SDR in dB with a causal
        512-tap FIR filter of the target as the allowed distortion - a delay or a colouring of the output costs nothing - and the
        tap of that filter's largest coefficient, the output's latency in samples (AudioMetrics.bss_sdr_multi / bss_sdr_batch at
        evaluation_sr); a dict = `taps` (1 .. 512).
        distribution (not in the reference): None = off, the result, its JSON and the launch sequence are what they are without the
        option; True = evaluate() adds result["distribution"] = {"settings": {...}, "dim": D, "n": files, "per_key": {key: {"fd", "kd"}}},
        the Fréchet distance and the kernel distance (unbiased MMD^2 x 1000) between the SET of a key's outputs and the set of
        targets (ssr_eval_amd.distribution) - corpus-level, not per file: per-file entries, each_speaker,
        averaged and confidence are unchanged to the bit.  Each file contributes one embedding vector for its target and one per
        key: the built-in log-mel statistics (distribution.embed_logmel_stats; fd on it is NOT comparable with published VGGish /
        CLAP FAD figures), or a dict's `embed`: a callable (waves: list of 1-D tensors at evaluation_sr, sr) -> [len(waves), D];
        further dict keys: `bandwidth` ("median" or the kernel's sigma), `scale`, `max_sweeps`, `metrics` (a subset of ("fd", "kd")).
        coherence (not in the reference): None = off; True = every key also gets msc / coh_sdr / coh_bw, the mean Welch-averaged
        magnitude-squared coherence of the output with the target, the power of the output that is a linear function of the target
        over the power that is not, in dB, and the width in Hz of the bins with a coherence of at least 0.5 - and msc_hf /
        coh_sdr_hf, the first two above the key's own cutoff (key_cutoff_hz; mp3 keys: NaN) (AudioMetrics.coherence_multi /
        coherence_batch at evaluation_sr); a dict = `n_fft` (256, 512, 1024 or 2048; default 1024), `hop`
        (default n_fft // 2), `band` ((lo_hz, hi_hz), the band scored), `threshold` (of coh_bw, in (0, 1]) and / or `split` (the
        same split frequency in Hz for every key, mp3 included).
        loudness (not in the reference): None = off; True = every key also gets lufs / true_peak_db, the gated integrated loudness
        (ITU-R BS.1770-4) in LUFS and the 4x oversampled peak in dBTP of the output, and lufs_diff / true_peak_diff, those minus the
        target's - a testee that rescales or clips its output shows here, whatever the level-sensitive keys say
        (AudioMetrics.loudness_multi / loudness_batch at evaluation_sr, an integer in 8000 .. 192000 Hz).  A
        file shorter than 400 ms, or below -70 LUFS throughout, has NaN for lufs and lufs_diff.
        bandwidth (not in the reference): None = off; True = every key also gets bw_hz, the frequency below which 0.97 of the output's
        summed spectral magnitudes lies (BasicTestee's cutoff rule as a metric), bw_diff, that minus the target's, hf_diff, the
        output's power above the key's own cutoff relative to its total minus the target's, in dB (key_cutoff_hz; mp3 keys and keys
        with no bin above the cutoff: NaN), and ltas_dist, the RMS difference in dB of the two long-term average spectra in
        third-octave bands - all invariant to gain (AudioMetrics.bandwidth_multi / bandwidth_batch at evaluation_sr, DESIGN.md
        section 22); a dict = `n_fft` (256, 512, 1024 or 2048; default 2048), `hop` (default n_fft // 2), `band` ((lo_hz, hi_hz), the
        band scored), `split` (the same split frequency in Hz for every key, mp3 included), `rolloff` (in (0, 1)) and / or `drop_db`.
        auditory (not in the reference): None = off; True = every key also gets nsim, the neurogram similarity index of the output's
        and the target's gammatone spectrograms (Hines & Harte 2012; 1 = identical images), and nsim_hf, the same over the bands
        whose centre frequency is at or above the key's own cutoff (key_cutoff_hz; mp3 keys and keys with no band above the cutoff:
        NaN) - invariant to the output's gain (AudioMetrics.nsim_multi / nsim_batch at evaluation_sr); a dict =
        `n_bands` (3 to 64; default 32), `band` ((lo_hz, hi_hz) of the centre frequencies; default 50 Hz to 0.45 evaluation_sr),
        `range_db` (default 60), `split` (the same split frequency in Hz for every key, mp3 included) and / or `match_level`.
        modulation (not in the reference): None = off; True = every key also gets srmr, the output's speech-to-reverberation
        modulation energy ratio (Falk, Zheng & Chan 2010; needs no target: high for clean speech, low for reverberation and for
        stationary texture), srmr_diff, that minus the target's, mod_dist, the RMS difference in dB of the output's and the target's
        modulation spectra (32 gammatone bands x 8 modulation bands from 4 to 128 Hz), and mod_dist_hf, the same over the bands
        whose centre frequency is at or above the key's own cutoff (key_cutoff_hz; mp3 keys and keys with no band above the cutoff:
        NaN) - all invariant to the output's gain (AudioMetrics.modulation_multi / modulation_batch at evaluation_sr, DESIGN.md
        section 24); a dict = `n_bands` (3 to 64; default 32), `band` ((lo_hz, hi_hz) of the centre frequencies), `env_rate` (800 to
        6400 Hz; default 1600), `range_db` (default 60), `kstar` (5 .. 8: a constant upper band instead of the adaptive one) and / or
        `split` (the same split frequency in Hz for every key, mp3 included).
        csii (not in the reference): None = off; True = every key also gets csii, the coherence speech intelligibility index of the
        output against the target (Kates & Arehart 2005: the coherence signal-to-distortion ratio per critical band up to 8.5 kHz,
        weighted with the band importance of ANSI S3.5-1997; 1 = the output is a linear function of the target), csii_mid, the same
        over the target's mid-level segments, i3, the intelligibility fitted to the low- and mid-level values, and csii_hf, csii
        over the bands whose centre is at or above the key's own cutoff (key_cutoff_hz; mp3 keys and keys with no band above the
        cutoff: NaN) - all invariant to the output's gain (AudioMetrics.csii_multi / csii_batch at evaluation_sr, DESIGN.md section
        26); a dict = `n_fft` (256, 512, 1024 or 2048; default 16 ms), `hop` (default n_fft // 2), `band` ((lo_hz, hi_hz) of the band
        centres kept) and / or `split` (the same split frequency in Hz for every key, mp3 included).
        nmr (not in the reference): None = off; True = every key also gets nmr, the total noise-to-mask ratio of the output against
        the target in dB (the error spectrum per quarter-Bark band over the masking threshold the target itself produces - the FFT
        ear model of ITU-R BS.1387, restated; negative = masked), rdf, the share of frames with a band at least 1.5 dB over the
        threshold, and nmr_hf, nmr over the bands whose centre is at or above the key's own cutoff (key_cutoff_hz; mp3 keys and
        keys with no band above the cutoff: NaN) (AudioMetrics.nmr_multi / nmr_batch at evaluation_sr); a
        dict = `n_fft` (256, 512, 1024 or 2048; default 32 ms), `level_db` (the level of a full-scale sine in dB SPL; default 92)
        and / or `split` (the same split frequency in Hz for every key, mp3 included).  Its keys sit behind those of every other
        family.
        align (not in the reference): None = off, the result, its JSON and the launch sequence are what they are without the option;
        True = the delay of every output against its target is searched within 1024 samples either way and taken out before any
        metric sees the output (AudioMetrics.align_batch at evaluation_sr, after the resampling): the shift
        is a copy by whole samples, zero-filled at the edge the output is moved away from, the target is never cropped, and every
        key also gets delay, the delay taken out in samples (positive: the output was late), and align_corr, the normalised
        cross-correlation at that delay (NaN for digital silence: nothing is shifted); a dict = `max_lag` (1 .. 4096 samples) and /
        or `subsample` (True: the shift is by the whole samples plus the parabola's sub-sample estimate, through a 33-tap windowed
        sinc, and delay holds both).  save_processed_result keeps the aligned output.
        iir_exact (not in the reference): True = the setting_lowpass_filtering keys come from the kernel that is bit-identical to
        scipy.signal.sosfiltfilt; False = from the segment-parallel kernel (backend.sosfiltfilt_multi(exact=False): the same filter
        within 1e-10 of each signal's peak, not SciPy's bits; measured times: DESIGN.md section 14).
        bootstrap (not in the reference): None = off, the result and its JSON are what they are without the option; a number of
        replicates B, or a dict of n_boot / level / seed / resample ("utterance" or "speaker") = evaluate() adds
        result["confidence"] = {"settings": {...}, "averaged": {key: {metric: {"se", "lo", "hi"}}}}, the percentile bootstrap of the
        "averaged" block (ssr_eval_amd.stats.bootstrap_ci)."""
        self.bootstrap = None if bootstrap is None else bootstrap_option(bootstrap)
        self.align = align
        self._align = None if align is None else _align_option(align)
        self.distribution = None if distribution is None else check_distribution_option(distribution)
        self._last_embeddings = None
        if not isinstance(iir_exact, bool):
            raise ValueError("iir_exact must be True or False")
        self.iir_exact = iir_exact
        self.evaluationset_sr = evaluation_sr
        self.audio_metrics = AudioMetrics(self.evaluationset_sr, precision=precision, device=device)
        # every family option is checked here, before the caller's settings are touched (the mel checks need audio_metrics)
        options = dict(lsd_split=lsd_split, stoi=stoi, waveform=waveform, mel=mel, mel_dtw=mel_dtw, quality=quality, pitch=pitch,
                       phase=phase, mrstft=mrstft, bss_sdr=bss_sdr, coherence=coherence, loudness=loudness,
                       bandwidth=bandwidth, auditory=auditory, modulation=modulation, csii=csii, nmr=nmr)
        for f in _ALL_FAMILIES + _OPEN_FAMILIES:
            if options[f.option] is not None:
                f.check(self, options[f.option])
            setattr(self, f.option, options[f.option])
        self.testee = testee
        self.test_name = test_name
        self.test_data_root = test_data_root
        self.save_processed_result = save_processed_result
        self.setting_lowpass_filtering = self._cutoff2sr(setting_lowpass_filtering)
        self.setting_fft = self._cutoff2sr(setting_fft)
        self.setting_subsampling = self._cutoff2sr(setting_subsampling)
        self.setting_mp3_compression = setting_mp3_compression
        self.model_input_sr = input_sr
        self.model_output_sr = output_sr
        assert self.evaluationset_sr <= 48000, "Our evaluation set only support up to 48 kHz target sampling rate"
        self.unexpected_symbol_test_folder = "_.*#()_+=!@$%^&~"
        self._device = device
        if test_data_root is not None and not os.path.exists(test_data_root):
            os.makedirs(test_data_root, exist_ok=True)
        if download:
            raise RuntimeError("dataset download (eval.py:102-119: wget/tar from Zenodo) is host tooling outside this "
                               "library; place VCTK test speakers under %r" % (test_data_root,))

    # ---- configuration quirks kept from the reference -------------------------------------------------
    def _cutoff2sr(self, dic):
        """Doubles the caller's cutoff list IN PLACE (eval.py:121-126): keys name 2*cutoff."""
        if dic is None:
            return None
        dic["cutoff_freq"] = [x * 2 for x in dic["cutoff_freq"]]
        return dic

    def cache_file_name(self, key, file, suffix=".flac"):
        stem = os.path.splitext(os.path.basename(file))[0]
        return os.path.join(os.path.dirname(file), stem + "_" + key + suffix)

    def get_test_file_list(self, path):
        keep = []
        for f in os.listdir(path):
            if not (f.endswith(".wav") or f.endswith(".flac")):
                continue
            if "DS_Store" in f or "proc" in f:
                continue
            keep.append(f)
        return keep

    # ---- degradations (eval.py:334-421): same keys, same `low_rate == sr -> -1` quirk -----------------
    def _iir_family(self, tag, ftype, x, sr):
        ret = {}
        for low_rate in self.setting_lowpass_filtering["cutoff_freq"]:
            for order in self.setting_lowpass_filtering["filter_order"]:
                if low_rate == sr:
                    low_rate -= 1
                key = "proc_%s_%s_%s_%s" % (tag, low_rate, order, sr)
                ret[key] = lowpass(x, low_rate // 2, sr, order=order, _type=ftype)
                assert ret[key].shape == x.shape, str((ret[key].shape, x.shape))
        return ret

    def lowpass_butterworth(self, file, x, sr):
        return self._iir_family("bw", "butter", x, sr)

    def lowpass_bessel(self, file, x, sr):
        return self._iir_family("bessel", "bessel", x, sr)

    def lowpass_ellip(self, file, x, sr):
        return self._iir_family("el", "ellip", x, sr)

    def lowpass_chebyshev(self, file, x, sr):
        return self._iir_family("ch", "cheby1", x, sr)

    def _fft_plan_keys(self, sr):
        keys, ratios = [], []
        for low_rate in self.setting_fft["cutoff_freq"]:
            if low_rate == sr:
                low_rate -= 1
            keys.append("proc_fft_%s_%s" % (low_rate, sr))
            ratios.append((low_rate // 2) / int(sr / 2))          # lowpass.py:193-194
        return keys, ratios

    def lowpass_stft_hard(self, file, x, sr):
        keys, ratios = self._fft_plan_keys(sr)
        ys = stft_hard_lowpass_multi([x], ratios, self._device)          # one call for the cutoffs of setting_fft
        return {k: y[0] for k, y in zip(keys, ys)}

    def lowpass_subsampling(self, file, x, sr):
        ret = {}
        for low_rate in self.setting_subsampling["cutoff_freq"]:
            if low_rate == sr:
                low_rate -= 1
            ret["proc_subsampling_%s_%s" % (low_rate, sr)] = lowpass(x, low_rate // 2, sr, order=1, _type="subsampling")
        return ret

    def _run_sox(self, args):
        """One sox invocation (the reference uses os.system, eval.py:309-314).  The codec is host tooling."""
        import shutil
        import subprocess
        if shutil.which("sox") is None:
            raise RuntimeError("mp3 degradation needs the `sox` codec on PATH (ssr_eval/eval.py:309-311 shells out to it)")
        subprocess.run(["sox"] + list(args), check=True)

    def mp3_encoding(self, file, x, sr):
        """eval.py:302-325.  sox encodes `file` to mp3 at every bit rate and decodes it again (host codec, exactly as
        the reference); the decoded signal is brought to len(x) and aligned with x by the position of the maximum of
        their full cross-correlation - that search runs on the GPU (ssr_xcorr_argmax), all bit rates
        of the file in one launch."""
        from .io import load_audio, write_wav
        if not isinstance(file, str) or not os.path.exists(file):
            raise RuntimeError("mp3 degradation encodes the source FILE with sox; no file path was given (%r)" % (file,))
        keys, decoded = [], []
        for low_kbps in self.setting_mp3_compression["low_kbps"]:
            key = "proc_mp3_%s_%s" % (low_kbps, sr)
            temp_file = self.cache_file_name("temp", file, suffix=".wav")     # reference: .flac - lossless either way
            target_mp3_file = self.cache_file_name(key, file, suffix=".mp3")
            self._run_sox([file, "-C", str(low_kbps), target_mp3_file])
            self._run_sox([target_mp3_file, temp_file])
            os.remove(target_mp3_file)
            y = load_audio(temp_file, sr)
            os.remove(temp_file)
            y, _ = self.unify_length(y, x)
            keys.append(key)
            decoded.append(np.ascontiguousarray(y, dtype=np.float32))
        ret = {}
        if not keys:
            return ret
        peaks = B.xcorr_argmax(decoded, [np.asarray(x, np.float32)] * len(decoded), self._device)
        for key, y, peak in zip(keys, decoded, peaks):
            shifted = self.shift(y, int(peak) - x.shape[0])         # eval.py:319-320
            write_wav(self.cache_file_name(key, file, suffix=".wav"), shifted, sr)   # the reference caches a .flac here
            ret[key] = shifted
            assert ret[key].shape == x.shape, str((ret[key].shape, x.shape))
            assert np.sum(ret[key] - x) != 0.0
        return ret

    def shift(self, x, shift):
        ret = np.zeros_like(x)
        if shift > 0:
            ret[:-shift] = x[shift:]
        elif shift < 0:
            ret[-shift:] = x[:shift]
        else:
            ret[:] = x          # the reference's `ret[:-0]` form would raise here
        return ret

    def pad(self, x, y):
        n = max(x.shape[0], y.shape[0])
        grow = lambda a, like: a if a.shape[0] == n else np.concatenate((a, np.zeros(n - a.shape[0], like.dtype)))
        return grow(x, y), grow(y, x)

    def unify_length(self, x, target):
        n = target.shape[0]
        if x.shape[0] >= n:
            return x[:n], target
        return np.concatenate((x, np.zeros(n - x.shape[0], target.dtype))), target

    def preprocess_array(self, x, sr, file="<array>"):
        """eval.py:229-270 for an in-memory waveform at the model's input rate."""
        ret = {}
        lp = self.setting_lowpass_filtering
        if lp is not None and "butter" in lp["filter"]:
            ret.update(self.lowpass_butterworth(file, x, sr))
        if lp is not None and "cheby" in lp["filter"]:
            ret.update(self.lowpass_chebyshev(file, x, sr))
        if lp is not None and "ellip" in lp["filter"]:
            ret.update(self.lowpass_ellip(file, x, sr))
        if lp is not None and "bessel" in lp["filter"]:
            ret.update(self.lowpass_bessel(file, x, sr))
        if self.setting_subsampling is not None:
            ret.update(self.lowpass_subsampling(file, x, sr))
        if self.setting_mp3_compression is not None:
            ret.update(self.mp3_encoding(file, x, sr))
        if self.setting_fft is not None:
            ret.update(self.lowpass_stft_hard(file, x, sr))
        return ret

    def preprocess_arrays(self, xs, sr, files=None, resident=None, keep_on_device=False):
        """preprocess_array for a list of waveforms with every degradation batched over the list (one launch
        sequence per (filter, cutoff, order) instead of one per file).  Key order per item is the reference's
        (eval.py:243-269: butter, cheby, ellip, bessel, subsampling, mp3, fft).  `files`: the source paths, needed
        by the mp3 degradation only (sox encodes the file itself).  `resident`: the same waveforms as device tensors when the
        caller has uploaded them already (used by the degradations that take float32 device input).  keep_on_device: the
        degraded signals stay device tensors (and `xs` may be device tensors): the resident evaluation path."""
        rets = [dict() for _ in xs]
        if not xs:
            return rets

        def put(key, ys):
            for ret, x, y in zip(rets, xs, ys):
                assert y.shape == x.shape, str((y.shape, x.shape))
                ret[key] = y
        lp = self.setting_lowpass_filtering
        if lp is not None:
            # every (filter, cutoff, order) of the setting over the same waveforms: ONE launch with the designs side by side
            # (lowpass_iir_multi; one after the other they were 94 % of a pass - profiles/r05_notes.md section 9)
            keys, specs = [], []
            for word, tag, ftype in (("butter", "bw", "butter"), ("cheby", "ch", "cheby1"), ("ellip", "el", "ellip"),
                                     ("bessel", "bessel", "bessel")):
                if word not in lp["filter"]:
                    continue
                for low_rate in lp["cutoff_freq"]:
                    for order in lp["filter_order"]:
                        if low_rate == sr:
                            low_rate -= 1
                        keys.append("proc_%s_%s_%s_%s" % (tag, low_rate, order, sr))
                        specs.append((low_rate // 2, order, ftype))
            for key, ys in zip(keys, lowpass_iir_multi(xs, specs, sr, keep_on_device=keep_on_device, exact=self.iir_exact)):
                put(key, ys)
        if self.setting_subsampling is not None:
            for low_rate in self.setting_subsampling["cutoff_freq"]:
                if low_rate == sr:
                    low_rate -= 1
                put("proc_subsampling_%s_%s" % (low_rate, sr),
                    lowpass_batch(xs, low_rate // 2, sr, order=1, _type="subsampling", keep_on_device=keep_on_device))
        if self.setting_mp3_compression is not None:
            if files is None:
                raise RuntimeError("mp3 degradation encodes the source files with sox: pass `files`")
            for ret, f, x in zip(rets, files, xs):
                ret.update(self.mp3_encoding(f, x.cpu().numpy() if isinstance(x, torch.Tensor) else x, sr))
        if self.setting_fft is not None:
            keys, ratios = self._fft_plan_keys(sr)
            src = xs if resident is None else resident
            ys = stft_hard_lowpass_multi(list(src), ratios, self._device, keep_on_device=keep_on_device)
            for i, ret in enumerate(rets):
                for j, k in enumerate(keys):
                    ret[k] = ys[j][i]
        return rets

    def preprocess(self, file, sr):
        from .io import load_audio
        return self.preprocess_array(load_audio(file, sr), sr, file)

    # ---- evaluation -----------------------------------------------------------------------------------
    def _testee_takes_device_tensors(self):
        """The resident path hands `infer` device tensors and takes device tensors back - no D2H / H2D round trip per degraded
        input.  It is used when the testee is the base class's identity `infer` (which does not look at its input) or
        declares `accepts_device_tensors = True`; every other testee gets and returns ndarrays, as in the reference."""
        return bool(getattr(self.testee, "accepts_device_tensors", False)) or type(self.testee).infer is BasicTestee.infer

    def _infer_and_collect(self, processed_inputs, device_mode=False):
        """Run the plugin on every degraded input; -> (keys, processed waveforms at output_sr, extra metrics)."""
        keys, outs, extras = [], [], []
        for k, v in processed_inputs.items():
            ret = self.testee.infer(v)                              # PLUGIN BOUNDARY (eval.py:138-143)
            processed, add = ret if isinstance(ret, tuple) else (ret, {})
            if isinstance(processed, torch.Tensor):
                processed = processed.detach()
                if not (device_mode and processed.is_cuda):
                    processed = processed.cpu().numpy()
            keys.append(k)
            outs.append(processed if isinstance(processed, torch.Tensor) else np.asarray(processed))
            extras.append(add)
        return keys, outs, extras

    def split_cutoff_hz(self, key):
        """The split frequency of `key` under lsd_split (None: no cutoff - NaN values)."""
        return key_cutoff_hz(key) if self.lsd_split is True else float(self.lsd_split)

    def evaluate_arrays(self, items, files=None, resident_inputs=None, device_mode=False, deferred=False):
        """items: list of (target waveform @ evaluation_sr, input waveform @ input_sr).
        -> list of {key: {metric: float}} (one dict per item), everything batched on the GPU.
        resident_inputs: the input waveforms as device tensors, if already uploaded.  device_mode: the inputs ARE device
        tensors and stay so through degradation, `infer` and resampling (_testee_takes_device_tensors).
        deferred: every launch is queued and a function is returned that waits for the metric values and builds the result -
        evaluate() queues the next batch of files before it calls it."""
        all_keys, all_proc, all_tgt, all_extra, owner = [], [], [], [], []
        xs = [x for _, x in items] if device_mode else [np.asarray(x) for _, x in items]
        degraded = self.preprocess_arrays(xs, self.model_input_sr, files, resident_inputs, keep_on_device=device_mode)
        for i, (target, x) in enumerate(items):
            keys, outs, extras = self._infer_and_collect(degraded[i], device_mode)
            for k, o, e in zip(keys, outs, extras):
                # a float64 output (IIR-degraded input through a pass-through testee) stays float64, as in the
                # reference: librosa.resample and AudioMetrics.evaluation keep the dtype they are given
                if isinstance(o, torch.Tensor):
                    o = o if o.dtype in (torch.float32, torch.float64) else o.float()
                else:
                    o = o if o.dtype == np.float64 else o.astype(np.float32)
                all_keys.append(k); all_proc.append(o)
                all_tgt.append(target if isinstance(target, torch.Tensor) else np.asarray(target, np.float32))
                all_extra.append(e); owner.append(i)
        if self.model_output_sr != self.evaluationset_sr and all_proc:
            # eval.py:144-150; float64 and float32 outputs are resampled in their own dtype
            # (key-major order: the IIR keys are [design][file] slices of one buffer - in that order resample_poly reads them where they
            # lie, and its output is already grouped by key for the metric stage)
            seen, pos = collections.Counter(), []
            for o_ in owner:
                pos.append(seen[o_]); seen[o_] += 1
            for want64 in (False, True):
                idx = sorted((i for i, o in enumerate(all_proc) if B._is_f64(o) == want64), key=lambda i: (pos[i], owner[i]))
                if idx:
                    ys = B.resample_poly([all_proc[i] for i in idx], self.evaluationset_sr, self.model_output_sr, self._device)
                    for i, y in zip(idx, ys):
                        all_proc[i] = y                             # stays in HBM: the metric stage is the only consumer
        # the delay stage: the outputs are replaced by their compensated copies (device views of one buffer per dtype, one call per
        # dtype); the delays stay on the device until the batch's values are collected
        delays = None
        if self._align is not None and all_proc:
            all_proc, delays = self.audio_metrics.align_batch(all_proc, all_tgt, *self._align, resident=True, deferred=True)
        values, K, multi = None, 0, False
        if all_proc:
            counts = collections.Counter(owner)
            per_item = [counts.get(i, 0) for i in range(len(items))]
            K = per_item[0] if per_item else 0
            multi = K > 1 and all(c == K for c in per_item)
            if multi:
                # every file has the same K degradation keys (the normal case): one target, K estimates - the target is transformed
                # once per file instead of once per key (ssr_pair_metrics_multi; evaluation_multi falls back by itself when the
                # signals are float64 or their lengths differ between keys)
                by_key = [[all_proc[i * K + k] for i in range(len(items))] for k in range(K)]
                values = self.audio_metrics.evaluation_multi(by_key, [all_tgt[i * K] for i in range(len(items))], resident=True, deferred=True)
            else:
                values = self.audio_metrics.evaluation_batch(all_proc, all_tgt, resident=True, deferred=True)
        # the optional families, queued behind the four metrics in the same deferred batch, in the registries' order; the multi path
        # analyses each target once for its K estimates
        queued = []
        if all_proc:
            same_keys = multi and all(all_keys[i * K:(i + 1) * K] == all_keys[:K] for i in range(len(items)))
            for f in _ALL_FAMILIES + _OPEN_FAMILIES:
                if getattr(self, f.option) is None:
                    continue
                if multi and (same_keys or not f.per_key):
                    args, kw = f.arguments(self, all_keys[:K])
                    rows = getattr(self.audio_metrics, f.multi)(by_key, [all_tgt[i * K] for i in range(len(items))], *args,
                                                                resident=True, deferred=True, **kw)
                    queued.append(lambda rows=rows: [r for row in rows() for r in row])
                else:
                    args, kw = f.arguments(self, all_keys)
                    queued.append(getattr(self.audio_metrics, f.batch)(all_proc, all_tgt, *args, resident=True, deferred=True, **kw))
        # the distribution option: one embedding per target (once per file) and one per (file, key), queued behind the families
        embedded = None
        if self.distribution is not None and all_proc:
            first = {}
            for j, i in enumerate(owner):
                first.setdefault(i, j)
            waves = [all_tgt[first[i]] for i in sorted(first)] + list(all_proc)
            waves = [w if isinstance(w, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(w)) for w in waves]
            embedded = (sorted(first), embed_waves(self.distribution, self.audio_metrics, waves, self.evaluationset_sr))
        self._last_processed = None
        keep = list(zip(owner, all_keys, all_proc)) if self.save_processed_result else None

        def finish():
            results = [dict() for _ in items]
            if values is not None:
                rows = values()
                vals = [rows[i][k] for i in range(len(items)) for k in range(K)] if multi else rows
                for flat in queued:
                    for v, x in zip(vals, flat()):
                        v.update(x)
                if delays is not None:
                    for v, d in zip(vals, delays()):
                        v[ALIGN_KEYS[0]] = d["delay"] + (d["delay_frac"] if self._align[1] else 0.0)
                        v[ALIGN_KEYS[1]] = d["align_corr"]
                for i, k, v, e in zip(owner, all_keys, vals, all_extra):
                    v.update(e)                                 # the testee's extra metrics last, as the reference's update
                    results[i][k] = v
            if keep is not None:
                self._last_processed = {(i, k): (y.cpu().numpy() if isinstance(y, torch.Tensor) else y) for i, k, y in keep}
            if self.distribution is not None:
                # per item: {"": the target's vector, key: the output's}
                rows = [dict() for _ in items]
                if embedded is not None:
                    have, e = embedded
                    for n_, i in enumerate(have):
                        rows[i][""] = e[n_]
                    for j, (i, k) in enumerate(zip(owner, all_keys)):
                        rows[i][k] = e[len(have) + j]
                self._last_embeddings = rows
            return results
        return finish if deferred else finish()

    def evaluate_files(self, files, decoded=None, deferred=False):
        """eval.py:128-156 for a LIST of files in one batched pass (decode on the host, everything else on the GPU).
        decoded: the files' io.decode_async(raw=True) / decode_batch result if the caller already has it.
        The decoded files cross the bus once (16-bit PCM as int16, converted on the GPU: backend.upload_decoded); the
        evaluation-rate targets (the reference shells out to `sox -r`, eval.py:133-134) and the model-rate inputs
        (librosa.load(file, sr=input_sr), eval.py:242) are resampled from that one upload and stay in HBM.
        deferred: as evaluate_arrays - the launches of the batch are queued, the returned function collects its results."""
        from .io import PackedBatch, RawAudio, decode_packed_async, to_rate_resident, write_wav
        if decoded is None:
            decoded = decode_packed_async(files, self._device)()
        if isinstance(decoded, PackedBatch):
            srs = list(decoded.srs)
            decoded_host = None
        else:
            decoded = [d if isinstance(d, RawAudio) else RawAudio(None, np.ascontiguousarray(d[0], np.float32), 1, int(d[1]))
                       for d in decoded]
            srs = [d.sr for d in decoded]
            decoded_host = decoded
        on_dev = B.upload_decoded(decoded, self._device)
        targets = to_rate_resident(on_dev, srs, self.evaluationset_sr)
        same_rate = all(sr == int(self.model_input_sr) for sr in srs)
        if self._testee_takes_device_tensors():
            inputs = to_rate_resident(on_dev, srs, self.model_input_sr)
            # (the reference loads the file twice: target and input never share a buffer, whatever a testee does to its input)
            items = [(t, x.clone() if x is t else x) for t, x in zip(targets, inputs)]
            res = self.evaluate_arrays(items, files, inputs if same_rate else None, device_mode=True, deferred=True)
        else:
            # an ndarray testee: the inputs go to the host (from the decoder's arrays where they exist, else from the upload)
            inputs = [(decoded_host[i].to_float() if decoded_host is not None else on_dev[i].cpu().numpy())
                      if srs[i] == int(self.model_input_sr) else None for i in range(len(srs))]
            need = [i for i, x in enumerate(inputs) if x is None]
            if need:
                ys = to_rate_resident([on_dev[i] for i in need], [srs[i] for i in need], self.model_input_sr)
                for i, y in zip(need, ys):
                    inputs[i] = y.cpu().numpy()
            res = self.evaluate_arrays(list(zip(targets, inputs)), files, on_dev if same_rate else None, deferred=True)

        def finish():
            out = res()
            if self.save_processed_result:
                for (i, k), y in self._last_processed.items():
                    write_wav(files[i] + k + "_processed_" + self.test_name + ".wav", y, self.evaluationset_sr)
            return out
        return finish if deferred else finish()

    def evaluate_single(self, file):
        """eval.py:128-156 for one file."""
        return self.evaluate_files([file])[0]

    def default_batch_files(self):
        """Files per launch sequence when the caller names none: 64 - enough rows to fill the chip and enough batches that the host's
        queueing of one hides under the GPU work of the one before (7.4-7.7 k files/s on the 367-file bench tree, 7.2 k at 128) - or
        256 when the IIR degradations are on: their launch is a serial recurrence that lasts as long as its longest utterance however
        many recurrences run beside it, so a pass wants FEW, WIDE launches (36 keys, 367 files: 0.94 s per pass at 64, 0.74 at 256;
        one batch of 367 loses the overlap of file reads with GPU work: 0.92).  Capped so that a batch's float64 signals (one per
        IIR key and file, twice: filtered and resampled) stay inside a quarter of the device's free memory."""
        lp = self.setting_lowpass_filtering
        n_iir = 0 if not lp else len(lp.get("filter", ())) * len(lp.get("cutoff_freq", ())) * len(lp.get("filter_order", ()))
        if n_iir < 8:
            return 64
        try:
            import torch
            free = int(torch.cuda.mem_get_info(self._device)[0])
        except Exception:
            return 64
        per_file = n_iir * 10 * 48000 * 8 * 2                      # a 10 s file at 48 kHz, float64, filtered + resampled
        return int(max(64, min(256, (free // 4) // max(per_file, 1))))

    def evaluate(self, limit_test_nums=-1, limit_test_speaker=-1, save_json=True, batch_files=None, shard="round-robin"):
        """eval.py:171-227: walk speakers/files, evaluate, aggregate as mean of speaker means, write JSON.
        Files are evaluated `batch_files` at a time (one ragged launch sequence per batch; None: default_batch_files()).  With
        torch.distributed initialised the (speaker, file) list is sharded over the ranks - round-robin, or shard="balanced":
        by audio duration read from the file headers, longest first to the lightest rank (every rank computes the
        same deal) - and the per-utterance rows are exchanged once (ssr_eval_amd.dist); every rank returns the full result.
        Every batch runs on the caller's stream."""
        from datetime import datetime
        work = []                                                   # (speaker, file) in the reference's order
        speakers = []
        for speaker in sorted(os.listdir(self.test_data_root)):
            if not os.path.isdir(os.path.join(self.test_data_root, speaker)):
                continue
            if "p" not in speaker and "s" not in speaker:
                continue
            if limit_test_speaker > 0 and len(speakers) >= limit_test_speaker:
                break
            files = sorted(self.get_test_file_list(os.path.join(self.test_data_root, speaker)))
            assert len(files) != 0, os.path.join(self.test_data_root, speaker)
            if limit_test_nums > 0:
                files = files[:limit_test_nums]
            speakers.append(speaker)
            work += [(speaker, f) for f in files]
        rank, world = D.rank_world()
        if shard not in ("round-robin", "balanced"):
            raise ValueError("shard must be 'round-robin' or 'balanced'")
        from .io import decode_packed_async, duration_hint
        if shard == "balanced" and world > 1:
            weights = [int(round(1000.0 * duration_hint(os.path.join(self.test_data_root, *w)))) for w in work]      # milliseconds
            mine = D.shard_indices_balanced(weights, rank, world)
        else:
            mine = D.shard_indices(len(work), rank, world)
        paths = [os.path.join(self.test_data_root, *work[i]) for i in mine]
        local, local_emb = [], []
        step = max(1, int(batch_files if batch_files is not None else self.default_batch_files()))   # files per launch sequence
        batches = pipeline_batches(paths, step)
        # the file reads of batch k+1 (straight into a page-locked arena) run under the GPU work of batch k
        ahead = decode_packed_async(batches[0], self._device) if batches else None
        # ... and the host work of batch k+1 (descriptors, launches) under the GPU work of batch k: a batch's metric values are
        # collected only after the next batch has been queued (no host wait in between - backend._h2d, backend.Pending)
        # (the reads of batch k+1 are started AFTER batch k has been queued: sixteen reader threads next to the launching thread
        # cost it 2-3 ms per batch; they run while it waits for batch k-1's values instead)
        # All batches share the caller's stream: device objects cached across batches and replaced when they grow (the sinc plan's
        # time register, staging twins) are ordered by that one stream.
        collect = None
        for k, batch in enumerate(batches):
            decoded = ahead()
            queued = self.evaluate_files(batch, decoded, deferred=True)
            ahead = decode_packed_async(batches[k + 1], self._device) if k + 1 < len(batches) else None
            if collect is not None:
                local += collect()
                local_emb += self._last_embeddings or []
            collect = queued
        if collect is not None:
            local += collect()
            local_emb += self._last_embeddings or []
        return self._assemble(work, speakers, mine, local, save_json, datetime.now(), local_emb if self.distribution is not None else None)

    def _gather_embeddings(self, local_emb, keys, mine, n_total, gather=None):
        """The rank's embedding rows (per file: {"": target, key: output}) -> the table [n_total, (1 + len(keys)) D] every rank holds."""
        rows = np.array([np.concatenate([r[""]] + [r[k] for k in keys]) for r in local_emb], dtype=np.float64) if local_emb and keys \
            else np.empty((0, 0), dtype=np.float64)
        return (gather or D.allgather_rows)(rows, mine, n_total)

    def _assemble(self, work, speakers, mine, local, save_json, now, local_emb=None):
        # Key order of the reference = insertion order of preprocess() (eval.py:243-269); metric order = the four
        # AudioMetrics keys, then whatever the testee added.  A rank that owns no file (world_size > number of files) has
        # neither, so the lists are agreed on across ranks: the first rank that has results defines the order.
        rank, world = D.rank_world()
        order = list(local[0].keys()) if local else []
        order += sorted({k for r in local for k in r} - set(order))
        mets = {m for r in local for v in r.values() for m in v}
        if world > 1:
            import torch.distributed as dist
            box = [None] * world
            dist.all_gather_object(box, (order, sorted(mets)))
            first = next((b[0] for b in box if b[0]), [])
            order = list(first) + sorted({k for b in box for k in b[0]} - set(first))
            mets = {m for b in box for m in b[1]}
        keys = order
        order_keys = open_key_order()
        mets = sorted(mets, key=lambda m: (order_keys.index(m) if m in order_keys else 99, m))
        rows = np.empty((len(local), len(keys) * len(mets)), dtype=np.float64)
        for i, r in enumerate(local):
            rows[i] = [r[k][m] for k in keys for m in mets]
        # ONE collective: the per-file rows and, behind them, the per-speaker sums + counts (added in rank order on every rank)
        spk_id = {s: i for i, s in enumerate(speakers)}
        table, buf = D.gather_rows_and_speaker_sums(rows, mine, len(work), [spk_id[work[i][0]] for i in mine], len(speakers))
        final_result = {s: {} for s in speakers}
        M = len(mets)
        by_spk = {s: [] for s in speakers}
        for n_, ((spk, f), vals) in enumerate(zip(work, table.tolist())):       # (one tolist: Python floats, not 54 k numpy scalars)
            final_result[spk][f] = {k: dict(zip(mets, vals[i * M:(i + 1) * M])) for i, k in enumerate(keys)}
            by_spk[spk].append(n_)

        # aggregation (eval.py:200-216, utils.py:24-28): per speaker np.mean over its files of every metric, then np.mean over the
        # speakers.  np.mean of the reference's Python list = NumPy's pairwise sum of a contiguous float64 vector: the same sum, to
        # the bit, as the mean along the contiguous last axis of the transposed block (tests/golden/aggregate.json holds the
        # reference's values) - 1,184 np.mean calls of 46 floats each were 10 % of a pass with 37 keys.
        def nest(vec):
            vec = vec.tolist()
            return {k: dict(zip(mets, vec[i * M:(i + 1) * M])) for i, k in enumerate(keys)}
        spk_means = np.empty((len(speakers), table.shape[1]), dtype=np.float64)
        for si, spk in enumerate(speakers):
            spk_means[si] = np.ascontiguousarray(table[by_spk[spk]].T).mean(axis=1) if by_spk[spk] and table.shape[1] else np.nan
        result_cache = {spk: nest(spk_means[si]) for si, spk in enumerate(speakers)}
        averaged = nest(np.ascontiguousarray(spk_means.T).mean(axis=1)) if len(speakers) and table.shape[1] else {}
        # the same aggregate from the float64 sums + counts that rode along; kept for cross-checking
        self.last_allreduce_average = D.mean_of_speaker_means(buf)[1] if len(keys) else None
        final_result["each_speaker"] = result_cache
        final_result["averaged"] = averaged
        if self.bootstrap is not None:
            # every rank holds the gathered table and the replicates are a function of (table, settings): the same bits everywhere
            conf = {}
            if len(work) and table.shape[1]:
                ci = bootstrap_ci(table, [w[0] for w in work], device=self._device, **self.bootstrap)
                conf = {k: {m: {"se": se, "lo": lo, "hi": hi} for m, se, lo, hi in zip(mets, *(ci[n][i * M:(i + 1) * M].tolist()
                                                                                      for n in ("se", "lo", "hi")))}
                        for i, k in enumerate(keys)}
            final_result["confidence"] = {"settings": dict(self.bootstrap), "averaged": conf}
        if local_emb is not None:
            # one more collective, only with the option on: the embedding rows travel with the file's global index; every rank then
            # holds the same table and computes the same bits
            final_result["distribution"] = distribution_block(self.distribution, keys, self._gather_embeddings(local_emb, keys, mine, len(work)))
        if save_json and rank == 0:
            os.makedirs("results", exist_ok=True)
            write_json(final_result, os.path.join("results", str(now.date()) + "-" + str(now.time()) + "-"
                                                  + self.test_name + ".json"))
        return final_result
