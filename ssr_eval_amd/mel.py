"""Mel filterbanks for the mel-spectrogram distances, built on the host.

``mel_filterbank`` follows torchaudio's documented ``melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate, norm, mel_scale)``
algorithm in torch-CPU float32, operation for operation, so that the table has the bits of ``MelScale(...).fb`` for the same
arguments (NVSR's baseline: ``MelScale(n_mels=128, sample_rate=44100, n_stft=1025)``):

* the band edges of the mel axis from Hz in Python float64 (HTK: 2595 log10(1 + f / 700); Slaney: linear below 1 kHz at
  200 / 3 Hz per mel, logarithmic above at ln(6.4) / 27 per mel);
* ``n_mels + 2`` points equally spaced in mel (``torch.linspace``, float32) and back to Hz;
* triangular filters: for bin frequency f and points f_{m}, f_{m+1}, f_{m+2},
  w = max(0, min((f - f_m) / (f_{m+1} - f_m), (f_{m+2} - f) / (f_{m+2} - f_{m+1})));
* ``norm="slaney"``: filter m scaled by 2 / (f_{m+2} - f_m) (constant area).

Unlike torchaudio, a filter that comes out all zero is an error: its log-mel value would be the clamp on both sides and it
would dominate mel_lsd with a constant.
"""
import math

import numpy as np
import torch

MEL_OPTIONS = ("n_mels", "f_min", "f_max", "norm", "mel_scale", "n_cep")
_MIN_LOG_HZ = 1000.0
_F_SP = 200.0 / 3


def _logstep():
    return math.log(6.4) / 27.0


def hz_to_mel(freq, mel_scale="htk"):
    """One frequency in Hz -> mel (Python float64)."""
    if mel_scale == "htk":
        return 2595.0 * math.log10(1.0 + (freq / 700.0))
    if freq < _MIN_LOG_HZ:
        return freq / _F_SP
    return _MIN_LOG_HZ / _F_SP + math.log(freq / _MIN_LOG_HZ) / _logstep()


def mel_to_hz(mels, mel_scale="htk"):
    """float32 tensor of mels -> Hz (float32 tensor)."""
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (mels / 2595.0) - 1.0)
    freqs = _F_SP * mels
    min_log_mel = _MIN_LOG_HZ / _F_SP
    above = mels >= min_log_mel
    freqs[above] = _MIN_LOG_HZ * torch.exp(_logstep() * (mels[above] - min_log_mel))
    return freqs


def check_options(rate, n_mels=128, f_min=0.0, f_max=None, norm=None, mel_scale="htk", n_cep=13):
    """-> the normalised option tuple (n_mels, f_min, f_max, norm, mel_scale, n_cep); ValueError for anything else."""
    if isinstance(n_mels, bool) or not isinstance(n_mels, (int, np.integer)) or not 2 <= int(n_mels) <= 256:
        raise ValueError("n_mels must be an integer in 2..256")
    if isinstance(n_cep, bool) or not isinstance(n_cep, (int, np.integer)) or not 1 <= int(n_cep) < int(n_mels):
        raise ValueError("n_cep must be an integer in 1..n_mels - 1")
    if norm not in (None, "slaney"):
        raise ValueError("norm must be None or 'slaney'")
    if mel_scale not in ("htk", "slaney"):
        raise ValueError("mel_scale must be 'htk' or 'slaney'")
    f_max = float(rate // 2) if f_max is None else f_max
    for name, v in (("f_min", f_min), ("f_max", f_max)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v) or v < 0:
            raise ValueError("%s must be a finite frequency >= 0 in Hz" % name)
    if not f_min < f_max:
        raise ValueError("f_min must be below f_max")
    return int(n_mels), float(f_min), float(f_max), norm, mel_scale, int(n_cep)


def mel_filterbank(n_freqs, f_min, f_max, n_mels, sample_rate, norm=None, mel_scale="htk", check_empty=True):
    """float32 [n_freqs, n_mels] torch-CPU tensor: torchaudio's melscale_fbanks table for these arguments.  check_empty: raise
    ValueError where a filter has no non-zero weight."""
    if norm not in (None, "slaney"):
        raise ValueError("norm must be None or 'slaney'")
    if mel_scale not in ("htk", "slaney"):
        raise ValueError("mel_scale must be 'htk' or 'slaney'")
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_pts = torch.linspace(hz_to_mel(f_min, mel_scale), hz_to_mel(f_max, mel_scale), n_mels + 2)
    f_pts = mel_to_hz(m_pts, mel_scale)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)                # [n_freqs, n_mels + 2]: f_j - f
    down = -slopes[:, :-2] / f_diff[:-1]                               # rising edge of filter m: (f - f_m) / (f_{m+1} - f_m)
    up = slopes[:, 2:] / f_diff[1:]                                    # falling edge: (f_{m+2} - f) / (f_{m+2} - f_{m+1})
    fb = torch.max(torch.zeros(1), torch.min(down, up))
    if norm == "slaney":
        fb *= (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels])).unsqueeze(0)
    if check_empty:
        empty = (fb.max(dim=0).values == 0.0).nonzero().flatten().tolist()
        if empty:
            raise ValueError("mel filter(s) %s have only zero weights at n_freqs=%d, rate=%d: use fewer mels (n_mels=%d) or a lower f_min"
                             % (empty[:8], n_freqs, sample_rate, n_mels))
    return fb
