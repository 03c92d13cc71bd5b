"""Float64 oracle of the mel-spectrogram distances, written from the definitions (test infrastructure).

Magnitude images come from oracle/stft.py (the reference's librosa framing, |.| in float32 as AudioMetrics.wav_to_spectrogram
gives them); everything after that is float64 NumPy:
  M = S W;  mel_lsd = mean_t sqrt(mean_m log10(G^2 / (E + 1e-12)^2 + 1e-12)^2);  mel_l1 = mean |ln+E - ln+G|;
  mcd = mean_t (10 / ln 10) sqrt(2 sum_{d=1..n_cep} c_d^2),  c = orthonormal DCT-II over m of ln+E - ln+G.
"""
import numpy as np

from oracle import metrics as om
from oracle import stft as ostft

EPS = 1e-12
FLOOR = 1e-5
NAMES = ("mel_lsd", "mel_l1", "mcd")


def magnitudes(wav, rate, n_fft=None, hop=None):
    """[T, F] float32 magnitude image at AudioMetrics(rate)'s transform size (or n_fft / hop)."""
    nf, hp = om.stft_params(rate)
    return ostft.stft_mag_TF(np.asarray(wav), n_fft or nf, hop or hp)


def dct_matrix(n_mels, n_cep):
    """[n_cep, n_mels]: rows d = 1 .. n_cep of the orthonormal DCT-II."""
    d = np.arange(1, n_cep + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / n_mels) * np.cos(np.pi * d * (2 * m + 1) / (2 * n_mels))


def mel(S, W):
    return np.asarray(S, np.float64) @ np.asarray(W, np.float64)


def ln_plus(x):
    return np.log(np.maximum(x, FLOOR))


def distances_from_mel(E, G, n_cep=13):
    """{mel_lsd, mel_l1, mcd} of two [T, n_mels] float64 mel images."""
    E, G = np.asarray(E, np.float64), np.asarray(G, np.float64)
    d = np.log10(G ** 2 / (E + EPS) ** 2 + EPS) ** 2
    lsd = float(np.mean(np.sqrt(np.mean(d, axis=1))))
    dl = ln_plus(E) - ln_plus(G)
    l1 = float(np.mean(np.abs(dl)))
    c = dl @ dct_matrix(E.shape[1], n_cep).T
    mcd = float(np.mean(10.0 / np.log(10.0) * np.sqrt(2.0 * np.sum(c * c, axis=1))))
    return {"mel_lsd": lsd, "mel_l1": l1, "mcd": mcd}


def distances_from_images(Se, St, W, n_cep=13):
    return distances_from_mel(mel(Se, W), mel(St, W), n_cep)


def distances(est, tgt, rate, W, n_cep=13, n_fft=None, hop=None):
    """The three distances of two waveforms (truncated to the common length, as AudioMetrics does)."""
    m = min(len(est), len(tgt))
    return distances_from_images(magnitudes(est[:m], rate, n_fft, hop), magnitudes(tgt[:m], rate, n_fft, hop), W, n_cep)
