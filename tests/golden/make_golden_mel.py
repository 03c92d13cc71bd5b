#!/usr/bin/env python
"""Mel filterbank vectors -> tests/golden/reference_mel.npz (build container only).

Imports the reference's own mel front end (examples/NVSR/mel_scale.py: torchaudio's MelScale / melscale_fbanks, which NVSR's
baseline uses) by path and runs it on torch-CPU.  The file written holds data only: for every configuration the filterbank
``MelScale(...).fb`` [n_stft, n_mels], and ``MelScale.forward`` on two seeded non-negative [60, n_stft] images (the tests
regenerate the inputs from their seeds: numpy Generator streams are stable), and torch's CPU capability on the generating host.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/examples/NVSR/mel_scale.py"

# name -> (sample_rate, n_stft, n_mels, f_min, f_max, norm, mel_scale)
CONFIGS = {
    "nvsr_44100": (44100, 1025, 128, 0.0, None, None, "htk"),
    "htk_48000": (48000, 1115, 128, 0.0, None, None, "htk"),
    "slaney_slaney_16000": (16000, 372, 80, 0.0, None, "slaney", "slaney"),
    "slaney_24000": (24000, 558, 100, 0.0, None, None, "slaney"),
    "band_20_8000_44100": (44100, 1025, 64, 20.0, 8000.0, None, "htk"),
    "htk_slaney_32000": (32000, 744, 96, 0.0, None, "slaney", "htk"),
}
# forward vectors: (config, seed)
FORWARD = [("nvsr_44100", 1101), ("slaney_slaney_16000", 1602)]


def image(seed, F, T=60):
    """A non-negative [T, F] float32 magnitude-like image."""
    rng = np.random.default_rng(seed)
    x = np.abs(rng.standard_normal((T, F))) * np.exp(-np.arange(F) / (F / 4.0))[None, :]
    return x.astype(np.float32)


def main():
    spec = importlib.util.spec_from_file_location("ref_mel_scale", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out, meta = {}, {}
    for name, (sr, n_stft, n_mels, f_min, f_max, norm, scale) in CONFIGS.items():
        m = mod.MelScale(n_mels=n_mels, sample_rate=sr, f_min=f_min, f_max=f_max, n_stft=n_stft, norm=norm, mel_scale=scale)
        out["fb_" + name] = m.fb.numpy().astype(np.float32)
        meta[name] = [sr, n_stft, n_mels, f_min, f_max, norm, scale]
    for name, seed in FORWARD:
        sr, n_stft, n_mels, f_min, f_max, norm, scale = CONFIGS[name]
        m = mod.MelScale(n_mels=n_mels, sample_rate=sr, f_min=f_min, f_max=f_max, n_stft=n_stft, norm=norm, mel_scale=scale)
        x = torch.from_numpy(image(seed, n_stft))
        out["fwd_" + name] = m(x.T.contiguous()).T.contiguous().numpy()        # [60, n_mels]
        out["fwd_seed_" + name] = np.int64(seed)
    out["configs_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    # torch's CPU kernels for pow / exp are dispatched by CPU capability: the tables are this capability's bits
    out["cpu_capability"] = np.frombuffer(torch.backends.cpu.get_cpu_capability().encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "reference_mel.npz"), **out)
    print("wrote", sorted(out))


if __name__ == "__main__":
    sys.exit(main())
