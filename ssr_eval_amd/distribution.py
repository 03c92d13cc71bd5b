"""Distribution distances of embedding sets: does the SET of outputs sound like the set of targets?

``frechet_distance`` is the Fréchet distance of the Gaussians fitted to two sets (the arithmetic of FAD), ``kernel_distance`` the
unbiased MMD^2 with a Gaussian kernel times ``scale`` (the arithmetic of KAD).  Both are "everything after the embedding": any array
of embeddings is accepted.  The network behind published FAD figures (VGGish, CLAP, PANNs) is not part of this library;
``embed_logmel_stats`` is a simple built-in embedding that makes ``SSR_Eval_Helper(distribution=True)`` work out of the box.  ``fd`` on
that embedding is NOT comparable with published VGGish / CLAP FAD figures: for those, pass your own ``embed=``.

Every number comes from libssrhip.so (ssr_frechet, ssr_kernel_distance, ssr_pairwise_distances); the median selection of the default
bandwidth is ``torch.kthvalue`` on the device buffer of distances.
"""
import math

import numpy as np
import torch

from . import backend as B

METRICS = ("fd", "kd")
OPTION_KEYS = ("embed", "bandwidth", "scale", "max_sweeps", "metrics")


def _sets(est):
    """est as (list of sets, was-a-list)."""
    if isinstance(est, (list, tuple)):
        return list(est), True
    return [est], False


def frechet_distance(est, ref, max_sweeps=B.DISTRIBUTION_MAX_SWEEPS, return_stats=False):
    """fd = |mu_r - mu_e|^2 + tr Sigma_r + tr Sigma_e - 2 tr sqrt(Sigma_r Sigma_e) of the embedding sets est [m, D] and ref [n, D] (float32
    or float64, NumPy or torch, host or resident), float64 throughout, covariances with ddof = 1.  est may be a list of sets scored
    against the one reference in one call: a list of values, each bit for bit what the set gives alone.  No clamp: identical sets
    give a value of rounding size of either sign.  Fewer than two rows in a set, a non-finite moment, or a Jacobi iteration that has
    not converged within max_sweeps sweeps (1 .. 200) give NaN.  fd is biased upwards for small sets (the covariance of m rows in D
    dimensions has rank <= m - 1): compare figures at equal set sizes, n and m several times D.
    return_stats: a dict per set - fd, dmu2, tr_ref, tr_est, tr_sqrt, sweeps_ref, sweeps_est, rank_ref - instead of the value."""
    sets, many = _sets(est)
    out = B.frechet_stats(ref, sets, max_sweeps)
    names = ("fd", "dmu2", "tr_ref", "tr_est", "tr_sqrt", "sweeps_ref", "sweeps_est", "rank_ref")
    res = [dict(zip(names, (float(v) if j < 5 else int(v) for j, v in enumerate(row)))) if return_stats else float(row[0]) for row in out]
    return res if many else res[0]


def median_gamma(ref):
    """The default bandwidth: gamma = 1 / (2 sigma^2), sigma the lower median of the pairwise distances |r_i - r_j|, i < j, over at most
    2048 evenly strided reference rows (row floor(i n / n_sub)); NaN with fewer than two rows or sigma = 0."""
    t = B._embedding_set(ref, "ref")
    n = int(t.shape[0])
    if n < 2:
        return math.nan
    n_sub = min(n, B.DISTRIBUTION_MAX_PAIR_ROWS)
    index = np.array([i * n // n_sub for i in range(n_sub)], np.int64)
    d = B.pairwise_distances(t, index, as_tensor=True)
    sigma = float(torch.kthvalue(d, (d.numel() - 1) // 2 + 1).values.item())
    return 1.0 / (2.0 * sigma * sigma) if sigma > 0.0 and math.isfinite(sigma) else math.nan


def _check_bandwidth(bandwidth):
    if isinstance(bandwidth, str):
        if bandwidth != "median":
            raise ValueError("bandwidth must be 'median' or a number > 0 (the kernel's sigma)")
        return bandwidth
    if isinstance(bandwidth, (bool, np.bool_)) or not isinstance(bandwidth, (int, float, np.integer, np.floating)) or \
            not (math.isfinite(bandwidth) and bandwidth > 0):
        raise ValueError("bandwidth must be 'median' or a number > 0 (the kernel's sigma)")
    return float(bandwidth)


def kernel_distance(est, ref, bandwidth="median", scale=1000.0):
    """kd = scale mmd2, the unbiased squared maximum mean discrepancy of est [m, D] and ref [n, D] with the Gaussian kernel
    exp(-|x - y|^2 / (2 sigma^2)); bandwidth: sigma, or "median" = median_gamma(ref).  est may be a list of sets (a list of values; the
    reference's own kernel sum is computed once).  Fewer than two rows in a set or a zero median give NaN."""
    sets, many = _sets(est)
    bandwidth = _check_bandwidth(bandwidth)
    scale = B.check_distribution_scale(scale)
    B._distribution_sets(ref, sets)
    gamma = median_gamma(ref) if bandwidth == "median" else 1.0 / (2.0 * bandwidth * bandwidth)
    if not (math.isfinite(gamma) and gamma > 0.0):
        res = [math.nan] * len(sets)
    else:
        res = [float(v) for v in B.kernel_sums(ref, sets, [gamma], scale)[:, 0, 0]]
    return res if many else res[0]


def distribution_distance(est, ref, bandwidth="median", scale=1000.0, max_sweeps=B.DISTRIBUTION_MAX_SWEEPS, metrics=METRICS):
    """{"fd": frechet_distance, "kd": kernel_distance} (or the subset `metrics` names) of est and ref; lists of values where est is a
    list of sets."""
    metrics = check_metrics(metrics)
    out = {}
    if "fd" in metrics:
        out["fd"] = frechet_distance(est, ref, max_sweeps)
    if "kd" in metrics:
        out["kd"] = kernel_distance(est, ref, bandwidth, scale)
    return out


def check_metrics(metrics):
    if isinstance(metrics, str) or not isinstance(metrics, (list, tuple)) or not metrics or set(metrics) - set(METRICS) or \
            len(set(metrics)) != len(metrics):
        raise ValueError("metrics must be a non-empty subset of ('fd', 'kd')")
    return tuple(m for m in METRICS if m in metrics)


def embed_logmel_stats(audio_metrics, waves):
    """The built-in embedding: per signal the time mean and the time standard deviation (ddof 0) of L = 10 log10(max(M, 1e-10)), M the
    image AudioMetrics.mel_spectrogram returns -> float64 [len(waves), 2 n_mels] on the device.  A fd on this embedding is NOT
    comparable with published VGGish / CLAP FAD figures; it orders systems evaluated with this library against each other."""
    rows = []
    for w in waves:
        w = w.float() if isinstance(w, torch.Tensor) else np.asarray(w, np.float32)      # (mel_spectrogram's transform takes float32)
        m = audio_metrics.mel_spectrogram(w, keep_on_device=True)
        L = 10.0 * torch.log10(torch.clamp(m.reshape(-1, m.shape[-1]).to(torch.float64), min=1e-10))
        rows.append(torch.cat([L.mean(dim=0), L.std(dim=0, unbiased=False)]))
    if not rows:
        return torch.empty((0, 0), dtype=torch.float64)
    return torch.stack(rows)


def check_option(v):
    """SSR_Eval_Helper's `distribution` option -> its settings with the defaults filled in, or ValueError."""
    msg = "distribution must be None, True or a dict of 'embed', 'bandwidth', 'scale', 'max_sweeps' and / or 'metrics'"
    if v is True:
        v = {}
    elif not isinstance(v, dict) or not v or set(v) - set(OPTION_KEYS):
        raise ValueError(msg)
    embed = v.get("embed", "logmel_stats")
    if not (callable(embed) or (isinstance(embed, str) and embed == "logmel_stats")):
        raise ValueError("embed must be 'logmel_stats' or a callable (waves, sr) -> [len(waves), D]; " + msg)
    return {"embed": embed, "bandwidth": _check_bandwidth(v.get("bandwidth", "median")), "scale": B.check_distribution_scale(v.get("scale", 1000.0)),
            "max_sweeps": B.check_distribution_max_sweeps(v.get("max_sweeps", B.DISTRIBUTION_MAX_SWEEPS)),
            "metrics": check_metrics(v.get("metrics", METRICS))}


def embed_waves(settings, audio_metrics, waves, sr):
    """The embeddings of `waves` (1-D tensors at rate sr) under the option's settings -> float64 ndarray [len(waves), D]."""
    embed = settings["embed"]
    e = embed_logmel_stats(audio_metrics, waves) if isinstance(embed, str) else embed(waves, sr)
    e = e.detach().cpu().numpy() if isinstance(e, torch.Tensor) else np.asarray(e)
    e = np.ascontiguousarray(e, dtype=np.float64)
    if e.ndim != 2 or e.shape[0] != len(waves) or not 1 <= e.shape[1] <= B.DISTRIBUTION_MAX_DIM:
        raise ValueError("embed must return [len(waves), D] with 1 <= D <= %d" % B.DISTRIBUTION_MAX_DIM)
    return e


def result_block(settings, keys, table, distance=None):
    """result["distribution"] from the gathered row table [files, (1 + len(keys)) D]: the target's embedding, then one per key.
    distance: what scores the sets (distribution_distance; a test without a device passes its own)."""
    distance = distribution_distance if distance is None else distance
    n, width = table.shape
    D = width // (1 + len(keys)) if keys else 0
    shown = dict(settings, embed=settings["embed"] if isinstance(settings["embed"], str) else "callable", metrics=list(settings["metrics"]))
    per_key = {}
    if keys and D:
        ref = np.ascontiguousarray(table[:, :D])
        ests = [np.ascontiguousarray(table[:, (1 + k) * D:(2 + k) * D]) for k in range(len(keys))]
        vals = distance(ests, ref,settings["bandwidth"], settings["scale"], settings["max_sweeps"], settings["metrics"])
        per_key = {key: {m: vals[m][k] for m in settings["metrics"]} for k, key in enumerate(keys)}
    return {"settings": shown, "dim": D, "n": int(n), "per_key": per_key}
