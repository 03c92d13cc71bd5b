"""Uncertainty of the aggregate (not in the reference): bootstrap confidence intervals of evaluate()'s "averaged"
block - the mean over speakers of each speaker's mean over its files - and a paired comparison of two evaluate() results.

The replicates and their summary are computed by libssrhip.so (backend.bootstrap_means / bootstrap_summary); matching the files of
two results and building their tables (_paired_tables) is host bookkeeping and needs no GPU."""
import json
import math
import numbers

import numpy as np

from . import backend as B

RESAMPLE = ("utterance", "speaker")
# what evaluate() adds to a result beside the speakers
_AGGREGATE_KEYS = ("each_speaker", "averaged", "confidence", "distribution")


def check_settings(n_boot=2000, level=0.95, seed=0, resample="utterance"):
    """ValueError unless the four settings are usable -> them as a dict of plain int / float / str."""
    if isinstance(n_boot, bool) or not isinstance(n_boot, numbers.Integral) or n_boot < 1:
        raise ValueError("n_boot must be an integer >= 1")
    if isinstance(level, bool) or not isinstance(level, numbers.Real) or not 0.0 < level < 1.0:
        raise ValueError("level must lie strictly between 0 and 1")
    if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not 0 <= seed < 1 << 64:
        raise ValueError("seed must be an integer in [0, 2^64)")
    if resample not in RESAMPLE:
        raise ValueError("resample must be 'utterance' or 'speaker'")
    return {"n_boot": int(n_boot), "level": float(level), "seed": int(seed), "resample": resample}


def bootstrap_option(value):
    """SSR_Eval_Helper(bootstrap=...): an int B or a dict of n_boot / level / seed / resample -> check_settings' dict."""
    if isinstance(value, dict):
        if not value or set(value) - {"n_boot", "level", "seed", "resample"}:
            raise ValueError("a bootstrap dict takes 'n_boot', 'level', 'seed' and / or 'resample'")
        return check_settings(**value)
    if isinstance(value, bool) or not isinstance(value, numbers.Integral):
        raise ValueError("bootstrap must be None, a number of replicates or a dict")
    return check_settings(n_boot=value)


def _group_by_speaker(speaker_ids):
    """(order, spk_off): the stable permutation that groups the rows by speaker (speakers in sorted order) and where each
    speaker's rows then start."""
    ids = list(speaker_ids)
    names = sorted(set(ids))
    code = {s: i for i, s in enumerate(names)}
    codes = np.array([code[s] for s in ids], dtype=np.int64)
    order = np.argsort(codes, kind="stable")
    spk_off = np.concatenate(([0], np.cumsum(np.bincount(codes, minlength=len(names))))).astype(np.int32)
    return order, spk_off


def _quantile_levels(level):
    return np.array([(1.0 - level) / 2.0, 1.0 - (1.0 - level) / 2.0], dtype=np.float64)


def bootstrap_ci(table, speaker_ids, n_boot=2000, level=0.95, seed=0, resample="utterance", return_replicates=False, device=None):
    """Percentile bootstrap of the mean of speaker means.  table: [N, K] float64 (one row per file, one column per key x metric; an
    ndarray or a tensor), speaker_ids: the speaker of every row (any sortable labels; the rows are stable-sorted by speaker here).
    resample "utterance": every speaker stays and redraws its own files with replacement (the speakers are the population of
    interest, the files a sample); "speaker": the speakers are redrawn with replacement as well (the speakers are themselves a
    sample).  The same drawn files serve every column of a replicate.
    -> {"estimate", "se", "lo", "hi"}: [K] float64 arrays - the plain mean of speaker means, the standard deviation of the replicates
    (ddof 1) and their (1 - level) / 2 and 1 - (1 - level) / 2 quantiles; with return_replicates also "replicates", the device
    tensor [n_boot, K], and "n_le0" / "n_ge0", how many replicates are <= 0 / >= 0.  A column with a non-finite entry: NaN (-1)."""
    st = check_settings(n_boot, level, seed, resample)
    dev_table = table if not isinstance(table, np.ndarray) and hasattr(table, "is_cuda") else None
    host = np.asarray(table.detach().cpu().numpy() if dev_table is not None else table, dtype=np.float64)
    if host.ndim != 2:
        raise ValueError("table must be [files, columns]")
    N, K = host.shape
    ids = list(speaker_ids)
    if len(ids) != N:
        raise ValueError("speaker_ids must name the speaker of every row of table")
    if N == 0:
        raise ValueError("table has no rows")
    order, spk_off = _group_by_speaker(ids)
    host = np.ascontiguousarray(host[order])
    means = np.stack([host[a:b].mean(axis=0) for a, b in zip(spk_off[:-1], spk_off[1:])]) if K else np.empty((len(spk_off) - 1, 0))
    res = {"estimate": means.mean(axis=0)}
    if K == 0:
        res.update(se=np.empty(0), lo=np.empty(0), hi=np.empty(0))
        return res
    reps = B.bootstrap_means(host, spk_off, st["n_boot"], st["seed"], st["resample"], device)
    _, se, qs, n_le0, n_ge0 = B.bootstrap_summary(reps, _quantile_levels(st["level"]))
    res.update(se=se, lo=qs[0], hi=qs[1])
    if return_replicates:
        res.update(replicates=reps, n_le0=n_le0, n_ge0=n_ge0)
    return res


def p_value(n_le0, n_ge0, n_boot):
    """Two-sided bootstrap p-value of "the aggregate of A - B is 0" from the replicate counts:
    min(1, 2 (min(n_le0, n_ge0) + 1) / (n_boot + 1)); NaN for a column without counts (-1)."""
    n_le0, n_ge0 = int(n_le0), int(n_ge0)
    if n_le0 < 0 or n_ge0 < 0:
        return math.nan
    return min(1.0, 2.0 * (min(n_le0, n_ge0) + 1) / (int(n_boot) + 1))


def _load_result(r):
    if isinstance(r, dict):
        return r
    with open(r, "r") as f:
        return json.load(f)


def _files_of(result):
    """{(speaker, file): {key: {metric: value}}} of an evaluate() result."""
    out = {}
    for spk, files in result.items():
        if spk in _AGGREGATE_KEYS or not isinstance(files, dict):
            continue
        for f, per_key in files.items():
            out[(spk, f)] = per_key
    return out


def _paired_tables(a, b):
    """Match two evaluate() results by (speaker, file) and intersect their keys and metrics.
    -> (table_a [N, K], table_b [N, K], speakers [N], columns [K] of (key, metric)): rows sorted by (speaker, file), columns in
    a's key and metric order.  ValueError (naming up to five of them) when a file is in one result only, or nothing is shared."""
    fa, fb = _files_of(a), _files_of(b)
    only = sorted(set(fa) ^ set(fb))
    if only:
        raise ValueError("%d file(s) are in only one of the two results: %s%s" % (
            len(only), ", ".join("%s/%s" % sf for sf in only[:5]), ", ..." if len(only) > 5 else ""))
    rows = sorted(fa)
    if not rows:
        raise ValueError("the results hold no per-file values")
    columns, seen = [], set()
    for sf in rows:                                      # a's order, first appearance first
        for k, mets in fa[sf].items():
            for m in mets:
                if (k, m) not in seen:
                    seen.add((k, m))
                    columns.append((k, m))
    columns = [(k, m) for k, m in columns if all(k in d[sf] and m in d[sf][k] for d in (fa, fb) for sf in rows)]
    if not columns:
        raise ValueError("the results share no (key, metric) that every file has")
    ta = np.array([[fa[sf][k][m] for k, m in columns] for sf in rows], dtype=np.float64).reshape(len(rows), len(columns))
    tb = np.array([[fb[sf][k][m] for k, m in columns] for sf in rows], dtype=np.float64).reshape(len(rows), len(columns))
    return ta, tb, [sf[0] for sf in rows], columns


def compare_results(a, b, n_boot=2000, level=0.95, seed=0, resample="utterance", device=None):
    """Paired comparison of two evaluate() results (the dicts, or the paths of the JSON files evaluate() wrote) over the same
    files: the bootstrap of the aggregate of the per-file differences A - B, the same drawn files for both systems.
    -> {key: {metric: {"diff", "se", "lo", "hi", "p"}}}: the difference of the two aggregates, its standard error, its percentile
    interval at `level` (which need not contain diff) and the two-sided p-value of p_value()."""
    st = check_settings(n_boot, level, seed, resample)
    ta, tb, speakers, columns = _paired_tables(_load_result(a), _load_result(b))
    with np.errstate(invalid="ignore"):
        r = bootstrap_ci(ta - tb, speakers, return_replicates=True, device=device, **st)
    out = {}
    for i, (k, m) in enumerate(columns):
        out.setdefault(k, {})[m] = {"diff": float(r["estimate"][i]), "se": float(r["se"][i]), "lo": float(r["lo"][i]),
                                    "hi": float(r["hi"][i]), "p": p_value(r["n_le0"][i], r["n_ge0"][i], st["n_boot"])}
    return out
