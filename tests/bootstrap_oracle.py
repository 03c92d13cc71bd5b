"""NumPy oracle of the bootstrap of the aggregate: Philox4x32-10 restated on uint64 arrays, the draws of both
resampling schemes, the replicates with every sum taken sequentially (np.cumsum) in the documented order, and the per-column
summary through NumPy's own mean / std / quantile.  Checker only: nothing in ssr_eval_amd imports it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
SCHEMES = {"utterance": 0, "speaker": 1}


def philox(counter, key):
    """Philox4x32-10 of counters [..., 4] (any integer dtype, values < 2^32) under key (k0, k1) -> uint32 [..., 4]."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)          # < 2^64: exact
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(MASK), p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def key_of(seed):
    seed = int(seed)
    return seed & MASK, (seed >> 32) & MASK


def pick(u, n):
    """Index in [0, n) selected by the 32-bit words u: the high half of the 64-bit product."""
    return ((np.asarray(u).astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def file_draws(bs, t, n, seed):
    """[len(bs), n]: the n file draws (indices in [0, n)) of slot t in the replicates bs."""
    bs = np.asarray(bs, np.int64)
    nblk = (n + 3) // 4
    ctr = np.zeros((len(bs), nblk, 4), np.int64)
    ctr[..., 0] = bs[:, None]
    ctr[..., 1] = np.arange(nblk)[None, :]
    ctr[..., 2] = t
    return pick(philox(ctr, key_of(seed)).reshape(len(bs), 4 * nblk)[:, :n], n)


def slot_speakers(n_boot, n_spk, seed, scheme):
    """[n_boot, n_spk]: the speaker of every slot of every replicate."""
    if scheme == "utterance":
        return np.broadcast_to(np.arange(n_spk), (n_boot, n_spk)).copy()
    assert scheme == "speaker", scheme
    nblk = (n_spk + 3) // 4
    ctr = np.zeros((n_boot, nblk, 4), np.int64)
    ctr[..., 0] = np.arange(n_boot)[:, None]
    ctr[..., 1] = np.arange(nblk)[None, :]
    ctr[..., 3] = 1
    return pick(philox(ctr, key_of(seed)).reshape(n_boot, 4 * nblk)[:, :n_spk], n_spk)


def _slots(spk_off, n_boot, seed, scheme):
    """Yields (t, bs, rows): for slot t, the replicates bs whose slot holds one speaker and the table rows [len(bs), n] they draw."""
    spk_off = np.asarray(spk_off, np.int64)
    S = len(spk_off) - 1
    spk = slot_speakers(n_boot, S, seed, scheme)
    for t in range(S):
        for s in np.unique(spk[:, t]):
            bs = np.nonzero(spk[:, t] == s)[0]
            n = int(spk_off[s + 1] - spk_off[s])
            yield t, bs, spk_off[s] + file_draws(bs, t, n, seed)


def draw_counts(spk_off, n_boot, seed, scheme):
    """[n_boot, N] int64: how often each table row is drawn in each replicate (all slots together)."""
    N = int(spk_off[-1])
    cnt = np.zeros((n_boot, N), np.int64)
    for _, bs, rows in _slots(spk_off, n_boot, seed, scheme):
        np.add.at(cnt, (np.repeat(bs, rows.shape[1]), rows.ravel()), 1)
    return cnt


def replicates(table, spk_off, n_boot, seed=0, scheme="utterance"):
    """[n_boot, K] float64.  Per replicate and column: for slot t = 0 .. S-1 the sequential sum of the drawn rows in draw order,
    divided by their number; those slot means added sequentially in slot order; divided by S."""
    table = np.asarray(table, np.float64)
    S, K = len(spk_off) - 1, table.shape[1]
    total = np.zeros((n_boot, K))
    for t, bs, rows in _slots(spk_off, n_boot, seed, scheme):       # t ascends: every replicate meets its slots in order
        n = rows.shape[1]
        step = max(1, (1 << 22) // max(1, n * K))
        for a in range(0, len(bs), step):
            total[bs[a:a + step]] += np.cumsum(table[rows[a:a + step]], axis=1)[:, -1, :] / n
    reps = total / S
    reps[:, ~np.isfinite(table).all(axis=0)] = np.nan
    return reps


def estimate(table, spk_off):
    """The aggregate itself: the plain mean over speakers of each speaker's mean over its files."""
    table = np.asarray(table, np.float64)
    return np.mean([table[a:b].mean(axis=0) for a, b in zip(spk_off[:-1], spk_off[1:])], axis=0)


def summary(reps, q):
    """(out [K, 2 + len(q)]: mean, standard error (ddof 1), quantiles; counts [K, 2]: replicates <= 0 and >= 0); a column holding a
    non-finite replicate: NaN and -1."""
    reps = np.asarray(reps, np.float64)
    B, K = reps.shape
    out = np.full((K, 2 + len(q)), np.nan)
    counts = np.full((K, 2), -1, np.int32)
    ok = np.isfinite(reps).all(axis=0)
    r = reps[:, ok]
    out[ok, 0] = r.mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[ok, 1] = r.std(axis=0, ddof=1) if B > 1 else np.nan
    if len(q):
        out[ok, 2:] = np.quantile(r, np.asarray(q, np.float64), axis=0).T
    counts[ok, 0] = (r <= 0).sum(axis=0)
    counts[ok, 1] = (r >= 0).sum(axis=0)
    return out, counts


def closed_form_se(table, spk_off):
    """Standard error of scheme "utterance" in closed form: (1 / S) sqrt(sum_s var_s (n_s - 1) / n_s^2), var_s with ddof 1 - the
    variance of a mean of n_s draws with replacement from the speaker's n_s values is (their ddof-0 variance) / n_s."""
    table = np.asarray(table, np.float64)
    S = len(spk_off) - 1
    acc = 0.0
    for a, b in zip(spk_off[:-1], spk_off[1:]):
        n = b - a
        acc = acc + table[a:b].var(axis=0, ddof=1) * (n - 1) / n ** 2
    return np.sqrt(acc) / S
