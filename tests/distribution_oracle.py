"""Float64 oracle of the distribution family for tests/test_distribution_host.py and
tests/test_gpu_distribution.py: the Fréchet distance by the nuclear-norm route (no matrix square root), the unbiased MMD^2 as three
explicit double loops, the median bandwidth by numpy.partition; the inputs of the tests, the packing of sets into one buffer and the
bars.  NumPy only; nothing here imports the library."""
import math

import numpy as np

TOL_MEAN = 1e-12          # of max |x|
TOL_COV = 1e-10           # of the largest diagonal entry
TOL_FD = 1e-9             # of S = tr Sigma_r + tr Sigma_e + |mu_r - mu_e|^2, full-rank inputs with cond(Sigma) <= 1e4
TOL_FD_DEFICIENT = 1e-6   # of S, rank-deficient inputs
TOL_KERNEL = 1e-10        # the three kernel means and mmd2
MAX_PAIR_ROWS = 2048


def moments(x):
    """(mu, Sigma with ddof = 1) of the rows of x, two passes; fewer than two rows: Sigma is NaN."""
    x = np.asarray(x, np.float64)
    n, d = x.shape
    mu = x.mean(axis=0) if n else np.full(d, np.nan)
    xc = x - mu
    cov = xc.T @ xc / (n - 1) if n >= 2 else np.full((d, d), np.nan)
    return mu, cov


def frechet(ref, est):
    """dict(fd, dmu2, tr_r, tr_e, tr_sqrt, S): tr sqrt(Sigma_r Sigma_e) = |R_c E_c^T|_* / sqrt((n - 1) (m - 1)), the sum of the singular
    values of the product of the centred data."""
    r, e = np.asarray(ref, np.float64), np.asarray(est, np.float64)
    n, m = len(r), len(e)
    if n < 2 or m < 2:
        return dict(fd=math.nan, dmu2=math.nan, tr_r=math.nan, tr_e=math.nan, tr_sqrt=math.nan, S=math.nan)
    mr, me = r.mean(axis=0), e.mean(axis=0)
    rc, ec = r - mr, e - me
    tr_r, tr_e = float(np.sum(rc * rc) / (n - 1)), float(np.sum(ec * ec) / (m - 1))
    dmu2 = float(np.sum((mr - me) ** 2))
    tr_sqrt = float(np.linalg.svd(rc @ ec.T, compute_uv=False).sum() / math.sqrt((n - 1) * (m - 1)))
    return dict(fd=dmu2 + tr_r + tr_e - 2.0 * tr_sqrt, dmu2=dmu2, tr_r=tr_r, tr_e=tr_e, tr_sqrt=tr_sqrt, S=tr_r + tr_e + dmu2)


def frechet_sqrtm(ref, est):
    """The published route: scipy.linalg.sqrtm of Sigma_r Sigma_e (full-rank sets only)."""
    from scipy.linalg import sqrtm
    (mr, cr), (me, ce) = moments(ref), moments(est)
    root = sqrtm(cr @ ce)
    return float(np.sum((mr - me) ** 2) + np.trace(cr) + np.trace(ce) - 2.0 * np.trace(root).real)


def rank_and_cond(x):
    """(rank, largest eigenvalue / smallest non-null eigenvalue) of the covariance of x; null: below 1e-9 of the largest."""
    w = np.linalg.eigvalsh(moments(x)[1])
    keep = w[w > 1e-9 * w.max()] if w.max() > 0 else w[:0]
    return len(keep), (float(keep.max() / keep.min()) if len(keep) else math.inf)


def sq_dist(x, y):
    d = x - y
    return float(np.dot(d, d))


def kernel_means(ref, est, gammas):
    """[n_gamma][4] = kd / scale (mmd2), mmd2, mean k(r, r), mean k(e, e) as three explicit double loops over the pairs."""
    r, e = np.asarray(ref, np.float64), np.asarray(est, np.float64)
    g = np.asarray(gammas, np.float64)
    n, m = len(r), len(e)
    if n < 2 or m < 2:
        return np.full((len(g), 4), np.nan)
    rr, ee, re = np.zeros(len(g)), np.zeros(len(g)), np.zeros(len(g))
    for i in range(n):
        for j in range(n):
            if i != j:
                rr += np.exp(-g * sq_dist(r[i], r[j]))
    for i in range(m):
        for j in range(m):
            if i != j:
                ee += np.exp(-g * sq_dist(e[i], e[j]))
    for i in range(n):
        for j in range(m):
            re += np.exp(-g * sq_dist(r[i], e[j]))
    rr, ee, re = rr / (n * (n - 1)), ee / (m * (m - 1)), re / (n * m)
    mmd2 = rr + ee - 2.0 * re
    return np.stack([mmd2, mmd2, rr, ee], axis=1)


def subsample_index(n, cap=MAX_PAIR_ROWS):
    n_sub = min(n, cap)
    return np.array([i * n // n_sub for i in range(n_sub)], np.int64)


def pairwise(x, index=None):
    """|x_i - x_j|, i < j, in row-major order of the upper triangle."""
    x = np.asarray(x, np.float64)
    if index is not None:
        x = x[np.asarray(index)]
    return np.array([math.sqrt(sq_dist(x[i], x[j])) for i in range(len(x)) for j in range(i + 1, len(x))])


def lower_median(d):
    """(value, position in d) of the lower median."""
    k = (len(d) - 1) // 2
    v = np.partition(d, k)[k]
    return float(v), int(np.argmin(np.abs(d - v)))


def median_gamma(ref):
    """gamma = 1 / (2 sigma^2), sigma the lower median of the pairwise distances of the evenly strided reference rows (NaN: fewer than
    two rows or sigma = 0)."""
    ref = np.asarray(ref, np.float64)
    if len(ref) < 2:
        return math.nan
    sigma, _ = lower_median(pairwise(ref, subsample_index(len(ref))))
    return 1.0 / (2.0 * sigma * sigma) if sigma > 0.0 else math.nan


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def gaussian_set(n, d, seed, cond=1e3, shift=0.0, scale=1.0, rank=None):
    """n rows of a Gaussian with a rotated covariance whose spectrum falls geometrically over `cond`; rank: the dimension of the subspace
    the rows (minus their mean) live in."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    s = np.sqrt(np.geomspace(1.0, 1.0 / cond, d)) if d > 1 else np.ones(1)
    if rank is not None:
        s[rank:] = 0.0
    return scale * ((rng.standard_normal((n, d)) * s) @ q.T) + shift + 0.3 * rng.standard_normal(d)


FRECHET_SHAPES = [(1, 5, 7), (2, 3, 3), (8, 40, 33), (33, 70, 80), (64, 300, 130), (65, 200, 129), (128, 400, 300)]      # (D, n, m)
DEFICIENT_SHAPES = [(32, 20, 150), (32, 150, 20), (32, 20, 24)]
KERNEL_SHAPES = [(2, 2, 1), (65, 63, 3), (64, 64, 32), (130, 70, 33), (200, 257, 128)]                                   # (n, m, D)
GAMMAS8 = [0.003, 0.01, 0.02, 0.05, 0.1, 0.3, 1.0, 2.5]


def frechet_sets(d, n, m, seed=0):
    """A reference and an estimate set whose sample covariances are well conditioned where they have full rank."""
    cond = 1e2 if min(n, m) < 4 * d else 1e3
    return gaussian_set(n, d, 100 + seed, cond), gaussian_set(m, d, 200 + seed, cond, shift=0.2, scale=1.1)


def pack(sets, dtype=np.float64, ld_extra=0, gap=0):
    """The sets in one buffer, rows ld = D + ld_extra apart, `gap` unused elements in front of every set; everything that is not a value
    is NaN.  -> (buffer, offsets int64, rows int64, D, ld)."""
    d = sets[0].shape[1]
    ld = d + ld_extra
    rows = np.array([len(s) for s in sets], np.int64)
    off, at = [], 0
    for s in sets:
        at += gap
        off.append(at)
        at += len(s) * ld
    buf = np.full(at + 1, np.nan, dtype)
    for s, o in zip(sets, off):
        view = buf[o:o + len(s) * ld].reshape(len(s), ld)
        view[:, :d] = s
    return buf, np.array(off, np.int64), rows, d, ld


def as_read(s, dtype):
    """The set as the kernels read it from a buffer of `dtype`, in float64."""
    return np.asarray(s).astype(dtype).astype(np.float64)


def check_frechet(out, mom, sets, dtype=np.float64, deficient=False, name=""):
    """out [K][8] and moments [1 + K][D + D D] of a run on sets = [ref, est_0, ...] against the oracle, at the bars -> the worst (mean / max |x|,
    cov / largest diagonal, fd / S) seen."""
    sets = [as_read(s, dtype) for s in sets]
    d = sets[0].shape[1]
    worst = [0.0, 0.0, 0.0]
    for s, m in zip(sets, mom):
        mu, cov = moments(s)
        if len(s) == 0:
            continue
        worst[0] = max(worst[0], float(np.max(np.abs(m[:d] - mu)) / max(np.max(np.abs(s)), 1e-300)))
        assert worst[0] <= TOL_MEAN, (name, "mean", worst[0])
        got = m[d:].reshape(d, d)
        if len(s) < 2:
            assert np.isnan(got).all(), (name, "covariance of fewer than two rows")
            continue
        assert same_bits(got, got.T), (name, "covariance not symmetric to the bit")
        scale = max(float(cov.diagonal().max()), 1e-300)
        worst[1] = max(worst[1], float(np.max(np.abs(got - cov)) / scale))
        assert worst[1] <= TOL_COV, (name, "cov", worst[1])
    for k, row in enumerate(out):
        o = frechet(sets[0], sets[1 + k])
        if math.isnan(o["fd"]):
            assert np.isnan(row[0]) and np.isnan(row[4]), (name, k, row)
            continue
        err = abs(row[0] - o["fd"]) / o["S"]
        worst[2] = max(worst[2], err)
        assert err <= (TOL_FD_DEFICIENT if deficient else TOL_FD), (name, k, "fd", err, row, o)
        assert abs(row[1] - o["dmu2"]) <= 1e-12 * o["S"] and abs(row[2] - o["tr_r"]) <= 1e-12 * o["S"] and abs(row[3] - o["tr_e"]) <= 1e-12 * o["S"], (name, row, o)
        assert abs(row[4] - o["tr_sqrt"]) <= (TOL_FD_DEFICIENT if deficient else TOL_FD) * o["S"], (name, k, "tr_sqrt")
        assert row[5] >= 1 and row[6] >= 1 and row[5] == int(row[5]) and row[6] == int(row[6]), (name, k, "sweeps", row)
        assert not np.isinf(row).any()
    return tuple(worst)


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()
