"""CPU tests of the distribution family (fd, kd): the float64 oracle (tests/distribution_oracle.py) pinned three
ways - to scipy.linalg.sqrtm on full-rank sets, to the closed form for D = 1 and to the closed form for commuting diagonal
covariances -; a g++ build of the kernel bodies (ssr_distribution.h) against the oracle - the shapes where the geometry can go wrong,
rank-deficient sets, the NaN rules, the data layouts, the bounded exit of the Jacobi, the bit-level properties -; the C ABI's argument
checks (they return before anything touches a device), the header / ctypes table / library agreement, and
SSR_Eval_Helper(distribution=...) validation and result shape.

Bars (distribution_oracle.TOL_*): means within 1e-12 max |x|, covariance entries within 1e-10 of the largest diagonal entry, fd within
1e-9 S on full-rank inputs with cond(Sigma) <= 1e4 (S = tr Sigma_r + tr Sigma_e + |dmu|^2) and within 1e-6 S on rank-deficient ones, the
three kernel means and mmd2 within 1e-10, rank_ref equal.  Worst differences seen in emulation: mean 3.6e-16 max |x|, covariance
1.1e-15 of the largest diagonal entry, fd 1.2e-14 S (D = 128) on full-rank sets and 2.3e-8 S on rank-deficient ones, kernel means
3.3e-14, at most 15 sweeps; on an MI355X: mean 3.6e-16, covariance 1.1e-15, fd 1.2e-14 S and 2.4e-8 S, kernel means 3.3e-14
(tests/test_gpu_distribution.py)."""
import ctypes as C
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest

import distribution_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
same_bits = O.same_bits


# ---- the oracle's pins ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,cond", [(16, 1e2), (32, 1e4), (64, 1e6)])
def test_oracle_matches_sqrtm_on_full_rank_sets(d, cond):
    r, e = O.gaussian_set(6 * d, d, 1, cond), O.gaussian_set(5 * d, d, 2, cond, shift=0.3, scale=1.2)
    o = O.frechet(r, e)
    err = abs(o["fd"] - O.frechet_sqrtm(r, e)) / o["S"]
    print(d, cond, "nuclear-norm route against sqrtm: %.3g S" % err)
    assert err <= 1e-9


def test_oracle_matches_the_closed_forms():
    rng = np.random.default_rng(3)
    r, e = 2.0 * rng.standard_normal((50, 1)) + 1.0, 0.5 * rng.standard_normal((70, 1)) - 2.0
    o = O.frechet(r, e)
    want = (r.mean() - e.mean()) ** 2 + (r.std(ddof=1) - e.std(ddof=1)) ** 2
    assert abs(o["fd"] - want) <= 1e-12 * o["S"]
    # commuting diagonal covariances: columns made exactly uncorrelated, fd = |dmu|^2 + sum (s_r - s_e)^2
    d = 6
    # (the orthonormal basis of CENTRED columns is centred itself: the sample covariance of q s sqrt(n - 1) is diag(s^2))
    xr, xe = rng.standard_normal((40, d)), rng.standard_normal((30, d))
    qr, qe = np.linalg.qr(xr - xr.mean(axis=0))[0], np.linalg.qr(xe - xe.mean(axis=0))[0]
    sr, se = np.linspace(1.0, 3.0, d), np.linspace(2.5, 0.5, d)
    r, e = qr * sr * math.sqrt(39), qe * se * math.sqrt(29) + 0.25
    cr, ce = O.moments(r)[1], O.moments(e)[1]
    assert np.max(np.abs(cr - np.diag(np.diag(cr)))) < 1e-10 and np.max(np.abs(ce - np.diag(np.diag(ce)))) < 1e-10
    o = O.frechet(r, e)
    want = o["dmu2"] + float(np.sum((np.sqrt(np.diag(cr)) - np.sqrt(np.diag(ce))) ** 2))
    assert abs(o["fd"] - want) <= 1e-9 * o["S"], (o, want)


def test_oracle_kernel_loops_and_median():
    r, e = O.gaussian_set(9, 4, 1, 10.0), O.gaussian_set(7, 4, 2, 10.0, shift=0.5)
    g = np.array([0.1, 0.7])
    got = O.kernel_means(r, e, g)
    d2 = lambda a, b: ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)      # noqa: E731
    for i, gi in enumerate(g):
        krr, kee, kre = np.exp(-gi * d2(r, r)), np.exp(-gi * d2(e, e)), np.exp(-gi * d2(r, e))
        rr, ee = (krr.sum() - 9) / 72, (kee.sum() - 7) / 42
        assert abs(got[i, 2] - rr) < 1e-14 and abs(got[i, 3] - ee) < 1e-14 and abs(got[i, 1] - (rr + ee - 2 * kre.mean())) < 1e-14
    assert np.isnan(O.kernel_means(r[:1], e, g)).all() and np.isnan(O.kernel_means(r, e[:1], g)).all()
    d = O.pairwise(r)
    assert len(d) == 36 and O.lower_median(d)[0] == np.sort(d)[17] and d[O.lower_median(d)[1]] == np.sort(d)[17]
    assert O.lower_median(np.array([3.0, 1.0, 2.0, 4.0]))[0] == 2.0
    assert list(O.subsample_index(5)) == [0, 1, 2, 3, 4] and list(O.subsample_index(10, 4)) == [0, 2, 5, 7]
    assert math.isnan(O.median_gamma(np.ones((5, 3)))) and math.isnan(O.median_gamma(r[:1]))


# ---- the kernel bodies compiled for the host ------------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "distribution_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libdistribution_emu.so")


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    lib = C.CDLL(EMU_SO)
    lib.frechet_emu.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    lib.kernel_distance_emu.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_double,
                                        C.c_void_p]
    lib.pairwise_emu.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def fd_run(lib, sets, dtype=np.float64, max_sweeps=60, moments=True, ld_extra=0, gap=0):
    """The emulation of ssr_frechet on sets = [ref, est_0, ...] -> (out [K][8], moments [1 + K][D + D D] or None)."""
    buf, off, rows, d, ld = O.pack(sets, dtype, ld_extra, gap)
    K = len(sets) - 1
    out = np.full((K, 8), -123.0)
    mom = np.full((K + 1, d + d * d), -123.0) if moments else None
    assert lib.frechet_emu(P(buf), int(dtype == np.float64), P(off), P(rows), K, d, ld, max_sweeps, P(out), P(mom)) == 0
    return out, mom


def kd_run(lib, sets, gammas, dtype=np.float64, scale=1000.0, ld_extra=0, gap=0):
    buf, off, rows, d, ld = O.pack(sets, dtype, ld_extra, gap)
    K, g = len(sets) - 1, np.ascontiguousarray(gammas, np.float64)
    out = np.full((K, len(g), 4), -123.0)
    assert lib.kernel_distance_emu(P(buf), int(dtype == np.float64), P(off), P(rows), K, d, ld, P(g), len(g), scale, P(out)) == 0
    return out


@pytest.mark.parametrize("d,n,m", O.FRECHET_SHAPES, ids=lambda v: str(v))
def test_emulated_frechet_shapes(emu, d, n, m):
    r, e = O.frechet_sets(d, n, m)
    for s in (r, e):
        rank, cond = O.rank_and_cond(s)
        assert rank == min(d, len(s) - 1) and cond <= 1e4, (rank, cond)
    out, mom = fd_run(emu, [r, e])
    worst = O.check_frechet(out, mom, [r, e], name=(d, n, m))
    print((d, n, m), "worst mean %.3g max|x|, cov %.3g, fd %.3g S; sweeps %d / %d, rank %d" % (worst + tuple(out[0, 5:])))
    assert out[0, 7] == O.rank_and_cond(r)[0] and out[0, 5] <= 30 and out[0, 6] <= 30
    # moments_out = NULL changes no bit
    assert same_bits(fd_run(emu, [r, e], moments=False)[0], out)


@pytest.mark.parametrize("d,n,m", O.DEFICIENT_SHAPES, ids=lambda v: str(v))
def test_emulated_frechet_rank_deficient(emu, d, n, m):
    r, e = O.frechet_sets(d, n, m)
    rank, cond = O.rank_and_cond(r)
    assert rank == min(d, n - 1) and cond < 1e6
    out, mom = fd_run(emu, [r, e])
    worst = O.check_frechet(out, mom, [r, e], deficient=True, name=(d, n, m))
    print((d, n, m), "rank-deficient: fd %.3g S; sweeps %d / %d, rank %d" % ((worst[2],) + tuple(out[0, 5:])))
    assert out[0, 7] == rank


def test_emulated_frechet_special_rows(emu):
    d = 8
    r, e = O.frechet_sets(d, 40, 33, seed=5)
    # a constant column: a null column of both covariances
    rc, ec = r.copy(), e.copy()
    rc[:, 3], ec[:, 3] = 2.5, 2.5
    out, mom = fd_run(emu, [rc, ec])
    O.check_frechet(out, mom, [rc, ec], deficient=True, name="constant column")
    assert out[0, 7] == d - 1
    # row means of 1e4 beside unit variance: the two-pass centring
    big = [O.gaussian_set(60, d, 7, 10.0) + 1e4, O.gaussian_set(50, d, 8, 10.0, scale=1.1) + 1e4]
    out, mom = fd_run(emu, big)
    worst = O.check_frechet(out, mom, big, name="means of 1e4")
    print("means of 1e4: cov %.3g of the largest diagonal entry, fd %.3g S" % worst[1:])
    # identical sets: a value of rounding size, of either sign, not clamped
    out, _ = fd_run(emu, [r, r.copy()])
    assert abs(out[0, 0]) <= 1e-12 * (out[0, 2] + out[0, 3]) and out[0, 1] == 0.0
    # n = 2, and fewer than two rows: NaN, no infinity
    out, mom = fd_run(emu, [r[:2], e])
    O.check_frechet(out, mom, [r[:2], e], deficient=True, name="n = 2")
    assert out[0, 7] == 1
    for sets in ([r[:1], e], [r, e[:1]], [r, e[:0]]):
        out, mom = fd_run(emu, sets)
        assert np.isnan(out[0, 0]) and np.isnan(out[0, 4]) and not np.isinf(out).any() and not np.isinf(mom).any()
    # a non-finite value in a set: NaN for that set only
    bad = e.copy()
    bad[5, 2] = np.inf
    out, _ = fd_run(emu, [r, bad, e])
    assert np.isnan(out[0, 0]) and out[0, 6] == -1 and not np.isinf(out).any() and same_bits(out[1], fd_run(emu, [r, e])[0][0])


def test_emulated_frechet_layouts_and_bit_level_properties(emu):
    d = 33
    res = np.zeros(4, np.int64)
    emu.distribution_geometry(d, P(res))
    chunk = int(res[0])
    assert chunk == max(256, 4 * d) and res[1] == 64 and res[3] == 1024
    r = O.gaussian_set(chunk + 1, d, 11, 1e2)                    # a row count one past a row chunk
    ests = [O.gaussian_set(m, d, 20 + m, 1e2, shift=0.1 * m / 70, scale=1.0 + m / 700) for m in (70, 2 * chunk, 131)]      # K = 3 sets of different m
    base, mom = fd_run(emu, [r] + ests)
    O.check_frechet(base, mom, [r] + ests, name="K = 3")
    # a set gives the same bits alone, as any of K and at any position; ld = D + 3 and NaN-filled gaps change nothing
    for k in range(3):
        alone, mom1 = fd_run(emu, [r, ests[k]])
        assert same_bits(alone[0], base[k]) and same_bits(mom1[1], mom[1 + k]) and same_bits(mom1[0], mom[0])
    back, _ = fd_run(emu, [r] + ests[::-1], ld_extra=3, gap=7)
    assert same_bits(back[::-1], base)
    # float32 rows: the bits of the widened values
    r32, e32 = r[:90].astype(np.float32), ests[0].astype(np.float32)
    out32, mom32 = fd_run(emu, [r32, e32], np.float32, ld_extra=3, gap=5)
    O.check_frechet(out32, mom32, [r32, e32], np.float32, name="float32")
    assert same_bits(out32, fd_run(emu, [r32.astype(np.float64), e32.astype(np.float64)])[0])
    # scaling both sets by a power of two scales fd by its square exactly
    for p2 in (2.0 ** -7, 2.0 ** 10):
        sc, _ = fd_run(emu, [p2 * r] + [p2 * x for x in ests])
        assert same_bits(sc[:, :5], base[:, :5] * p2 * p2) and same_bits(sc[:, 5:], base[:, 5:])


def test_emulated_jacobi_bounded_exit(emu):
    r, e = O.frechet_sets(32, 150, 140)
    out, _ = fd_run(emu, [r, e], max_sweeps=1)
    assert np.isnan(out[0, 0]) and np.isnan(out[0, 4]) and out[0, 5] == -1 and np.isfinite(out[0, 1:4]).all()
    full, _ = fd_run(emu, [r, e])
    assert 2 <= full[0, 5] <= 30 and 2 <= full[0, 6] <= 30
    exact, _ = fd_run(emu, [r, e], max_sweeps=int(max(full[0, 5:7])))
    assert same_bits(exact, full)


@pytest.mark.parametrize("n,m,d", O.KERNEL_SHAPES, ids=lambda v: str(v))
def test_emulated_kernel_distance_shapes(emu, n, m, d):
    r, e = O.gaussian_set(n, d, 1, 10.0, scale=1.0 / math.sqrt(d)), O.gaussian_set(m, d, 2, 10.0, shift=0.1, scale=1.0 / math.sqrt(d))
    want = O.kernel_means(r, e, O.GAMMAS8)
    got8 = kd_run(emu, [r, e], O.GAMMAS8, ld_extra=3, gap=5)
    worst = float(np.max(np.abs(got8[0, :, 1:] - want[:, 1:])))
    print((n, m, d), "worst kernel mean / mmd2 difference %.3g" % worst)
    assert worst <= O.TOL_KERNEL and same_bits(got8[0, :, 0], 1000.0 * got8[0, :, 1])
    # a row of gamma does not depend on the other gamma; 1 value of gamma
    for j in (0, 5):
        assert same_bits(kd_run(emu, [r, e], [O.GAMMAS8[j]])[0, 0], got8[0, j])
    # a set gives the same bits alone, as any of K and at any position; float32 rows
    e2 = O.gaussian_set(m + 3, d, 3, 10.0, scale=1.0 / math.sqrt(d))
    many = kd_run(emu, [r, e2, e, e2[:1]], O.GAMMAS8[:2])
    assert same_bits(many[1], got8[0, :2]) and same_bits(many[0], kd_run(emu, [r, e2], O.GAMMAS8[:2])[0]) and np.isnan(many[2]).all()
    r32, e32 = r.astype(np.float32), e.astype(np.float32)
    got32 = kd_run(emu, [r32, e32], O.GAMMAS8[:1], np.float32)
    assert np.max(np.abs(got32[0, :, 1:] - O.kernel_means(O.as_read(r, np.float32), O.as_read(e, np.float32), O.GAMMAS8[:1])[:, 1:])) <= O.TOL_KERNEL
    assert np.isnan(kd_run(emu, [r[:1], e], [0.1])).all() and np.isnan(kd_run(emu, [r, e[:0]], [0.1])).all()


@pytest.mark.parametrize("n", [2, 65, 130])
def test_emulated_pairwise_distances(emu, n):
    d = 5
    x = O.gaussian_set(n + 9, d, n, 10.0)
    index = (np.arange(n, dtype=np.int64) * 7) % (n + 9)
    for dtype in (np.float64, np.float32):
        buf, off, rows, _, ld = O.pack([x], dtype, ld_extra=2, gap=3)
        out = np.full(n * (n - 1) // 2, -1.0)
        assert emu.pairwise_emu(P(buf), int(dtype == np.float64), int(off[0]), n + 9, d, ld, P(index), n, P(out)) == 0
        want = O.pairwise(O.as_read(x, dtype), index)
        assert np.max(np.abs(out - want)) <= 1e-14 * max(1.0, want.max())
        if dtype == np.float64:
            v, at = O.lower_median(want)
            gv, gat = O.lower_median(out)
            assert gat == at and abs(gv - v) <= 1e-15 * v


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _fd(lib, rows, D=8, ld=None, off=None, K=None, max_sweeps=60, data=_DUMMY, out=_DUMMY, ws=_DUMMY, ws_bytes=1 << 50):
    rows = np.ascontiguousarray(rows, np.int64)
    off = np.zeros(len(rows), np.int64) if off is None else np.ascontiguousarray(off, np.int64)
    return lib.ssr_frechet(data, 1, P(off), P(rows), len(rows) - 1 if K is None else K, D, D if ld is None else ld, max_sweeps, out, None, ws,
                           ws_bytes, None)


def _kd(lib, rows, D=8, ld=None, off=None, K=None, gamma=(0.5,), n_gamma=None, scale=1000.0, data=_DUMMY, out=_DUMMY, ws=_DUMMY, ws_bytes=1 << 50):
    rows = np.ascontiguousarray(rows, np.int64)
    off = np.zeros(len(rows), np.int64) if off is None else np.ascontiguousarray(off, np.int64)
    g = np.ascontiguousarray(gamma, np.float64)
    return lib.ssr_kernel_distance(data, 1, P(off), P(rows), len(rows) - 1 if K is None else K, D, D if ld is None else ld, P(g),
                                   len(g) if n_gamma is None else n_gamma, scale, out, ws, ws_bytes, None)


def test_distribution_rejects_bad_arguments_before_launch():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E, U, W = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE
    for call in (_fd, _kd):
        assert call(lib, [10, 10], D=0) == E and "D must" in err()
        assert call(lib, [10, 10], D=1025, ld=2000) == U and "1024" in err()
        assert call(lib, [10, 10], D=8, ld=7) == E and "ld" in err()
        assert call(lib, [10, -1]) == E and "row counts" in err()
        assert call(lib, [-5, 10]) == E and call(lib, [10, 10], K=-1) == E
        assert call(lib, [10, 10], off=[0, -8]) == E and "offsets" in err()
        assert call(lib, [1 << 31, 10]) == U and "2^31" in err()
        assert call(lib, [10, 10], out=None) == E and call(lib, [10, 10], data=None) == E and "null" in err()
        assert call(lib, [10], K=0, data=None, out=None, ws=None, ws_bytes=0) == 0            # K = 0: nothing is enqueued
    for ms in (0, 201, -1):
        assert _fd(lib, [10, 10], max_sweeps=ms) == E and "max_sweeps" in err()
    for ng in (0, 9):
        assert _kd(lib, [10, 10], gamma=[0.5] * 9, n_gamma=ng) == E and "n_gamma" in err()
    for g in (0.0, -1.0, float("nan"), float("inf")):
        assert _kd(lib, [10, 10], gamma=[0.5, g]) == E and "gamma" in err()
    assert _kd(lib, [10, 10], scale=float("inf")) == E and "scale" in err()
    rows = np.array([300, 70, 1, 0], np.int64)
    need = lib.ssr_frechet_workspace_bytes(P(rows), 3, 33)
    assert need > 0 and _fd(lib, rows, D=33, ws_bytes=need - 1) == W and "workspace" in err() and _fd(lib, rows, D=33, ws=None) == W
    need = lib.ssr_kernel_distance_workspace_bytes(P(rows), 3, 33, 8)
    assert need > lib.ssr_kernel_distance_workspace_bytes(P(rows), 3, 33, 1) > 0
    assert _kd(lib, rows, D=33, gamma=[0.5] * 8, ws_bytes=need - 1) == W and "workspace" in err()
    for bad in ((P(rows), 3, 0), (P(rows), 3, 1025), (P(rows), -1, 8), (None, 3, 8), (P(np.array([5, -1], np.int64)), 1, 8)):
        assert lib.ssr_frechet_workspace_bytes(*bad) == 0 and lib.ssr_kernel_distance_workspace_bytes(*bad, 1) == 0
    assert lib.ssr_kernel_distance_workspace_bytes(P(rows), 3, 8, 0) == 0 and lib.ssr_kernel_distance_workspace_bytes(P(rows), 3, 8, 9) == 0
    # a launch of 2^32 threads: refused before anything is enqueued
    huge = np.array([1 << 22, 1 << 22], np.int64)
    assert lib.ssr_kernel_distance_workspace_bytes(P(huge), 1, 8, 1) == 0 and _kd(lib, huge) == U and "launch" in err()
    # ssr_pairwise_distances
    idx = np.arange(5, dtype=np.int64)
    pw = lambda n=5, rows=9, D=4, ld=4, index=idx, data=_DUMMY, out=_DUMMY, ws=_DUMMY, wsb=_lib.DISTRIBUTION_PAIRWISE_WORKSPACE: \
        lib.ssr_pairwise_distances(data, 1, 0, rows, D, ld, P(index), n, out, ws, wsb, None)      # noqa: E731
    assert pw(D=0) == E and pw(D=1025, ld=1025) == U and pw(ld=3) == E and pw(n=-1) == E and pw(n=2049) == E and pw(rows=-1) == E
    assert pw(index=np.array([0, 1, 2, 3, 9], np.int64)) == E and "index" in err() and pw(index=np.array([0, -1, 2, 3, 4], np.int64)) == E
    assert pw(out=None) == E and pw(data=None) == E and pw(wsb=_lib.DISTRIBUTION_PAIRWISE_WORKSPACE - 1) == W and pw(ws=None) == W
    assert pw(n=1) == 0 and pw(n=0, index=None) == 0


def test_header_ctypes_table_and_library_agree():
    from ssr_eval_amd import _lib
    path = os.path.join(ROOT, "ssr_eval_amd", "csrc", "ssr_hip_distribution.h")
    header = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    declared = set(re.findall(r"\b(ssr_[a-z_0-9]+)\s*\(", header))
    names = {"ssr_frechet_workspace_bytes", "ssr_frechet", "ssr_kernel_distance_workspace_bytes", "ssr_kernel_distance", "ssr_pairwise_distances"}
    assert declared == names == set(_lib.DISTRIBUTION_SIGNATURES)
    others = set(_lib.SIGNATURES) | set(_lib.COHERENCE_SIGNATURES) | set(_lib.LOUDNESS_SIGNATURES) | set(_lib.SPECTRUM_SIGNATURES) | \
        set(_lib.AUDITORY_SIGNATURES) | set(_lib.MODULATION_SIGNATURES)
    assert not names & others
    assert "#define SSR_DISTRIBUTION_MAX_DIM 1024" in header and "#define SSR_DISTRIBUTION_MAX_GAMMA 8" in header
    assert "#define SSR_DISTRIBUTION_PAIRWISE_WORKSPACE %d" % _lib.DISTRIBUTION_PAIRWISE_WORKSPACE in header
    assert (_lib.DISTRIBUTION_MAX_DIM, _lib.DISTRIBUTION_MAX_GAMMA, _lib.DISTRIBUTION_MAX_PAIR_ROWS) == (1024, 8, 2048)
    for name in names:
        n_args = len(re.search(r"\b%s\((.*?)\);" % name, header, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.DISTRIBUTION_SIGNATURES[name][1]), name
    lib = _lib.load()
    for name, (res, args) in _lib.DISTRIBUTION_SIGNATURES.items():
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name
    main = open(os.path.join(ROOT, "include", "ssr_hip.h")).read()
    inc = "#include \"../ssr_eval_amd/csrc/ssr_hip_distribution.h\""
    assert main.count(inc) == 1 and main.index(inc) > main.index("#include \"../ssr_eval_amd/csrc/ssr_hip_modulation.h\"")
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert all(" T %s\n" % name in exported for name in names)
    src = "#include \"%s\"\nint main(void) { return ssr_frechet_workspace_bytes(0, 0, 8) != 0 || SSR_DISTRIBUTION_MAX_DIM != 1024; }\n" % \
        os.path.join(ROOT, "include", "ssr_hip.h")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-"], input=src, text=True, check=True)


# ---- the Python layer without a device -------------------------------------------------------------------------------------------
def test_public_functions_validate_before_any_device_is_touched():
    import ssr_eval_amd as S
    from ssr_eval_amd import backend as B
    from ssr_eval_amd import distribution as DM
    assert all(callable(getattr(S, n)) for n in ("frechet_distance", "kernel_distance", "distribution_distance", "embed_logmel_stats"))
    x = np.zeros((5, 4))
    for bad in (np.zeros(5), np.zeros((5, 4), np.int32), np.zeros((5, 0)), np.zeros((5, 1025)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            S.frechet_distance(bad, x)
        with pytest.raises(ValueError):
            S.kernel_distance(x, bad, bandwidth=1.0)
    with pytest.raises(ValueError):
        S.frechet_distance(np.zeros((5, 3)), x)
    with pytest.raises(ValueError):
        S.frechet_distance([], x)
    for ms in (0, 201, 3.0, True, None):
        with pytest.raises(ValueError):
            S.frechet_distance(x, x, max_sweeps=ms)
    for bw in (0, -1.0, "mean", None, True, float("nan")):
        with pytest.raises(ValueError):
            S.kernel_distance(x, x, bandwidth=bw)
    for sc in ("1000", None, float("inf"), True):
        with pytest.raises(ValueError):
            S.kernel_distance(x, x, bandwidth=1.0, scale=sc)
    for g in ([], [0.1] * 9, [0.0], [float("nan")], "0.1"):
        with pytest.raises(ValueError):
            B.kernel_sums(x, [x], g)
    for m in ((), "fd", ("fd", "fd"), ("fad",), None):
        with pytest.raises(ValueError):
            S.distribution_distance(x, x, metrics=m)
    with pytest.raises(ValueError):
        B.pairwise_distances(x, np.arange(6))
    with pytest.raises(ValueError):
        B.pairwise_distances(np.zeros((3000, 2)))
    assert DM.check_metrics(["kd", "fd"]) == ("fd", "kd") and DM.METRICS == ("fd", "kd")


def test_helper_distribution_option_and_result_shape():
    import inspect
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee, compare_results
    from ssr_eval_amd import distribution as DM
    from ssr_eval_amd import eval as E
    from ssr_eval_amd import stats
    full_before = E.full_key_order()
    mk = lambda sr=44100, **kw: SSR_Eval_Helper(BasicTestee(), sr, sr, evaluation_sr=sr, test_data_root=None, **kw)      # noqa: E731
    assert mk().distribution is None and mk(distribution=None).distribution is None
    default = {"embed": "logmel_stats", "bandwidth": "median", "scale": 1000.0, "max_sweeps": 60, "metrics": ("fd", "kd")}
    assert mk(distribution=True).distribution == default
    stub = lambda waves, sr: np.stack([np.full(3, float(len(w))) for w in waves])      # noqa: E731
    got = mk(distribution={"embed": stub, "bandwidth": 2, "scale": 1, "max_sweeps": 100, "metrics": ["kd"]}).distribution
    assert got == {"embed": stub, "bandwidth": 2.0, "scale": 1.0, "max_sweeps": 100, "metrics": ("kd",)}
    for bad in (False, 1, "fd", (), {}, ["fd"], {"which": "fd"}, {"embed": "vggish"}, {"embed": None}, {"bandwidth": 0}, {"bandwidth": "mean"},
                {"bandwidth": None}, {"scale": "1000"}, {"scale": float("nan")}, {"max_sweeps": 0}, {"max_sweeps": 201}, {"max_sweeps": 60.0},
                {"metrics": ()}, {"metrics": "fd"}, {"metrics": ("fd", "lsd")}, {"metrics": None}):
        with pytest.raises(ValueError) as info:
            mk(distribution=bad)
        assert "distribution must be" in str(info.value) or "must" in str(info.value)
    with pytest.raises(ValueError, match="'embed', 'bandwidth', 'scale', 'max_sweeps' and / or 'metrics'"):
        mk(distribution={"gamma": 1.0})
    params = inspect.signature(SSR_Eval_Helper.__init__).parameters
    assert params["distribution"].kind is inspect.Parameter.KEYWORD_ONLY
    # not a per-file family: no registry row, full_key_order() as it was
    assert "distribution" not in [f.option for f in E._FAMILIES + E._LATER_FAMILIES + E._TAIL_FAMILIES]
    assert E.full_key_order() == full_before and E.full_key_order()[-2:] == ("nsim", "nsim_hf") and "fd" not in E.full_key_order()
    # a synthetic gathered row table: 5 files, target + 2 keys, D = 3, through the stub embedding and a stub distance
    h = mk(distribution={"embed": stub})
    keys = ["proc_fft_8000_44100", "proc_fft_16000_44100"]
    waves = [torch_zeros(10 + i) for i in range(5)]
    emb = DM.embed_waves(h.distribution, h.audio_metrics, waves, 44100)
    assert emb.shape == (5, 3) and emb.dtype == np.float64 and emb[2, 0] == 12.0
    local = [{"": emb[i], keys[0]: emb[i] + 1.0, keys[1]: emb[i] + 2.0} for i in range(5)]
    table = h._gather_embeddings(local[::2] + local[1::2], keys, [0, 2, 4, 1, 3], 5, gather=lambda rows, mine, n: np.asarray(rows)[np.argsort(mine)])
    assert table.shape == (5, 9) and np.array_equal(table[:, :3], emb) and np.array_equal(table[:, 6:], emb + 2.0)
    seen = {}

    def distance(ests, ref, bandwidth, scale, max_sweeps, metrics):
        seen.update(ests=ests, ref=ref, args=(bandwidth, scale, max_sweeps, metrics))
        return {"fd": [float(e.mean() - ref.mean()) for e in ests], "kd": [0.5, 0.25]}
    block = DM.result_block(h.distribution, keys, table, distance)
    assert list(block) == ["settings", "dim", "n", "per_key"] and block["dim"] == 3 and block["n"] == 5
    assert block["settings"] == {"embed": "callable", "bandwidth": "median", "scale": 1000.0, "max_sweeps": 60, "metrics": ["fd", "kd"]}
    assert block["per_key"] == {keys[0]: {"fd": 1.0, "kd": 0.5}, keys[1]: {"fd": 2.0, "kd": 0.25}}
    assert np.array_equal(seen["ref"], emb) and seen["args"] == ("median", 1000.0, 60, ("fd", "kd")) and len(seen["ests"]) == 2
    for bad in (lambda w, sr: np.zeros((len(w) + 1, 3)), lambda w, sr: np.zeros(3), lambda w, sr: np.zeros((len(w), 2000))):
        with pytest.raises(ValueError):
            DM.embed_waves({"embed": bad}, None, waves, 44100)
    # compare_results does not take the block for a speaker
    assert "distribution" in stats._AGGREGATE_KEYS
    res = {"p1": {"a.wav": {keys[0]: {"lsd": 1.0}}, "b.wav": {keys[0]: {"lsd": 2.0}}}, "each_speaker": {}, "averaged": {}, "distribution": block}
    assert set(stats._files_of(res)) == {("p1", "a.wav"), ("p1", "b.wav")}
    assert compare_results is not None


def torch_zeros(n):
    import torch
    return torch.zeros(n)
