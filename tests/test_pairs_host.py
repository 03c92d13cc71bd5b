"""CPU tests of what the per-pair metric families share (ssr_eval_amd/csrc/ssr_pairs.h), through a g++ build of the bodies
(tests/emu/pairs_emu.cpp): the run geometry - runs of consecutive pairs with one target, item prefix sums over runs and over
pairs, the frame window - against a NumPy restatement, and the prefix search on prefixes with repeated entries."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SRC = os.path.join(ROOT, "tests", "emu", "pairs_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libpairs_emu.so")
POISON = -777


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    lib = C.CDLL(EMU_SO)
    assert lib.pairs_nt() == 256
    return lib


P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731


def pair_index(n_est):
    """tgt_index of n_est pairs in runs of 1, 2, .. 5, 1, .. pairs: run k names target k + 1, except that run 3 names the target
    of run 1 again (a target that reappears in a later, non-adjacent run); target 0 is never referenced.  -> (index, n_tgt)"""
    idx, k = [], 0
    while len(idx) < n_est:
        idx += [(2 if k == 3 else k + 1)] * (k % 5 + 1)
        k += 1
    return np.array(idx[:n_est], np.int32), k + 1


def numpy_geometry(counts, idx):
    """(run_start, run prefix, pair prefix) from the run boundaries and the cumulative sums of the counts."""
    n = len(idx)
    first = np.concatenate(([0], 1 + np.flatnonzero(np.diff(idx)))).astype(np.int64) if n else np.zeros(0, np.int64)
    per_pair = counts[idx].astype(np.int64)
    run_start = np.concatenate((first, [n])).astype(np.int32)
    run_pre = np.concatenate(([0], np.cumsum(per_pair[first]))).astype(np.int64)
    pair_pre = np.concatenate(([0], np.cumsum(per_pair))).astype(np.int64)
    return run_start, run_pre, pair_pre


@pytest.mark.parametrize("n_est", [0, 1, 255, 256, 257, 2 * 256 + 3])
def test_run_geometry_matches_numpy(emu, n_est):
    idx, n_tgt = pair_index(n_est)
    rng = np.random.default_rng(n_est)
    counts = rng.integers(0, 40, n_tgt).astype(np.int32)
    counts[rng.random(n_tgt) < 0.3] = 0                       # targets without a tile / frame
    counts[0] = 1 << 30                                       # the unreferenced target: must not show anywhere
    if n_est > 8:
        assert (counts[idx] == 0).any() and len(set(idx)) < len(numpy_geometry(counts, idx)[0]) - 1
    want = numpy_geometry(counts, idx)
    n_runs, L = len(want[0]) - 1, 37
    run_start = np.full(n_runs + 2, POISON, np.int32)         # one guard element behind each array
    run_pre = np.full(n_runs + 2, POISON, np.int64)
    pair_pre = np.full(n_est + 2, POISON, np.int64)
    win = np.full(L + 1, float(POISON))
    emu.pairs_run_geometry(P(counts), P(idx), n_est, L, P(run_start), P(run_pre), P(pair_pre), P(win))
    assert np.array_equal(run_start[:-1], want[0]) and run_start[-1] == POISON
    assert np.array_equal(run_pre[:-1], want[1]) and run_pre[-1] == POISON
    assert np.array_equal(pair_pre[:-1], want[2]) and pair_pre[-1] == POISON
    assert want[2][-1] < 1 << 30
    # the families' frame window (Loizou's Hann): one libm cos per sample on either side
    i = np.arange(L)
    assert np.max(np.abs(win[:L] - 0.5 * (1.0 - np.cos(2.0 * np.pi * (i + 1) / (L + 1))))) <= 2 ** -52 and win[L] == POISON


def test_prefix_find_on_repeated_entries(emu):
    """The item that owns grid block g is the LAST one whose prefix entry is <= g: an item with no blocks shares its entry with
    its successor and is never returned."""
    counts = np.array([0, 3, 0, 0, 1, 2, 0, 4, 0], np.int64)
    off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    n, total = len(counts), int(off[-1])
    owner = np.repeat(np.arange(n), counts)
    emu.pairs_prefix_find.argtypes = [C.c_void_p, C.c_int, C.c_int64]
    for g in range(total):                                    # the first, the last and every boundary value (all of them)
        assert emu.pairs_prefix_find(P(off), n, g) == owner[g], g
    for g in np.unique(off[off < total]):                     # each boundary names the item that starts there ...
        s = emu.pairs_prefix_find(P(off), n, int(g))
        assert off[s] == g and counts[s] > 0
        if g > 0:                                             # ... and the block before it the item that ends there
            assert emu.pairs_prefix_find(P(off), n, int(g) - 1) == owner[int(g) - 1] < s
    assert emu.pairs_prefix_find(P(off), 1, 0) == 0
