"""CPU tests of the bootstrap of the aggregate: Philox4x32-10 known answers through the NumPy oracle
(tests/bootstrap_oracle.py) and through the kernel body, a g++ build of the kernel bodies (ssr_bootstrap.h) against the oracle, the
C ABI's argument checks (they return before anything touches a device), the host half of compare_results (_paired_tables, the
p-value formula, the settings) and a sanity check of the oracle against the closed-form standard error."""
import ctypes as C
import glob
import json
import math
import os
import subprocess

import numpy as np
import pytest

import bootstrap_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

KNOWN = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
QS = np.array([0.025, 0.975, 0.0, 1.0])


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


# ---- the oracle alone ---------------------------------------------------------------------------------------------------------
def test_oracle_philox_known_answers():
    for ctr, key, want in KNOWN:
        assert _hex(O.philox(np.array(ctr, np.int64), key)) == want
    both = O.philox(np.array([k[0] for k in KNOWN[:1]] * 3, np.int64), (0, 0))          # vectorised: a row per counter
    assert both.shape == (3, 4) and _hex(both[2]) == KNOWN[0][2]
    assert O.key_of((0x299f31d0 << 32) | 0xa4093822) == KNOWN[2][1]


def test_oracle_draws_are_indices_and_independent_of_the_batch():
    off = np.array([0, 3, 10, 11])
    for scheme in ("utterance", "speaker"):
        cnt = O.draw_counts(off, 50, 5, scheme)
        assert cnt.shape == (50, 11) and (cnt >= 0).all()
        spk = O.slot_speakers(50, 3, 5, scheme)
        sizes = np.diff(off)
        assert (cnt.sum(axis=1) == sizes[spk].sum(axis=1)).all()
        np.testing.assert_array_equal(O.draw_counts(off, 7, 5, scheme), cnt[:7])            # replicate b does not depend on B
    assert (O.draw_counts(off, 20, 5, "utterance")[:, 10] == 1).all()                       # a one-file speaker: its file, once
    assert not np.array_equal(O.draw_counts(off, 20, 5, "utterance"), O.draw_counts(off, 20, 6, "utterance"))


def test_oracle_standard_error_matches_the_closed_form():
    """3 speakers of 40, 25 and 60 iid normal files, B = 4,000: the bootstrap SE of scheme "utterance" within 5 % of
    (1 / S) sqrt(sum_s var_s (n_s - 1) / n_s^2).  The relative standard deviation of an SE from B replicates is about
    1 / sqrt(2 B) = 1.1 %: 5 % is 4.5 sigma."""
    rng = np.random.default_rng(2024)
    off = np.array([0, 40, 65, 125])
    table = rng.standard_normal((125, 3)) * np.array([1.0, 0.2, 5.0]) + np.array([0.0, 3.0, -40.0])
    table += np.repeat([0.0, 2.0, -1.0], np.diff(off))[:, None] * np.array([1.0, 0.2, 5.0])      # the speakers differ
    reps = O.replicates(table, off, 4000, seed=11, scheme="utterance")
    se = reps.std(axis=0, ddof=1)
    want = O.closed_form_se(table, off)
    assert np.abs(se / want - 1).max() < 0.05, (se, want)
    assert (np.abs(reps.mean(axis=0) - O.estimate(table, off)) < 5 * want / math.sqrt(4000)).all()      # E[replicate] = the estimate
    # redrawing the speakers as well can only add variance
    assert (O.replicates(table, off, 4000, seed=11, scheme="speaker").std(axis=0, ddof=1) > se).all()


# ---- the kernel bodies compiled for the host ---------------------------------------------------------------------------------
EMU_SRC = os.path.join(ROOT, "tests", "emu", "bootstrap_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libbootstrap_emu.so")


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    return C.CDLL(EMU_SO)


def _tile(emu):
    t, b = C.c_int(), C.c_int()
    emu.boot_geometry_emu(C.byref(t), C.byref(b))
    assert b.value == 16384
    return t.value


def _offsets(sizes):
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)


def _means(emu, table, off, n_boot, seed, scheme):
    table = np.ascontiguousarray(table, np.float64)
    reps = np.full((n_boot, table.shape[1]), -123.0)
    assert emu.boot_means_emu(P(table), C.c_int64(table.shape[0]), table.shape[1], P(off), len(off) - 1, n_boot, C.c_uint64(seed),
                              O.SCHEMES[scheme], P(reps)) == 0
    return reps


def _summary(emu, reps, q=QS):
    reps = np.ascontiguousarray(reps, np.float64)
    out = np.full((reps.shape[1], 2 + len(q)), -123.0)
    counts = np.full((reps.shape[1], 2), -7, np.int32)
    assert emu.boot_summary_emu(P(reps), reps.shape[0], reps.shape[1], P(np.ascontiguousarray(q)), len(q), P(out), P(counts)) == 0
    return out, counts


def test_emulated_philox_known_answers(emu):
    for ctr, key, want in KNOWN:
        out = np.zeros(4, np.uint32)
        emu.boot_philox_emu(P(np.array(ctr, np.uint32)), P(np.array(key, np.uint32)), P(out))
        assert _hex(out) == want


@pytest.mark.parametrize("scheme", ["utterance", "speaker"])
def test_emulated_draws_match_the_oracle_exactly(emu, scheme):
    """The table is the identity: replicate b of column i, times S n_s, is how often file i was drawn."""
    sizes = np.array([1, 5, 7, 64, _tile(emu) + 3])
    off = _offsets(sizes)
    N, S = int(off[-1]), len(sizes)
    scale = S * np.repeat(sizes, sizes)
    for seed in (3, (0xfeedbeef << 32) | 12345):
        for B in (1, 3, 257)[:2 if seed == 3 else 3]:
            reps = _means(emu, np.eye(N), off, B, seed, scheme)
            np.testing.assert_array_equal(np.round(reps * scale).astype(np.int64), O.draw_counts(off, B, seed, scheme))


@pytest.mark.parametrize("scheme", ["utterance", "speaker"])
def test_emulated_replicates_match_the_oracle(emu, scheme):
    sizes = np.array([1, 5, 7, 64, _tile(emu) + 3])
    off = _offsets(sizes)
    table = 100.0 + np.random.default_rng(8).standard_normal((int(off[-1]), 130))
    wide = _means(emu, table, off, 257, 21, scheme)
    for K in (1, 65, 130):
        got = wide if K == 130 else _means(emu, table[:, :K], off, 257, 21, scheme)
        want = O.replicates(table[:, :K], off, 257, 21, scheme)
        assert (np.abs(got - want) <= 1e-12 * np.abs(table[:, :K]).max(axis=0)).all()
        np.testing.assert_array_equal(got, wide[:, :K])                 # a table alone gives the bits it gives in a wider one


def test_emulated_summary_matches_numpy(emu):
    off = _offsets([5, 7, 64])
    rng = np.random.default_rng(9)
    table = rng.standard_normal((int(off[-1]), 4)) + np.array([0.0, 0.02, -0.05, 100.0])
    all_reps = O.replicates(table, off, 16384, 4, "utterance")
    scale = np.abs(table).max(axis=0)
    assert (np.abs(all_reps) > 1e-9 * scale).all()                      # no replicate so close to 0 that a count could flip
    for B in (1, 2, 1000, 16384):
        reps = _means(emu, table, off, B, 4, "utterance")
        np.testing.assert_array_equal(reps, all_reps[:B])               # (this oracle restates the kernel's order: same bits)
        out, counts = _summary(emu, reps)
        want, wcounts = O.summary(all_reps[:B], QS)
        np.testing.assert_array_equal(counts, wcounts)
        if B == 1:
            assert np.isnan(out[:, 1]).all() and (out[:, 2] == out[:, 3]).all()
            assert np.isnan(want[:, 1]).all()
            out[:, 1] = want[:, 1] = 0.0
        assert (np.abs(out[:, 2:] - want[:, 2:]) <= 1e-13 * np.abs(reps).max()).all()
        assert (np.abs(out - want) <= 1e-12 * np.abs(reps).max()).all()
    assert counts[3].tolist() == [0, 16384] and 0 < counts[0, 0] < 16384 and counts[0].sum() == 16384
    np.testing.assert_array_equal(_summary(emu, np.zeros((10, 2)))[1], np.full((2, 2), 10))       # every replicate is 0: both


def test_emulated_non_finite_columns(emu):
    off = _offsets([5, 7, 64, 200])
    table = np.random.default_rng(10).standard_normal((int(off[-1]), 70))
    clean = _means(emu, table, off, 50, 1, "speaker")
    dirty = table.copy()
    dirty[140, 3] = np.nan
    dirty[2, 7] = np.inf
    reps = _means(emu, dirty, off, 50, 1, "speaker")
    bad = np.zeros(70, bool)
    bad[[3, 7]] = True
    assert np.isnan(reps[:, bad]).all()
    np.testing.assert_array_equal(reps[:, ~bad], clean[:, ~bad])
    out, counts = _summary(emu, reps)
    wout, wcounts = _summary(emu, clean)
    assert np.isnan(out[bad]).all() and (counts[bad] == -1).all()
    np.testing.assert_array_equal(out[~bad], wout[~bad])
    np.testing.assert_array_equal(counts[~bad], wcounts[~bad])


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _abi_means(lib, off, n_rows=None, n_cols=3, n_boot=10, scheme=0, table=_DUMMY, reps=_DUMMY, n_spk=None, off_ptr=True):
    off = np.ascontiguousarray(off, np.int32)
    return lib.ssr_bootstrap_means(table, int(off[-1]) if n_rows is None else n_rows, n_cols, P(off) if off_ptr else None,
                                   len(off) - 1 if n_spk is None else n_spk, n_boot, 0, scheme, reps, None)


def _abi_summary(lib, q, n_boot=10, n_cols=3, reps=_DUMMY, out=_DUMMY, counts=_DUMMY, n_q=None):
    q = np.ascontiguousarray(q, np.float64)
    return lib.ssr_bootstrap_summary(reps, n_boot, n_cols, P(q), len(q) if n_q is None else n_q, out, counts, None)


def test_c_abi_rejects_bad_arguments_before_launch():
    from ssr_eval_amd import _lib
    lib = _lib.load()
    err = lambda: lib.ssr_last_error().decode()      # noqa: E731
    E, U = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
    good = [0, 4, 9]
    assert _abi_means(lib, good, table=None) == E and "null" in err()
    assert _abi_means(lib, good, reps=None) == E and "null" in err()
    assert _abi_means(lib, good, off_ptr=False) == E and "null" in err()
    assert _abi_means(lib, good, n_spk=0) == E and "n_spk" in err()
    assert _abi_means(lib, good, n_cols=0) == E and "n_cols" in err()
    assert _abi_means(lib, good, n_rows=0) == E and "n_rows" in err()
    assert _abi_means(lib, [0, 4, 4, 9]) == E and "empty speaker" in err()
    assert _abi_means(lib, [0, 6, 4, 9]) == E and "ascend" in err()
    assert _abi_means(lib, [1, 4, 9]) == E and "spk_off" in err()
    assert _abi_means(lib, good, n_rows=10) == E and "spk_off" in err()
    assert _abi_means(lib, good, n_boot=0) == E and "n_boot" in err()
    assert _abi_means(lib, good, n_boot=16385) == U and "n_boot" in err()
    assert _abi_means(lib, good, scheme=2) == E and "scheme" in err()
    assert _abi_means(lib, np.arange(514)) == U and "speakers" in err()
    assert _abi_summary(lib, [0.5], reps=None) == E and "null" in err()
    assert _abi_summary(lib, [0.5], out=None) == E and "null" in err()
    assert _abi_summary(lib, [0.5], counts=None) == E and "null" in err()
    assert _abi_summary(lib, np.linspace(0, 1, 9)) == E and "n_q" in err()
    assert _abi_summary(lib, [0.5], n_q=-1) == E and "n_q" in err()
    for q in (-0.01, 1.01, float("nan")):
        assert _abi_summary(lib, [0.5, q]) == E and "q must" in err()
    assert _abi_summary(lib, [0.5], n_boot=0) == E and "n_boot" in err()
    assert _abi_summary(lib, [0.5], n_boot=16385) == U and "n_boot" in err()
    assert _abi_summary(lib, [0.5], n_cols=0) == E and "n_cols" in err()
    t, b = C.c_int(), C.c_int()
    assert lib.ssr_bootstrap_geometry(C.byref(t), C.byref(b)) == 0 and t.value >= 4 and t.value % 4 == 0 and b.value == 16384
    assert lib.ssr_bootstrap_geometry(None, C.byref(b)) == E and "null" in err()


# ---- the host half of the Python surface ---------------------------------------------------------------------------------------
def _result(speakers, keys=("proc_fft_8000_44100", "proc_fft_16000_44100"), mets=("lsd", "ssim"), shift=0.0, seed=0):
    rng = np.random.default_rng(seed)
    res = {}
    for spk, files in speakers.items():
        res[spk] = {f: {k: {m: float(rng.standard_normal() + shift) for m in mets} for k in keys} for f in files}
    res["each_speaker"] = {spk: {k: {m: 0.0 for m in mets} for k in keys} for spk in speakers}
    res["averaged"] = {k: {m: 0.0 for m in mets} for k in keys}
    return res


SPEAKERS = {"p360": ["a.wav", "b.wav", "c.wav"], "p361": ["a.wav"], "s5": ["x.flac", "y.flac"]}


def test_paired_tables_do_not_depend_on_the_order_of_either_result(tmp_path):
    from ssr_eval_amd.stats import _paired_tables
    a, b = _result(SPEAKERS, seed=1), _result(SPEAKERS, seed=2)
    ta, tb, spk, cols = _paired_tables(a, b)
    assert ta.shape == tb.shape == (6, 4) and spk == ["p360"] * 3 + ["p361"] + ["s5"] * 2
    assert cols == [(k, m) for k in ("proc_fft_8000_44100", "proc_fft_16000_44100") for m in ("lsd", "ssim")]
    assert ta[1, 3] == a["p360"]["b.wav"]["proc_fft_16000_44100"]["ssim"] and tb[5, 0] == b["s5"]["y.flac"]["proc_fft_8000_44100"]["lsd"]
    shuffled = {s: {f: b[s][f] for f in reversed(list(b[s]))} for s in reversed(list(SPEAKERS))}
    shuffled["confidence"] = {"settings": {}, "averaged": {}}
    ta2, tb2, spk2, cols2 = _paired_tables(a, shuffled)
    np.testing.assert_array_equal(ta2, ta)
    np.testing.assert_array_equal(tb2, tb)
    assert spk2 == spk and cols2 == cols
    # ... and a result read back from its JSON is the same result
    from ssr_eval_amd.stats import _load_result
    path = tmp_path / "b.json"
    path.write_text(json.dumps(b, indent=4))
    np.testing.assert_array_equal(_paired_tables(a, _load_result(str(path)))[1], tb)


def test_paired_tables_intersect_keys_and_metrics():
    from ssr_eval_amd.stats import _paired_tables
    a = _result(SPEAKERS, keys=("k1", "k2", "k3"), mets=("lsd", "ssim", "stoi"), seed=3)
    b = _result(SPEAKERS, keys=("k3", "k2", "k9"), mets=("ssim", "lsd", "mcd"), seed=4)
    ta, tb, _, cols = _paired_tables(a, b)
    assert cols == [("k2", "lsd"), ("k2", "ssim"), ("k3", "lsd"), ("k3", "ssim")]
    assert ta[0].tolist() == [a["p360"]["a.wav"][k][m] for k, m in cols] and tb[3].tolist() == [b["p361"]["a.wav"][k][m] for k, m in cols]
    with pytest.raises(ValueError, match="share no"):
        _paired_tables(_result(SPEAKERS, keys=("k1",)), _result(SPEAKERS, keys=("k2",)))


def test_paired_tables_name_the_unmatched_files():
    from ssr_eval_amd.stats import _paired_tables
    more = dict(SPEAKERS, p999=["f%d.wav" % i for i in range(7)])
    with pytest.raises(ValueError) as e:
        _paired_tables(_result(SPEAKERS), _result(more))
    msg = str(e.value)
    assert "7 file(s)" in msg and msg.count("p999/") == 5 and "p999/f0.wav" in msg and "p999/f4.wav" in msg and "f5.wav" not in msg
    less = {"p360": ["a.wav", "b.wav"], "p361": ["a.wav"], "s5": ["x.flac", "y.flac"]}
    with pytest.raises(ValueError, match="p360/c.wav"):
        _paired_tables(_result(less), _result(SPEAKERS))
    with pytest.raises(ValueError, match="no per-file"):
        _paired_tables({"averaged": {}}, {"averaged": {}})


def test_p_value_formula():
    from ssr_eval_amd.stats import p_value
    assert p_value(2000, 2000, 2000) == 1.0                       # every replicate is 0
    assert p_value(0, 2000, 2000) == 2 / 2001                     # no replicate at or below 0
    assert p_value(2000, 0, 2000) == 2 / 2001
    assert p_value(49, 1951, 2000) == 100 / 2001
    assert p_value(1200, 800, 2000) == 1602 / 2001
    assert p_value(1000, 1001, 2000) == 1.0                       # capped
    assert math.isnan(p_value(-1, -1, 2000))


def test_settings_and_helper_option():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee, bootstrap_ci, compare_results      # noqa: F401  (exported)
    from ssr_eval_amd.stats import bootstrap_option, check_settings
    assert check_settings() == {"n_boot": 2000, "level": 0.95, "seed": 0, "resample": "utterance"}
    assert bootstrap_option(500) == {"n_boot": 500, "level": 0.95, "seed": 0, "resample": "utterance"}
    assert bootstrap_option({"level": 0.9, "resample": "speaker"}) == {"n_boot": 2000, "level": 0.9, "seed": 0, "resample": "speaker"}
    mk = lambda v: SSR_Eval_Helper(BasicTestee(), 44100, 44100, test_data_root=None, bootstrap=v)      # noqa: E731
    assert mk(None).bootstrap is None and mk(200).bootstrap["n_boot"] == 200
    assert mk({"n_boot": 300, "seed": 1 << 40}).bootstrap == {"n_boot": 300, "level": 0.95, "seed": 1 << 40, "resample": "utterance"}
    for bad in (0, -5, True, 2.5, "200", {}, {"B": 10}, {"level": 1.0}, {"level": 0}, {"seed": -1}, {"seed": 1 << 64},
                {"resample": "file"}, {"n_boot": 0}):
        with pytest.raises(ValueError):
            mk(bad)
    with pytest.raises(ValueError):
        bootstrap_ci(np.zeros((3, 2)), ["a", "b"])                # a speaker for every row
    with pytest.raises(ValueError):
        bootstrap_ci(np.zeros(3), ["a", "b", "c"])
