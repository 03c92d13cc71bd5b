"""CPU tests of the segment-parallel sosfiltfilt (exact=False): a g++ build of the kernel bodies (ssr_iir_pit.h) against
scipy.signal.sosfiltfilt at 1e-10 of each signal's peak, the C ABI's argument checks (they return before anything touches a device)
and SSR_Eval_Helper(iir_exact=...) validation."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest
from scipy import signal

from oracle import lowpass as olp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SRC = os.path.join(ROOT, "tests", "emu", "iir_pit_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libiir_pit_emu.so")
P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
FS = 44100
TOL = 1e-10                                      # max|y - scipy| <= TOL * max|scipy| per signal

DESIGNS = [(t, o, c) for t in ("butter", "cheby1", "ellip", "bessel") for o in (2, 5, 10) for c in (1000, 4000, 12000)]
DESIGNS.append(("ellip", 10, 1000))              # (already in the product: kept as the issue's named worst case)


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    return C.CDLL(EMU_SO)


def sos_edge(sos):
    """scipy.signal.sosfiltfilt's default padlen."""
    ntaps = 2 * sos.shape[0] + 1 - min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum()))
    return 3 * ntaps


def run_emu(emu, designs, sigs, dtype):
    """-> [design][signal] float64 arrays from the emulated kernels, all designs and signals in ONE call."""
    D = len(designs)
    sos_h, zi_h = np.zeros((D, 8, 6)), np.zeros((D, 8, 2))
    for d, s in enumerate(designs):
        sos_h[d, :s.shape[0]] = s
        zi_h[d, :s.shape[0]] = signal.sosfilt_zi(s)
    ns = np.array([s.shape[0] for s in designs], np.int32)
    eg = np.array([sos_edge(s) for s in designs], np.int32)
    lens = np.array([len(s) for s in sigs], np.int32)
    off = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    x = np.concatenate(sigs).astype(dtype)
    total = int(lens.sum())
    y = np.full((D, total), np.nan)
    fn = emu.iir_pit_emu if dtype == np.float32 else emu.iir_pit_emu_f64
    assert fn(P(x), P(off), P(lens), len(sigs), C.c_int64(total), P(sos_h), P(zi_h), P(ns), P(eg), D, P(y), C.c_int64(total)) == 0
    return [[y[d, o:o + n] for o, n in zip(off, lens)] for d in range(D)]


def rel_err(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("ftype,order,cutoff", DESIGNS)
def test_emulated_segments_match_scipy(emu, ftype, order, cutoff, dtype):
    L = emu.iir_pit_segment_len()
    sos = olp.iir_sos(cutoff, FS, order, ftype)
    edge = sos_edge(sos)
    rng = np.random.default_rng(order * 100000 + cutoff)
    sigs = []
    assert L - 1 > edge                                # (every length below is one SciPy accepts)
    for n in (edge + 1, L - 1, L, L + 1, 2 * L + 3, 20000):
        noise = rng.standard_normal(n) * 0.1
        sigs += [noise.astype(dtype), (0.5 + noise).astype(dtype)]
    got = run_emu(emu, [sos], sigs, dtype)[0]
    worst = 0.0
    for s, g in zip(sigs, got):
        ref = signal.sosfiltfilt(sos, s)
        assert ref.dtype == np.float64 and g.shape == ref.shape
        worst = max(worst, rel_err(g, ref))
        assert rel_err(g, ref) <= TOL, (ftype, order, cutoff, len(s), rel_err(g, ref))
    print("%s order %d %d Hz %s: worst %.2e" % (ftype, order, cutoff, np.dtype(dtype).name, worst))


def test_emulated_result_does_not_depend_on_the_batch(emu):
    """The cuts count from each signal's own first extended sample and every design uses its own edge: a signal alone, in a
    batch, and beside designs of other edges gives the same bits."""
    rng = np.random.default_rng(3)
    L = emu.iir_pit_segment_len()
    sigs = [rng.standard_normal(n).astype(np.float32) for n in (700, 64, 5 * L + 1, 3001)]
    designs = [olp.iir_sos(4000, FS, 10, "ellip"), olp.iir_sos(1000, FS, 2, "butter"), olp.iir_sos(12000, FS, 5, "cheby1")]
    both = run_emu(emu, designs, sigs, np.float32)
    for d, sos in enumerate(designs):
        alone = run_emu(emu, [sos], sigs, np.float32)[0]
        for i, s in enumerate(sigs):
            np.testing.assert_array_equal(both[d][i], alone[i])
            np.testing.assert_array_equal(run_emu(emu, [sos], [s], np.float32)[0][0], alone[i])
            assert rel_err(alone[i], signal.sosfiltfilt(sos, s)) <= TOL


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
@pytest.mark.parametrize("name", ["ssr_sosfiltfilt_fast", "ssr_sosfiltfilt_fast_f64"])
def test_c_abi_rejects_bad_arguments_before_launch(name):
    from ssr_eval_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, name)
    p = C.c_void_p(0x1000)            # never dereferenced: every call below fails its host-side checks first
    ns, eg = (C.c_int32 * 3)(1, 3, 5), (C.c_int32 * 3)(9, 15, 27)
    need = lib.ssr_sosfiltfilt_fast_workspace_bytes(1000, 2, eg, 3)
    assert need >= 8 * (3 * 1000 + 2 * 2 * (9 + 15 + 27))                 # at least the three forward images
    assert lib.ssr_sosfiltfilt_fast_workspace_bytes(1000, 2, None, 3) == 0
    assert lib.ssr_sosfiltfilt_fast_workspace_bytes(1000, 0, eg, 3) == 0
    assert fn(None, p, p, 2, 1000, p, p, ns, eg, 3, p, 1000, p, need, None) == _lib.ERR_INVALID_ARG
    assert fn(p, p, p, 2, 1000, p, p, None, eg, 3, p, 1000, p, need, None) == _lib.ERR_INVALID_ARG
    assert fn(p, p, p, 2, 1000, p, p, ns, None, 3, p, 1000, p, need, None) == _lib.ERR_INVALID_ARG
    assert fn(p, p, p, 2, 1000, p, p, ns, eg, 3, None, 1000, p, need, None) == _lib.ERR_INVALID_ARG
    assert fn(p, p, p, 2, 1000, p, p, ns, eg, 0, p, 1000, p, need, None) == _lib.ERR_UNSUPPORTED          # 1 .. 48 designs
    assert fn(p, p, p, 2, 1000, p, p, ns, eg, 49, p, 1000, p, need, None) == _lib.ERR_UNSUPPORTED
    assert fn(p, p, p, 2, 1000, p, p, (C.c_int32 * 3)(1, 9, 4), eg, 3, p, 1000, p, need, None) == _lib.ERR_UNSUPPORTED   # > 8 sections
    assert fn(p, p, p, 2, 1000, p, p, ns, eg, 3, p, 999, p, need, None) == _lib.ERR_INVALID_ARG            # y_stride < the batch
    assert fn(p, p, p, 2, 1000, p, p, ns, eg, 3, p, 1000, p, need - 1, None) == _lib.ERR_WORKSPACE         # one byte short
    assert b"workspace" in lib.ssr_last_error()
    assert fn(p, p, p, 2, 1000, p, p, ns, eg, 3, p, 1000, None, need, None) == _lib.ERR_WORKSPACE
    assert fn(p, p, p, 0, 1000, p, p, ns, eg, 3, p, 1000, p, need, None) == 0                               # empty batch
    assert fn(p, p, p, 2, 0, p, p, ns, eg, 3, p, 1000, p, need, None) == _lib.ERR_INVALID_ARG             # items but no samples:
    assert fn(p, p, p, 2, -5, p, p, ns, eg, 3, p, 1000, p, need, None) == _lib.ERR_INVALID_ARG            # (workspace_bytes says 0 then)
    # the same codes as ssr_sosfiltfilt_multi's, check by check
    m = lib.ssr_sosfiltfilt_multi
    mneed = lib.ssr_sosfiltfilt_multi_workspace_bytes(1000, 2, eg, 3)
    for args_fast, args_multi in (
            ((None, p, p, 2, 1000, p, p, ns, eg, 3, p, 1000, p, need, None), (None, p, p, 2, 1000, p, p, ns, eg, 3, p, 1000, p, mneed, None)),
            ((p, p, p, 2, 1000, p, p, ns, eg, 49, p, 1000, p, need, None), (p, p, p, 2, 1000, p, p, ns, eg, 49, p, 1000, p, mneed, None)),
            ((p, p, p, 2, 1000, p, p, ns, eg, 3, p, 999, p, need, None), (p, p, p, 2, 1000, p, p, ns, eg, 3, p, 999, p, mneed, None)),
            ((p, p, p, 2, 1000, p, p, ns, eg, 3, p, 1000, p, need - 1, None), (p, p, p, 2, 1000, p, p, ns, eg, 3, p, 1000, p, mneed - 1, None))):
        assert fn(*args_fast) == m(*args_multi) != 0


def test_helper_iir_exact_option():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    mk = lambda **kw: SSR_Eval_Helper(BasicTestee(), 44100, 44100, test_data_root=None, **kw)     # noqa: E731
    assert mk().iir_exact is True and mk(iir_exact=False).iir_exact is False and mk(iir_exact=True).iir_exact is True
    for bad in ("no", 0, 1, None, "False"):
        with pytest.raises(ValueError):
            mk(iir_exact=bad)
    import inspect
    assert inspect.signature(SSR_Eval_Helper.__init__).parameters["iir_exact"].kind is inspect.Parameter.KEYWORD_ONLY


def test_python_signatures_default_to_the_exact_kernel():
    import importlib
    import inspect
    B, LP = importlib.import_module("ssr_eval_amd.backend"), importlib.import_module("ssr_eval_amd.lowpass")
    for f in (B.sosfiltfilt, B.sosfiltfilt_multi, LP.lowpass_iir_multi, LP.lowpass_batch):
        assert inspect.signature(f).parameters["exact"].default is True, f
    assert "exact" not in inspect.signature(LP.lowpass).parameters       # the reference's signature
