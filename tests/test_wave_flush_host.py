"""CPU tests of k_stft_wave's stash-and-flush epilogue (ssr_stft_wave.h, STASH): the previous frame's LSD close and the Nyquist bin, which
lane 0 did in every frame, are kept with the frame's owner lane (frame `it` of a chunk: lane it & 63) and finished by all lanes at once
every 64 frames and in the chunk's last, shorter block.  Through a g++ build of the kernel body (tests/emu/wave_flush_emu.cpp) the new
path is compared with the frame-by-frame code it replaces (the same body with STASH = false) at 2048 / 512, float64 and float32 plans,
LSD only and the full mask, with and without rows:

* chunks of 1, 63, 64, 65 and 131 frames, interleave 1 and 8 (66 frames per chunk at interleave 8), empty chunks, the last chunk of a
  ragged item, a chunk and a 64-block whose last frame is silent (target) and an item whose last frames are (estimate), no partial
  records (part == null), rows decided at run time (MAG = -1) and at compile time, no target rows (out_b == null), a padded row pitch,
  and a mask without LSD.
* Rows, pads and every value no frame owns: equal BIT FOR BIT (the outputs start as NaN patterns).
* The partial records: the new path adds the same terms in another order.  Two orders of summing n terms x_i differ by at most
  2 (n - 1) u sum|x_i| = (n - 1) 2^-52 sum|x_i| (u = 2^-53).  LSD of a chunk of f frames: a frame's 1,025 non-negative terms through 64
  lanes (n = 1,025 + 64), a division and a square root (2 roundings more; the root halves the relative error before it), then f frame
  values: n = 1,025 + 64 + 4 + f, relative to the value.  The six SISpec sums: n = 1,025 f terms; sums 1, 2, 4, 5 are sums of squares
  (relative to the value), 3 and 6 are sums of products d t, whose sum of magnitudes is at most sqrt(sum d^2 sum t^2) (Cauchy-Schwarz):
  the bound is relative to that.  Measured values are printed (profiles/wave_lane0_notes.md)."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SRC = os.path.join(ROOT, "tests", "emu", "wave_flush_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libwave_flush_emu.so")
N, HOP, F = 2048, 512, 1025
M_LSD, M_LOG_SISPEC, M_SISPEC = 1, 2, 4
EPS52 = 2.0 ** -52


@pytest.fixture(scope="module")
def emu():
    deps = [EMU_SRC] + glob.glob(os.path.join(ROOT, "ssr_eval_amd", "csrc", "*.h"))
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", EMU_SO, EMU_SRC])
    lib = C.CDLL(EMU_SO)
    lib.wave_flush_run.argtypes = [C.c_int] * 7 + [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_int64] + [C.c_void_p] * 3
    return lib


def frames_of(n):
    return 1 + n // HOP


def _silence(x, first_frame, last_frame):
    """zero every sample the frames first_frame .. last_frame see"""
    x[max(0, HOP * first_frame - N // 2):HOP * last_frame + N // 2] = 0.0


def make_batch(frames0):
    """Four ragged pairs: `frames0` frames with a silent stretch of the target across frames 63 .. 65 (a chunk's, and a 64-block's, last
    frame), 65 frames with the estimate silent over the last three, 1 sample, 2,047 samples."""
    rng = np.random.default_rng(frames0)
    lens = [HOP * (frames0 - 1) + 37, HOP * 64 + 100, 1, 2047]
    a = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    b = [(x + 0.01 * rng.standard_normal(len(x)).astype(np.float32)).astype(np.float32) for x in a]
    if frames0 > 66:
        _silence(b[0], 63, 65)
    _silence(a[1], 62, 64)
    return a, b


_BATCHES = {}


def batch(frames0):
    if frames0 not in _BATCHES:
        _BATCHES[frames0] = make_batch(frames0)
    return _BATCHES[frames0]


def run(lib, a, b, dt, stash, mag, mask, upc, S, rows=True, part=True, out_b=True, pitch=0, extra_chunks=0):
    lens = np.array([len(x) for x in a], np.int32)
    off = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    fa, fb = np.concatenate(a).astype(np.float32), np.concatenate(b).astype(np.float32)
    T = np.array([frames_of(int(n)) for n in lens])
    frame_off = np.concatenate(([0], np.cumsum(T)[:-1])).astype(np.int64)
    n_chunks = -(-int(T.max()) // upc)
    n_chunks = (-(-n_chunks // S) + extra_chunks) * S
    P = pitch if pitch else F
    oa = np.full((int(T.sum()), P), np.nan, np.float32) if rows else None
    ob = np.full((int(T.sum()), P), np.nan, np.float32) if rows and out_b else None
    pt = np.full((len(lens), n_chunks, 8), np.nan, np.float64) if part else None
    ptr = lambda x: x.ctypes.data if x is not None else None
    rc = lib.wave_flush_run(1 if dt == np.float64 else 0, stash, mag, HOP, 1 if rows else 0, mask, S, ptr(fa), ptr(fb), ptr(off), ptr(off),
                            ptr(lens), ptr(frame_off), len(lens), upc, n_chunks, pitch, ptr(oa), ptr(ob), ptr(pt))
    assert rc == 0, rc
    # frames per (item, chunk): units u0 + S it below min(span end, frames)
    nfr = np.zeros((len(lens), n_chunks), np.int64)
    for i, t in enumerate(T):
        for c in range(n_chunks):
            span0 = (c // S) * S * upc
            u1 = min(span0 + S * upc, int(t))
            nfr[i, c] = max(0, -(-(u1 - span0 - c % S) // S))
    return oa, ob, pt, nfr


def same_bits(x, y):
    return (x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32))


def compare(lib, frames0, dt, mask, upc, S, label, mag=-1, **kw):
    a, b = batch(frames0)
    oa0, ob0, p0, nfr = run(lib, a, b, dt, 0, -1, mask, upc, S, **kw)
    oa1, ob1, p1, _ = run(lib, a, b, dt, 1, mag, mask, upc, S, **kw)
    assert same_bits(oa0, oa1) and same_bits(ob0, ob1), "%s: rows differ" % label
    if oa1 is not None:
        cols = oa1[:, :F]
        assert not np.isnan(cols).any(), "%s: a row value was never written" % label
        if kw.get("pitch", 0):
            assert np.isnan(oa1[:, F:]).all(), "%s: the pad of a row was written" % label
    if p0 is None:
        return nfr
    assert np.isfinite(p1).all() and (p1[..., 7] == 0).all()
    assert (p1[nfr == 0] == 0).all(), "%s: an empty chunk reports something" % label
    worst = np.zeros(7)
    for i, c in zip(*np.nonzero(nfr)):
        f = int(nfr[i, c])
        old, new = p0[i, c], p1[i, c]
        scale = [abs(old[0]), old[1], old[2], np.sqrt(old[1] * old[2]), old[4], old[5], np.sqrt(old[4] * old[5])]
        terms = [F + 64 + 4 + f] + [F * f] * 6
        for q in range(7):
            d = abs(new[q] - old[q])
            if scale[q] == 0:
                assert d == 0, (label, i, c, q, new[q], old[q])
                continue
            worst[q] = max(worst[q], d / scale[q] / (terms[q] * EPS52))
            assert d <= terms[q] * EPS52 * scale[q], (label, i, c, q, new[q], old[q], d / scale[q], terms[q] * EPS52)
    print("%s %s mask %d: frames per chunk up to %d; largest |new - old| as a fraction of its bound: LSD %.3f, sums %s"
          % (label, np.dtype(dt).name, mask, int(nfr.max()), worst[0], " ".join("%.3f" % w for w in worst[1:])))
    if mask & M_LSD:
        assert (p1[..., 0][nfr > 0] > 0).all()
    return nfr


GEOMETRIES = [(1, 1), (63, 1), (64, 1), (65, 1), (131, 1), (17, 8)]


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("mask", [M_LSD, M_LSD | M_LOG_SISPEC | M_SISPEC])
@pytest.mark.parametrize("upc,S", GEOMETRIES)
def test_flush_gives_the_frame_by_frame_results(emu, upc, S, mask, dt):
    """Rows and partial records at every chunk length around the flush period, with an empty group of chunks behind the last one."""
    nfr = compare(emu, 131, dt, mask, upc, S, "upc %d S %d" % (upc, S), extra_chunks=1)
    assert nfr.max() == min(upc, 131) and (nfr == 0).any()
    if upc == 65:
        assert 1 in nfr[0] and 65 in nfr[0]                 # 131 frames: 65 + 65 + a last chunk of one


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_flush_in_interleaved_chunks_longer_than_a_block(emu, dt):
    """Interleave 8 with 66 frames per chunk (u = u0 + 8 it): one flush after 64 frames, one of two frames in the tail; the row offset
    of a lane is 8 rows times its number."""
    nfr = compare(emu, 8 * 66, dt, M_LSD | M_LOG_SISPEC | M_SISPEC, 66, 8, "upc 66 S 8")
    assert (nfr[0] == 66).all() and nfr.shape[1] == 8


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("mag", [-1, 1])
def test_flush_rows_without_partial_records_and_without_target_rows(emu, mag, dt):
    """part == null: the flush still runs, for the rows' column 1,024.  out_b == null: the target rows' stores are dropped by the range
    check (nothing to compare but the estimate rows - and nothing may fault).  A padded row pitch (the pair pipeline's)."""
    for kw in ({"part": False}, {"out_b": False}, {"pitch": 1028}, {"part": False, "out_b": False, "pitch": 1028}):
        compare(emu, 131, dt, M_LSD, 65, 1, "rows %s" % sorted(kw), mag=mag, **kw)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("mask", [M_LSD, M_LSD | M_LOG_SISPEC | M_SISPEC])
@pytest.mark.parametrize("mag", [-1, 0])
def test_flush_without_rows(emu, mag, mask, dt):
    compare(emu, 131, dt, mask, 65, 1, "no rows, MAG %d" % mag, mag=mag, rows=False)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_flush_without_lsd(emu, dt):
    """want_lsd false: the record's LSD stays exactly 0, the six sums take their Nyquist terms in the flush."""
    a, b = batch(131)
    compare(emu, 131, dt, M_SISPEC | M_LOG_SISPEC, 65, 1, "no LSD")
    _oa, _ob, p1, _nfr = run(emu, a, b, dt, 1, -1, M_SISPEC | M_LOG_SISPEC, 65, 1)
    assert (p1[..., 0] == 0).all() and (p1[0, :, 1:7] != 0).all()
