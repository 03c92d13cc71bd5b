"""GPU test (-m gpu) of the per-pair families on a batch larger than their geometry workgroup: 2 NT + 3 pairs (every thread of the
run / prefix scan owns several pairs, the trailing threads none), runs of 1 to 5 pairs per target, one target named by two separate
runs, and targets of four length classes: none, one with no frame or tile, a short one and one that spans several grid items.
Each family's promise - a pair has the same bits alone, in any batch and at any position - is checked as: the batch equals,
bit for bit, the same pairs scored in consecutive sub-batches of at most 64 pairs split at run boundaries.

stoi, wave, quality, pitch, phase and mrstft share one batch (lengths 0, 300, 701 and 5003).  bss, coherence, spectrum, auditory,
modulation, csii and loudness each have the batch tests/pairs_batch.py builds from their own count function and smallest frame
settings, with a per-pair parameter (band table, split bin, split band) from a cycle of period 7; pairs_batch.check_family compares
every output of the entry point, with and without the optional ones, repeats the call, checks the rows without a value, and holds
the pairs at the seams of the geometry (0, NT - 1, NT, NT + 1, 2 NT + 2, the target two runs name) to the family's float64 oracle at
the bars of its own tests.  tests/test_pairs_batch_host.py runs the same checks on the kernel bodies compiled for the host."""
import numpy as np
import pytest
import torch

import pairs_batch as PB

pytestmark = pytest.mark.gpu

FS = 16000
NT = 256                                   # threads of the geometry workgroups (ssr_pairs.h, ssr_phase.h, ssr_stoi.h, ssr_pitch.h)
N_EST = 2 * NT + 3
LENGTHS = (0, 300, 701, 5003)              # 300: below every family's frame (480), half transform (512) and STOI's 256 at 10 kHz
SUB = 64


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"


@pytest.fixture(scope="module")
def batch():
    """(targets, estimates, tgt_index): run k has k % 5 + 1 pairs and names target k, except run 3, which names target 1 again."""
    rng = np.random.default_rng(515)
    idx, k = [], 0
    while len(idx) < N_EST:
        idx += [1 if k == 3 else k] * (k % 5 + 1)
        k += 1
    idx = np.array(idx[:N_EST], np.int32)
    tgts = [np.convolve(rng.standard_normal(LENGTHS[t % 4] + 14), np.hanning(15) / 4, "valid").astype(np.float32)[:LENGTHS[t % 4]]
            for t in range(k)]
    ests = [(tgts[t] + 0.2 * rng.standard_normal(len(tgts[t]))).astype(np.float32) for t in idx]
    assert sorted({len(t) for t in tgts}) == list(LENGTHS) and len(ests) == N_EST
    return tgts, ests, idx


def sub_batches(idx):
    """[a, b) pair ranges of at most SUB pairs that end where a run ends."""
    ends = list(1 + np.flatnonzero(np.diff(idx))) + [len(idx)]
    out, a, last = [], 0, 0
    for e in ends:
        if e - a > SUB:
            out.append((a, last))
            a = last
        last = e
    out.append((a, len(idx)))
    assert all(0 < b - a <= SUB for a, b in out) and out[0][0] == 0 and all(x[1] == y[0] for x, y in zip(out, out[1:]))
    return out


def family(name):
    from ssr_eval_amd import _lib, backend as B
    return {
        "stoi": lambda t, e, i: B.stoi(t, e, i, FS, which=_lib.STOI_BOTH),
        "wave": lambda t, e, i: B.wave_metrics(t, e, i, FS),
        "quality": lambda t, e, i: B.quality_metrics(t, e, i, FS),
        "pitch": lambda t, e, i: B.pitch_metrics(t, e, i, FS),
        "phase": lambda t, e, i: B.phase_metrics(t, e, i),
        "mrstft": lambda t, e, i: B.mrstft_metrics(t, e, i),
    }[name]


@pytest.mark.parametrize("name", ["stoi", "wave", "quality", "pitch", "phase", "mrstft"])
def test_large_batch_equals_its_sub_batches_bit_for_bit(batch, name):
    tgts, ests, idx = batch
    f = family(name)
    whole = np.ascontiguousarray(f(tgts, ests, idx), np.float64).reshape(N_EST, -1)
    parts = []
    for a, b in sub_batches(idx):
        used = list(dict.fromkeys(idx[a:b].tolist()))                  # the sub-batch's targets, renumbered from 0
        local = np.array([used.index(t) for t in idx[a:b]], np.int32)
        parts.append(np.ascontiguousarray(f([tgts[t] for t in used], ests[a:b], local), np.float64).reshape(b - a, -1))
    parts = np.concatenate(parts)
    assert whole.shape == parts.shape and whole.shape[1] >= 2
    diff = np.flatnonzero((whole.view(np.uint64) != parts.view(np.uint64)).any(axis=1))      # (NaN rows compare by bit pattern)
    assert diff.size == 0, (name, diff[:8], whole[diff[:2]], parts[diff[:2]])
    # the batch exercises what it is meant to: rows without a value and rows with one
    lens = np.array([len(e) for e in ests])
    assert np.isfinite(whole[lens == LENGTHS[3]]).any()
    if name != "stoi":                                        # (STOI's value below 30 frames is 1e-5, not NaN)
        assert np.isnan(whole[lens == 0]).all()


# ---- the later families, each on its own batch (tests/pairs_batch.py) -------------------------------------------------------------------
def later_family(name):
    """run(batch, opt) of pairs_batch.check_family through the family's backend entry point"""
    from ssr_eval_amd import backend as B
    if name == "bss":
        return lambda b, opt: B.bss_sdr(b.tgts, b.ests, b.idx, b.cfg["taps"], return_filter=opt)
    if name == "coherence":
        import coherence_oracle as O
        return lambda b, opt: B.coherence_metrics(b.tgts, b.ests, b.idx, b.cfg["N"], b.cfg["H"], O.band_table(b.par["bands"], len(b.ests)),
                                                  b.cfg["thr"], return_spectrum=opt)
    if name == "spectrum":
        def spectrum(b, opt):
            c = PB.case_spectrum(b)
            return B.spectrum_metrics(c.tgts, c.ests, c.index, c.N, c.H, (c.lo, c.hi), c.rho, c.drop, c.bands, c.splits, return_ltas=opt)
        return spectrum
    if name == "auditory":
        return lambda b, opt: B.auditory_metrics(b.tgts, b.ests, b.idx, b.cfg["fs"], b.cfg["n_bands"], None, B.AUDITORY_RANGE_DB, True,
                                                 b.par["splits"], opt, opt, b.cfg["hop"])
    if name == "modulation":
        def modulation(b, opt):
            c = PB.case_modulation(b)                             # (the oracle's designs are the call's own within 1e-14)
            fc, coef, mod, S, ktab = B.modulation_design(c.fs, c.hop, c.n_bands, None, c.kstar)
            assert np.max(np.abs(coef - c.coef)) <= 1e-14 and np.max(np.abs(mod - c.mod)) <= 1e-15 and S == c.S and np.array_equal(ktab, c.ktab)
            return B.modulation_metrics(c.tgts, c.ests, c.index, c.fs, c.n_bands, None, B.MODULATION_ENV_RATE, c.range_db, c.kstar, c.splits,
                                        opt, c.hop)
        return modulation
    if name == "csii":
        from test_csii_host import split_bands
        return lambda b, opt: B.csii_metrics(b.tgts, b.ests, b.idx, b.cfg["fs"], b.cfg["N"], b.cfg["H"], None,
                                             split_bands(b.cfg["fs"], b.cfg["N"], None, b.par["splits"], len(b.ests)), return_bands=opt)
    return lambda b, opt: B.loudness_metrics(b.ests, b.cfg["fs"], return_blocks=opt)


def later_check(name):
    """check(sub-batch, outputs): the family's comparison with its oracle, at the bars of its own GPU test"""
    if name == "bss":
        from test_gpu_bss import check_rows
        return lambda b, o: PB.check_bss(b, o, check_rows)
    if name == "auditory":
        def auditory(b, o):                                       # the oracle scores with the coefficients the call used, as test_gpu_auditory's
            from ssr_eval_amd import backend as B
            coef = B.gammatone_design(b.cfg["fs"], b.cfg["n_bands"])[1]
            assert np.max(np.abs(coef - b.cfg["coef"])) <= 1e-14
            PB.check_auditory(PB.Batch(b.name, b.tgts, b.ests, b.idx, b.par, dict(b.cfg, coef=coef)), o)
        return auditory
    return PB.CHECK[name]


@pytest.mark.parametrize("name", PB.NAMES)
def test_large_batch_of_a_later_family_equals_its_sub_batches_and_meets_the_oracle(name):
    assert PB.NT == NT and PB.N_EST == N_EST and PB.SUB == SUB and len(PB.NAMES) == 7
    PB.check_family(name, later_family(name), later_check(name))
