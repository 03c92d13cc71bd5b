"""GPU tests (-m gpu) of the bootstrap of the aggregate: k_boot_means' draws against the NumPy oracle
(tests/bootstrap_oracle.py) exactly, its replicates within float64 round-off and bit-identical for a table alone and inside a wider
one, k_boot_summary against NumPy on the GPU's own replicates and against the oracle's, the cap on B, non-finite columns,
determinism across runs and streams, and the Python surface: bootstrap_ci, SSR_Eval_Helper(bootstrap=...) and compare_results."""
import numpy as np
import pytest
import torch

import bootstrap_oracle as O

pytestmark = pytest.mark.gpu

QS = np.array([0.025, 0.975, 0.0, 1.0])


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"


def _offsets(sizes):
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)


@pytest.fixture(scope="module")
def sizes():
    """Speakers of one file, fewer files than a Philox block, fewer than a wave, a wave, and three more than an index tile."""
    from ssr_eval_amd import backend as B
    tile, cap = B.bootstrap_geometry()
    assert cap == 16384
    return np.array([1, 5, 7, 64, tile + 3])


@pytest.fixture(scope="module")
def normal_table(sizes):
    return 100.0 + np.random.default_rng(8).standard_normal((int(sizes.sum()), 130))


@pytest.fixture(scope="module")
def summary_case():
    """(table, spk_off, the oracle's 16,384 replicates): columns whose replicates straddle 0, lean to one side, or stay positive."""
    off = _offsets([5, 7, 64])
    table = np.random.default_rng(9).standard_normal((int(off[-1]), 4)) + np.array([0.0, 0.02, -0.05, 100.0])
    return table, off, O.replicates(table, off, 16384, 4, "utterance")


def _reps(table, off, n_boot, seed, scheme):
    from ssr_eval_amd import backend as B
    return B.bootstrap_means(table, off, n_boot, seed, scheme).cpu().numpy()


@pytest.mark.parametrize("seed,n_boot", [(3, 1), (3, 3), (3, 257), ((0xfeedbeef << 32) | 12345, 1), ((0xfeedbeef << 32) | 12345, 3),
                                         ((0xfeedbeef << 32) | 12345, 257)])
@pytest.mark.parametrize("scheme", ["utterance", "speaker"])
def test_draws_match_the_oracle_exactly(sizes, scheme, seed, n_boot):
    """The table is the N x N identity: replicate b of column i, times S n_s, is how often file i was drawn."""
    off = _offsets(sizes)
    N = int(off[-1])
    reps = _reps(np.eye(N), off, n_boot, seed, scheme)
    scale = len(sizes) * np.repeat(sizes, sizes)
    np.testing.assert_array_equal(np.round(reps * scale).astype(np.int64), O.draw_counts(off, n_boot, seed, scheme))


@pytest.mark.parametrize("scheme", ["utterance", "speaker"])
def test_replicates_match_the_oracle_and_do_not_depend_on_the_width(sizes, normal_table, scheme):
    """Within 1e-12 max|column| of the oracle (a float64 sum of n <= 3,000 terms errs by at most n 2^-53 = 3.3e-13 relative to the
    mean magnitude); columns 0 .. 64 of the K = 130 run are the bits of a run on those 65 columns alone."""
    off = _offsets(sizes)
    got = {K: _reps(normal_table[:, :K], off, 257, 21, scheme) for K in (1, 65, 130)}
    for K, r in got.items():
        want = O.replicates(normal_table[:, :K], off, 257, 21, scheme)
        err = np.abs(r - want) / np.abs(normal_table[:, :K]).max(axis=0)
        print("K = %d, %s: max error %.3g of max|column|" % (K, scheme, err.max()))
        assert (err <= 1e-12).all()
    np.testing.assert_array_equal(got[130][:, :65], got[65])
    np.testing.assert_array_equal(got[65][:, :1], got[1])


@pytest.mark.parametrize("n_boot", [1, 2, 1000, 16384])
def test_summary(summary_case, n_boot):
    from ssr_eval_amd import backend as B
    table, off, oracle_reps = summary_case
    scale = np.abs(table).max(axis=0)
    assert (np.abs(oracle_reps) > 1e-9 * scale).all()          # no oracle replicate so close to 0 that a count could flip
    dev = B.bootstrap_means(table, off, n_boot, 4, "utterance")
    mean, se, qs, n_le0, n_ge0 = B.bootstrap_summary(dev, QS)
    reps = dev.cpu().numpy()
    top = np.abs(reps).max()
    # against NumPy on the GPU's own replicates
    assert (np.abs(qs - np.percentile(reps, 100 * QS, axis=0)) <= 1e-13 * top).all()
    assert (np.abs(mean - reps.mean(axis=0)) <= 1e-12 * top).all()
    np.testing.assert_array_equal(n_le0, (reps <= 0).sum(axis=0))
    np.testing.assert_array_equal(n_ge0, (reps >= 0).sum(axis=0))
    if n_boot == 1:
        assert np.isnan(se).all() and (qs[0] == qs[1]).all() and (qs[0] == reps[0]).all()
    else:
        assert (np.abs(se - reps.std(axis=0, ddof=1)) <= 1e-12 * top).all()
    # against the oracle's replicates
    want, wcounts = O.summary(oracle_reps[:n_boot], QS)
    assert (np.abs(reps - oracle_reps[:n_boot]) <= 1e-12 * scale).all()
    assert (np.abs(mean - want[:, 0]) <= 1e-12 * scale).all() and (np.abs(qs - want[:, 2:].T) <= 1e-12 * scale).all()
    if n_boot > 1:
        assert (np.abs(se - want[:, 1]) <= 1e-12 * scale).all()
    np.testing.assert_array_equal(np.stack([n_le0, n_ge0], axis=1), wcounts)
    if n_boot == 16384:
        assert (n_le0[3], n_ge0[3]) == (0, 16384) and 0 < n_le0[0] < 16384


def test_more_replicates_than_the_cap_are_unsupported(summary_case):
    from ssr_eval_amd import backend as B
    from ssr_eval_amd._lib import SsrHipError
    table, off, _ = summary_case
    with pytest.raises(SsrHipError, match="error -2"):
        B.bootstrap_means(table, off, 16385, 0, "utterance")
    with pytest.raises(SsrHipError, match="error -2"):
        B.bootstrap_summary(torch.zeros((16385, 1), dtype=torch.float64, device="cuda"), QS)


def test_non_finite_columns_are_nan_and_the_others_untouched():
    from ssr_eval_amd import backend as B
    off = _offsets([5, 7, 64, 200])
    table = np.random.default_rng(10).standard_normal((int(off[-1]), 70))
    dirty = table.copy()
    dirty[140, 3] = np.nan
    dirty[2, 7] = np.inf
    bad = np.zeros(70, bool)
    bad[[3, 7]] = True
    for scheme in ("utterance", "speaker"):
        clean_dev, dirty_dev = (B.bootstrap_means(t, off, 300, 1, scheme) for t in (table, dirty))
        clean, reps = clean_dev.cpu().numpy(), dirty_dev.cpu().numpy()
        assert np.isnan(reps[:, bad]).all()
        np.testing.assert_array_equal(reps[:, ~bad], clean[:, ~bad])
        got, want = B.bootstrap_summary(dirty_dev, QS), B.bootstrap_summary(clean_dev, QS)
        for g, w in zip(got[:3], want[:3]):
            assert np.isnan(g[..., bad]).all()
            np.testing.assert_array_equal(g[..., ~bad], w[..., ~bad])
        for g, w in zip(got[3:], want[3:]):
            assert (g[bad] == -1).all()
            np.testing.assert_array_equal(g[~bad], w[~bad])


def test_two_runs_and_a_second_stream_give_the_same_bits(sizes, normal_table):
    from ssr_eval_amd import backend as B
    off = _offsets(sizes)
    table = torch.from_numpy(normal_table).cuda()

    def run():
        dev = B.bootstrap_means(table, off, 500, 77, "speaker")
        return (dev.cpu().numpy(),) + B.bootstrap_summary(dev, QS)
    first, second = run(), run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    for other in (second, third):
        for a, b in zip(first, other):
            assert a.tobytes() == b.tobytes()


def test_bootstrap_ci_sorts_by_speaker_and_matches_the_oracle():
    from ssr_eval_amd import bootstrap_ci
    rng = np.random.default_rng(12)
    names = np.array(["p361"] * 9 + ["p360"] * 4 + ["s5"] * 30)
    order = rng.permutation(len(names))
    table = rng.standard_normal((len(names), 6)) + 2.0
    got = bootstrap_ci(table[order], names[order].tolist(), n_boot=400, level=0.9, seed=5, resample="speaker", return_replicates=True)
    # the stable sort by speaker: p360, p361, s5, each speaker's rows in the order they were given
    srt = np.argsort(names[order], kind="stable")
    grouped, off = table[order][srt], _offsets([4, 9, 30])
    want = O.replicates(grouped, off, 400, 5, "speaker")
    scale = np.abs(table).max(axis=0)
    assert (np.abs(got["replicates"].cpu().numpy() - want) <= 1e-12 * scale).all()
    wsum, _ = O.summary(want, [0.05, 0.95])
    np.testing.assert_array_equal(got["estimate"], O.estimate(grouped, off))
    for name, col in (("se", 1), ("lo", 2), ("hi", 3)):
        assert (np.abs(got[name] - wsum[:, col]) <= 1e-12 * scale).all()
    plain = bootstrap_ci(table[order], names[order].tolist(), n_boot=400, level=0.9, seed=5, resample="speaker")
    assert sorted(plain) == ["estimate", "hi", "lo", "se"] and plain["lo"].tobytes() == got["lo"].tobytes()


# ---- SSR_Eval_Helper(bootstrap=...) and compare_results on a small wav tree ---------------------------------------------------
FS = 44100
COUNTS = {"p360": 5, "p361": 1, "s5": 7}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """evaluate() of the identity testee with bootstrap=200 and without, and of a testee that adds noise of 1e-3 RMS."""
    from scipy.io import wavfile
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    rng = np.random.default_rng(31)
    root = tmp_path_factory.mktemp("boot") / "vctk_test"
    n = int(0.6 * FS)
    for spk, c in COUNTS.items():
        (root / spk).mkdir(parents=True)
        for i in range(c):
            x = 0.1 * rng.standard_normal(n) * (1 + np.sin(np.arange(n) * (3.0 + i) / FS))
            wavfile.write(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), FS, np.round(x * 32767).astype(np.int16))

    class Noisy(BasicTestee):
        def __init__(self):
            super().__init__()
            self.rng = np.random.default_rng(32)

        def infer(self, x):
            return (np.asarray(x) + 1e-3 * self.rng.standard_normal(len(x))).astype(np.float32)

    def run(testee, **kw):
        h = SSR_Eval_Helper(testee, test_name="t", input_sr=FS, output_sr=FS, evaluation_sr=FS, test_data_root=str(root),
                            setting_fft={"cutoff_freq": [4000]}, **kw)
        return h.evaluate(save_json=False)
    return {"boot": run(BasicTestee(), bootstrap=200), "plain": run(BasicTestee()), "none": run(BasicTestee(), bootstrap=None),
            "noisy": run(Noisy())}


def test_evaluate_confidence_is_bootstrap_ci_of_the_per_file_block(runs):
    from ssr_eval_amd import bootstrap_ci
    res, plain = runs["boot"], runs["plain"]
    assert "confidence" not in plain and plain == runs["none"]
    assert {k: v for k, v in res.items() if k != "confidence"} == plain
    conf = res["confidence"]
    assert conf["settings"] == {"n_boot": 200, "level": 0.95, "seed": 0, "resample": "utterance"}
    key = "proc_fft_8000_44100"
    assert list(conf["averaged"]) == [key] and list(conf["averaged"][key]) == list(res["averaged"][key])
    mets = list(res["averaged"][key])
    rows, spk = [], []
    for s in COUNTS:
        for f in res[s]:
            rows.append([res[s][f][key][m] for m in mets])
            spk.append(s)
    assert len(rows) == 13
    ci = bootstrap_ci(np.array(rows), spk, n_boot=200)
    for i, m in enumerate(mets):
        got = conf["averaged"][key][m]
        assert sorted(got) == ["hi", "lo", "se"]
        assert (got["se"], got["lo"], got["hi"]) == (ci["se"][i], ci["lo"][i], ci["hi"][i]), m
        assert abs(ci["estimate"][i] - res["averaged"][key][m]) <= 1e-12 * max(1.0, abs(ci["estimate"][i]))
        assert got["se"] > 0 and got["lo"] < got["hi"]


def test_compare_results(runs, tmp_path):
    import json
    from ssr_eval_amd import compare_results
    a, b = runs["plain"], runs["noisy"]
    cmp_ = compare_results(a, b, n_boot=300, seed=3)
    key = "proc_fft_8000_44100"
    assert list(cmp_) == [key] and list(cmp_[key]) == list(a["averaged"][key])
    for m, v in cmp_[key].items():
        assert sorted(v) == ["diff", "hi", "lo", "p", "se"]
        assert abs(v["diff"] - (a["averaged"][key][m] - b["averaged"][key][m])) <= 1e-12, m
        assert v["se"] >= 0 and v["lo"] <= v["hi"] and 0 < v["p"] <= 1
    assert cmp_[key]["lsd"]["diff"] != 0 and cmp_[key]["lsd"]["se"] > 0
    # the JSON files evaluate() writes are taken as well, and the result with a confidence block is the same result
    pa, pb = tmp_path / "a.json", tmp_path / "b.json"
    pa.write_text(json.dumps(runs["boot"], indent=4))
    pb.write_text(json.dumps(b, indent=4))
    assert compare_results(str(pa), str(pb), n_boot=300, seed=3) == cmp_
    same = compare_results(a, a, n_boot=300)
    for m, v in same[key].items():
        assert v == {"diff": 0.0, "se": 0.0, "lo": 0.0, "hi": 0.0, "p": 1.0}, m
