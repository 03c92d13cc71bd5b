"""GPU tests (-m gpu) of the SSIM kernel choice of the pair pipeline on wide images: n_fft 2048 (F = 1025: two strips of 512
outputs) and n_fft 1024 (F = 513: one strip) go through the eight-column kernel k_ssim<8, true>, through ssr_pair_metrics and
through the virtual items of ssr_pair_metrics_multi.  Ragged pairs whose frame counts give a tile of the row loop every shape -
7 (one output row), 8, 20 (one whole fourteen-step trip), 27, 28 and 41 frames - against the oracle, and the same pairs inside a
batch large enough to change the row tiles against the pairs run alone."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
FRAMES = (7, 8, 20, 27, 28, 41)
CONFIGS = [(2048, 512), (1024, 256)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from ssr_eval_amd import _lib
    _lib.load()


def _pairs(seed, lens):
    rng = np.random.default_rng(seed)
    tgts = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    ests = [(t + 0.02 * rng.standard_normal(len(t))).astype(np.float32) for t in tgts]
    return ests, tgts


def _lens(hop, frames=FRAMES):
    return [(t - 1) * hop + 37 for t in frames]          # 1 + len // hop frames


def _oracle(est, tgt, n_fft, hop):
    from oracle import metrics as om
    w = om.evaluation(est, tgt, n_fft=n_fft, hop=hop)
    return np.array([w["lsd"], w["ssim"]])


@pytest.mark.parametrize("n_fft,hop", CONFIGS)
def test_ragged_pairs_against_the_oracle(n_fft, hop):
    from ssr_eval_amd import backend as B
    plan = B.get_plan(n_fft, hop, "f64")
    lens = _lens(hop)
    assert [plan.frames(n) for n in lens] == list(FRAMES)
    ests, tgts = _pairs(n_fft, lens)
    got = B.pair_metrics(plan, ests, tgts, B.M_LSD | B.M_SSIM)
    for i in range(len(lens)):
        want = _oracle(ests[i], tgts[i], n_fft, hop)
        print("n_fft %d T %d: lsd %.9g ssim %.12g, relative to the oracle %s" % (n_fft, FRAMES[i], got[i, 0], got[i, 3],
                                                                              np.abs(got[i, [0, 3]] - want) / np.abs(want)))
        np.testing.assert_allclose(got[i, [0, 3]], want, rtol=1e-5, err_msg="pair %d (T = %d)" % (i, FRAMES[i]))


def test_multi_three_keys_on_four_targets_against_the_oracle():
    from ssr_eval_amd import backend as B
    n_fft, hop = 2048, 512
    plan = B.get_plan(n_fft, hop, "f64")
    lens = _lens(hop, (7, 20, 28, 41))
    _, tgts = _pairs(3, lens)
    rng = np.random.default_rng(4)
    ests = [[(t * (0.6 + 0.2 * k) + (0.01 + 0.01 * k) * rng.standard_normal(len(t))).astype(np.float32) for t in tgts] for k in range(3)]
    got = B.pair_metrics_multi(plan, ests, tgts, B.M_LSD | B.M_SSIM)
    assert got.shape == (4, 3, 4)
    for k in range(3):
        for i in range(4):
            want = _oracle(ests[k][i], tgts[i], n_fft, hop)
            np.testing.assert_allclose(got[i, k, [0, 3]], want, rtol=1e-5, err_msg="key %d target %d" % (k, i))


def _big_lens(hop, n):
    """The six ragged pairs, one of 376 frames and short ones up to n items: rows per tile = ceil(370 n / 4096) instead of the
    eight rows every one of these pairs gets alone."""
    return _lens(hop) + [375 * hop + 11] + [46 * hop + 5 * i for i in range(n - len(FRAMES) - 1)]


@pytest.mark.parametrize("n_fft,hop", CONFIGS)
def test_a_pair_in_a_large_batch_equals_the_pair_alone(n_fft, hop):
    """The SSIM partial sums are added in a fixed order, and the row tiles (which follow the batch) change the float64 order alone:
    1e-10 relative between a pair inside 128 pairs (12 rows per tile) and the same pair alone (8)."""
    from ssr_eval_amd import backend as B
    plan = B.get_plan(n_fft, hop, "f64")
    lens = _big_lens(hop, 128)
    ests, tgts = _pairs(n_fft + 1, lens)
    got = B.pair_metrics(plan, ests, tgts, B.M_LSD | B.M_SSIM)
    assert np.isfinite(got[:, [0, 3]]).all()
    for i in list(range(len(FRAMES) + 1)) + [64, 127]:
        alone = B.pair_metrics(plan, [ests[i]], [tgts[i]], B.M_LSD | B.M_SSIM)[0]
        print("n_fft %d pair %d: ssim %.15g alone %.15g" % (n_fft, i, got[i, 3], alone[3]))
        assert abs(got[i, 3] - alone[3]) <= 1e-10 * abs(alone[3]), (i, got[i, 3], alone[3])


def test_multi_in_a_large_batch_equals_the_target_alone():
    from ssr_eval_amd import backend as B
    n_fft, hop, K = 2048, 512, 3
    plan = B.get_plan(n_fft, hop, "f64")
    lens = _big_lens(hop, 48)                                     # 144 virtual items: 14 rows per tile
    _, tgts = _pairs(5, lens)
    rng = np.random.default_rng(6)
    ests = [[(t * (0.6 + 0.2 * k) + (0.01 + 0.01 * k) * rng.standard_normal(len(t))).astype(np.float32) for t in tgts] for k in range(K)]
    got = B.pair_metrics_multi(plan, ests, tgts, B.M_LSD | B.M_SSIM)
    assert np.isfinite(got[:, :, [0, 3]]).all()
    for i in list(range(len(FRAMES) + 1)) + [47]:
        alone = B.pair_metrics_multi(plan, [[ests[k][i]] for k in range(K)], [tgts[i]], B.M_LSD | B.M_SSIM)[0]
        for k in range(K):
            assert abs(got[i, k, 3] - alone[k, 3]) <= 1e-10 * abs(alone[k, 3]), (i, k, got[i, k, 3], alone[k, 3])
