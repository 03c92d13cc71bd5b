"""CPU tests: the eight-column SSIM kernel of the pair pipeline (ssr_ssim_body<8, true>, strips of 512 outputs) on the host
emulation, against the four-column kernel it replaces on wide images and against the oracle.

Widths: 518 (exactly one eight-column strip), 519 (a last strip of ONE output), 525 (a narrow last strip: 7 outputs, 13 input
columns) and 1025 (the product width); rows padded to a multiple of four floats, NaN in the padding.
Row tiles: a tile of r output rows takes 6 + r row steps - six warm-up steps, then whole trips of fourteen, then the short tail:
r = 1 (7 steps: warm-up plus one), 14 (20: exactly one whole trip), 15 (21: a trip and one step), 28 (34 = 6 + 2 x 14); every image
height leaves a short last tile, and two shorter (ragged) items end in other tiles of the same geometry."""
import numpy as np
import pytest

import emu_lib as E
from oracle import ssim as ossim

WIDTHS = (518, 519, 525, 1025)
#        rows_per_tile, T of the longest item (tiles of the longest item), T of the two ragged items
TILES = [(1, 10, (9, 7)),          # 4 tiles of one row; items of 3 and 1 output rows
         (14, 25, (22, 11)),       # 14 + 5; 14 + 2; 5 (first tile short, second empty)
         (15, 24, (21, 8)),        # 15 + 3; 15; 2
         (28, 38, (36, 30))]       # 28 + 4; 28 + 2; 24


def _images(F, T, seed):
    rng = np.random.default_rng(seed)
    a = np.abs(rng.standard_normal((T, F))).astype(np.float32) * 50
    b = (a * (1 + 0.2 * rng.standard_normal((T, F)))).astype(np.float32)
    return a, b


@pytest.mark.parametrize("rows_per_tile,T,T_ragged", TILES)
@pytest.mark.parametrize("F", WIDTHS)
def test_eight_columns_against_four_and_the_oracle(F, rows_per_tile, T, T_ragged):
    """Per-item SSIM from the partial sums added in the fixed tile order (the finalisation body): the two variants form the same
    float32 value for every output and add aligned quads of them in float32 alike, so they differ by the order of the float64
    additions alone - n 2^-53 relative with n <= 4e5 outputs, bound 1e-10; and each is within 1e-5 of the oracle."""
    a, b = _images(F, T, 1000 * F + T)
    xs = [a] + [a[:t] for t in T_ragged]
    ys = [b] + [b[:t] for t in T_ragged]
    sp4, Ts = E.ssim_parts(xs, ys, rows_per_tile=rows_per_tile, cpt=4, contig=True)
    sp8, _ = E.ssim_parts(xs, ys, rows_per_tile=rows_per_tile, cpt=8, contig=True)
    assert sp8.shape[1] == -(-(T - 6) // rows_per_tile) * -(-(F - 6) // 512)
    assert np.isfinite(sp4).all() and np.isfinite(sp8).all()
    out4, out8 = E.finalize(None, sp4, Ts, F, 8), E.finalize(None, sp8, Ts, F, 8)
    for i in range(len(xs)):
        want = ossim.structural_similarity(xs[i], ys[i])
        print("F %d rows/tile %d T %d: ssim8 %.15f rel. to four columns %.2e, to the oracle %.2e"
              % (F, rows_per_tile, Ts[i], out8[i, 3], abs(out8[i, 3] - out4[i, 3]) / abs(out4[i, 3]), abs(out8[i, 3] - want) / abs(want)))
        assert abs(out8[i, 3] - out4[i, 3]) <= 1e-10 * abs(out4[i, 3])
        assert abs(out8[i, 3] - want) <= 1e-5 * abs(want)
        assert abs(out4[i, 3] - want) <= 1e-5 * abs(want)
        # the plain sums of the records as well (the same tile order, added here)
        s4, s8 = 0.0, 0.0
        for v in sp4[i]:
            s4 += v
        for v in sp8[i]:
            s8 += v
        assert abs(s8 - s4) <= 1e-10 * abs(s4)
