"""The deferred dW2 (| dW6) tiling as the library plans it (vaeb_dw2_plan: host only, the code the
training step and its flush launch run): every element of the (H + 1) x (D g) weight-gradient
matrix -- H weight rows and the bias row, g = 2 column blocks [W2 | W6] for the Gaussian decoder
-- belongs to exactly one tile worker, and one tile per workgroup is planned only where the tiles
fit the CUs that the encoder's workgroups leave free."""
import numpy as np
import pytest

from vaeb_amd import _lib

B = 100
CASES = [
    ("mnist", 784, 500, 20, _lib.DEC_BERNOULLI),
    ("gauss_560", 560, 272, 4, _lib.DEC_GAUSSIAN),
    ("gauss_56_split_inside_a_tile", 56, 272, 2, _lib.DEC_GAUSSIAN),
    ("scalar_path_D50", 50, 272, 4, _lib.DEC_BERNOULLI),
    ("bias_row_last_of_tile", 784, 319, 20, _lib.DEC_BERNOULLI),
    ("bias_row_alone", 784, 320, 20, _lib.DEC_BERNOULLI),
    ("large", 4096, 2048, 20, _lib.DEC_BERNOULLI),
]


@pytest.mark.parametrize("name,D,H,Z,dec", CASES, ids=[c[0] for c in CASES])
def test_tiles_cover_the_matrix_exactly_once(name, D, H, Z, dec):
    pl = _lib.dw2_plan(D, H, Z, B, decoder=dec)
    g = 2 if dec == _lib.DEC_GAUSSIAN else 1
    rows, cols = H + 1, D * g
    assert pl["width"] in (32, 48, 64)
    assert pl["split"] == (D if g == 2 else 0)
    assert len(pl["ranges"]) == pl["workers"]
    hits = np.zeros((rows, cols), np.int32)
    for r0, r1, c0, c1 in pl["ranges"]:
        assert 0 <= r0 < r1 <= rows and 0 <= c0 < c1 <= cols, (r0, r1, c0, c1)
        assert r1 - r0 <= 64 and c1 - c0 <= pl["width"]
        hits[r0:r1, c0:c1] += 1
    assert hits.min() == 1 and hits.max() == 1
    # one tile per workgroup only where each gets a CU of its own beside the encoder
    if pl["paired"]:
        assert pl["width"] == 32
    else:
        assert pl["workers"] <= pl["free_cus"]


def test_mnist_plan():
    pl = _lib.dw2_plan(784, 500, 20, B)
    assert (pl["width"], pl["workers"], pl["paired"]) == (48, 136, False)
    assert pl["free_cus"] == 256 - 112


def test_the_narrowest_fitting_width_is_taken():
    """32 columns where they fit, 64 where only they do, the paired form where nothing does."""
    assert _lib.dw2_plan(104, 272, 4, 36)["width"] == 32
    # 784-500 at B = 208: 13 x 16 = 208 encoder workgroups leave 48 CUs; 8 x 13 = 104 tiles of 64 do not fit
    assert _lib.dw2_plan(784, 500, 20, 208)["paired"]
    # B = 132: 9 x 16 = 144 encoder workgroups leave 112: 17 x 8 = 136 of 48 do not fit, 13 x 8 = 104 of 64 do
    pl = _lib.dw2_plan(784, 500, 20, 132)
    assert (pl["width"], pl["workers"], pl["paired"]) == (64, 104, False)
    big = _lib.dw2_plan(4096, 2048, 20, B)
    assert big["paired"] and big["workers"] == 33 * 128


VEC_CASES = [
    # D, H, Z, B, decoder -> width, paired, workers, free_cus
    ("D_not_mult_of_4", 786, 500, 20, 132, _lib.DEC_BERNOULLI, 32, True, 200, 112),
    ("H_not_mult_of_4", 784, 498, 20, 132, _lib.DEC_BERNOULLI, 32, True, 200, 112),
    ("scalar_path_still_takes_48", 786, 500, 20, 100, _lib.DEC_BERNOULLI, 48, False, 136, 144),
    ("gaussian", 784, 500, 20, 132, _lib.DEC_GAUSSIAN, 32, True, 392, 112),
]


@pytest.mark.parametrize("name,D,H,Z,Bc,dec,width,paired,workers,free", VEC_CASES, ids=[c[0] for c in VEC_CASES])
def test_64_wide_tiles_only_with_16_byte_accesses(name, D, H, Z, Bc, dec, width, paired, workers, free):
    """64-wide tiles are a candidate only where the dW2 group may use 16-byte accesses (the one
    predicate the weight-gradient launches use: H, D and the group's arena offsets % 4 == 0).
    At B = 132 the 48-wide tiles do not fit, so without them the plan is the paired form."""
    pl = _lib.dw2_plan(D, H, Z, Bc, decoder=dec)
    assert (pl["width"], bool(pl["paired"]), pl["workers"], pl["free_cus"]) == (width, paired, workers, free)


def test_bias_row_placement():
    last = _lib.dw2_plan(784, 319, 20, B)["ranges"][-1]
    assert last[:2] == (256, 320)            # rows 256..318 and the bias row 319 in one tile
    alone = _lib.dw2_plan(784, 320, 20, B)["ranges"][-1]
    assert alone[:2] == (320, 321)           # the bias row is a tile row of its own
