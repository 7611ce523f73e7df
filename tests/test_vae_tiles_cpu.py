"""CPU: the tile plan of the parallel VAE decode (flexam_amd/vae_tiles.py) -- the grid and every rank's crops, on the decoder's stage
list with its stage costs as literals.  The costs are exact integers that follow from the weight shapes (_DecoderEngine._stage_cost);
tests/test_vae_gpu.py asserts that the engines still give these, at the real widths and at the small test VAE's."""
import pytest

from flexam_amd import vae_tiles as T

STAGES = [(True, 3), (True, 3), (True, 3), (False, 3)]             # (2x upsample, residual blocks) of Decoder3d, any width
REAL_COST = [192937984, 385875968, 217055232, 50069504]            # dec_dim 256 (Wan2.2 VAE)
SMALL_COST = [753664, 1507328, 1097728, 262144]                    # dec_dim 16 (oracle.cases.VAE_SMALL)
TILED = [(2, 8, 4), (4, 8, 4), (8, 8, 4), (8, 32, 4), (4, 20, 4), (4, 8, 14), (6, 12, 6)]   # test_vae_tiled_decode_is_exact's (world, h, w)


def test_tile_grid_and_plan_of_the_clip():
    """The 97 x 512 x 896 clip (latent 32 x 56) at the real widths: 2 x 4 tiles on 8 ranks, 2 x 2 on 4; rank 5 of 8 is the second row
    of tiles, second column."""
    assert T.band_grid(STAGES, REAL_COST, 32, 56, 8) == (2, 4) and T.band_grid(STAGES, REAL_COST, 32, 56, 4) == (2, 2)
    gr, gc = T.band_grid(STAGES, REAL_COST, 32, 56, 2)
    assert gr * gc == 2
    crops, (lo, hi, clo, chi), held = T.stripe_plan(STAGES, (2, 4), 32, 56, 5)
    assert (hi - lo, chi - clo) == (256, 224) and max(crops) == 3


def test_row_bands_of_the_clip_height():
    """h = 32 is the clip's latent height: the row pattern of every rank of eight at the real size."""
    grid = T.band_grid(STAGES, SMALL_COST, 32, 4, 8)
    assert grid == (8, 1)
    plans = [T.stripe_plan(STAGES, grid, 32, 4, r)[0] for r in range(8)]
    assert {k: v[:2] for k, v in plans[4].items()} == {1: (20, 52), 2: (14, 50), 3: (13, 59)}
    assert 0 in plans[0] and 0 in plans[7]


@pytest.mark.parametrize("world,h,w", TILED)
def test_tiles_partition_the_frame(world, h, w):
    gr, gc = T.band_grid(STAGES, SMALL_COST, h, w, world)
    assert gr * gc == world
    covered = [[0] * (16 * w) for _ in range(16 * h)]
    for rank in range(world):
        crops, (lo, hi, clo, chi), (rows, cols) = T.stripe_plan(STAGES, (gr, gc), h, w, rank)
        assert (hi - lo, chi - clo) == (16 * h // gr, 16 * w // gc)
        assert 0 <= lo and hi <= rows and 0 <= clo and chi <= cols          # the own window lies inside what the tile holds
        assert all(0 <= a < b and 0 <= ca < cb for a, b, ca, cb in crops.values())
        # assemble_tiles puts the window of rank (ri, ci) at (ri * rows, ci * columns of a window): that must be the share of the frame
        # the need walk planned the tile for, and the shares of all ranks must cover every pixel once
        ri, ci = divmod(rank, gc)
        r0, c0 = T.axis_need(STAGES, h, ri, gr)[2], T.axis_need(STAGES, w, ci, gc)[2]
        assert (r0, c0) == (ri * (hi - lo), ci * (chi - clo))
        for y in range(r0, r0 + hi - lo):
            for x in range(c0, c0 + chi - clo):
                covered[y][x] += 1
    assert all(v == 1 for row in covered for v in row)


def test_a_world_that_does_not_divide_the_frame_is_refused():
    with pytest.raises(ValueError, match="does not divide"):
        T.band_grid(STAGES, SMALL_COST, 4, 4, 3)
