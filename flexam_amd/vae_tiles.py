"""Tile planner of the parallel VAE decode (AutoencoderKLWan3_8.enable_parallel_decode): integer logic only, no GPU.

Every rank decodes one tile of a rows x columns grid of the output EXACTLY, with no exchange: it keeps, of the activation entering each
decoder stage, the rows x columns its tile's receptive field reaches.  All the planner knows of the decoder is, per stage,
    stages = [(up, n_res), ...]   does the stage end in a 2x spatial upsample; how many residual blocks it has
    cost   = [number, ...]        its matrix work per pixel of ITS resolution (_DecoderEngine._stage_cost)
conv1 and the middle block (global attention) in front of the stages always run on full frames; the head conv and the 2x unpatchify
follow the last stage."""
import torch


def axis_need(stages, n: int, part: int, parts: int):
    """One axis of a tile: [lo, hi) of the activation ENTERING each stage that part `part` of `parts` needs for its share of the
    2 n 2^ups output rows (or columns) to come out exact, and that share [r0, r1) itself.  Walking back from the output, what a stage
    must deliver grows by the receptive field of what follows: 1 for the head conv, 1 (at the upsampled resolution) for a resample conv,
    2 per residual block (two 3x3(x3) convs); a 2x upsample halves the range."""
    N = [n]
    for up, _ in stages:
        N.append(N[-1] * (2 if up else 1))
    n_out = 2 * N[-1]                                      # unpatchify doubles once more
    if n_out % parts:
        raise ValueError(f"{n_out} output rows / columns do not divide over {parts} parts")
    r0, r1 = part * n_out // parts, (part + 1) * n_out // parts
    lo, hi = r0 // 2 - 1, -(-r1 // 2) + 1                  # what the head conv's 3x3 window touches
    need = [None] * len(stages)
    for si in range(len(stages) - 1, -1, -1):
        up, n_res = stages[si]
        lo, hi = max(0, lo), min(N[si + 1], hi)
        if up:                                             # resample conv: 3x3 at the upsampled resolution = (y - 1) // 2 .. (y + 1) // 2 of the low one
            lo, hi = (lo - 1) // 2, -(-(hi + 1) // 2)
        lo, hi = lo - 2 * n_res, hi + 2 * n_res
        need[si] = (max(0, lo), min(N[si], hi))
    return need, N, r0, r1


def band_grid(stages, cost, h: int, w: int, world: int):
    """(rows, columns) of the tile grid: the factorisation of `world` whose SLOWEST tile does the least matrix work (area of what it
    holds in every stage x that stage's work per pixel).  A 97 x 512 x 896 clip on 8 ranks: 2 x 4 (0.72 of the work of 8 row bands: a
    tile's halo is a fixed number of rows / columns, so squarer tiles carry less of it)."""
    best, best_c = None, None
    for gr in range(world, 0, -1):                         # row bands first: another grid must beat them by 2 %
        if world % gr:
            continue
        gc = world // gr
        try:
            worst = 0.0
            for ri in range(gr):
                nr = axis_need(stages, h, ri, gr)[0]
                for ci in range(gc):
                    nc = axis_need(stages, w, ci, gc)[0]
                    worst = max(worst, sum((c * (r1 - r0) * (c1 - c0) for c, (r0, r1), (c0, c1) in zip(cost, nr, nc)), 0.0))
        except ValueError:
            continue
        if best is None or worst < best_c * 0.98:
            best, best_c = (gr, gc), worst
    if best is None:
        raise ValueError(f"a [{16 * h}, {16 * w}] frame does not divide into {world} equal tiles")
    return best


def stripe_plan(stages, grid, h: int, w: int, rank: int):
    """The tile of `rank` (= row * gc + column) in `grid` = (gr, gc).  The tile is re-cropped at EVERY stage where that removes >= 1/8 of
    what is held (cropping once, entering stage 2, row bands only: 0.47 of a whole decode per rank at 8 ranks; per-stage row bands 0.35;
    the 2 x 4 grid band_grid picks for the 512 x 896 clip ~0.26).
    Returns (crops, (lo, hi, clo, chi), (rows, cols)): crops = {stage: (a, b, ca, cb)} relative to what is held when entering that stage;
    the tile's video is rows x cols pixels and has its own pixels at [lo, hi) x [clo, chi)."""
    gr, gc = grid
    ri, ci = divmod(rank, gc)
    nr, _, r0, r1 = axis_need(stages, h, ri, gr)
    nc, _, c0, c1 = axis_need(stages, w, ci, gc)
    crops, cur, ccur = {}, (0, h), (0, w)
    for si, (up, _) in enumerate(stages):
        (a, b), (ca, cb) = nr[si], nc[si]
        held, kept = (cur[1] - cur[0]) * (ccur[1] - ccur[0]), (b - a) * (cb - ca)
        if held - kept >= max(1, held // 8):
            crops[si] = (a - cur[0], b - cur[0], ca - ccur[0], cb - ccur[0])
            cur, ccur = (a, b), (ca, cb)
        if up:
            cur, ccur = (2 * cur[0], 2 * cur[1]), (2 * ccur[0], 2 * ccur[1])
    own = (r0 - 2 * cur[0], r1 - 2 * cur[0], c0 - 2 * ccur[0], c1 - 2 * ccur[0])
    return crops, own, (2 * (cur[1] - cur[0]), 2 * (ccur[1] - ccur[0]))


def assemble_tiles(tiles, grid):
    """Tiles [3, F, rows, cols] of all ranks (rank = row * gc + column) -> the frame."""
    gr, gc = grid
    return torch.cat([torch.cat(list(tiles[r * gc:(r + 1) * gc]), dim=3) for r in range(gr)], dim=2)
