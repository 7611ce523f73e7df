"""CPU: the cases of tests/attn_window_frames_cases.py (windowed attention with the window counted in frames) are not blind, they reach
every path of the kernel's tile walk, and the planner hip.attn_window_frames_tiles equals a brute-force enumeration.

Not blind: for every case the mask is altered by ONE key at either end of every row's window range [lo, hi] -- add hi + 1, drop hi, add
lo - 1, drop lo -- and every row whose key set that alters moves by at least attn_window_cases.SENSITIVITY_ULPS (8) bf16 ulps in some
channel, every other row stays bit-identical.  A kernel that lets one key too many in, or leaves one out, at a frame boundary of any row
therefore misses the 1-ulp bound of tests/test_attn_window_frames_gpu.py.

Least change of an altered row over the four alterations, in ulps, as computed here (case order of CASES): 72.5, 44.3, 63.7, 63.3,
19.2, 35.3, 128.0, 15.8, 15.8, 68.5, 35.3, 50.4 -- the two cases with frames of 448 tokens are the least sensitive (one key among some
900 to 1300 visible ones)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_cases as W  # noqa: E402
import attn_window_frames_cases as F  # noqa: E402
import attn_window_sink_cases as S  # noqa: E402


@pytest.mark.parametrize("case", F.CASES, ids=F.ids(F.CASES))
def test_cases_are_sensitive_to_one_key_at_either_end_of_every_row(case):
    q, k, v = case.inputs()
    for t in (q, k, v):
        assert torch.equal(t.to(torch.bfloat16).double(), t)                      # the kernels get exactly these values
    s = torch.einsum("blhd,bmhd->bhlm", q, k)
    assert torch.equal(s, s.round())                                              # integer scores: every p is a power of two
    ok = case.allowed()
    assert bool(ok.any(1).all()) and bool(ok.diagonal().all())                    # no empty row: every row sees its own frame
    for i in (0, case.L // 2, case.L - 1):                                        # row_range is the rule's range
        lo, hi = F.row_range(case.L, case.window, case.T, i)
        inside = torch.zeros(case.L, dtype=torch.bool)
        inside[lo:hi + 1] = True
        assert torch.equal(inside | (torch.arange(case.L) < case.sink), ok[i])
    want = case.want(q, k, v)
    least, n_altered = float("inf"), 0
    for name, mask in F.altered_masks(case.L, case.window, case.T, case.sink):
        other = F.reference(q, k, v, mask)
        altered = (mask != ok).any(1)                                             # [L]
        ulps = ((other - want).abs() / F.bf16_ulp(want)).amax(-1)                 # [B, L, H]: the most affected channel
        if altered.any():
            least = min(least, float(ulps[:, altered].min()))
            n_altered += int(altered.sum())
        assert torch.equal(other[:, ~altered], want[:, ~altered]), (case.name, name)
    print(f"{case.name}: {n_altered} altered rows, least change {least:.1f} ulps")
    assert n_altered > 0 and least >= W.SENSITIVITY_ULPS, (case.name, least)      # (a window that holds everything can still lose a key)


def test_the_cases_are_the_twelve_and_cover_the_paths_of_the_walk():
    """T below, equal to and above a key tile, and above a query block; a ragged last frame and a ragged last query block; query blocks
    that straddle a frame boundary; one-run and two-run walks (the latter in five cases, counted by enumeration); both unbounded sides;
    sinks below a tile, tile-aligned and unaligned; a window that ends up holding everything; more than one batch and head twice."""
    C = F.CASES
    assert [(c.L, c.window, c.T, c.sink) for c in C] == [
        (600, (1, 1), 48, 0), (600, (1, 0), 100, 70), (1111, (2, 1), 64, 0), (1111, (0, 0), 200, 128), (1111, (-1, 0), 100, 0),
        (600, (0, -1), 100, 0), (70, (1, 1), 7, 5), (1344, (1, 1), 448, 0), (1500, (0, 1), 448, 448), (900, (0, 0), 300, 1),
        (600, (3, 3), 300, 0), (1111, (1, 1), 37, 300)]
    assert sum(c.B >= 2 and c.H >= 3 for c in C) >= 2
    assert any(c.T < F.KV_TILE for c in C) and any(c.T == F.KV_TILE for c in C) and any(F.KV_TILE < c.T < F.Q_BLOCK for c in C)
    assert any(c.T > F.Q_BLOCK for c in C)
    assert any(c.L % c.T for c in C) and any(c.L % F.Q_BLOCK for c in C) and any(c.L % c.T == 0 for c in C)
    assert any(q0 // c.T != (min(q0 + F.Q_BLOCK, c.L) - 1) // c.T for c in C for q0 in range(0, c.L, F.Q_BLOCK))      # a block over a frame boundary
    assert any(c.window[0] < 0 for c in C) and any(c.window[1] < 0 for c in C)
    assert any(0 < c.sink < F.KV_TILE for c in C) and any(c.sink and c.sink % F.KV_TILE == 0 for c in C)
    assert any(c.sink > F.KV_TILE and c.sink % F.KV_TILE for c in C)
    assert sum(bool(c.allowed().all()) for c in C) == 1
    gaps, one_run = [], False
    for c in C:
        runs = F.runs_brute(c.L, c.window, c.T, c.sink)
        assert all(1 <= len(r) <= 2 for r in runs)
        gaps.append(sum(len(r) == 2 for r in runs))
        one_run |= any(len(r) == 1 for r in runs)
    assert gaps == F.GAP_BLOCKS and sum(g > 0 for g in gaps) == 5 and one_run


WINDOWS = [(0, 0), (1, 1), (1, 0), (0, 1), (2, 1), (3, 3), (-1, 0), (0, -1), (-1, 2), (2, -1), (-1, -1), (40, 40)]
SINKS = [0, 1, 5, 63, 64, 65, 128, 300, 448]


def _planner_is_the_brute_force(hip, L, window, T, sink):
    got = hip.attn_window_frames_tiles(L, window, T, sink)
    # a window without a left bound drops the sink, as flexam_attn_fwd_window_frames does (nothing lies to the left of such a window)
    assert got == F.runs_brute(L, window, T, 0 if window[0] < 0 else sink), (L, window, T, sink)
    return got


@pytest.mark.parametrize("case", F.CASES, ids=F.ids(F.CASES))
def test_planner_equals_brute_force_at_the_cases(case):
    from flexam_amd import hip
    assert (hip.ATTN_Q_BLOCK, hip.ATTN_KV_TILE) == (F.Q_BLOCK, F.KV_TILE)
    _planner_is_the_brute_force(hip, case.L, case.window, case.T, case.sink)


@pytest.mark.parametrize("L", [1, 63, 64, 65, 70, 256, 257, 600, 900, 1111, 1344, 1500])
def test_planner_equals_brute_force_around_the_cases(L):
    from flexam_amd import hip
    for T in (1, 7, 37, 48, 63, 64, 65, 100, 200, 256, 300, 448, L, L + 9):
        for window in WINDOWS:
            for sink in (SINKS if T in (37, 64, 100, 448) else [0, 70]) + [L, L + 9]:
                _planner_is_the_brute_force(hip, L, window, T, sink)
    for window in WINDOWS:                                   # T = 1: frames are tokens
        for sink in SINKS:
            if window[0] >= 0 or sink == 0:                  # (attn_window_sink_tiles keeps the sink tiles under an unbounded left side)
                assert hip.attn_window_frames_tiles(L, window, 1, sink) == hip.attn_window_sink_tiles(L, window, sink), (L, window, sink)
            assert torch.equal(F.allowed(L, window, 1, sink), S.allowed(L, window, sink))
    with pytest.raises(ValueError):
        hip.attn_window_frames_tiles(L, (1, 1), 0)
    with pytest.raises(ValueError):
        hip.attn_window_frames_tiles(L, (1, 1), 7, -1)


def test_planner_at_the_flagship_shape():
    """L = 11648 (26 frames of 448 tokens = 7 key tiles), 46 query blocks x 182 key tiles = 8372 visits for full attention: the visits of
    +-2, +-5, +-12 frames, frame-block-causal and per-frame attention, without a sink and with the reference image (448 tokens) as the
    sink -- against brute-force enumeration at that shape, and against the figures worked out from the rule."""
    from flexam_amd import hip
    L, T = 11648, 448
    count = lambda runs: sum(b - a + 1 for r in runs for a, b in r)
    table = {(2, 2): (1652, 1932), (5, 5): (3262, 3507), (12, 12): (6167, 6328), (-1, 0): (4459, 4459), (0, 0): (455, 763)}
    assert hip.attn_kv_tiles(L) == 182 and count(hip.attn_window_frames_tiles(L, (-1, -1), T)) == 46 * 182 == 8372
    for window, want in table.items():
        for sink, n in zip((0, 448), want):
            runs = hip.attn_window_frames_tiles(L, window, T, sink)
            assert len(runs) == 46 and runs == F.runs_brute(L, window, T, sink), (window, sink)
            assert count(runs) == n, (window, sink, count(runs))
    # every frame boundary is a tile boundary: no tile of any window range is cut by a row's range
    assert T % F.KV_TILE == 0


def test_the_model_takes_window_frames_and_hands_it_to_every_self_attention():
    """The constructor argument, the path from_pretrained's transformer_additional_kwargs take (from_config), the config entry and the
    modules; cross-attention gets none; window_size and window_frames together raise; the default is (-1, -1)."""
    from flexam_amd.wan_transformer3d_FlexAM import Wan2_2Transformer3DModel_FlexAM as Model
    from oracle import dit as O
    kw = dict(O.DIT_TINY)
    kw.pop("eps")
    m = Model.from_config(kw, window_frames=(1, 0), window_sink=64)
    assert tuple(m.config["window_frames"]) == (1, 0) and m.window_frames == (1, 0) and m.config["window_sink"] == 64
    assert tuple(m.config["window_size"]) == (-1, -1)
    assert all(b.self_attn.window_frames == (1, 0) and b.self_attn.window_sink == 64 and b.self_attn.window_size == (-1, -1) for b in m.blocks)
    assert not any(hasattr(b.cross_attn, "window_frames") for b in m.blocks)
    d = Model(**kw)
    assert tuple(d.config["window_frames"]) == (-1, -1) and all(b.self_attn.window_frames == (-1, -1) for b in d.blocks)
    assert Model(**kw, window_frames=[-1, 0]).blocks[0].self_attn.window_frames == (-1, 0)
    with pytest.raises(ValueError, match="window_frames"):
        Model(**kw, window_size=(40, 40), window_frames=(1, 0))
    assert Model(**kw, window_size=(40, 40)).config["window_frames"] == (-1, -1)          # either alone is accepted


def test_frame_tokens_come_from_the_token_grid_and_whole_frames_are_required():
    from flexam_amd.wan_transformer3d_FlexAM import frame_tokens
    assert frame_tokens([[4, 8, 8]], 256) == 64 and frame_tokens(torch.tensor([[26, 16, 28], [26, 16, 28]]), 11648) == 448
    with pytest.raises(NotImplementedError, match="250.*64"):
        frame_tokens([[4, 8, 8]], 250)
