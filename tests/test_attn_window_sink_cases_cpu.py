"""CPU: the cases of tests/attn_window_sink_cases.py (windowed attention with a sink) are not blind, they reach every path of the
kernel's tile walk, and the planner hip.attn_window_sink_tiles equals a brute-force enumeration.

Not blind: for every case, moving either edge of the window or the sink by one key in either direction changes every row whose key set
that move alters by at least attn_window_cases.SENSITIVITY_ULPS (8) bf16 ulps in some channel and leaves every other row bit-identical.
A kernel that lets one key too many in, or leaves one out, at an edge or at the sink of any row therefore misses the 1-ulp bound of
tests/test_attn_window_sink_gpu.py.

Least change of an altered row over the moves, in ulps, as computed here (case order of CASES): 46.8, 40.8, 63.5, 42.2, 128.0, 45.6,
74.4, 35.1, 35.5."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_cases as W  # noqa: E402
import attn_window_sink_cases as S  # noqa: E402
from test_attn_window_cases_cpu import WINDOWS  # noqa: E402


@pytest.mark.parametrize("case", S.CASES, ids=S.ids(S.CASES))
def test_cases_are_sensitive_to_one_key_at_either_edge_and_at_the_sink(case):
    q, k, v = case.inputs()
    for t in (q, k, v):
        assert torch.equal(t.to(torch.bfloat16).double(), t)                      # the kernels get exactly these values
    s = torch.einsum("blhd,bmhd->bhlm", q, k)
    assert torch.equal(s, s.round())                                              # integer scores: every p is a power of two
    want = case.want(q, k, v)
    ok = S.allowed(case.L, case.window, case.sink)
    assert bool(ok.any(1).all())                                                  # no empty row
    least = float("inf")
    for window, sink in S.moves(case.window, case.sink):
        other = S.reference(q, k, v, window, sink)
        altered = (S.allowed(case.L, window, sink) != ok).any(1)                  # [L]
        ulps = ((other - want).abs() / S.bf16_ulp(want)).amax(-1)                 # [B, L, H]: the most affected channel
        if altered.any():
            least = min(least, float(ulps[:, altered].min()))
        assert torch.equal(other[:, ~altered], want[:, ~altered]), (case.name, window, sink)
    print(f"{case.name}: least change of an altered row {least:.1f} ulps")
    assert least < float("inf") and least >= W.SENSITIVITY_ULPS, (case.name, least)


def test_the_cases_cover_the_paths_of_the_walk():
    """A sink unaligned to tiles, one below one tile, sink = 1, a tile-aligned one and one that is the whole sequence; query blocks with
    one run of tiles and with two (counted by enumeration); a ragged L; windows narrower and wider than a query block; more than one
    batch and head; a tile wholly below the sink that the window does not reach (interior by the sink alone)."""
    C = S.CASES
    assert any(c.sink % S.KV_TILE and c.sink > S.KV_TILE for c in C) and any(1 < c.sink < S.KV_TILE for c in C)
    assert any(c.sink == 1 for c in C) and any(c.sink % S.KV_TILE == 0 and c.sink < c.L for c in C) and any(c.sink >= c.L for c in C)
    assert any(c.L % S.KV_TILE and c.L % S.Q_BLOCK for c in C) and any(c.B >= 2 and c.H >= 3 for c in C)
    spans = [c.window[0] + c.window[1] + 1 for c in C]
    assert any(s < S.Q_BLOCK for s in spans) and any(s > S.Q_BLOCK for s in spans)
    gaps, one_run, sink_interior = [], False, False
    for c in C:
        runs = S.runs_brute(c.L, c.window, c.sink)
        assert all(1 <= len(r) <= 2 for r in runs)
        gaps.append(sum(len(r) == 2 for r in runs))
        one_run |= any(len(r) == 1 for r in runs)
        win = W.allowed(c.L, c.window)
        for q0 in range(0, c.L, S.Q_BLOCK):
            for t in range(c.sink // S.KV_TILE):
                sink_interior |= not bool(win[q0:q0 + S.Q_BLOCK, t * S.KV_TILE:(t + 1) * S.KV_TILE].any())
    assert gaps == S.GAP_BLOCKS == [1, 3, 4, 2, 0, 2, 4, 2, 0] and one_run and sink_interior


SINKS = [0, 1, 5, 63, 64, 65, 128, 448]


@pytest.mark.parametrize("L", [1, 63, 64, 65, 70, 256, 257, 600, 1111, 1500])
def test_planner_equals_brute_force(L):
    from flexam_amd import hip
    assert (hip.ATTN_Q_BLOCK, hip.ATTN_KV_TILE) == (S.Q_BLOCK, S.KV_TILE)
    for window in WINDOWS:
        for sink in SINKS + [L, L + 9]:
            assert hip.attn_window_sink_tiles(L, window, sink) == S.runs_brute(L, window, sink), (L, window, sink)
        assert hip.attn_window_sink_tiles(L, window, 0) == [[r] for r in hip.attn_window_tiles(L, window)], (L, window)
    with pytest.raises(ValueError):
        hip.attn_window_sink_tiles(L, (3, 2), -1)


def test_planner_at_the_flagship_shape():
    """L = 11648 (26 frames of 448 tokens), +-2 frames: 1400, 1688 and 1964 of the 46 x 182 (query block, key tile) pairs with no sink,
    with the reference image (448 tokens) and with the reference image and the first frame (896) as the sink."""
    from flexam_amd import hip
    count = lambda sink: sum(b - a + 1 for runs in hip.attn_window_sink_tiles(11648, (896, 896), sink) for a, b in runs)
    assert [count(s) for s in (0, 448, 896)] == [1400, 1688, 1964]
    assert len(hip.attn_window_sink_tiles(11648, (896, 896), 0)) == 46 and hip.attn_kv_tiles(11648) == 182


def test_the_model_takes_window_sink_and_hands_it_to_every_self_attention():
    """The constructor argument, the path from_pretrained's transformer_additional_kwargs take (from_config), the config entry and the
    modules; a negative count raises, and without a window the sink is accepted."""
    from flexam_amd.wan_transformer3d_FlexAM import Wan2_2Transformer3DModel_FlexAM as Model
    from oracle import dit as O
    kw = dict(O.DIT_TINY)
    kw.pop("eps")
    m = Model.from_config(kw, window_size=(40, 40), window_sink=64)
    assert m.config["window_sink"] == 64 and m.window_sink == 64 and tuple(m.config["window_size"]) == (40, 40)
    assert all(b.self_attn.window_sink == 64 and b.self_attn.window_size == (40, 40) for b in m.blocks)
    assert not any(hasattr(b.cross_attn, "window_sink") for b in m.blocks)
    assert Model(**kw).config["window_sink"] == 0 and Model(**kw, window_sink=7).blocks[0].self_attn.window_sink == 7
    with pytest.raises(ValueError, match="window_sink"):
        Model(**kw, window_size=(40, 40), window_sink=-1)


def test_without_a_sink_the_restatement_is_the_window_cases_reference():
    for L, window in ((600, (100, 37)), (70, (3, 2)), (600, (-1, 0))):
        q, k, v = S.build(L)
        assert torch.equal(S.reference(q, k, v, window, 0), W.reference(q, k, v, window))
        assert torch.equal(S.allowed(L, window, 0), W.allowed(L, window))
