"""Integer-score cases for the windowed bf16 flash-attention kernel with a sink (flexam_attn_fwd_window_sink: attn_window_kernel of
csrc/attn.hip with AttnParams::win_sink > 0), shared by tests/test_attn_window_sink_cases_cpu.py (which proves the cases are not blind
and holds the planner hip.attn_window_sink_tiles to a brute-force count) and tests/test_attn_window_sink_gpu.py (which runs them).  Not a
test module.  Geometry, `allowed`, `bf16_ulp` and `edge_moves` are those of tests/attn_window_cases.py.

The mask: sink >= 0 leading keys are visible to every query, whatever the right side of the window says (the model is not causal);
query i sees key j iff
    j < sink  or  ((left < 0 or j >= i - left) and (right < 0 or j <= i + right)).

Construction (head dim 128, head index h; everything else is 0):
    q[:, :, h, 0] = 1        k[:, j, h, 0] = (j // 64 + h) % 2        v[:, j, h, j % 128] = 1
Every score is 0 or 1 in exp2 units, constant over a key tile and alternating from tile to tile, so every p is 1 or 1/2 whatever reference
the online softmax holds.  Output channel c is the softmax mass of the visible keys congruent to c modulo 128: a key let in or left out
moves its channel by a large fraction, wherever in the row's key set it lies.  (The edge markers of tests/attn_window_cases.py collide
with a marker for the sink in rows whose edge is congruent to the sink modulo 64: those rows move by 0.0 - 0.4 ulps only.)"""
import math
import os
import sys
from dataclasses import dataclass

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_cases as W  # noqa: E402

KV_TILE, Q_BLOCK, HEAD_DIM = W.KV_TILE, W.Q_BLOCK, W.HEAD_DIM
bf16_ulp, edge_moves = W.bf16_ulp, W.edge_moves


def allowed(L, window, sink):
    """[L, L] bool: row i sees key j."""
    return W.allowed(L, window) | (torch.arange(L)[None, :] < sink)


def build(L, B=1, H=2):
    """q, k, v [B, L, H, 128] float64 holding 0 and 1."""
    q = torch.zeros(B, L, H, HEAD_DIM, dtype=torch.float64)
    k, v = torch.zeros_like(q), torch.zeros_like(q)
    j = torch.arange(L)
    for h in range(H):
        q[:, :, h, 0] = 1.0
        k[:, j, h, 0] = ((j // KV_TILE + h) % 2).double()
        v[:, j, h, j % HEAD_DIM] = 1.0
    return q, k, v


def reference(q, k, v, window, sink):
    """Masked softmax-attention in float64, scores in exp2 units: [B, L, H, 128].  Nothing of the kernel's walk is in it."""
    s = torch.einsum("blhd,bmhd->bhlm", q, k)
    s = s.masked_fill(~allowed(q.shape[1], window, sink), -math.inf)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return torch.einsum("bhlm,bmhd->blhd", p / p.sum(-1, keepdim=True), v)


def moves(window, sink):
    """The (window, sink) pairs one key away: either bounded edge of the window or the sink, in either direction."""
    return [(w, sink) for w in edge_moves(window)] + [(window, sink + 1)] + ([(window, sink - 1)] if sink > 0 else [])


def runs_brute(L, window, sink):
    """Per query block the runs of key tiles that hold a visible (row, key) pair, by enumeration: [[(first, last), ...], ...]."""
    ok = allowed(L, window, sink)
    out = []
    for q0 in range(0, L, Q_BLOCK):
        seen = ok[q0:q0 + Q_BLOCK].any(0)
        hit = [t for t in range(-(-L // KV_TILE)) if bool(seen[t * KV_TILE:(t + 1) * KV_TILE].any())]
        runs = []
        for t in hit:
            if runs and runs[-1][1] == t - 1:
                runs[-1][1] = t
            else:
                runs.append([t, t])
        out.append([tuple(r) for r in runs])
    return out


@dataclass(frozen=True)
class Case:
    L: int
    window: tuple
    sink: int
    B: int = 1
    H: int = 2

    @property
    def name(self):
        return f"L{self.L}-w{self.window[0]}_{self.window[1]}-s{self.sink}-b{self.B}h{self.H}"

    def inputs(self):
        return build(self.L, self.B, self.H)

    def want(self, q, k, v):
        return reference(q, k, v, self.window, self.sink)


# a sink unaligned to tiles (ragged L, B = 2, H = 3); a tile-aligned sink with a wide window; two tiles of sink under a window narrower
# than a query block; an anti-causal band with one sink tile; a sink below one tile on a few keys (B = 2, H = 3); a window wider than a
# query block; sink = 1; a frame of sink (7 tiles) under a narrow window; the sink is the whole sequence
CASES = [Case(600, (100, 37), 70, B=2, H=3), Case(1111, (200, 100), 192), Case(1111, (64, 64), 128), Case(600, (0, 200), 64),
         Case(70, (3, 2), 5, B=2, H=3), Case(900, (255, 100), 100), Case(1111, (100, 37), 1), Case(1111, (70, 70), 448),
         Case(600, (100, 37), 600)]
# query blocks whose tile set has a gap, by enumeration (tests/test_attn_window_sink_cases_cpu.py holds runs_brute to them)
GAP_BLOCKS = [1, 3, 4, 2, 0, 2, 4, 2, 0]


def ids(cases):
    return [c.name for c in cases]
