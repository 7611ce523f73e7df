"""Integer-score cases for the windowed bf16 flash-attention kernel with the window counted in frames (flexam_attn_fwd_window_frames:
attn_window_kernel of csrc/attn.hip with AttnParams::win_frame > 0), shared by tests/test_attn_window_frames_cases_cpu.py (which proves the
cases are not blind and holds the planner hip.attn_window_frames_tiles to a brute-force count) and tests/test_attn_window_frames_gpu.py
(which runs them).  Not a test module.  Construction (`build`) and `bf16_ulp` are those of tests/attn_window_sink_cases.py: q = 1 in
channel 0, k alternating 0 / 1 per key tile, v one-hot at j % 128, so every score is 0 or 1 in exp2 units and output channel c is the
softmax mass of the visible keys congruent to c modulo 128.

The mask: frames of T tokens are counted from token 0, frame(t) = t // T; window_frames = (a, b), a negative side unbounded; sink >= 0
leading keys are visible to every query.  Query i sees key j iff
    j < sink  or  ((a < 0 or j // T >= i // T - a) and (b < 0 or j // T <= i // T + b)).
Lq == Lk = L, and L need not be a multiple of T (a ragged last frame).  Every row sees its own frame: no row is empty."""
import math
import os
import sys
from dataclasses import dataclass

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_sink_cases as S  # noqa: E402

KV_TILE, Q_BLOCK, HEAD_DIM = S.KV_TILE, S.Q_BLOCK, S.HEAD_DIM
build, bf16_ulp = S.build, S.bf16_ulp


def allowed(L, window_frames, T, sink):
    """[L, L] bool: row i sees key j.  The rule above, term for term."""
    a, b = window_frames
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    return (j < sink) | ((torch.tensor(a < 0) | (j // T >= i // T - a)) & (torch.tensor(b < 0) | (j // T <= i // T + b)))


def row_range(L, window_frames, T, i):
    """(lo, hi): the first and the last key of row i's window, clipped to [0, L)."""
    a, b = window_frames
    return (0 if a < 0 else max(0, (i // T - a) * T)), (L - 1 if b < 0 else min(L - 1, (i // T + b + 1) * T - 1))


def reference(q, k, v, ok):
    """Masked softmax-attention in float64 under the [L, L] mask `ok`, scores in exp2 units: [B, L, H, 128].  Nothing of the kernel's
    walk is in it."""
    s = torch.einsum("blhd,bmhd->bhlm", q, k)
    s = s.masked_fill(~ok, -math.inf)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return torch.einsum("bhlm,bmhd->blhd", p / p.sum(-1, keepdim=True), v)


def altered_masks(L, window_frames, T, sink):
    """The mask with ONE key added or dropped at either end of EVERY row's window range [lo, hi] at once: add hi + 1, drop hi, add
    lo - 1, drop lo (where that key exists, is not already visible through the sink, and the range keeps a key).  [(name, mask), ...]."""
    ok = allowed(L, window_frames, T, sink)
    rows = torch.arange(L)
    lo, hi = (torch.tensor(x) for x in zip(*(row_range(L, window_frames, T, i) for i in range(L))))
    out = []
    for name, key, value in (("add hi+1", hi + 1, True), ("drop hi", hi, False), ("add lo-1", lo - 1, True), ("drop lo", lo, False)):
        m = ok.clone()
        sel = (key >= 0) & (key < L) & (value | ((hi > lo) & (key >= sink)))      # a dropped key is one the window alone shows, not the last
        m[rows[sel], key[sel]] = value
        out.append((name, m))
    return out


def runs_brute(L, window_frames, T, sink):
    """Per query block the runs of key tiles that hold a visible (row, key) pair, by enumeration: [[(first, last), ...], ...]."""
    ok = allowed(L, window_frames, T, sink)
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
    window: tuple          # (a, b) in frames
    T: int
    sink: int
    B: int = 1
    H: int = 2

    @property
    def name(self):
        return f"L{self.L}-f{self.window[0]}_{self.window[1]}-T{self.T}-s{self.sink}-b{self.B}h{self.H}"

    def inputs(self):
        return build(self.L, self.B, self.H)

    def allowed(self):
        return allowed(self.L, self.window, self.T, self.sink)

    def want(self, q, k, v):
        return reference(q, k, v, self.allowed())


# T below a key tile; T between a tile and a query block with an unaligned sink (B = 2, H = 3); T equal to a tile; per-frame attention
# with a tile-aligned sink; frame-block-causal; its mirror; a few keys with a sink below a tile (B = 2, H = 3); the flagship's 448-token
# frame (7 tiles: no window tile is masked); the same with a ragged last frame and a frame of sink; T above a query block, sink = 1; a
# window that holds everything; T = 37 (frames that straddle tiles and blocks everywhere) under a large unaligned sink
CASES = [Case(600, (1, 1), 48, 0), Case(600, (1, 0), 100, 70, B=2, H=3), Case(1111, (2, 1), 64, 0), Case(1111, (0, 0), 200, 128),
         Case(1111, (-1, 0), 100, 0), Case(600, (0, -1), 100, 0), Case(70, (1, 1), 7, 5, B=2, H=3), Case(1344, (1, 1), 448, 0),
         Case(1500, (0, 1), 448, 448), Case(900, (0, 0), 300, 1), Case(600, (3, 3), 300, 0), Case(1111, (1, 1), 37, 300)]
# query blocks whose tile set has a gap, by enumeration (tests/test_attn_window_frames_cases_cpu.py holds runs_brute to them)
GAP_BLOCKS = [0, 1, 0, 4, 0, 0, 0, 0, 2, 2, 0, 3]


def ids(cases):
    return [c.name for c in cases]
