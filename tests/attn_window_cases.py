"""Integer-score cases for the windowed bf16 flash-attention kernel (attn_window_kernel of csrc/attn.hip), shared by
tests/test_attn_window_cases_cpu.py (which proves the cases are not blind and holds the tile planner to a brute-force count) and
tests/test_attn_window_gpu.py (which runs them).  Not a test module.

The mask is flash-attn's: window = (left, right), a negative side unbounded; query i sees key j iff
(left < 0 or j >= i - left) and (right < 0 or j <= i + right); causal is right = 0.  Lq == Lk.

Every score is an integer in exp2 units, so every p is an exact power of two whatever reference the online softmax holds; V holds small
positive integers.  The kernel's output must then be the float64 masked softmax-attention rounded once to bf16: `reference` below, which
has nothing of the kernel's walk (tile ranges, edge tiles, interior tiles) in it.

Construction (head dim 128, channels 0 .. 63 used): key j of head h has 4 in channel (j + 5 h) % 64; row i has + 2 in the channels
(i + d + 5 h) % 64 for d in {-left - 1, -left, right, right + 1}, over the bounded sides only; v[j, c] = (7 j + 3 c + h) % 13 + 1.  The two
keys just inside and the two just outside each edge then score 8 against a background of 0 (and so do the keys 64 apart from them): a
key wrongly let in or left out at an edge carries a weight comparable to the whole rest of the row."""
import math
from dataclasses import dataclass

import torch

KV_TILE, Q_BLOCK, HEAD_DIM = 64, 256, 128       # geometry of csrc/attn.hip (tests/test_abi_cpu.py holds the header to it)
SENSITIVITY_ULPS = 8.0
LN2 = math.log(2.0)                             # softmax_scale of the scale-in-kernel form: float32(LN2) * float32(log2 e) == 1.0f
# fp32 softmax-attention over at most 70 keys against float64, relative (p and v are positive: nothing cancels): the worst case of 70
# additions in the row sum and 70 in the weighted sum at 2^-24 each, plus the exponential, the division and the products: under 256 x 2^-24
FP32_REL = 2.0 ** -16


def allowed(L, window):
    """[L, L] bool: row i sees key j."""
    left, right = window
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    ok = torch.ones(L, L, dtype=torch.bool)
    if left >= 0:
        ok &= j >= i - left
    if right >= 0:
        ok &= j <= i + right
    return ok


def build(L, window, B=1, H=2):
    """q, k, v [B, L, H, 128] float64 holding small integers (exact in bf16)."""
    left, right = window
    q = torch.zeros(B, L, H, HEAD_DIM, dtype=torch.float64)
    k = torch.zeros(B, L, H, HEAD_DIM, dtype=torch.float64)
    v = torch.zeros(B, L, H, HEAD_DIM, dtype=torch.float64)
    i, c = torch.arange(L), torch.arange(HEAD_DIM)
    ds = ([-left - 1, -left] if left >= 0 else []) + ([right, right + 1] if right >= 0 else [])
    for h in range(H):
        k[:, i, h, (i + 5 * h) % 64] = 4.0
        for d in ds:
            q[:, i, h, (i + d + 5 * h) % 64] += 2.0
        v[:, :, h, :] = ((7 * i[:, None] + 3 * c[None, :] + h) % 13 + 1).double()
    return q, k, v


def reference(q, k, v, window, scale=None):
    """Masked softmax-attention in float64: [B, L, H, 128].  scale None: the scores are in exp2 units (what the kernels are given); else
    the usual softmax(scale q.k)."""
    s = torch.einsum("blhd,bmhd->bhlm", q, k) * (1.0 if scale is None else scale / LN2)
    s = s.masked_fill(~allowed(q.shape[1], window), -math.inf)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return torch.einsum("bhlm,bmhd->blhd", p / p.sum(-1, keepdim=True), v)


def bf16_ulp(x):
    """Spacing of bf16 at |x| (8 significant bits)."""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def edge_moves(window):
    """The windows one key wider or narrower at one bounded edge."""
    left, right = window
    out = []
    if left >= 0:
        out += [(left + 1, right)] + ([(left - 1, right)] if left > 0 else [])
    if right >= 0:
        out += [(left, right + 1)] + ([(left, right - 1)] if right > 0 else [])
    return out


def tiles_brute(L, window):
    """Per query block the first and last key tile that holds an admissible (row, key) pair, by enumeration."""
    ok = allowed(L, window)
    out = []
    for q0 in range(0, L, Q_BLOCK):
        seen = ok[q0:q0 + Q_BLOCK].any(0)
        hit = [t for t in range(-(-L // KV_TILE)) if bool(seen[t * KV_TILE:(t + 1) * KV_TILE].any())]
        assert hit == list(range(hit[0], hit[-1] + 1))          # a contiguous range: the union of the rows' intervals
        out.append((hit[0], hit[-1]))
    return out


@dataclass(frozen=True)
class Case:
    L: int
    window: tuple
    B: int = 1
    H: int = 2

    @property
    def name(self):
        return f"L{self.L}-w{self.window[0]}_{self.window[1]}-b{self.B}h{self.H}"

    def inputs(self):
        return build(self.L, self.window, self.B, self.H)

    def want(self, q, k, v):
        return reference(q, k, v, self.window)


# narrower than a query block (ragged L, B = 2, H = 3); causal; anti-causal; wider than a query block; a left-bounded causal band over
# 18 key tiles; a few keys (B = 2, H = 3); a window longer than the sequence.  (Windows of a thousand keys are blind under this
# construction -- (1111, 700, 500) moves an altered row by 2.7 ulps only: the background outweighs the edge keys.)
CASES = [Case(600, (100, 37), B=2, H=3), Case(600, (-1, 0)), Case(600, (0, -1)), Case(600, (255, 256)), Case(1111, (300, 0)),
         Case(70, (3, 2), B=2, H=3), Case(70, (80, 75))]


def ids(cases):
    return [c.name for c in cases]
