"""Integer-score cases for the windowed bf16 flash-attention kernel at a query offset (flexam_attn_fwd_window_at: attn_window_at_kernel of
csrc/attn.hip), shared by tests/test_attn_window_at_cases_cpu.py (which proves the cases are not blind -- to a key at either end of a
row's range and to the offset itself -- and holds the planner hip.attn_window_at_tiles to a brute-force count) and
tests/test_attn_window_at_gpu.py (which runs them).  Not a test module.  Construction (`build`) and `bf16_ulp` are those of
tests/attn_window_sink_cases.py: q = 1 in channel 0, k alternating 0 / 1 per key tile, v one-hot at j % 128, so every score is 0 or 1 in
exp2 units and output channel c is the softmax mass of the visible keys congruent to c modulo 128.  q does not depend on the row: a row's
output is a function of its mask alone, which is what makes a wrong offset visible.

A case is a rank's call of a sequence of Lk tokens cut over `ranks` ranks: chunk = ceil(Lk / ranks), the call's rows are the global tokens
q_offset = rank * chunk .. q_offset + chunk - 1, pad rows (global tokens from Lk on) included; the keys are the first Lk tokens.  rank =
None is the all-to-all form: q_offset = 0 and every one of the ranks * chunk padded rows.

The mask: global token g sees key j (0 <= j < Lk) iff
    j < sink  or  lo(g) <= j <= hi(g)
with lo = g - a, hi = g + b for a token window (T = 0) and lo = (g // T - a) T, hi = (g // T + b + 1) T - 1 for a window of frames of T
tokens; window = (a, b), a negative side unbounded, and a < 0 drops the sink (nothing lies to the left of such a window: the rule of the
sibling entry points).  A row that sees no key is zeros."""
import functools
import math
import os
import sys
from dataclasses import dataclass
from typing import Optional

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_sink_cases as S  # noqa: E402

KV_TILE, Q_BLOCK, HEAD_DIM = S.KV_TILE, S.Q_BLOCK, S.HEAD_DIM
build, bf16_ulp = S.build, S.bf16_ulp


def row_ranges(rows, window, T):
    """(lo, hi) int64 tensors: the unclipped window of every global token in `rows`; an unbounded side is -2^40 / 2^40."""
    a, b = window
    g = torch.as_tensor(rows, dtype=torch.int64)
    t = max(int(T), 1)                                           # a token window is a window of one-token frames
    f = g // t
    lo = (f - a) * t if a >= 0 else torch.full_like(g, -(1 << 40))
    hi = (f + b + 1) * t - 1 if b >= 0 else torch.full_like(g, 1 << 40)
    return lo, hi


def allowed(rows, Lk, window, T, sink):
    """[len(rows), Lk] bool: global token rows[i] sees key j.  The rule above, term for term."""
    lo, hi = row_ranges(rows, window, T)
    j = torch.arange(Lk)[None, :]
    return (j < (sink if window[0] >= 0 else 0)) | ((j >= lo[:, None]) & (j <= hi[:, None]))


def reference(q, k, v, ok):
    """Masked softmax-attention in float64 under the [Lq, Lk] mask `ok`, scores in exp2 units: [B, Lq, H, 128]; a row that sees no key is
    zeros.  Nothing of the kernel's walk is in it."""
    s = torch.einsum("blhd,bmhd->bhlm", q, k)
    s = s.masked_fill(~ok, -math.inf)
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - m.masked_fill(m == -math.inf, 0.0))
    return torch.einsum("bhlm,bmhd->blhd", p / p.sum(-1, keepdim=True).clamp_min(1.0), v)       # (an empty row: p = 0 everywhere)


@functools.lru_cache(maxsize=None)
def _sequence(Lk, window, T, sink, ranks, B, H):
    """Inputs of the padded sequence and its float64 masked attention, every padded row a query: computed once per split."""
    chunk = -(-Lk // ranks)
    q, k, v = build(ranks * chunk, B, H)
    k, v = k[:, :Lk], v[:, :Lk]
    return q, k, v, reference(q, k, v, allowed(range(ranks * chunk), Lk, window, T, sink))


@dataclass(frozen=True)
class Case:
    Lk: int
    window: tuple          # (a, b): tokens (T = 0) or frames of T tokens
    T: int
    sink: int
    ranks: int
    rank: Optional[int]    # None: the all-to-all form, offset 0 and all ranks * chunk rows
    B: int = 1
    H: int = 2

    @property
    def chunk(self):
        return -(-self.Lk // self.ranks)

    @property
    def q_offset(self):
        return 0 if self.rank is None else self.rank * self.chunk

    @property
    def Lq(self):
        return self.ranks * self.chunk if self.rank is None else self.chunk

    @property
    def rows(self):
        return range(self.q_offset, self.q_offset + self.Lq)

    @property
    def name(self):
        form = f"f{self.window[0]}_{self.window[1]}-T{self.T}" if self.T else f"w{self.window[0]}_{self.window[1]}"
        where = "a2a" if self.rank is None else f"r{self.rank}"
        return f"L{self.Lk}-{form}-s{self.sink}-{where}of{self.ranks}-b{self.B}h{self.H}"

    def _seq(self):
        return _sequence(self.Lk, self.window, self.T, self.sink, self.ranks, self.B, self.H)

    def inputs(self):
        """q [B, Lq, H, 128]: the chunk's rows of the padded sequence; k, v [B, Lk, H, 128]: the real tokens."""
        q, k, v, _ = self._seq()
        return q[:, self.q_offset:self.q_offset + self.Lq], k, v

    def allowed(self):
        return allowed(self.rows, self.Lk, self.window, self.T, self.sink)

    def want(self):
        """The float64 masked attention of the full sequence, this call's rows."""
        return self._seq()[3][:, self.q_offset:self.q_offset + self.Lq]

    def empty_rows(self):
        """[Lq] bool: the rows that see no key."""
        return ~self.allowed().any(1)


def altered_masks(case):
    """The case's mask with ONE key added or dropped at either end of EVERY row's window range [lo, hi] (clipped to the keys) at once: add
    hi + 1, drop hi, add lo - 1, drop lo -- where that key exists, is not visible through the sink anyway, and the row has a range that
    keeps a key.  [(name, mask, [Lq] bool rows altered), ...]."""
    ok = case.allowed()
    lo, hi = row_ranges(case.rows, case.window, case.T)
    lo, hi = lo.clamp_min(0), hi.clamp_max(case.Lk - 1)
    sink = case.sink if case.window[0] >= 0 else 0
    rows = torch.arange(case.Lq)
    out = []
    for name, key, value in (("add hi+1", hi + 1, True), ("drop hi", hi, False), ("add lo-1", lo - 1, True), ("drop lo", lo, False)):
        sel = (lo <= hi) & (key >= 0) & (key < case.Lk) & (key >= sink) & (value | (hi > lo))
        m = ok.clone()
        m[rows[sel], key[sel]] = value
        out.append((name, m, sel))
    return out


def runs_brute(case):
    """Per query block of the call the runs of key tiles that hold a visible (row, key) pair, by enumeration; [] for a block that sees
    nothing: [[(first, last), ...], ...]."""
    return runs_of(case.allowed(), case.Lk)


def runs_of(ok, Lk):
    out = []
    for r0 in range(0, ok.shape[0], Q_BLOCK):
        seen = ok[r0:r0 + Q_BLOCK].any(0)
        hit = [t for t in range(-(-Lk // KV_TILE)) if bool(seen[t * KV_TILE:(t + 1) * KV_TILE].any())]
        runs = []
        for t in hit:
            if runs and runs[-1][1] == t - 1:
                runs[-1][1] = t
            else:
                runs.append([t, t])
        out.append([tuple(r) for r in runs])
    return out


def _split(Lk, window, T, sink, ranks, only=None, wide=None):
    """Every rank of one split (or the ranks in `only`); `wide`: the rank that runs B = 2, H = 3."""
    return [Case(Lk, window, T, sink, ranks, r, **(dict(B=2, H=3) if r == wide else {})) for r in (range(ranks) if only is None else only)]


# 1: chunk 278, offsets off every tile and block boundary, one pad row; B = 2, H = 3 on rank 1
# 2: causal, two pad rows that still see keys            3: the right side unbounded
# 4: chunk 86; the two pad rows see nothing (sink 0) or the sink alone (sink 5)
# 5: the flagship's 448-token frame: a rank is a frame (3), chunks straddle frames (4, 8)
# 6: frames of 37 straddle tiles and blocks everywhere, large unaligned sink
# 7: per-frame attention, one pad row in a frame that does not exist: nothing (sink 0) or the sink frame (sink 448)
# 8: the all-to-all form: offset 0, 1113 rows, the pad rows behind the keys
# 9: five keys over four ranks: a call with one real row and one pad row, and a call that is all pads (zeros out, no key read)
CASES = (_split(1111, (100, 37), 0, 70, 4, wide=1) + _split(1111, (-1, 0), 0, 0, 3) + _split(600, (0, -1), 0, 0, 2)
         + _split(600, (0, 0), 0, 0, 7) + _split(600, (0, 0), 0, 5, 7)
         + _split(1344, (1, 1), 448, 0, 3) + _split(1344, (1, 1), 448, 0, 4) + _split(1344, (1, 1), 448, 0, 8)
         + _split(1111, (1, 1), 37, 300, 4) + _split(896, (0, 0), 448, 0, 3) + _split(896, (0, 0), 448, 448, 3)
         + [Case(1111, (100, 37), 0, 70, 3, None)] + _split(5, (0, 0), 0, 0, 4, only=(2, 3)))


def ids(cases):
    return [c.name for c in cases]
