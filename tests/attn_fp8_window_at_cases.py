"""Integer-score cases for the windowed MXFP8 self-attention at a query offset on chunked records (flexam_attn_fwd_fp8_window_at:
attn8_window_at_kernel / attn8_window_at_oshift_kernel of csrc/attn_fp8.inc), shared by tests/test_attn_fp8_window_at_cases_cpu.py (which
proves on the restatement alone that they are not blind) and tests/test_attn_fp8_window_at_gpu.py (which runs them).  Not a test module.

A case is a sequence of L tokens cut over `ranks` ranks the way resolve_mode pads the MXFP8 record gather: lc = 64 ceil(L / (64 ranks))
rows per rank.  Rank r's call has Lq = lc, q_offset = r lc, Lk = L; its records are the pack of each rank's lc keys, stacked rank-major
([ranks][B][H][lc / 64] records).  Global tokens from L on are pad rows: queries, never keys.

Operands: WR.integer_case of the L real tokens (integer scores, operands that pack losslessly).  A pad row g >= L carries the query AND,
in its rank's records, the key and value of real token g - pads (pads = ranks lc - L): integers too, so that a kernel which lets a pad
key in moves the output, and a pad row's scores stay integers.  The mask is tests/attn_window_at_cases.py's `allowed` (the rule of
flexam_attn_fwd_window_at), the walk tests/mxfp8_window_restatement.py's `window_pass` over the rows that see a key; a row that sees none
is zeros, with an output shift as well."""
import functools
import os
import sys
from dataclasses import dataclass

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_at_cases as A  # noqa: E402
import mxfp8_restatement as R  # noqa: E402
import mxfp8_window_restatement as WR  # noqa: E402

KV_TILE = A.KV_TILE
bf16_ulp = WR.bf16_ulp


def chunk_rows(L, ranks):
    """lc: the rows of a rank under the record gather's padding (dit_layout.resolve_mode: Lp a multiple of 64 x ranks)."""
    return KV_TILE * -(-L // (KV_TILE * ranks))


def pad_sequence(x, L, ranks):
    """[B, L, H, 128] -> [B, ranks lc, H, 128]: pad row g carries real row g - pads."""
    pads = ranks * chunk_rows(L, ranks) - L
    assert 0 <= pads <= L
    return torch.cat([x, x[:, L - pads:L]], dim=1)


def restate(q_rows, k, v, ok, shift=None):
    """q_rows [B, Lq, H, 128], k, v [B, Lk, H, 128] (bf16 values as handed to the pack, q in exp2 units) under ok [Lq, Lk] -> float64
    [B, Lq, H, 128]: WR.window_pass over the rows that see a key (+ shift [B, H * 128]), zeros for the others."""
    B, Lq, H, D = q_rows.shape
    qd, kd, vd = R.dequant_rows(q_rows), R.dequant_rows(k), R.dequant_v(v)
    live = ok.any(dim=1)
    out = torch.zeros(B, Lq, H, D, dtype=torch.float64)
    if not bool(live.any()):
        return out
    for b in range(B):
        for h in range(H):
            o = WR.window_pass(qd[b, h][live] @ kd[b, h].t(), vd[b, h], ok[live])
            if shift is not None:
                o = o + shift[b].double().cpu().view(H, D)[h]
            out[b, live, h] = o
    return out


@functools.lru_cache(maxsize=None)
def _sequence(L, window, sink, T, ranks, B, H, seed):
    q, k, v = (t.to(torch.bfloat16) for t in WR.integer_case(B, H, L, window, seed, T))
    return pad_sequence(q, L, ranks), pad_sequence(k, L, ranks), pad_sequence(v, L, ranks)


@dataclass(frozen=True)
class Call:
    """One rank's call.  (The attributes A.altered_masks reads are here: Lk, Lq, rows, window, T, sink, allowed().)"""
    Lk: int
    ranks: int
    rank: int
    window: tuple
    sink: int = 0
    T: int = 0
    shifted: bool = False
    B: int = 1
    H: int = 2

    @property
    def lc(self):
        return chunk_rows(self.Lk, self.ranks)

    Lq = lc

    @property
    def chunk_tiles(self):
        return self.lc // KV_TILE

    @property
    def q_offset(self):
        return self.rank * self.lc

    @property
    def rows(self):
        return range(self.q_offset, self.q_offset + self.lc)

    @property
    def seed(self):
        return self.Lk + self.sink + self.T

    @property
    def name(self):
        form = f"f{self.window[0]}_{self.window[1]}-T{self.T}" if self.T else f"w{self.window[0]}_{self.window[1]}"
        return f"L{self.Lk}-{form}-s{self.sink}-r{self.rank}of{self.ranks}" + ("-oshift" if self.shifted else "")

    def padded(self):
        """q, k, v [B, ranks lc, H, 128] bf16 of the padded sequence: rank c's pack input is rows [c lc, (c + 1) lc) of all three."""
        return _sequence(self.Lk, self.window, self.sink, self.T, self.ranks, self.B, self.H, self.seed)

    def inputs(self):
        """q of this call's rows; k, v of the Lk real tokens."""
        q, k, v = self.padded()
        return q[:, self.q_offset:self.q_offset + self.lc], k[:, :self.Lk], v[:, :self.Lk]

    def shift(self):
        """fp32 [B, H * 128] or None: whole numbers of the channel's own sign (nothing cancels in O / l + shift)."""
        if not self.shifted:
            return None
        v = self.padded()[2]
        sign = torch.sign(v[0, 0].float()).reshape(1, self.H * 128)
        return (sign * (1 + torch.arange(self.H * 128) % 5).float()).expand(self.B, -1).contiguous()

    def allowed(self):
        return A.allowed(self.rows, self.Lk, self.window, self.T, self.sink)

    def empty_rows(self):
        return ~self.allowed().any(dim=1)

    def want(self, ok=None, k=None, v=None):
        """The restatement of this call (under another mask or other keys: the blindness proofs)."""
        q, k0, v0 = self.inputs()
        return restate(q, k0 if k is None else k, v0 if v is None else v, self.allowed() if ok is None else ok, self.shift())


def _split(L, ranks, window, sink=0, T=0, shifted=False):
    return [Call(L, ranks, r, window, sink, T, shifted) for r in range(ranks)]


# L = 70 on 2 ranks (lc = 64): rank 1 is 6 real rows + 58 pad rows, one ragged tile; under (3, 2) without a sink the pad rows from global
#   token 73 on see no key
# L = 600 on 2 ranks (lc = 320): the chunk boundary at tile 5, a unit of 256 rows + one of 64; a sink edge inside a tile and a gap between
#   the sink tiles and the window tiles on rank 1; units that grow (no left bound, the sink dropped); frame boundaries inside tiles
# L = 1111 on 3 ranks (lc = 384): 41 pad rows on rank 2, the chunk division by chunk_tiles = 6
CASES = (_split(70, 2, (3, 2)) + _split(70, 2, (3, 2), sink=5) + _split(70, 2, (-1, 0)) + _split(70, 2, (1, 1), sink=5, T=7)
         + _split(70, 2, (3, 2), shifted=True)
         + _split(600, 2, (100, 37), sink=70) + _split(600, 2, (-1, 0), sink=70) + _split(600, 2, (1, 1), T=48)
         + _split(1111, 3, (200, 100), sink=192) + _split(1111, 3, (64, 64), sink=128) + _split(1111, 3, (2, 1), T=64))


def ids(cases):
    return [c.name for c in cases]


def chunk_shifted_keys(call):
    """k, v [B, Lk, H, 128] as a kernel reads them that takes chunk c where chunk c + 1 is meant: key j >= lc is key j - lc."""
    _, k, v = call.inputs()
    j = torch.arange(call.Lk)
    src = torch.where(j >= call.lc, j - call.lc, j)
    return k[:, src], v[:, src]
