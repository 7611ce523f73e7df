"""Integer-score cases for the bf16 flash-attention kernels (csrc/attn.hip), shared by tests/test_attn_exact_cases_cpu.py (which proves
the cases are not blind) and tests/test_attn_exact_gpu.py (which runs them).  Not a test module.

Every score q.k is an integer in exp2 units, so every p = exp2(s - ref) is an exact power of two whatever reference the online softmax
holds (deferred rescale, wave-wide trigger, split ranges, merge); V holds small integers of one sign per channel.  The kernel's output
must then be the plain float64 softmax-attention of the same inputs rounded once to bf16: `reference` below, nothing of the kernel's walk.

Channels (head dim 128):
    0 ..  63   position code: key j has 4 in channel j % 64; row i has 3 in channels a and (a + P/2) % P, P = min(64, Lk)
   64 .. 110   tile code:     key j has 4 in channel 64 + (j // 64) % T; row i has 3 in channels 64 + b and 64 + (b + 1) % T
  111          lastkey cases: 1 in the rows, -log2(multiplicity) on the last key
  112 .. 119   key ramp 0 .. RAMP_TOP spread over 8 channels; +1 in the rising-ramp rows, -1 in the falling-ramp rows
  120 .. 123   8 on the marker keys (the last real key of a call);    1 in the rows of kind 2: +32 there
  124 .. 127   8 on the first key of every split range;               1 in the rows of kind 3: +32 there
with T = ceil(Lk / 64), a = (i + 3 bh) % (P/2), b = (i // 32 + bh) % T.  A plain row scores 24 on four keys (two positions in each of two
adjacent tiles), 12 on the keys that match one code and 0 elsewhere: every key has p >= 0.24 in some row.  Four rows of every 32-row
wave are special (one of each kind, at positions that move by 5 from wave to wave, so the plain rows of two adjacent waves cover every
position): they move the reference, the plain rows of the same wave are rescaled along with them."""
import math
from dataclasses import dataclass

import torch

KV_TILE, Q_BLOCK, HEAD_DIM = 64, 256, 128       # geometry of csrc/attn.hip (tests/test_abi_cpu.py holds the header to it)
RAMP_TOP = 48
RESCALE_THR = 8.0                               # RESCALE_THR_LOG2 of csrc/attn.hip
SENSITIVITY_ULPS = 8.0
LN2 = math.log(2.0)                             # softmax_scale of the scale-in-kernel cases: float32(LN2) * float32(log2 e) == 1.0f


def tiles(lk):
    return -(-lk // KV_TILE)


def split_starts(lk, kv_splits):
    """First key of every key range but the first, as attn_run cuts them: ranges of ceil(tiles / S) whole tiles, empty ones dropped."""
    t = tiles(lk)
    per = -(-t // max(1, min(kv_splits, t)))
    return [s * per * KV_TILE for s in range(1, -(-t // per))]


def row_kinds(lq):
    """-1 for a plain row, else 0 rising ramp, 1 falling ramp, 2 marker keys, 3 range starts."""
    i = torch.arange(lq)
    ph = (i % 32 - 5 * (i // 32)) % 32
    return torch.where(ph % 8 == 0, ph // 8, torch.full_like(ph, -1))


def build(lq, lk, B=1, H=2, seed=0, markers=None, range_starts=(), special=True, flat=False, mult=1):
    """q [B, lq, H, 128], k, v [B, lk, H, 128] float64 holding small integers (exact in bf16).  flat: q = 0, every key weighs 1 / lk
    (for cases with too few rows to point at every key).  mult: the last key will be counted `mult` times (a power of two); its
    row of k takes -log2(mult) back in every row but the falling ramps, so that it shares its rows with the other keys they point at
    instead of drowning them."""
    T = tiles(lk)
    assert T <= 47, "the tile code has 47 channels"
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros(B, lq, H, HEAD_DIM, dtype=torch.float64)
    k = torch.zeros(B, lk, H, HEAD_DIM, dtype=torch.float64)
    i, j = torch.arange(lq), torch.arange(lk)
    P = min(KV_TILE, lk)                            # positions a tile really has (a short context: fewer than 64)
    half = (P + 1) // 2
    k[:, j, :, j % 64] = 4.0
    k[:, j, :, 64 + (j // 64) % T] = 4.0
    ramp = torch.round(j.double() * RAMP_TOP / max(lk - 1, 1))
    for c in range(8):
        k[:, :, :, 112 + c] = (ramp // 8 + (c < ramp % 8).double())[None, :, None]
    for key in ((lk - 1,) if markers is None else markers):
        k[:, key, :, 120:124] = 8.0
    for key in range_starts:
        k[:, key, :, 124:128] = 8.0
    if mult != 1:
        assert 2 ** int(math.log2(mult)) == mult
        k[:, lk - 1, :, 111] = -math.log2(mult)
        q[..., 111] = 0.0 if flat else 1.0
    if not flat:
        for b in range(B):
            for h in range(H):
                bh = b * H + h
                a, t = (i + 3 * bh) % half, (i // 32 + bh) % T
                q[b, i, h, a] = 3.0
                q[b, i, h, (a + half) % P] = 3.0
                q[b, i, h, 64 + t] = 3.0
                q[b, i, h, 64 + (t + 1) % T] = 3.0
        if special:
            kind = row_kinds(lq)
            q[:, kind == 0, :, 112:120] = 1.0
            q[:, kind == 1] = 0.0                           # the falling ramp alone: the row maximum is the first key
            q[:, kind == 1, :, 112:120] = -1.0
            q[:, kind == 2, :, 120:124] = 1.0
            q[:, kind == 3, :, 124:128] = 1.0
    sign = torch.where(torch.rand(B, 1, H, HEAD_DIM, generator=g) < 0.5, -1.0, 1.0).double()
    v = torch.randint(1, 9, (B, lk, H, HEAD_DIM), generator=g).double() * sign
    return q, k, v


def scores(q, k, mult=1):
    """[B, H, Lq, Lk] float64 scores in exp2 units; a last key counted `mult` times carries + log2(mult)."""
    s = torch.einsum("blhd,bmhd->bhlm", q, k)
    if mult != 1:
        s[..., -1] += math.log2(mult)
    return s


def weights(q, k, mult=1):
    s = scores(q, k, mult)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return p / p.sum(-1, keepdim=True)


def reference(q, k, v):
    """Plain softmax-attention in float64 with the scores in exp2 units: [B, Lq, H, 128]."""
    return torch.einsum("bhlm,bmhd->blhd", weights(q, k), v)


def reference_lastkey(q, k, v, mult):
    """The same over a context that really holds `mult` copies of the last key."""
    B, _, H, D = k.shape
    more = (B, mult - 1, H, D)
    return reference(q, torch.cat([k, k[:, -1:].expand(more)], 1), torch.cat([v, v[:, -1:].expand(more)], 1))


def bf16_ulp(x):
    """Spacing of bf16 at |x| (8 significant bits)."""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def bf16_exact(x):
    return bool(torch.equal(x.to(torch.bfloat16).double(), x))


def sensitivity(q, k, v, mult=1, rows_per_key=4):
    """(least ulps any key moves its most affected output when DROPPED, the same when COUNTED TWICE, the keys where).  Per key the
    rows_per_key rows that weigh it most are examined (a lower bound of the maximum over all rows); every row is a compared row.
    The duplicated key of a lastkey case is exempt."""
    p_all = weights(q, k, mult)
    B, H, lq, lk = p_all.shape
    o_all = torch.einsum("bhlm,bmhd->bhld", p_all, v)
    n = lk - 1 if mult != 1 else lk
    worst = [math.inf, math.inf, None, None]
    for b in range(B):
        for h in range(H):
            pk = p_all[b, h, :, :n]
            r = min(rows_per_key, lq)                      # the rows where the key weighs most, and where it shares a row most evenly
            idx = torch.cat([pk.topk(r, dim=0).indices, (pk * (1 - pk)).topk(r, dim=0).indices])
            p = pk.gather(0, idx)                                                    # [2r, n]
            o = o_all[b, h][idx]                                                     # [r, n, 128]
            dv = (o - v[b, :n, h][None]).abs() / bf16_ulp(o)
            drop = (p / (1 - p).clamp_min(1e-300))[..., None] * dv
            twice = (p / (1 + p))[..., None] * dv
            for slot, moved in ((0, drop), (1, twice)):
                per_key = moved.amax((0, 2))
                m, at = per_key.min(0)
                if float(m) < worst[slot]:
                    worst[slot], worst[slot + 2] = float(m), (b, h, int(at))
    return tuple(worst)


def reference_moves(s):
    """How often the deferred-rescale reference of each row of s [.., Lk] moves: it starts at the maximum of the first 32-key half
    tile and is raised to a later half tile's maximum when that exceeds it by more than 2^RESCALE_THR."""
    ref = s[..., :32].amax(-1)
    n = torch.zeros_like(ref)
    for lo in range(32, s.shape[-1], 32):
        m = s[..., lo:lo + 32].amax(-1)
        up = m > ref + RESCALE_THR
        n += up
        ref = torch.where(up, m, ref)
    return n


# ----------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class Case:
    name: str
    instance: str                 # the kernel instance the case pins: "<KIND,PRE>", "FULL" or "SHORT" (checked against dispatch())
    lq: int
    lk: int
    B: int = 1
    H: int = 2
    prescaled: bool = False
    splits: tuple = None          # (kv_splits, split_from_unit); None: one pass over the keys
    env: tuple = ()               # ((name, value), ..) of the library's per-call switches
    mult: int = 1                 # > 1: attn_fwd_lastkey
    special: bool = True
    flat: bool = False
    sets: tuple = ()              # partial + merge: ((lo, hi, kv_splits), ..) in call order, a partition of the keys
    cu_budget: int = 0            # set_cu_budget for the call (SHORT: several units per workgroup)

    @property
    def scale(self):
        return None if self.prescaled else LN2

    def range_starts(self):
        if self.sets:
            return sorted({lo + s for lo, hi, n in self.sets for s in [0] + split_starts(hi - lo, n)} - {0})
        return split_starts(self.lk, self.splits[0]) if self.splits else []

    def markers(self):
        return tuple(hi - 1 for _, hi, _ in self.sets) if self.sets else (self.lk - 1,)

    def inputs(self):
        return build(self.lq, self.lk, self.B, self.H, seed=self.lq * 7 + self.lk, markers=self.markers(), range_starts=self.range_starts(),
                     special=self.special, flat=self.flat, mult=self.mult)

    def want(self, q, k, v):
        return reference_lastkey(q, k, v, self.mult) if self.mult != 1 else reference(q, k, v)


def dispatch(lk, prescaled, split, partial, mult, env):
    """The instance attn_run launches (csrc/attn.hip), restated."""
    env = dict(env)
    cross = lk <= 1024
    if cross and prescaled and tiles(lk) <= 4 and not split and not partial and env.get("FLEXAM_ATTN_SHORT") != "0":
        return "SHORT"
    if not cross and prescaled and lk >= KV_TILE and mult == 1 and env.get("FLEXAM_ATTN_FULL") != "0":
        return "FULL"
    return f"<{int(cross)},{'true' if prescaled else 'false'}>"


def _lq(lk):
    """Rows enough for two walks through every (position, tile) pair, and a ragged last q block."""
    return max(300, 64 * tiles(lk) + 44)


NO_FULL = (("FLEXAM_ATTN_FULL", "0"),)
NO_SHORT = (("FLEXAM_ATTN_SHORT", "0"),)
TWO_LAUNCHES = (("FLEXAM_ATTN_FUSED_TAIL", "0"),)
ONE_LAUNCH = (("FLEXAM_ATTN_FUSED_TAIL", "1"),)

GENERAL = (
    [Case(f"scale-lk{lk}", "<1,false>", _lq(lk), lk) for lk in (31, 32, 33, 63, 64, 65, 127, 256, 1024)]
    + [Case("scale-lk1", "<1,false>", 300, 1)]
    + [Case(f"scale-lk{lk}", "<0,false>", _lq(lk), lk, B=2, H=1) for lk in (1025, 1111)]
    + [Case("scale-lq1", "<1,false>", 1, 5, flat=True), Case("scale-lq31", "<1,false>", 31, 31, special=False)]
    + [Case(f"scale-lq{lq}", "<1,false>", lq, 100) for lq in (255, 256, 257, 300)]
)
PRE = (
    [Case(f"pre-lk{lk}", "<1,true>", _lq(lk), lk, prescaled=True) for lk in (257, 320, 1000, 1024)]
    + [Case(f"pre-nofull-lk{lk}", "<0,true>", _lq(lk), lk, prescaled=True, env=NO_FULL) for lk in (1025, 1111)]
)
# 3 heads x 8 q blocks on 8 workgroups: every workgroup walks 3 units, those of units 6-8 and 15-17 cross into the next head
SHORT = (
    [Case(f"short-lk{lk}", "SHORT", 2000, lk, H=3, prescaled=True, cu_budget=8) for lk in (1, 33, 64, 65, 128, 200, 256)]
    + [Case("short-lk200-all-cus", "SHORT", 2000, 200, H=3, prescaled=True)]
)
# 17, 17, 17, 18, 18, 18, 19, 20, 22 tiles: every tail length 1-4 of the main loop, window shifts 63, 1, 0 and mid values
FULL = [Case(f"full-lk{lk}", "FULL", _lq(lk), lk, B=1 + n % 2, H=2 - n % 2, prescaled=True)
        for n, lk in enumerate((1025, 1087, 1088, 1089, 1111, 1152, 1216, 1280, 1345))]
# 1345 keys = 22 tiles, the last one the shifted window of one new key: 22 x 1, 11 x 2, 7 x 3 + 1 (a last range that is only the shifted
# tile), 5 x 4 + 2, 4 x 5 + 2 tiles per range.  1111 keys = 18 tiles through the general instances: 18 x 1, 9 x 2, 6 x 3, 4 x 4 + 2, 3 x 5 + 3.
SPLIT = (
    [Case(f"split-full-{s}", "FULL", _lq(1345), 1345, prescaled=True, splits=(s, 0)) for s in (22, 11, 8, 6, 5)]
    + [Case(f"split-scale-{s}", "<0,false>", _lq(1111), 1111, splits=(s, 0)) for s in (18, 9, 6, 5, 4)]
    + [Case("split-pre-cross-3", "<1,true>", _lq(1000), 1000, prescaled=True, splits=(3, 0)),
       Case("split-pre-nofull-5", "<0,true>", _lq(1111), 1111, prescaled=True, splits=(5, 0), env=NO_FULL)]
    + [Case(f"split-full-8-from5-{e[0][1]}", "FULL", _lq(1345), 1345, prescaled=True, splits=(8, 5), env=e) for e in (TWO_LAUNCHES, ONE_LAUNCH)]
    + [Case(f"split-scale-4-from3-{e[0][1]}", "<0,false>", _lq(1111), 1111, splits=(4, 3), env=e) for e in (TWO_LAUNCHES, ONE_LAUNCH)]
)
# the sequence-parallel pattern: the local chunk [130, 420), the keys before it, the 1080 keys after it (> 1024: FULL as a partial call when
# q is pre-scaled) in 3 ranges; no bound on a tile edge
PARTIAL = [Case(f"partial-{'pre' if pre else 'scale'}", "FULL" if pre else "<0,false>", _lq(1500), 1500, prescaled=pre,
                sets=((130, 420, 1), (0, 130, 1), (420, 1500, 3))) for pre in (False, True)]
LASTKEY = [Case(f"lastkey-{name}-lk{lk}-x{mult}", inst, 300, lk, prescaled=pre, mult=mult, env=env)
           for name, inst, pre, env in (("scale", "<1,false>", False, ()), ("short", "SHORT", True, ()), ("pre", "<1,true>", True, NO_SHORT))
           for lk in (1, 32, 65, 100) for mult in (2, 512)]
# out= a row and column slice of a larger buffer; a ragged last q block
STRIDED = [Case("strided-full", "FULL", _lq(1111), 1111, prescaled=True),
           Case("strided-split-3", "<0,false>", _lq(1111), 1111, splits=(3, 0))]

ALL = GENERAL + PRE + SHORT + FULL + SPLIT + PARTIAL + LASTKEY + STRIDED


def ids(cases):
    return [c.name for c in cases]
