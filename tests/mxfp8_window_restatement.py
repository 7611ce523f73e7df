"""The windowed walk of the MXFP8 self-attention (attn8_window_kernel of csrc/attn_fp8.inc, flexam_attn_fwd_fp8_window) restated in
float64 on top of tests/mxfp8_restatement.py: the same operand quantisation, reference rule, P rounding and units of O, under a boolean
mask allowed[L, L] (row i sees key j).  Not a test module.  The masks come from the `allowed` helpers of tests/attn_window_cases.py,
tests/attn_window_sink_cases.py and tests/attn_window_frames_cases.py (`mask` below); nothing of the kernel's tile plan is in here.

  walk    per query row over ALL 32-key half tiles in ascending order, one key range (whole work units); a score the row does not see
          is masked; a half tile in which the row sees no key contributes nothing to it and sets nothing;
  start   the row's first reference is floor(max of the scores it sees in the first half tile that has one) - 6, with rd = 0 there;
  then    the rules of R.range_pass over the visible scores only: a half tile whose visible maximum exceeds ref + 8.5 moves the
          reference by floor(max - ref - 6), capped so that rd <= 96 COUNTED FROM THE ROW'S OWN START, and clamps its scores to
          ref + 8.5; l is multiplied by 2^-delta on a move; p = exp2(s - ref) as a float32 value, exactly 0 for an invisible score
          (which is in no row sum); l adds the unrounded p, O adds e4m3(p) 2^rd v;
  output  O 2^-rd / l in float64 (the caller rounds it to bf16).
With quant=False the operands are taken as given and P is not rounded: the walk is then exact masked softmax attention."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_cases as W  # noqa: E402
import attn_window_frames_cases as F  # noqa: E402
import attn_window_sink_cases as S  # noqa: E402
import mxfp8_restatement as R  # noqa: E402


def mask(L, window, sink=0, frame_tokens=0):
    """allowed[L, L] of a token window (frame_tokens = 0) or a frame window, with a sink: the case modules' rules."""
    if frame_tokens > 0:
        return F.allowed(L, window, frame_tokens, sink)
    return S.allowed(L, window, sink) if sink else W.allowed(L, window)


def window_pass(s, v, ok, quant=True, trace=None):
    """s [R, L] float64 scores (exp2 units) of R query rows, v [L, 128] float64, ok [R, L] bool -> the rows' outputs [R, 128].
    trace: a dict that receives the rows' final rd and the first key of the half tile each row started in."""
    n, L = s.shape
    o = torch.zeros(n, v.shape[1], dtype=torch.float64)
    l = torch.zeros(n, dtype=torch.float64)
    rd = torch.zeros(n, dtype=torch.float64)
    ref = torch.zeros(n, dtype=torch.float64)
    started = torch.zeros(n, dtype=torch.bool)
    start_key = torch.zeros(n, dtype=torch.long)
    for a in range(0, L, R.HALF):
        b = min(a + R.HALF, L)
        vis = ok[:, a:b]
        live = vis.any(dim=1)
        if not bool(live.any()):
            continue
        sc = s[:, a:b].masked_fill(~vis, -math.inf)
        mx = sc.amax(dim=1)                                        # -inf for a row that sees nothing here
        first = live & ~started
        ref = torch.where(first, torch.floor(mx) - R.REF_HEAD, ref)
        move = started & live & (mx - ref > R.RESCALE_THR)
        delta = torch.where(move, torch.minimum(torch.floor(mx - ref - R.REF_HEAD), R.RD_MAX - rd), torch.zeros_like(rd))
        ref, rd = ref + delta, rd + delta
        l = l * torch.pow(2.0, -delta)
        sc = torch.where(move[:, None], torch.minimum(sc, (ref + R.RESCALE_THR)[:, None]), sc)
        start_key = torch.where(first, torch.full_like(start_key, a), start_key)
        started = started | live
        p = torch.where(vis, torch.pow(2.0, sc - ref[:, None]), torch.zeros_like(sc))
        if quant:
            p = p.float().double()
            pq = R.e4m3(p)
        else:
            pq = p
        l = l + p.sum(dim=1)
        o = o + (pq * torch.pow(2.0, rd)[:, None]) @ v[a:b]
    assert bool(started.all()), "a row that sees no key"
    if trace is not None:
        trace.update(rd=rd, start_key=start_key)
    return o * torch.pow(2.0, -rd)[:, None] / l[:, None]


def attention(q, k, v, ok, quant=True):
    """q, k, v [B, L, H, 128] (bf16 as handed to the pack, q in exp2 units) under allowed[L, L] -> float64 [B, L, H, 128], every row."""
    B, L, H, D = q.shape
    if quant:
        qd, kd, vd = R.dequant_rows(q), R.dequant_rows(k), R.dequant_v(v)
    else:
        qd, kd, vd = (t.double().cpu().permute(0, 2, 1, 3) for t in (q, k, v))
    out = torch.empty(B, L, H, D, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            out[b, :, h] = window_pass(qd[b, h] @ kd[b, h].t(), vd[b, h], ok, quant)
    return out


def masked_softmax(q, k, v, ok):
    """Exact masked softmax attention in float64, scores in exp2 units: [B, L, H, 128]."""
    qd, kd, vd = (t.double().cpu() for t in (q, k, v))
    s = torch.einsum("blhd,bmhd->bhlm", qd, kd).masked_fill(~ok, -math.inf)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return torch.einsum("bhlm,bmhd->blhd", p / p.sum(-1, keepdim=True), vd)


# ----------------------------------------------------------------------------- integer operands for the windowed kernel
def row_ranges(L, window, frame_tokens=0):
    """(lo, hi) [L] each: the first and the last key of every row's WINDOW (the sink aside), clipped to [0, L)."""
    ok = mask(L, window, 0, frame_tokens)
    j = torch.arange(L)
    lo = torch.where(ok, j[None, :], torch.full((L, L), L)).amin(dim=1)
    hi = torch.where(ok, j[None, :], torch.full((L, L), -1)).amax(dim=1)
    return lo, hi


def integer_case(B, H, L, window, seed, frame_tokens=0):
    """q, k, v [B, L, H, 128] float32 holding small integers (|x| <= 15: they pack losslessly, as _integer_case's of
    tests/test_attn_fp8_restated_gpu.py do), every score an integer in exp2 units, V in 1 .. 8 with one sign per channel.
      channels 0-7    a key ramp j % 120 (in eighths over the channels); rows = 0 mod 3 carry 2 there: their scores climb by 2 per key, so
                      a row that starts late in its unit -- its window's first key lies tiles behind the unit's first -- climbs more than
                      96 + 8.5 above its OWN first reference inside a window of 60 keys or more, and its reference stops at the cap
      channels 8-71   key j carries 4 in channel 8 + j % 64; rows = 1 mod 3 (which carry nothing else) have 1 in the channel of their
                      window's first key lo (score 4), 2 in that of its last key hi (score 8), 10 in the channel of hi + 1, the first key they do not see to the right (score 40),
                      and 10 in that of lo - 1 likewise (later assignments replace earlier ones where two of the three channels
                      coincide), every other score being 0.  Under a window narrower than 64 keys the row's maximum then sits on its
                      last visible key, and a mask one key too wide lets a weight of 2^32 times that maximum in; under a wider one the
                      keys 64 apart from the two outside ones are visible at score 40 as well, and a mask off by one adds or drops a
                      key of the row's largest weight
      channels 72-127 noise for the other rows: q in {-1, 0, 1}, half of them nonzero, k in {-1, 0, 1}."""
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros(B, L, H, 128)
    k = torch.zeros(B, L, H, 128)
    j = torch.arange(L)
    ramp = (j % 120).float()
    for c in range(8):
        k[:, :, :, c] = (ramp // 8 + (c < ramp % 8).float())[None, :, None]
    k[:, j, :, 8 + j % 64] = 4.0
    kind = j % 3
    q[:, kind == 0, :, 0:8] = 2.0
    lo, hi = row_ranges(L, window, frame_tokens)
    edge = j[kind == 1]
    q[:, edge, :, 8 + lo[edge] % 64] = 1.0
    q[:, edge, :, 8 + hi[edge] % 64] = 2.0
    right = edge[hi[edge] + 1 < L]
    q[:, right, :, 8 + (hi[right] + 1) % 64] = 10.0
    left = edge[lo[edge] > 0]
    q[:, left, :, 8 + (lo[left] - 1) % 64] = 10.0
    q[..., 72:] = torch.randint(-1, 2, (B, L, H, 56), generator=g).float() * (torch.rand(B, L, H, 56, generator=g) < 0.5)
    q[:, edge, :, 72:] = 0.0
    k[..., 72:] = torch.randint(-1, 2, (B, L, H, 56), generator=g).float()
    sign = torch.where(torch.rand(H, 128, generator=g) < 0.5, -1.0, 1.0)
    v = torch.randint(1, 9, (B, L, H, 128), generator=g).float() * sign
    return q, k, v


def bf16_ulp(x):
    return torch.pow(2.0, torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)
