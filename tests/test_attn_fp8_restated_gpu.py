"""The MXFP8 self-attention kernel (csrc/attn_fp8.inc) against its float64 restatement (tests/mxfp8_restatement.py): the same operand
quantisation, online-softmax walk, P rounding, split plan and merge, so what is left between the two is the kernel's implementation.

(a) Integer cases: small integer Q, K (|x| <= 15) and V (1..8, one sign per channel) pack losslessly, every score is an integer and
    every p a power of two.  The only rounding left is fp32 accumulation of sums without cancellation (O, l) and the output's bf16
    rounding, so every element must lie within 1 bf16 ulp of the restatement.  The rows move the reference several times within
    a tile and across tiles and reach the rd = 96 cap (a key ramp), put the row maximum on the last real key of a ragged tail tile
    and on the first key of a split range (marker keys), and hold keys 9, 10 and 11 binades below the reference (the noise
    channels), which e4m3 keeps, ties to zero and flushes while l still counts them.  Two key ranges hold fewer than 32 keys in
    their only tile (L = 20; L = 1040 with kv_splits = 5), with every real score 16 or more binades below 0.
(b) Random cases (unit-variance logits, sharpness 1 and 3): what is left is fp32 accumulation order of the scores, v_exp_f32
    against exact exp2, and the e4m3 flip where p lies within that rounding of a midpoint between two codes (one such flip moves an
    output by about 2^-3 p v / l, i.e. by 1/L of a row at short L).  Both sides are compared after rounding to bf16: 1-2 % of the
    elements differ by more than one bf16 ulp.  Bound: rel-RMS <= 3.2e-3 (measured 2.3e-4 .. 2.6e-3), 20 times below the
    format's 6.5e-2 against fp32 attention (tests/test_attn_fp8_gpu.py), where the same cases measure 4.9e-2 .. 8.8e-2."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp8_restatement as R  # noqa: E402
from test_attn_fp8_gpu import _inputs, _ref  # noqa: E402

pytestmark = pytest.mark.gpu
REL_RMS = 3.2e-3            # 20x below the format's 6.5e-2; measured 2.3e-4 .. 2.6e-3 (largest at L = 40: one flipped p is 1/L of a row)


@pytest.fixture(scope="module")
def H():
    from flexam_amd import hip
    hip.load_library()
    return hip


def _bf16_ulp(x):
    a = x.abs().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 7)


def _rows(L, seed, n=48):
    """All rows of a short sequence; else the first and last rows of q blocks and tiles and a random sample."""
    if L <= 320:
        return list(range(L))
    g = torch.Generator().manual_seed(seed)
    fixed = {0, 1, 31, 32, 63, 64, 255, 256, L - 65, L - 64, L - 2, L - 1}
    return sorted(fixed | set(torch.randint(0, L, (n,), generator=g).tolist()))


# ----------------------------------------------------------------------------- (a) integer scores
def _integer_case(B, Hh, L, seed, marker_keys=(), range_starts=(), deep=False, ramp_top=120):
    """q, k, v [B, L, H, 128] bf16 holding small integers.  Channels 0-7: a key ramp 0 .. ramp_top seen by every third row; 8-15: +64 on the
    last real key for rows = 1 mod 3; 16-23: +64 on the first key of every split range for rows = 2 mod 3; 24-31: -40 on every key for
    the deep rows (all of them with deep=True); 32-127: noise (q in {-1, 0, 1} half of the time nonzero, k in {-1, 0, 1}: sd 5.7)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros(B, L, Hh, 128)
    k = torch.zeros(B, L, Hh, 128)
    r = torch.arange(L)
    ramp = torch.round(torch.arange(L) * float(ramp_top) / max(L - 1, 1))
    for c in range(8):
        k[:, :, :, c] = (ramp // 8 + (c < ramp % 8).float())[None, :, None]
    kind = r % 3
    if deep:
        q[:, :, :, 24:32] = -1.0
        k[:, :, :, 24:32] = 5.0
        qn = torch.randint(-1, 2, (B, L, Hh, 16), generator=g).float()
        q[..., 32:48] = qn
    else:
        q[:, kind == 0, :, 0:8] = 1.0
        q[:, kind == 1, :, 8:16] = 1.0
        q[:, kind == 2, :, 16:24] = 1.0
        for key in marker_keys:
            k[:, key, :, 8:16] = 8.0
        for key in range_starts:
            k[:, key, :, 16:24] = 8.0
        qn = torch.randint(-1, 2, (B, L, Hh, 96), generator=g).float() * (torch.rand(B, L, Hh, 96, generator=g) < 0.5)
        q[..., 32:] = qn
    k[..., 32:] = torch.randint(-1, 2, (B, L, Hh, 96), generator=g).float()
    sign = torch.where(torch.rand(Hh, 128, generator=g) < 0.5, -1.0, 1.0)
    v = torch.randint(1, 9, (B, L, Hh, 128), generator=g).float() * sign
    return [t.to(torch.bfloat16).cuda() for t in (q, k, v)]


INTEGER_CASES = [
    # name, B, H, L, (kv_splits, split_from_unit) or None (the default plan), deep
    ("ragged-tail", 1, 2, 1111, (1, 0), False),          # one range: the ramp rows reach the cap
    ("split-2", 1, 2, 1111, (2, 0), False),
    ("split-4-fused-tail", 1, 2, 1111, (4, 5), False),
    ("steep-ramp", 2, 1, 96, (1, 0), False),
    ("short-range-L20", 1, 2, 20, None, True),
    ("short-last-range", 1, 2, 1040, (5, 0), True),
]


@pytest.mark.parametrize("name,B,Hh,L,splits,deep", INTEGER_CASES, ids=[c[0] for c in INTEGER_CASES])
def test_integer_scores_within_one_bf16_ulp_of_the_restatement(H, name, B, Hh, L, splits, deep):
    S, from_unit = splits if splits is not None else H.attn_split_plan(B * Hh, L, L, H.num_cus())
    starts = [lo for lo, _ in R.split_ranges(L, S)][1:] if S > 1 else []
    q, k, v = _integer_case(B, Hh, L, L + S, marker_keys=(L - 1,), range_starts=starts, deep=deep)
    kw = {} if splits is None else dict(kv_splits=splits[0], split_from_unit=splits[1])
    o = H.attn_fwd_fp8(H.attn_fp8_pack(q, k, v), L, **kw).double().cpu()
    rows = _rows(L, L)
    want = R.attention(q, k, v, rows, kv_splits=S, split_from_unit=from_unit if S > 1 else None)
    got = o[:, rows]
    if deep:                                                   # the case's premise: every real score 16 or more binades below 0
        s = torch.einsum("blhd,bmhd->bhlm", q.double().cpu(), k.double().cpu())
        assert float(s.max()) <= -16.0
    err = (got - want).abs()
    bad = err > _bf16_ulp(want)
    print(name, "max |err| / ulp", float((err / _bf16_ulp(want)).max()), "elements off by more than 1 ulp:", int(bad.sum()))
    assert torch.isfinite(got).all()
    assert not bad.any(), (f"{int(bad.sum())} elements more than 1 bf16 ulp from the restatement; first at "
                           f"{bad.nonzero()[0].tolist()}: got {float(got[bad][0])}, want {float(want[bad][0])}")


# ----------------------------------------------------------------------------- (b) random data
RANDOM_CASES = [
    # B, H, L, splits (None: the default plan), sharp, env
    (1, 1, 40, None, 1.0, None),
    (1, 1, 64, None, 3.0, None),
    (1, 1, 65, None, 1.0, None),
    (1, 2, 96, None, 3.0, None),
    (1, 1, 300, None, 1.0, None),
    (2, 3, 1111, None, 3.0, None),
    (1, 2, 1111, (2, 0), 1.0, None),
    (1, 2, 1111, (4, 5), 3.0, None),
    (1, 2, 1111, (4, 5), 1.0, "0"),               # FLEXAM_ATTN_FUSED_TAIL=0: whole units and split units in two launches
    (1, 1, 2912, None, 3.0, None),
    (2, 11, 2912, None, 1.0, None),               # 264 units on 256 CUs: the default plan splits the last round
]


@pytest.mark.parametrize("B,Hh,L,splits,sharp,fused", RANDOM_CASES)
def test_random_data_against_the_restatement(H, B, Hh, L, splits, sharp, fused, monkeypatch):
    if fused is not None:
        monkeypatch.setenv("FLEXAM_ATTN_FUSED_TAIL", fused)
    q, k, v = _inputs(B, Hh, L, 100 + L, sharp=sharp)
    if splits is None:
        S, from_unit = H.attn_split_plan(B * Hh, L, L, H.num_cus())
        if B * Hh == 22:
            assert S > 1 and 0 < from_unit < B * Hh * ((L + 255) // 256)
        kw = {}
    else:
        S, from_unit = splits
        kw = dict(kv_splits=S, split_from_unit=from_unit)
    o = H.attn_fwd_fp8(H.attn_fp8_pack(q, k, v), L, **kw).float().cpu()
    rows = _rows(L, L)
    want = R.attention(q, k, v, rows, kv_splits=S, split_from_unit=from_unit if S > 1 else None).float().to(torch.bfloat16).float()
    got = o[:, rows]
    rel = float((got - want).norm() / want.norm())
    off = float(((got - want).abs() > _bf16_ulp(want.double()).float()).float().mean())
    fp32 = _ref(q, k, v).cpu()[:, rows]
    rel32 = float((got - fp32).norm() / fp32.norm())
    print(f"B={B} H={Hh} L={L} splits={(S, from_unit)} sharp={sharp} fused_tail={fused}: rel-RMS vs restatement {rel:.2e} "
          f"(elements > 1 ulp apart: {off:.1e}); vs fp32 attention {rel32:.2e}")
    assert torch.isfinite(got).all() and rel <= REL_RMS


def test_chunked_records_with_fewer_queries_than_keys(H):
    """attn_fwd_fp8_chunked at the bench's rank-of-four shape: 24 heads, 11648 keys in 4 chunks of 46 tiles (the last one padded), the
    2944 queries of one rank (Lq != Lk); the default plan splits the units of the last round."""
    B, Hh, chunk, n_chunks, lk = 1, 24, 2944, 4, 11648
    q, k, v = _inputs(B, Hh, chunk * n_chunks, 5)
    for t in (q, k, v):
        t[:, lk:] = 0
    per = [H.attn_fp8_pack(*(t[:, c * chunk:(c + 1) * chunk].contiguous() for t in (q, k, v))) for c in range(n_chunks)]
    kv8 = torch.stack([p[2] for p in per]).contiguous()
    c = 1
    got = H.attn_fwd_fp8_chunked(per[c][0], per[c][1], kv8, chunk, lk).float().cpu()
    S, from_unit = H.attn_split_plan(B * Hh, chunk, lk, H.num_cus())
    assert S > 1
    rows = [0, 255, 256, 1000, 2047, 2943]
    ql = q[:, c * chunk:(c + 1) * chunk]
    want = R.attention(ql, k[:, :lk], v[:, :lk], rows, kv_splits=S, split_from_unit=from_unit).float().to(torch.bfloat16).float()
    got = got[:, rows]
    rel = float((got - want).norm() / want.norm())
    fp32 = _ref(ql[:, rows], k[:, :lk], v[:, :lk]).cpu()
    rel32 = float((got - fp32).norm() / fp32.norm())
    print(f"chunked, Lq {chunk} Lk {lk}, plan {(S, from_unit)}: rel-RMS vs restatement {rel:.2e}; vs fp32 attention {rel32:.2e}")
    assert torch.isfinite(got).all() and rel <= REL_RMS
