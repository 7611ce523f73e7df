"""CPU: the restatement of the MXFP8 attention and of e4m3 rounding (tests/mxfp8_restatement.py) that the GPU tests hold the kernels to --
checked here against float64 softmax attention (quantisation off), against torch's float8_e4m3fn cast at every code, midpoint and
across the subnormal range, and for the documented moves of the row reference on a hand-built row."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp8_restatement as R  # noqa: E402


def _torch_code(x):
    return x.float().to(torch.float8_e4m3fn).view(torch.uint8)


def test_e4m3_codes_and_values_round_trip():
    t = R.e4m3_table()
    assert t[0] == 0 and t[1] == 2.0 ** -9 and t[8] == 2.0 ** -6 and t[126] == 448.0
    assert bool((t[1:] > t[:-1]).all())
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    finite = (codes & 127) != 127
    want = codes.view(torch.float8_e4m3fn).double()
    assert torch.equal(R.e4m3_value(codes)[finite], want[finite])
    assert torch.isnan(R.e4m3_value(codes)[~finite]).all()


def test_e4m3_rounding_equals_torchs_cast_at_codes_midpoints_and_subnormals():
    t = R.e4m3_table()
    mids = (t[1:] + t[:-1]) / 2                                   # every tie: exactly representable in float32
    eps = torch.tensor([0.0, 1e-7, -1e-7, 1e-3, -1e-3], dtype=torch.float64)
    x = torch.cat([t, mids, (mids[:, None] * (1 + eps)).flatten(), (t[:, None] * (1 + eps)).flatten(),
                   torch.tensor([455.0, 463.9, 464.0])])
    sub = torch.linspace(2.0 ** -10, 2.0 ** -6, 4097, dtype=torch.float64)                # the subnormal range, fine steps
    x = torch.cat([x, sub, 2.0 ** -10 * torch.tensor([0.5, 0.999, 1.0, 1.001, 1.5, 2.5, 3.5])]).float()
    x = torch.cat([x, -x])
    got, want = R.e4m3_code(x), _torch_code(x)
    assert torch.equal(got, want), x[got != want][:8]
    # ties go to the even code: the tie between codes 2c and 2c + 1 stays at 2c, between 2c + 1 and 2c + 2 goes up
    c = R.e4m3_code(mids.float())
    assert torch.equal(c.long(), 2 * ((torch.arange(126) + 1) // 2))
    r = torch.Generator().manual_seed(0)
    y = (torch.randn(100000, generator=r) * torch.pow(2.0, torch.randint(-14, 8, (100000,), generator=r).float()))
    assert torch.equal(R.e4m3_code(y), _torch_code(y))


def test_restatement_without_quantisation_is_softmax_attention():
    g = torch.Generator().manual_seed(4)
    B, H, L = 1, 2, 300
    q = torch.randn(B, L, H, 128, generator=g, dtype=torch.float64) * 0.4
    k = torch.randn(B, L, H, 128, generator=g, dtype=torch.float64)
    v = torch.randn(B, L, H, 128, generator=g, dtype=torch.float64)
    rows = [0, 1, 63, 64, 150, 255, 256, 299]
    s = torch.einsum("blhd,bmhd->bhlm", q, k) * math.log(2.0)
    want = torch.einsum("bhlm,bmhd->blhd", torch.softmax(s, dim=-1), v)[:, rows]
    got = R.attention(q, k, v, rows, quant=False)
    assert float((got - want).abs().max()) <= 1e-12
    # split ranges merged as the merge kernel does: the same numbers
    got3 = R.attention(q, k, v, rows, kv_splits=3, quant=False)
    assert float((got3 - want).abs().max()) <= 1e-12
    # a key range whose first half tile is mostly padding: the reference comes from the valid keys alone
    got1 = R.attention(q[:, :20] - 30.0, k[:, :20], v[:, :20], [0, 5, 19], quant=False)
    s1 = torch.einsum("blhd,bmhd->bhlm", q[:, :20] - 30.0, k[:, :20]) * math.log(2.0)
    want1 = torch.einsum("bhlm,bmhd->blhd", torch.softmax(s1, dim=-1), v[:, :20])[:, [0, 5, 19]]
    assert float((got1 - want1).abs().max()) <= 1e-12


def test_reference_moves_at_the_documented_scores_and_saturates():
    """One row, hand-built scores: half tile 0 max 3.4 -> ref0 = 3 - 6 = -3; half tile 1 max 5.5 (= ref + 8.5: no move); half tile 2 max
    5.6 (> ref + 8.5: delta = floor(5.6 + 3 - 6) = 2, ref = -1); half tile 3 max 200 (delta capped at 96 - 2 = 94: ref 93, scores
    clamped to 101.5)."""
    lk = 128
    s = torch.full((1, lk), -50.0, dtype=torch.float64)
    s[0, 5], s[0, 40], s[0, 70], s[0, 127] = 3.4, 5.5, 5.6, 200.0
    v = torch.zeros(lk, 128, dtype=torch.float64)
    v[:, 0] = 1.0
    v[127, 1] = 1.0
    _, ref, l = R.range_pass(s, v, 0, lk, lk, quant=False)
    assert float(ref[0]) == 93.0
    # walk the same row by hand
    ref_h = -3.0
    lh = 2.0 ** (3.4 - ref_h) + 2.0 ** (5.5 - ref_h) + 30 * 2.0 ** (-50 - ref_h) + 31 * 2.0 ** (-50 - ref_h)
    ref_h += 2
    lh = lh * 2.0 ** -2 + 2.0 ** (5.6 - ref_h) + 31 * 2.0 ** (-50 - ref_h)
    ref_h += 94
    lh = lh * 2.0 ** -94 + 2.0 ** (101.5 - ref_h) + 31 * 2.0 ** (-50 - ref_h)
    assert abs(float(l[0]) - lh) <= 1e-12 * lh
    for lo_ref, thr in ((-3.0, 5.5), (-3.0, 5.5 + 1e-9)):
        s2 = torch.full((1, 64), -20.0, dtype=torch.float64)
        s2[0, 0], s2[0, 40] = 3.0, thr
        _, r2, _ = R.range_pass(s2, v[:64], 0, 64, 64, quant=False)
        assert float(r2[0]) == (lo_ref if thr == 5.5 else lo_ref + 2.0)
    # at the cap: O stays in the units of ref0, the output weighs key 127 with 2^(101.5 - 93) against the rest
    out = R.attend_rows(s, v, lk, [(0, lk)], quant=False)
    assert abs(float(out[0, 0]) - 1.0) <= 1e-12
    assert abs(float(out[0, 1]) - 2.0 ** 8.5 / (l[0] * 1.0)) <= 1e-12


def test_split_ranges_follow_the_launch_plan():
    assert R.split_ranges(1040, 5) == [(0, 256), (256, 512), (512, 768), (768, 1024), (1024, 1088)]
    assert R.split_ranges(1024, 4) == [(0, 256), (256, 512), (512, 768), (768, 1024)]
    assert R.split_ranges(300, 4) == [(0, 128), (128, 256), (256, 320)]          # ceil(5 / 4) = 2 tiles per range: 3 ranges
