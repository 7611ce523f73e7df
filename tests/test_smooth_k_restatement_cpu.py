"""CPU: the claims FLEXAM_SAGE_SMOOTH_K rests on, checked on the restatements alone (tests/smooth_k_restatement.py): subtracting the token
mean of K changes nothing in exact attention, removes the price MXFP8 pays for a channel offset all keys share, and the admissible sets
the GPU test holds the shifted producer to leave it almost no choice."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp8_restatement as MX  # noqa: E402
import rmsnorm_rope_mx_restatement as R  # noqa: E402
import smooth_k_restatement as S  # noqa: E402


def test_exact_attention_does_not_see_the_shift():
    """softmax(q.(k - c)) = softmax(q.k): the walk with quant=False (exact softmax attention in float64) on k and on k - mean_tokens(k),
    all 300 rows of the offset case, and with a shift that is NOT the mean (any vector per batch and head is exact).
    Measured: 7e-16 and 2e-15 rel-RMS (float64 all the way); bound 1e-6."""
    q, k, v = S.offset_case()
    rows = list(range(q.shape[1]))
    exact = MX.attention(q, k, v, rows, quant=False)
    smooth = MX.attention(q.double(), k.double() - S.token_mean(k), v.double(), rows, quant=False)
    other = MX.attention(q.double(), k.double() - 3.0 * torch.randn(1, 1, 2, 128, generator=torch.Generator().manual_seed(1)).double(),
                         v.double(), rows, quant=False)
    print("exact attention, k - mean against k:", S.rel_rms(smooth, exact), "; k - c against k:", S.rel_rms(other, exact))
    assert S.rel_rms(smooth, exact) <= 1e-6 and S.rel_rms(other, exact) <= 1e-6


def test_the_offset_is_what_mxfp8_pays_for_and_the_mean_removes_it():
    """B = 1, H = 2, L = 300, an offset ~ N(0, 8^2) per (head, channel) in K, unit-variance logits (offset_case's defaults, seed 300):
    rel-RMS of the MXFP8 walk against exact attention is 2.13e-1 on K as it is and 5.43e-2 on K - mean_tokens(K) -- the format's own
    figure (FORMAT_BOUND = 6.5e-2, what tests/test_attn_fp8_gpu.py asks of offset-free data), 3.9 times less."""
    plain, smooth, _ = S.errors(*S.offset_case())
    print(f"MXFP8 against exact attention: plain {plain:.3e}, smooth {smooth:.3e}, ratio {plain / smooth:.2f}")
    assert smooth <= S.FORMAT_BOUND
    assert plain >= 2 * smooth


@pytest.mark.parametrize("name", S.SHIFTED_CASES)
def test_the_shifted_admissible_set_leaves_little_choice(name):
    """The inputs of the GPU test of flexam_rmsnorm_rope_mx_shift (shifted_case: an offset of twice the noise std in K, the token mean as
    the shift): ambiguous codes and scale bytes stay under AMBIGUOUS_CAP = 1e-3 of all, for q (Admissible) and for k (ShiftedAdmissible:
    one more rounding, u |y - shift|, see the restatement's docstring).  Measured: k codes 3.7e-4 .. 4.0e-4, k scale bytes <= 5.2e-5, q
    codes 1.0e-4 .. 1.2e-4; at four times the noise std 6.2e-4 .. 6.8e-4, at eight times past the cap.  The shift does remove the
    offset: the mean of y - shift over the tokens is zero to float32's rounding of the shift."""
    c = S.shifted_case(name)
    aq, ak = S.shifted_admissible(name)
    print(f"{name}: ambiguous codes q {aq.ambiguous_codes:.3g} k {ak.ambiguous_codes:.3g}, scale bytes q {aq.ambiguous_scales:.3g} k {ak.ambiguous_scales:.3g}")
    for a in (aq, ak):
        assert a.ambiguous_codes <= R.AMBIGUOUS_CAP and a.ambiguous_scales <= R.AMBIGUOUS_CAP
    resid = ak.y.reshape(c.B, c.L, R.C).mean(dim=1).abs()
    assert float((resid - S.U * c.shift.double().abs()).max()) <= 1e-12
    # the offset is there before the shift: the unrotated half of the channels keeps a mean of the size of the rows themselves
    y, _ = R.reference(c.qkv[:, R.C:2 * R.C], c.wk, c.cos, c.sin, c.L, c.offset, c.eps)
    assert float(c.shift.abs().mean()) > 0.1 * float(y.abs().mean())


def test_k_mean_bound_counts_what_the_docstring_counts():
    assert S.k_mean_bound(1.0, 16, 70, True) == R.DELTA + 88 * S.U
    assert S.k_mean_bound(2.0, 1111, 1, False) == 2 * 1114 * S.U
