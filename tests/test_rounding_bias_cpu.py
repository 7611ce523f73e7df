"""CPU: the lean check of tests/rounding_bias.py is not blind, and does not cry wolf.

Attention (with a DEFERRED reference: the maximum of the first 32 keys is subtracted, not the row maximum, so P is not bounded by 1 and
its rounding is that of a general value), a LayerNorm-modulate, a GEMM with and without tanh-GELU and a softmax are restated in float64
on the data sets the GPU tests use, with the bf16 conversions written as bit operations: round-to-nearest-even, and truncation.
  * Round-to-nearest-even everywhere passes assert_no_lean for 8 seeds.
  * A truncated P, a truncated output, an output truncated in one column of every 16 and in one row of every 64 (attention and GEMM)
    each fail it, with a mean of -0.35 ulp or lower in the affected class.
  * The exclusion rule drops at most 1 % of every data set it is applied to.

Measured here (8 seeds, round-to-nearest-even; Lk = 200): attention overall mean within +-0.003 at flat logits and +-0.013 at peaked
ones, column classes within +-0.009 / +-0.018; row classes within +-0.027 at flat logits, up to 0.13 at peaked logits (not asserted
there, see tests/rounding_bias.py).  LayerNorm overall within +-0.012, column classes +-0.019 (plain; inputs on the bf16 grid repeat
values within a row), +-0.007 modulated; GEMM and GELU column classes within +-0.010, row classes +-0.023; softmax +-0.008 / +-0.016.
Defects: P truncated -0.44 overall (flat and peaked); output truncated -0.50 / -0.51; one column or row class truncated -0.49 ..
-0.52 in that class, the overall mean then only -0.01 .. -0.04.  Excluded: 0.28 .. 0.41 % of the LayerNorm, RMSNorm + RoPE,
GroupNorm and GEMM data sets."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rounding_bias as RB  # noqa: E402
import test_dit_row_kernels_gpu as DR  # noqa: E402
from gemm_checks import _gelu64  # noqa: E402
from test_text_encoder_kernels_gpu import softmax_ref  # noqa: E402

F32, F64 = torch.float32, torch.float64
SEEDS = range(8)
HIGH16 = -65536                                  # 0xFFFF0000 as an int32
DEFECT = -0.35
COL, ROW = 5, 37                                 # the column class (of 16) and the row class (of 64) the partial defects hit
ATTN_LK = 200


# ----------------------------------------------------------------------------- conversions, as bit operations
def rne(x):
    """float64 -> the bf16 nearest (ties to even), as float64."""
    b = x.to(F32).view(torch.int32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) & HIGH16).view(F32).double()


def chop(x):
    """float64 -> the bf16 next towards zero: the low 16 bits dropped."""
    return (x.to(F32).view(torch.int32) & HIGH16).view(F32).double()


def chop_cols(x):
    out = rne(x)
    out[..., COL::16] = chop(x)[..., COL::16]
    return out


def chop_rows(x):
    out = rne(x)
    out[..., ROW::64, :] = chop(x)[..., ROW::64, :]
    return out


def test_the_conversions_are_bf16():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1 << 16, generator=g, dtype=F64) * torch.exp2(torch.randint(-20, 20, (1 << 16,), generator=g).double())
    x[:4] = torch.tensor([1.00390625, 1.01171875, -1.00390625, -1.01171875], dtype=F64)        # ties: to 1.0 (even), to 1.015625
    assert torch.equal(rne(x), x.float().to(torch.bfloat16).double())
    assert rne(x)[:4].tolist() == [1.0, 1.015625, -1.0, -1.015625]
    c = chop(x)
    assert bool((c.abs() <= x.float().double().abs()).all()) and bool(((c - x.float().double()).abs() < RB.bf16_ulp(x)).all())
    assert torch.equal(rne(c), c)


# ----------------------------------------------------------------------------- the restatements
def attention(q, k, v, prescaled, cvt_p=rne, cvt_o=rne):
    """Online-softmax attention as the kernel holds it, without its walk: p = exp2(s - ref) against a reference that is NOT the row
    maximum, P converted to bf16 for the PV product, the row sum l taken from the unrounded p, the output converted once."""
    s = RB.attn_scores(q, k, prescaled)
    p = torch.exp2(s - s[..., :32].amax(-1, keepdim=True))
    o = torch.einsum("bhlm,bmhd->bhld", cvt_p(p), v.double()) / p.sum(-1, keepdim=True)
    return cvt_o(o)                                                                  # [B, H, Lq, 128]: the q row second to last


@pytest.fixture(scope="module")
def attn():
    """(q, k, v, want [B, H, Lq, 128]) per (sharpness, seed), once."""
    out = {}
    for sharp in RB.SHARP:
        for seed in SEEDS:
            q, k, v = RB.attn_data(seed, RB.ATTN_LQ, ATTN_LK, sharp, True)
            out[sharp, seed] = (q, k, v, RB.attn_rows_last(RB.attn_reference(q, k, v, True)))
    return out


@pytest.fixture(scope="module")
def gemm():
    a, w, b = RB.gemm_data(0)
    y = RB.gemm_reference(a, w, b)
    return y, RB.keep_mask(y)


def ln_want(seed, modulated):
    x, tab, rows = RB.ln_data(seed)
    r = rows.long()
    return DR.ln_ref(x, 1e-6, **(dict(sh=tab[r, 0], sc=tab[r, 1]) if modulated else {}))[0]


def softmax_want(seed):
    s, b = RB.softmax_bias_data(seed)
    return softmax_ref(s, 0.125, b, None)


# ----------------------------------------------------------------------------- round-to-nearest-even passes
@pytest.mark.parametrize("sharp", list(RB.SHARP))
def test_rne_attention_does_not_lean(attn, sharp):
    """8 seeds; the row classes are asserted at flat logits only (tests/rounding_bias.py says why)."""
    for seed in SEEDS:
        q, k, v, want = attn[sharp, seed]
        got = attention(q, k, v, True)
        RB.assert_no_lean(got, want, rows=sharp == "flat", what=f"attention {sharp} seed {seed}", row_floor=RB.SMALL_ROW_FLOOR)
        r = RB.lean(got, want, rows=True)
        print(f"   row classes ({sharp}): worst {r.worst_row():+.4f}")


def test_rne_scale_in_kernel_form_does_not_lean():
    q, k, v = RB.attn_data(11, RB.ATTN_LQ, ATTN_LK, "peaked", False)
    RB.assert_no_lean(attention(q, k, v, False), RB.attn_rows_last(RB.attn_reference(q, k, v, False)), what="attention, exp(scale q.k)")


def test_rne_row_kernels_and_gemm_do_not_lean():
    for seed in SEEDS:
        for modulated in (False, True):
            want = ln_want(seed, modulated)
            keep = RB.keep_mask(want)
            RB.assert_cap(keep, "ln_modulate")
            RB.assert_no_lean(rne(want), want, keep, what=f"ln_modulate modulated={modulated} seed {seed}")
        y = RB.gemm_reference(*RB.gemm_data(seed))
        keep = RB.keep_mask(y)
        RB.assert_cap(keep, "gemm")
        RB.assert_no_lean(rne(y), y, keep, rows=True, what=f"gemm seed {seed}", row_floor=RB.SMALL_ROW_FLOOR)
        RB.assert_no_lean(rne(_gelu64(y)), _gelu64(y), keep, rows=True, what=f"gemm + gelu seed {seed}", row_floor=RB.SMALL_ROW_FLOOR)
        want = softmax_want(seed)
        RB.assert_no_lean(rne(want), want, rows=True, what=f"softmax seed {seed}")


# ----------------------------------------------------------------------------- every defect is caught
def rejected(got, want, keep=None, rows=False, what=""):
    with pytest.raises(AssertionError, match="lean"):
        RB.assert_no_lean(got, want, keep, rows, what, row_floor=RB.SMALL_ROW_FLOOR)
    return RB.lean(got, want, keep, rows)


@pytest.mark.parametrize("sharp", list(RB.SHARP))
def test_attention_defects_are_rejected(attn, sharp):
    q, k, v, want = attn[sharp, 0]
    r = rejected(attention(q, k, v, True, cvt_p=chop), want, what=f"P truncated ({sharp})")
    assert r.mean <= DEFECT and max(r.cols) <= DEFECT, str(r)
    r = rejected(attention(q, k, v, True, cvt_o=chop), want, what=f"O truncated ({sharp})")
    assert r.mean <= DEFECT and max(r.cols) <= DEFECT, str(r)
    r = rejected(attention(q, k, v, True, cvt_o=chop_cols), want, what=f"O truncated in one column of 16 ({sharp})")
    assert r.cols[COL] <= DEFECT and abs(r.mean) <= RB.BOUND, str(r)                  # the overall mean alone would not see it
    r = rejected(attention(q, k, v, True, cvt_o=chop_rows), want, rows=True, what=f"O truncated in one row of 64 ({sharp})")
    assert r.rows[ROW] <= DEFECT and abs(r.mean) <= RB.BOUND and max(abs(c) for c in r.cols) <= RB.BOUND, str(r)


@pytest.mark.parametrize("epi", ["none", "gelu"])
def test_gemm_defects_are_rejected(gemm, epi):
    y, keep = gemm
    want = _gelu64(y) if epi == "gelu" else y
    r = rejected(chop(want), want, keep, what=f"gemm {epi}: output truncated")
    assert r.mean <= DEFECT and max(r.cols) <= DEFECT, str(r)
    r = rejected(chop_cols(want), want, keep, what=f"gemm {epi}: one column of 16")
    assert r.cols[COL] <= DEFECT and abs(r.mean) <= RB.BOUND, str(r)
    r = rejected(chop_rows(want), want, keep, rows=True, what=f"gemm {epi}: one row of 64")
    assert r.rows[ROW] <= DEFECT and abs(r.mean) <= RB.BOUND, str(r)


@pytest.mark.parametrize("family", ["ln plain", "ln modulated", "softmax"])
def test_row_kernel_defects_are_rejected(family):
    want = softmax_want(0) if family == "softmax" else ln_want(0, family == "ln modulated")
    keep = None if family == "softmax" else RB.keep_mask(want)
    r = rejected(chop(want), want, keep, what=f"{family}: output truncated")
    assert r.mean <= DEFECT and max(r.cols) <= DEFECT, str(r)
    r = rejected(chop_cols(want), want, keep, what=f"{family}: one column of 16")
    assert r.cols[COL] <= DEFECT and abs(r.mean) <= RB.BOUND, str(r)


def test_too_few_elements_in_a_class_is_refused():
    want = torch.rand(64, 512, dtype=F64) + 0.5                                      # 2048 per column class
    with pytest.raises(AssertionError, match="kept elements"):
        RB.assert_no_lean(rne(want), want)


# ----------------------------------------------------------------------------- the exclusion cap, on every data set that has one
def test_exclusion_cap_on_every_data_set():
    """LayerNorm (plain, modulated), RMSNorm + RoPE (q, k), GroupNorm + SiLU (its pre-activation), and the three GEMMs (bf16 weights,
    e4m3 weights, the e4m3 x e4m3 pair; GELU shares their y).  Gaussian data: the rule drops 0.3 .. 0.4 %."""
    shares = {}
    for modulated in (False, True):
        shares[f"ln modulated={modulated}"] = RB.assert_cap(RB.keep_mask(ln_want(3, modulated)), "ln_modulate")
    q, k, wq, wk = RB.rms_data(3)
    for name, x, w in (("q", q, wq), ("k", k, wk)):
        for rope in (True, False):
            shares[f"rmsnorm_rope {name} rope={rope}"] = RB.assert_cap(RB.keep_mask(DR.rope_ref(x.float(), w, RB.RMS_HD, rope)[0]), name)
    x, gamma, beta = RB.groupnorm_data(3)
    shares["groupnorm"] = RB.assert_cap(RB.keep_mask(RB.groupnorm_preact(x, gamma, beta, RB.GN_GROUPS)), "groupnorm")
    a, w, b = RB.gemm_data(3)
    shares["gemm bf16"] = RB.assert_cap(RB.keep_mask(RB.gemm_reference(a, w, b)), "gemm")
    shares["gemm w8"] = RB.assert_cap(RB.keep_mask(RB.gemm_reference(a, RB.e4m3_weights(w), b)), "gemm_w8")
    (a8, sa), (w8, sw) = RB.quantize_rows_host(a), RB.quantize_rows_host(w)
    shares["gemm fp8"] = RB.assert_cap(RB.keep_mask(RB.gemm_reference(a8, w8, b, sa, sw)), "gemm_fp8")
    print({k: f"{100 * v:.2f} %" for k, v in shares.items()})
    assert all(0.001 <= v for v in shares.values()), "the rule drops nothing: it is not being applied"
