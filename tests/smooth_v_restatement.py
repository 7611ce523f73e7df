"""A torch (CPU, float64) restatement of smooth-V, the preprocessing of V behind FLEXAM_SAGE_SMOOTH_V=1 (flexam_attn_fp8_pack_shift_kv and
flexam_attn_fwd_fp8_oshift in csrc/attn_fp8.inc / attn.hip) -- the yardstick of tests/test_smooth_v_gpu.py.  Written from the comments of
include/flexam_hip.h; the attention walk, the e4m3 rounding and the scale rule are tests/mxfp8_restatement.py's, the pack's layouts
tests/rmsnorm_rope_mx_restatement.py's, both by import.

The claim.  The rows of softmax sum to 1, so softmax(S).(V - 1 c^T) + c^T = softmax(S).V for ANY vector c per (batch, head).  What changes
is what e4m3 resolves: V carries one E8M0 scale per channel and 32-key half tile and e4m3's error is relative to the ELEMENT, so a channel
offset all keys share is paid for in every product; and the e4m3 rounding of P multiplies the offset too -- the plain output is
sum p~ (v - c) / l + c sum p~ / l with sum p~ / l != 1 (the row sum l is taken from the unrounded exponentials).  With c = the token mean of
V both are gone: the kernel sees V - c, and c comes back in fp32 in front of the output's one rounding to bf16.

The metric.  An offset in V is an offset in the output, which a plain rel-RMS is dominated by: `centred` takes the token mean of V out of
both sides, leaving the part of the output that tells queries apart.  Exact attention merely rounded to bf16 has a `floor` there (the
rounding is relative to the whole element, offset included) that no kernel writing bf16 can beat; errors are compared in squares above it."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp8_restatement as MX  # noqa: E402
import rmsnorm_rope_mx_restatement as R  # noqa: E402,F401  (the pack's bytes: R.pack_bytes(q, k, shifted_v(v, mean)))

LOG2E = 1.4426950408889634


def rel_rms(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def offset_case_v(B=1, Hh=2, L=300, bias=4.0, seed=None):
    """q, k, v [B, L, H, 128] bf16 from ONE generator (manual_seed(L) unless a seed is given), drawn in the order q, k, offset, v:
    q ~ N(0, 1) 128^-1/2 log2(e) (the prescaled form the pack takes: unit-variance logits), k ~ N(0, 1), v ~ N(0, 1) + an offset per
    (head, channel) ~ N(0, bias^2) that all keys and batches share."""
    g = torch.Generator().manual_seed(L if seed is None else seed)
    q = torch.randn(B, L, Hh, 128, generator=g) * (128 ** -0.5 * LOG2E)
    k = torch.randn(B, L, Hh, 128, generator=g)
    off = torch.randn(Hh, 128, generator=g) * bias
    v = torch.randn(B, L, Hh, 128, generator=g) + off
    return tuple(t.to(torch.bfloat16) for t in (q, k, v))


def token_mean(v):
    """v [B, L, H, 128] -> float64 [B, 1, H, 128]."""
    return v.double().cpu().mean(dim=1, keepdim=True)


def shifted_v(v, mean):
    """What flexam_attn_fp8_pack_shift_kv quantises below L: float32(v) - float32 shift, one float32 subtraction (keys past L stay zero:
    the restatement's pack and walk pad with zeros behind this).  mean [B, H * 128] or [B, 1, H, 128]."""
    B, _, Hh, D = v.shape
    return v.float().cpu() - mean.float().cpu().reshape(B, 1, Hh, D)


def smooth_output(q, k, v, mean, rows, kv_splits=1, split_from_unit=None):
    """flexam_attn_fwd_fp8_oshift on the operands of (q, k, v - mean) with o_shift = mean: the walk on the shifted V, the float32 mean
    added to O / l in front of the rounding to bf16 (which is the caller's) -> float64 [B, len(rows), H, 128]."""
    B, _, Hh, D = v.shape
    out = MX.attention(q, k, shifted_v(v, mean), rows, kv_splits=kv_splits, split_from_unit=split_from_unit)
    return out + mean.float().cpu().reshape(B, 1, Hh, D).double()


def centred(out, v):
    """out [B, rows, H, 128] minus the token mean of v: the part of an attention output that tells queries apart (float64)."""
    return out.double().cpu() - token_mean(v)


def centred_error(out, exact, v):
    """rel-RMS of centred(out) against centred(exact)."""
    return rel_rms(centred(out, v), centred(exact, v))


def bf16(x):
    """x rounded to bf16, as float64 (the output's one rounding)."""
    return x.float().to(torch.bfloat16).double()


def errors(q, k, v, rows=None):
    """Centred errors against exact attention of the bf16-rounded outputs on one key range: (plain MXFP8 walk, smooth-V with the float32
    of the float64 token mean, floor = exact attention rounded to bf16), and the exact output."""
    rows = list(range(q.shape[1])) if rows is None else rows
    exact = MX.attention(q, k, v, rows, quant=False)
    plain = MX.attention(q, k, v, rows)
    smooth = smooth_output(q, k, v, token_mean(v).float(), rows)
    return centred_error(bf16(plain), exact, v), centred_error(bf16(smooth), exact, v), centred_error(bf16(exact), exact, v), exact


def excess_ratio(e_plain, e_smooth, floor):
    """(e_plain^2 - floor^2) / (e_smooth^2 - floor^2): how much of the error above the bf16 floor the shift removes."""
    return (e_plain ** 2 - floor ** 2) / (e_smooth ** 2 - floor ** 2)
