"""A torch (CPU, float64) restatement of smooth-K, the preprocessing of K behind FLEXAM_SAGE_SMOOTH_K=1 (flexam_k_mean,
flexam_rmsnorm_rope_mx_shift and flexam_attn_fp8_pack_shift in csrc/attn_fp8.inc) -- the yardstick of tests/test_smooth_k_gpu.py.  Written
from the comments of include/flexam_hip.h; the attention walk, the e4m3 rounding and the scale rule are tests/mxfp8_restatement.py's, the
producer's values, layouts and admissible sets tests/rmsnorm_rope_mx_restatement.py's, both by import.

The claim.  q.(k_j - c) = q.k_j - q.c, and q.c is one number per query row, so softmax attention does not change for ANY vector c per
(batch, head); what changes is what e4m3 resolves: its error is relative to the ELEMENT, so a channel offset all keys share is paid for
in every score, and with c = the token mean of K it is gone.  `errors` measures exactly that on constructed data.

The mean.  flexam_k_mean cuts the L tokens of a batch into `parts` runs of T = ceil(L / parts) tokens, adds each run in token order in
float32, adds the parts in index order and multiplies by the float32 1 / L.  Against the float64 mean of the float64 values y its error per
channel is at most, in units of u = 2^-24 (one rounding to nearest) and to first order,
    delta    every summand: the kernel's float32 y is within delta * mag of the float64 one (the 30 u <= DELTA = 2^-19 of
             rmsnorm_rope_mx_restatement -- the same arithmetic without the scale rule's 2 u); NONE when k is taken as given (bf16 to
             float32 is exact);
    T - 1    the adds of one part, each relative to a partial sum that is at most sum_t |y_t|;
    parts-1  the adds of the parts, likewise;
    2        1 / L rounded to float32 and the product with it
  <= (delta + (T + parts + 2) u) * mean_t(mag), mag = the producer's magnitude (|k| for the as-given form): `k_mean_bound`.

The shifted producer.  flexam_rmsnorm_rope_mx_shift subtracts shift[b][c] from the rotated y in float32: ONE more rounding, relative to
the result.  Its admissible set is Admissible's with y' = y - shift and tol = DELTA * mag + u |y'| (30 u of mag as counted there, 1 u of
|y'| for the subtraction); the shift itself is an input, taken as given.  After the subtraction |y'| can be far below mag, so more
elements sit within tol of a rounding boundary than in the unshifted cases: the GPU test's inputs are chosen (and tests/
test_smooth_k_restatement_cpu.py holds them to it) so that the ambiguous share stays under AMBIGUOUS_CAP."""
import functools
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp8_restatement as MX  # noqa: E402
import rmsnorm_rope_mx_restatement as R  # noqa: E402

U = 2.0 ** -24
LOG2E = 1.4426950408889634
FORMAT_BOUND = 6.5e-2          # MXFP8 attention against exact attention on unit-variance logits (tests/test_attn_fp8_gpu.py)


def rel_rms(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ----------------------------------------------------------------------------- the constructed data
def offset_case(B=1, Hh=2, L=300, bias=8.0, sharp=1.0, seed=300):
    """q, k, v [B, L, H, 128] bf16 from ONE generator, drawn in the order q, offset, k, v: q ~ N(0, 1) 128^-1/2 log2(e) sharp (the
    prescaled form the pack takes: unit-variance logits times `sharp`), k ~ N(0, 1) + an offset per (head, channel) ~ N(0, bias^2) that
    all keys and batches share, v ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, L, Hh, 128, generator=g) * (128 ** -0.5 * LOG2E * sharp)
    off = torch.randn(Hh, 128, generator=g) * bias
    k = torch.randn(B, L, Hh, 128, generator=g) + off
    v = torch.randn(B, L, Hh, 128, generator=g)
    return tuple(t.to(torch.bfloat16) for t in (q, k, v))


def token_mean(k):
    """k [B, L, H, 128] -> float64 [B, 1, H, 128]."""
    return k.double().mean(dim=1, keepdim=True)


def shifted_k(k, mean):
    """What flexam_attn_fp8_pack_shift quantises: float32(k) - float32 shift, one float32 subtraction.  mean [B, H * 128] or [B, 1, H, 128]."""
    B, _, Hh, D = k.shape
    return k.float().cpu() - mean.float().cpu().reshape(B, 1, Hh, D)


def errors(q, k, v, rows=None):
    """rel-RMS against exact attention (the walk with quant=False) of the MXFP8 walk on k as it is and on k - mean_tokens(k):
    (plain, smooth), and the exact output."""
    rows = list(range(q.shape[1])) if rows is None else rows
    exact = MX.attention(q, k, v, rows, quant=False)
    plain = MX.attention(q, k, v, rows)
    smooth = MX.attention(q, shifted_k(k, token_mean(k)), v, rows)
    return rel_rms(plain, exact), rel_rms(smooth, exact), exact


# ----------------------------------------------------------------------------- the mean
def k_mean_bound(mag_mean, tokens_per_part, parts, normed):
    """The bound of the module docstring on |flexam_k_mean - float64 mean| per channel; mag_mean = mean over the tokens of mag."""
    return ((R.DELTA if normed else 0.0) + (tokens_per_part + parts + 2) * U) * mag_mean


@functools.lru_cache(maxsize=None)
def mean_inputs(B, L, offset):
    """k [B L, 3072] bf16 rows, wk, cos / sin [L + offset, 64] for the k_mean tests: the k columns, weight and tables of the producer's case
    of this shape where there is one (its zero, quiet, scaled and outlier rows included), else drawn the same way."""
    for name, c in R.CASES.items():
        if (c["B"], c["L"], c["offset"]) == (B, L, offset):
            ci = R.case_inputs(name)
            return types.SimpleNamespace(B=B, L=L, offset=offset, eps=ci.eps, k=ci.qkv[:, R.C:2 * R.C], wk=ci.wk,
                                         cos=ci.cos[:L + offset], sin=ci.sin[:L + offset])
    g = torch.Generator().manual_seed(77 + 1000 * L + B)
    k = (torch.randn(B * L, R.C, generator=g) * 1.5).to(torch.bfloat16)
    wk = torch.rand(R.C, generator=g) + 0.5
    ang = torch.rand(L + offset, R.HD // 2, generator=g) * 6.28
    return types.SimpleNamespace(B=B, L=L, offset=offset, eps=R.EPS, k=k, wk=wk, cos=ang.cos(), sin=ang.sin())


@functools.lru_cache(maxsize=None)
def mean_reference(B, L, offset, normed):
    """(float64 mean [B, 3072], mean over the tokens of mag [B, 3072]) of mean_inputs: of reference()'s y when normed, of k itself otherwise."""
    c = mean_inputs(B, L, offset)
    if normed:
        y, mag = R.reference(c.k, c.wk, c.cos, c.sin, L, offset, c.eps)
    else:
        y = c.k.double()
        mag = y.abs()
    return y.reshape(B, L, R.C).mean(dim=1), mag.reshape(B, L, R.C).mean(dim=1)


# ----------------------------------------------------------------------------- the shifted producer
class ShiftedAdmissible(R.Admissible):
    """The admissible scale bytes and codes of the K operand of flexam_rmsnorm_rope_mx_shift: Admissible's sets around y' = y - shift
    with tol = delta * mag + u |y'|; shift float32 [B, 3072], rows m = b * tokens_per_batch + token."""

    def __init__(self, x, w, cos, sin, tokens_per_batch, token_offset, eps, shift, delta=R.DELTA):
        y, mag = R.reference(x, w, cos, sin, tokens_per_batch, token_offset, eps)
        s = shift.double().cpu().reshape(-1, 1, R.HEADS, 4, 32).expand(-1, tokens_per_batch, -1, -1, -1).reshape(y.shape)
        self.y = y - s
        self.tol = delta * mag + U * self.y.abs()
        a = self.y.abs()
        self.e_lo = R.e8m0_byte((a - self.tol).amax(dim=-1).clamp(min=0))
        self.e_hi = R.e8m0_byte((a + self.tol).amax(dim=-1))
        self.e_nom = R.e8m0_byte(a.amax(dim=-1))
        self.zero_in = (self.y - self.tol <= 0) & (self.y + self.tol >= 0)
        lo, hi = self._code_ranks(self.e_nom)
        self.code_nom = MX.e4m3_code(self.y * torch.pow(2.0, 127.0 - self.e_nom.double()).unsqueeze(-1))
        self.ambiguous_codes = float((lo != hi).double().mean())
        self.ambiguous_scales = float((self.e_lo != self.e_hi).double().mean())


SHIFTED_CASES = ("ragged", "tile-plus-one", "two-q-blocks")
OFFSET_STDS = 2.0              # the offset of the shifted cases in units of the rows' noise std (1.5): at 4 the ambiguous share doubles, at 8 it exceeds the cap


@functools.lru_cache(maxsize=None)
def shifted_case(name, stds=OFFSET_STDS):
    """The producer's case `name` with an offset in K for the shift to remove: k rows = the case's rows + an offset per (batch, channel)
    ~ N(0, (stds * 1.5)^2); the rotation angles zero for the pairs 0 .. 31 of every head (those channels keep their offset: a rotation
    by random angles averages it away) and the case's random ones for 32 .. 63; shift = the float32 of the float64 token mean of the
    float64 K.  -> the case's namespace with qkv, cos, sin replaced and `shift` [B, 3072] added (CPU tensors, not to be modified)."""
    c = R.case_inputs(name)
    g = torch.Generator().manual_seed(4000 + c.L)
    off = torch.randn(c.B, R.C, generator=g) * (stds * 1.5)
    qkv = c.qkv.clone()
    qkv[:, R.C:2 * R.C] = (c.qkv[:, R.C:2 * R.C].float().reshape(c.B, c.L, R.C) + off[:, None, :]).reshape(c.M, R.C).to(torch.bfloat16)
    cos, sin = c.cos.clone(), c.sin.clone()
    cos[:, :32], sin[:, :32] = 1.0, 0.0
    y, _ = R.reference(qkv[:, R.C:2 * R.C], c.wk, cos, sin, c.L, c.offset, c.eps)
    shift = y.reshape(c.B, c.L, R.C).mean(dim=1).float()
    d = dict(vars(c))
    d.update(qkv=qkv, cos=cos, sin=sin, shift=shift)
    return types.SimpleNamespace(**d)


@functools.lru_cache(maxsize=None)
def shifted_admissible(name, stds=OFFSET_STDS):
    """(Admissible of q, ShiftedAdmissible of k) of shifted_case(name): computed once, shared."""
    c = shifted_case(name, stds)
    return (R.Admissible(c.qkv[:, :R.C], c.wq, c.cos, c.sin, c.L, c.offset, c.eps),
            ShiftedAdmissible(c.qkv[:, R.C:2 * R.C], c.wk, c.cos, c.sin, c.L, c.offset, c.eps, c.shift))


def check_shifted_operands(name, q8, qs, kv8):
    """The operand buffers (CPU) after flexam_rmsnorm_rope_mx_shift on shifted_case(name) -> (verdict of q, verdict of k), rows below L."""
    c = shifted_case(name)
    aq, ak = shifted_admissible(name)
    flat = lambda t: t.reshape((c.M,) + tuple(t.shape[2:]))
    qc, qsc = R.q_rows_inv(q8, qs, c.L)
    kc, ksc = R.k_record_inv(kv8, c.L)
    return aq.check(flat(qc), flat(qsc), "q"), ak.check(flat(kc), flat(ksc), "k")
