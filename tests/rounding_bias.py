"""Rounding bias of a bf16 output: the signed error in bf16 ulps against an UNROUNDED float64 reference, its mean, and the data sets the
lean tests run on.  Shared by tests/test_rounding_bias_cpu.py (which proves the check is not blind) and tests/test_rounding_bias_gpu.py
(which runs the kernels).  Not a test module.

A distance bound of one ulp or more cannot tell round-to-nearest-even from truncation: both stay within one ulp per element.  What
differs is the MEAN of the signed error  e = sign(want) (got - want) / ulp_bf16(want):  0 for round-to-nearest-even, -0.5 for a
truncated output, -0.42 .. -0.48 for a truncated softmax P of attention.  `lean` measures that mean over all elements and per class of
output column modulo 16 (a lane's 8-element fragment, a 16- or 32-byte store), optionally per class of output row modulo 64;
`assert_no_lean` bounds each by BOUND = 0.05 ulp.

Why 0.05.  Honest rounding gives e a standard deviation of 0.29 (uniform on +-1/2) to 0.36 (a value near the top of its binade has half
the relative ulp, and fp32 noise adds a little): a class mean over MIN_PER_CLASS = 4096 independent elements has sigma <= 0.006.  In
attention the rounding of P is shared by the 128 channels of a row, so elements are not independent: at peaked logits the overall mean
over 1000 rows has sigma about 0.006 (measured on the CPU restatement, tests/test_rounding_bias_cpu.py).  0.05 is 8 sigma above that and
8 times below the smallest defect in scope.  It is not tuned to what a GPU shows.

Row classes hold MIN_PER_CLASS elements too where the shape allows it (softmax_bias_rows at 512 x 512: 4096).  A row class of the GEMM
(M = 300: 4 or 5 rows of 512) holds 2048 elements or more before exclusions, one of attention (600 rows: 9 or 10 rows of 2 heads x
128) 2304: those callers pass row_floor = SMALL_ROW_FLOOR = 2000, at which independent elements keep sigma <= 0.008, 0.05 is 6 sigma.
In attention the 128 channels of a row share the roundings of the row's P values.  At flat logits a hundred keys or more carry a row
and those average out within it: a class mean has sigma 0.009 at 200 keys (measured, CPU restatement), 0.05 is 5.5 sigma.  At PEAKED
logits a few keys carry a row, a row's mean has sigma about 0.2 and a class of 19 rows about 0.045: the row classes say nothing at
0.05 there and are not asserted (measured: up to 0.13 under honest rounding); nor with a weighted last key, which carries most of a
row whatever the logits.

Exclusions apply only where the output is a sum of signed terms (LayerNorm, RMSNorm + RoPE, GroupNorm, GEMM, and GELU / SiLU of such a
sum), where fp32 accumulation noise is not negligible next to the ulp of a tiny element: `keep_mask(s)` drops |s| < 2^-8 rms(s), s the
float64 value that was summed (the pre-activation under GELU / SiLU), rms per row.  `assert_cap` holds the dropped share to 1 % from the
reference alone.  Softmax outputs, products and attention outputs get no exclusion (attention's V has one sign per channel)."""
import math
import os
import sys
from dataclasses import dataclass

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attn_exact_cases import bf16_ulp  # noqa: E402

BOUND = 0.05
COL_CLASSES, ROW_CLASSES = 16, 64
MIN_PER_CLASS = 4096
SMALL_ROW_FLOOR = 2000                          # row classes of the M = 300 GEMM and of 600-row attention (the docstring says why)
DROP_CAP = 0.01
LN2, LOG2E = math.log(2.0), 1.0 / math.log(2.0)
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


# ----------------------------------------------------------------------------- the measure
def signed_ulp_error(got, want, keep=None):
    """sign(want) (got - want) / ulp_bf16(want) over the kept elements (1-D when keep is given).  got: the bf16 output as float64;
    want: the float64 reference, not rounded.  Negative: got lies nearer zero than want."""
    e = torch.sign(want) * (got - want) / bf16_ulp(want)
    return e if keep is None else e[keep]


@dataclass
class Lean:
    mean: float                 # over all kept elements
    cols: list                  # mean per class of output column (last dim) % 16
    col_counts: list
    dropped: float              # share of elements left out
    rows: list = None           # mean per class of output row (second to last dim) % 64, when asked for
    row_counts: list = None

    def worst_col(self):
        return max(self.cols, key=abs)

    def worst_row(self):
        return max(self.rows, key=abs) if self.rows else 0.0

    def __str__(self):
        s = f"mean {self.mean:+.4f}, worst column class {self.worst_col():+.4f}, excluded {100 * self.dropped:.2f} %"
        return s + (f", worst row class {self.worst_row():+.4f}" if self.rows else "")


def _class_means(e, k, idx, n):
    """(means, counts) of e over the kept elements by class idx (int64, e's shape)."""
    idx = idx.expand(e.shape).reshape(-1)
    w = k.reshape(-1).to(F64)
    sums = torch.zeros(n, dtype=F64, device=e.device).index_add_(0, idx, e.reshape(-1) * w)
    cnt = torch.zeros(n, dtype=F64, device=e.device).index_add_(0, idx, w)
    return (sums / cnt.clamp_min(1)).tolist(), [int(c) for c in cnt.tolist()]


def lean(got, want, keep=None, rows=False):
    """got, want [..., R, C] float64 (a bf16 tensor is widened): the last dim is the output column, the one before it the output row."""
    got, want = got.to(F64), want.to(F64)
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), "a NaN or inf in the output"
    k = torch.ones_like(want, dtype=torch.bool) if keep is None else keep
    e = torch.where(k, signed_ulp_error(got, want), torch.zeros_like(want))
    kept = int(k.sum())
    col = torch.arange(want.shape[-1], device=want.device) % COL_CLASSES
    cols, col_counts = _class_means(e, k, col, COL_CLASSES)
    out = Lean(float(e.sum()) / max(kept, 1), cols, col_counts, 1.0 - kept / k.numel())
    if rows:
        row = (torch.arange(want.shape[-2], device=want.device) % ROW_CLASSES)[:, None]
        out.rows, out.row_counts = _class_means(e, k, row, ROW_CLASSES)
    return out


def assert_no_lean(got, want, keep=None, rows=False, what="", row_floor=MIN_PER_CLASS):
    """|mean| <= BOUND overall and in each of the 16 column classes (each with MIN_PER_CLASS kept elements or more); with rows, in each
    of the 64 row classes too (each with row_floor kept elements or more).  Prints the figures first and returns them."""
    r = lean(got, want, keep, rows)
    print(f"{what}: {r}")
    assert min(r.col_counts) >= MIN_PER_CLASS, f"{what}: a column class has only {min(r.col_counts)} kept elements"
    assert abs(r.mean) <= BOUND, f"{what}: the output leans by {r.mean:+.4f} ulp overall"
    bad = [(c, round(m, 4)) for c, m in enumerate(r.cols) if not abs(m) <= BOUND]
    assert not bad, f"{what}: column classes (column % 16, mean ulp) lean: {bad}"
    if rows:
        assert min(r.row_counts) >= row_floor, f"{what}: a row class has only {min(r.row_counts)} kept elements"
        bad = [(c, round(m, 4)) for c, m in enumerate(r.rows) if not abs(m) <= BOUND]
        assert not bad, f"{what}: row classes (row % 64, mean ulp) lean: {bad}"
    return r


def keep_mask(s):
    """The elements of a signed sum s [..., C] (float64) that are compared: |s| >= 2^-8 rms(s), rms over the row."""
    return s.abs() >= 2.0 ** -8 * s.pow(2).mean(-1, keepdim=True).sqrt()


def assert_cap(keep, what=""):
    """At most DROP_CAP of the elements dropped: from the reference alone, before any kernel runs."""
    dropped = 1.0 - float(keep.sum()) / keep.numel()
    assert dropped <= DROP_CAP, f"{what}: the exclusion rule drops {100 * dropped:.2f} % of the elements (cap 1 %)"
    return dropped


# ----------------------------------------------------------------------------- data: attention
HEADS, HEAD_DIM = 2, 128
ATTN_LQ = 600                                   # 2 whole q blocks of 256 rows and a ragged one
SHARP = {"flat": 1.0, "peaked": 6.0}            # std of a score in exp2 units; 6 moves the deferred reference (RESCALE_THR_LOG2 = 8)
SOFTMAX_SCALE = HEAD_DIM ** -0.5                # of the scale-in-kernel forms


def attn_data(seed, lq, lk, sharp, prescaled, device="cpu"):
    """q [1, lq, 2, 128], k, v [1, lk, 2, 128] bf16.  k ~ N(0, 1); v = sign_c U(0.5, 2), one sign per channel and head (outputs stay
    away from zero); q ~ N(0, s^2) with s such that a score has std SHARP[sharp] in exp2 units: drawn ALREADY scaled (then rounded)
    for the pre-scaled forms, drawn for softmax_scale = 1 / sqrt(128) otherwise."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(1, lk, HEADS, HEAD_DIM, generator=g, dtype=F64)
    sign = torch.where(torch.rand(1, 1, HEADS, HEAD_DIM, generator=g) < 0.5, -1.0, 1.0).double()
    v = sign * (0.5 + 1.5 * torch.rand(1, lk, HEADS, HEAD_DIM, generator=g, dtype=F64))
    q_std = SHARP[sharp] / math.sqrt(HEAD_DIM) if prescaled else SHARP[sharp] / (SOFTMAX_SCALE * LOG2E * math.sqrt(HEAD_DIM))
    q = torch.randn(1, lq, HEADS, HEAD_DIM, generator=g, dtype=F64) * q_std
    return tuple(t.to(BF).to(device) for t in (q, k, v))


def attn_scores(q, k, prescaled, last_key_multiplicity=1, mask=None):
    """[B, H, Lq, Lk] float64 scores in exp2 units of bf16 q, k: q.k for a pre-scaled q, softmax_scale log2(e) q.k otherwise; a last key
    counted m times carries + log2 m (ln m on its logit); mask [Lq, Lk] bool, False = not seen."""
    s = torch.einsum("blhd,bmhd->bhlm", q.double(), k.double())
    if not prescaled:
        s = s * (SOFTMAX_SCALE * LOG2E)
    if last_key_multiplicity != 1:
        s[..., -1] += math.log2(last_key_multiplicity)
    if mask is not None:
        s = s.masked_fill(~mask.to(s.device), -math.inf)
    return s


def attn_reference(q, k, v, prescaled, last_key_multiplicity=1, mask=None):
    """Plain float64 softmax-attention [B, Lq, H, 128] of the bf16 inputs, on their device: exp2(q.k) for a pre-scaled q,
    exp(softmax_scale q.k) otherwise.  Nothing of the kernel's walk is in it."""
    s = attn_scores(q, k, prescaled, last_key_multiplicity, mask)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return torch.einsum("bhlm,bmhd->blhd", p / p.sum(-1, keepdim=True), v.double())


def attn_rows_last(t):
    """[B, L, H, 128] -> [B, H, L, 128]: the q row second to last, as `lean` reads it."""
    return t.transpose(1, 2)


# ----------------------------------------------------------------------------- data: GEMM
GEMM_M, GEMM_N, GEMM_K = 300, 512, 2048
GEMM_M_TALL = 1300                              # enough 256-wide tiles for a whole round of 8 CUs and a tail behind it


def gemm_data(seed, device="cpu", m=GEMM_M):
    """a [m, K] ~ N(0, 1), w [N, K] ~ N(0, 1 / K) bf16 and a bias on the bf16 grid (fp32): y = a w^T + b has std about 1.1, so GELU
    sees its bend and both tails."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(m, GEMM_K, generator=g, dtype=F64).to(BF)
    w = (torch.randn(GEMM_N, GEMM_K, generator=g, dtype=F64) / math.sqrt(GEMM_K)).to(BF)
    b = (torch.randn(GEMM_N, generator=g, dtype=F64) * 0.5).to(BF).float()
    return a.to(device), w.to(device), b.to(device)


def gemm_reference(a, w, b, a_scale=None, w_scale=None):
    """float64 a w^T (x the row scales of an fp8 pair) + b of operands of any storage type, read exactly."""
    y = a.double() @ w.double().t()
    if a_scale is not None:
        y = y * a_scale.double()[:, None] * w_scale.double()[None, :]
    return y + b.double()


def e4m3_weights(w):
    """bf16 weights -> float8_e4m3fn storage (qfloat8); the reference upcasts these codes exactly."""
    return w.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


def quantize_rows_host(x):
    """The shape of flexam_quantize_rows_fp8 with torch's cast (row scale amax / 448): the CPU stand-in that gives the fp8 GEMM's data
    set its distribution for the exclusion-cap check; the GPU test quantises with the kernel."""
    scale = (x.float().abs().amax(1) / 448.0).clamp_min(1e-30)
    return (x.float() / scale[:, None]).to(torch.float8_e4m3fn), scale


# ----------------------------------------------------------------------------- data: row kernels
LN_M, LN_C = 64, 3072
RMS_B, RMS_L, RMS_C, RMS_HD = 8, 32, 3072, 128                  # M = 256 rows: 8 sequences of 32 tokens, 24 of them rotated
T5_M, T5_C = 48, 4096
SMB_M, SMB_N = 512, 512
MUL_N = 1 << 18
SMR_C, SMR_H, SMR_W = 640, 15, 30                               # the VAE encoder's middle attention: n = 450 positions
GN_C, GN_F, GN_H, GN_W, GN_GROUPS = 256, 2, 16, 24, 32


def on_bf16_grid(x):
    """fp32 values that bf16 holds exactly."""
    return x.to(BF).float()


def ln_data(seed, device="cpu"):
    """x [64, 3072] ~ N(0.5, 2) fp32 on the bf16 grid; a [4, 2, C] (shift | 1 + scale) table and a row index, as the DiT block has."""
    g = torch.Generator().manual_seed(seed)
    x = on_bf16_grid(torch.randn(LN_M, LN_C, generator=g) * 2 + 0.5)
    tab = torch.randn(4, 2, LN_C, generator=g) * 0.5
    tab[:, 1] += 1.0
    rows = torch.randint(0, 4, (LN_M,), generator=g, dtype=torch.int32)
    return x.to(device), on_bf16_grid(tab).to(device), rows.to(device)


def rms_data(seed):
    """q, k [8, 32, 3072] bf16 and their fp32 weights on the bf16 grid (host tensors: the float64 restatement that is reused builds its
    angle table there)."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(RMS_B, RMS_L, RMS_C, generator=g, dtype=F64) * 1.5).to(BF)
    k = torch.randn(RMS_B, RMS_L, RMS_C, generator=g, dtype=F64).to(BF)
    wq, wk = (on_bf16_grid(1 + 0.1 * torch.randn(RMS_C, generator=g)) for _ in range(2))
    return q, k, wq, wk


def t5_data(seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    x = on_bf16_grid(torch.randn(T5_M, T5_C, generator=g) * 3 + 0.25)
    w = on_bf16_grid(1 + 0.3 * torch.randn(T5_C, generator=g))
    return x.to(device), w.to(device)


def softmax_bias_data(seed, device="cpu"):
    """Scores and a relative-position bias [512, 512] fp32 on the bf16 grid."""
    g = torch.Generator().manual_seed(seed)
    s = on_bf16_grid(torch.randn(SMB_M, SMB_N, generator=g) * 4)
    b = on_bf16_grid(torch.randn(SMB_M, SMB_N, generator=g) * 2)
    return s.to(device), b.to(device)


def mul_data(seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.randn(MUL_N, generator=g) * 4).to(BF).to(device) for _ in range(2))


def softmax_rows_data(seed, device="cpu"):
    """Scores [n, round_up(n, 4)] fp32 on the bf16 grid, n = 450."""
    g = torch.Generator().manual_seed(seed)
    n = SMR_H * SMR_W
    return on_bf16_grid(torch.randn(n, (n + 3) // 4 * 4, generator=g) * 3).to(device)


def groupnorm_data(seed):
    """x [C, F, H, W] fp32 on the bf16 grid, gamma, beta [C] likewise (host tensors, for the layout helpers)."""
    g = torch.Generator().manual_seed(seed)
    x = on_bf16_grid(torch.randn(GN_C, GN_F, GN_H, GN_W, generator=g) * 2 + 0.3)
    gamma = on_bf16_grid(1 + 0.3 * torch.randn(GN_C, generator=g))
    beta = on_bf16_grid(0.3 * torch.randn(GN_C, generator=g))
    return x, gamma, beta


def groupnorm_preact(x, gamma, beta, groups, eps=1e-5):
    """float64 GroupNorm of x [C, F, H, W] (statistics over a group's channels and all positions), before the SiLU: [F, H, W, C]."""
    c = x.shape[0]
    xg = x.double().reshape(groups, -1)
    mu = xg.mean(1, keepdim=True)
    y = ((xg - mu) * ((xg - mu).pow(2).mean(1, keepdim=True) + eps).rsqrt()).reshape(x.shape)
    y = y * gamma.double().view(c, 1, 1, 1) + beta.double().view(c, 1, 1, 1)
    return y.permute(1, 2, 3, 0)


def silu64(y):
    return y / (1.0 + torch.exp(-y))
