"""GPU: the DiT block's row kernels and the sampler step's helpers (csrc/dit_elementwise.hip), called directly through flexam_amd.hip
at every instance their dispatch selects, against float64 torch restatements written here (the formulas of oracle/dit.py evaluated in
float64).  tests/test_hip_kernels.py calls most of these once, at the DiT width 3072 or at 256: that reaches one of the eight wave-form
instances of ln_modulate, one block-form instance, and none of the paths a 3072-wide row does not take.

Tolerances (test_hip_kernels.py's header): a bf16 output is within 1 bf16 ulp (2^-8 |want|) of the float64 value plus `slack`, the
fp32 rounding its inputs carry into it (2^-20 of the magnitudes that enter, stated per kernel); an fp32 output is within a few fp32
ulps of those magnitudes; pure data movement and integer / power-of-two arithmetic are held bit for bit.  The docstring of every test
names the instance its shapes select: the choice is made from the arguments alone (C, M, alignment, row pitch)."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dit as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import checksum_restatement as CR  # noqa: E402

pytestmark = pytest.mark.gpu
BF, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
SENT = 12352.0                       # a bf16 value no kernel here writes: cells outside an output view must keep it


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def H():
    from flexam_amd import hip
    hip.device_check()
    return hip


def close(got, want, slack, ulps=1.0, msg=""):
    """|got - want| <= ulps * 2^-8 |want| + slack elementwise (ulps = 0 for fp32 outputs); NaN fails."""
    got, want = got.double().cpu(), want.double().cpu()
    err = (got - want).abs()
    tol = ulps * 2.0 ** -8 * want.abs() + (slack.double().cpu() if torch.is_tensor(slack) else slack)
    bad = ~(err <= tol)
    assert not bool(bad.any()), f"{msg}: {int(bad.sum())}/{bad.numel()} off, worst err {float(err.nan_to_num(math.inf).max()):.4g}"


def padded(rows, cols, pad, dtype, fill):
    """A [rows, cols] view of a [rows, cols + pad] device buffer filled with `fill`: a strided operand with a known border."""
    buf = torch.full((rows, cols + pad), fill, dtype=dtype, device=dev())
    return buf, buf[:, :cols]


def keeps(buf, cols, fill, what):
    pad = buf[:, cols:]
    assert torch.equal(pad.cpu(), torch.full(pad.shape, fill, dtype=buf.dtype)), f"{what}: a cell past the row was written"


def up32(v):
    """The smallest fp32 value >= v (a bound passed to a kernel stays a bound)."""
    f = np.float32(v)
    return float(np.nextafter(f, np.float32(np.inf)) if float(f) < v else f)


# ----------------------------------------------------------------------------- ln_modulate / ln_modulate_fp8
def ln_instance(c):
    """flexam_ln_modulate's dispatch (dit_elementwise.hip): wave per row for C % 512 == 0 and C <= 4096, else the block form with
    VPT = ceil(C / 1024) vectors per thread, 5..8 running as VPT 8."""
    if c % 512 == 0 and c <= 4096:
        return f"wave-NV8={c // 512}"
    v = -(-c // 1024)
    return f"block-VPT={8 if v > 4 else v}"


LN_WIDTHS = [512 * k for k in range(1, 9)] + [8, 264, 1032, 1544, 2056, 3080, 5120, 8192]
LN_MODES = ("plain", "row_index", "rows_per_batch", "affine+table")


def ln_rows(g, m, c):
    """fp32 rows: row 0 has mean 1e3 over a spread of 1 (a one-pass E[x^2] - E[x]^2 loses the variance to cancellation), row 1 is
    constant (variance 0, rstd = eps^-1/2), the rest N(0.5, 2)."""
    x = torch.randn(m, c, generator=g, dtype=F64) * 2 + 0.5
    x[0] = 1e3 + torch.randn(c, generator=g, dtype=F64)
    x[1] = 2.0
    return x.float()


def ln_ref(x, eps, w=None, b=None, sh=None, sc=None):
    """float64 WanLayerNorm (FX.py:192-202, population variance), the optional affine step, then y * scale + shift; and the slack:
    the fp32 mean's rounding (2^-20 of max |x| in the kernel's sums) is carried out by rstd and the multipliers."""
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    rstd = ((x - mu).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    y = (x - mu) * rstd
    mag = x.abs().amax(-1, keepdim=True) * rstd
    if w is not None:
        y, mag = y * w.double() + b.double(), mag * w.double().abs() + b.double().abs()
    if sc is not None:
        y, mag = y * sc.double() + sh.double(), mag * sc.double().abs() + sh.double().abs()
    return y, 2.0 ** -20 * mag + 1e-30


def ln_case(g, m, c, mode):
    """(kernel keyword arguments on the device, float64 reference arguments) of one modulation form; the table is [rows, 2, C]
    (shift | scale), so tab_ld = 2C, and ln_w / ln_b are the two rows of one [2, C] tensor."""
    tab = torch.randn(4, 2, c, generator=g) * 0.5
    tab[:, 1] += 1.0
    lnwb = torch.randn(2, c, generator=g) * 0.5
    lnwb[0] += 1.0
    rows = torch.randint(0, 4, (m,), generator=g, dtype=torch.int32)
    td, ld = tab.to(dev()), lnwb.to(dev())
    if mode == "plain":
        return {}, {}
    if mode == "row_index":
        r = rows.long()
        return dict(shift=td[:, 0], scale=td[:, 1], row_index=rows.to(dev())), dict(sh=tab[r, 0], sc=tab[r, 1])
    if mode == "rows_per_batch":
        r = torch.arange(m) // 10
        return dict(shift=td[:, 0], scale=td[:, 1], rows_per_batch=10), dict(sh=tab[r, 0], sc=tab[r, 1])
    r = rows.long()
    return (dict(shift=td[:, 0], scale=td[:, 1], row_index=rows.to(dev()), ln_w=ld[0], ln_b=ld[1]),
            dict(w=lnwb[0], b=lnwb[1], sh=tab[r, 0], sc=tab[r, 1]))


@pytest.mark.parametrize("c", LN_WIDTHS, ids=[f"{ln_instance(c)}-C{c}" for c in LN_WIDTHS])
def test_ln_modulate_every_instance_and_form(H, c):
    """flexam_ln_modulate at the instance named in the id: wave form NV8 = 1..8 (C = 512 .. 4096), block form VPT 1 (C = 8: one
    vector; 264: a part-used last vector round), 2 (1032, 1544), 3 (2056), 4 (3080) and 8 (5120: five used, 8192: all eight).  Each in
    the four modulation forms, from a strided x whose pad holds NaN into a strided out whose pad must keep its sentinel."""
    g = torch.Generator().manual_seed(c)
    m, eps = 37, 1e-6
    x = ln_rows(g, m, c)
    xbuf, xd = padded(m, c, 4, F32, math.nan)
    xd.copy_(x)
    for mode in LN_MODES:
        kw, rk = ln_case(g, m, c, mode)
        obuf, out = padded(m, c, 8, BF, SENT)
        H.ln_modulate(xd, out=out, eps=eps, **kw)
        want, slack = ln_ref(x, eps, **rk)
        close(out, want, slack, msg=f"ln_modulate C={c} {mode}")
        keeps(obuf, c, SENT, f"ln_modulate C={c} {mode}")


def gelu_tanh64(z):
    return 0.5 * z * (1 + torch.tanh(math.sqrt(2 / math.pi) * (z + 0.044715 * z ** 3)))


@pytest.mark.parametrize("nv8", range(1, 9), ids=[f"wave-NV8={k}-C{512 * k}" for k in range(1, 9)])
def test_ln_modulate_fp8_every_instance_and_form(H, nv8):
    """flexam_ln_modulate_fp8, instance ln_modulate_wave_kernel<NV8, true> with C = 512 NV8, in the four modulation forms:
      * row_scale = amax / 448 of the float64 row;
      * the dequantised row e4m3(q) * row_scale is within half an e4m3 ulp (2^-4 relative) of the float64 row, plus half the
        subnormal step (2^-10 row_scale);
      * next_scale is the documented bound (1.07 |y|_2 next_wnorm + next_bias) / 448 and is at least the true
        max_j |gelu(a . w_j + b_j)| / 448 of the GEMM it feeds, for weights that include each row's own direction (where
        Cauchy-Schwarz is tight), with next_wnorm / next_bias computed exactly and rounded up."""
    c = 512 * nv8
    g = torch.Generator().manual_seed(100 + nv8)
    m, eps = 19, 1e-6
    x = ln_rows(g, m, c)
    xbuf, xd = padded(m, c, 4, F32, math.nan)
    xd.copy_(x)
    for mode in LN_MODES:
        kw, rk = ln_case(g, m, c, mode)
        want, slack = ln_ref(x, eps, **rk)
        norm = want.norm(dim=1, keepdim=True).clamp_min(1e-300)                    # row 1 is all zero in the plain form
        wn = torch.cat([want / norm * (0.5 + torch.rand(m, 1, generator=g, dtype=F64)),
                        torch.randn(5, c, generator=g, dtype=F64) * 0.03])          # w_j: each row's direction, then random rows
        bn = torch.randn(m + 5, generator=g, dtype=F64) * 0.5
        wnorm, bmax = up32(float(wn.norm(dim=1).max())), up32(float(bn.abs().max()))
        qbuf = torch.full((m, c + 16), 0x5A, dtype=U8, device=dev())
        rs = torch.full((m,), math.nan, device=dev())
        ns = torch.full((m,), math.nan, device=dev())
        H.ln_modulate_fp8(xd, qbuf[:, :c], rs, eps=eps, next_scale=ns, next_wnorm=wnorm, next_bias=bmax, **kw)
        what = f"ln_modulate_fp8 C={c} {mode}"
        assert bool((qbuf[:, c:] == 0x5A).all()), f"{what}: a byte past the row was written"
        rs, ns = rs.double().cpu(), ns.double().cpu()
        amax = want.abs().amax(1)
        rs_want = torch.where(amax > 0, amax / 448, 1.0)                           # an all-zero row (row 1, plain) is scaled by 1
        assert bool(((rs - rs_want).abs() <= (2.0 ** -20 * amax + slack.amax(1)) / 448).all()), f"{what}: row scale"
        deq = qbuf[:, :c].cpu().view(torch.float8_e4m3fn).double() * rs[:, None]
        close(deq, want, 2.0 ** -10 * rs[:, None] + 2 * slack, ulps=16.0, msg=f"{what}: dequantised row")
        bound = (1.07 * want.norm(dim=1) * wnorm + bmax) / 448
        assert bool(((ns - bound).abs() <= 1e-5 * bound).all()), f"{what}: next_scale is not the documented bound"
        true = gelu_tanh64(deq @ wn.t() + bn).abs().amax(1) / 448
        assert bool((ns >= true).all()), f"{what}: next_scale below the GEMM output it bounds"


# ----------------------------------------------------------------------------- rmsnorm_rope / rmsnorm_rope_scatter
GRID = (2, 3, 4)                     # 24 rotated tokens, then pass-through tokens up to L
L, B, LC, TOK0 = 29, 2, 11, 16       # a rank's chunk: tokens 16 .. 26 of each sample (rotated and pass-through ones)


def rope_ref(x, w, hd, rope, eps=1e-6):
    """float64 WanRMSNorm over the row (oracle.dit.rms_norm) then the 3-axis RoPE (oracle.dit.rope_apply, float64 angles) of the
    FULL sequences x [B, L, C]; the slack is 2^-20 of the pair magnitudes |re| + |im| the rotation mixes."""
    b, l, c = x.shape
    y = O.rms_norm(x.double(), w.double(), eps)
    pair = y.view(b, l, c // 2, 2).abs().sum(-1, keepdim=True).expand(b, l, c // 2, 2).reshape(b, l, c)
    if rope:
        y = O.rope_apply(y.view(b, l, c // hd, hd), GRID, O.rope_angles(1024, hd)).reshape(b, l, c)
    return y, 2.0 ** -20 * pair + 1e-30


def chunk(t):
    """[B, L, ...] -> the [B * LC, ...] rows of tokens TOK0 .. TOK0 + LC."""
    return t[:, TOK0:TOK0 + LC].reshape(B * LC, *t.shape[2:])


RMS_CASES = [(3072, 128), (3072, 64), (5120, 128), (5120, 64)]


@pytest.mark.parametrize("c,hd", RMS_CASES, ids=[f"VPT{-(-c // 1024) if c <= 4096 else 8}-C{c}-hd{hd}" for c, hd in RMS_CASES])
def test_rmsnorm_rope_chunk_of_the_sequence(H, c, hd):
    """flexam_rmsnorm_rope, rmsnorm_rope_kernel<VPT, false> (VPT 3 at C = 3072, 8 at 5120), on a rank's chunk of two sequences:
    tokens_per_batch = 11 < M = 22 rows, token_offset = 16, so row m rotates by global token 16 + m % 11 -- compared with the float64
    oracle applied to the whole sequences, which the in-place scatter test cannot do.  q and k in place as column slices of one
    [M, 3C] qkv buffer (ld = 3C); q alone with RoPE (the self-attention q of the all-gather mode, dit_engine.py:943) out of place into a
    strided buffer; q and k out of place without RoPE; q alone in place without RoPE (cross-attention)."""
    from flexam_amd.rope import rope_tables
    g = torch.Generator().manual_seed(c + hd)
    q = (torch.randn(B, L, c, generator=g, dtype=F64) * 1.5).to(BF)
    k = torch.randn(B, L, c, generator=g, dtype=F64).to(BF)
    v = torch.randn(B, L, c, generator=g, dtype=F64).to(BF)
    wq, wk = (1 + 0.1 * torch.randn(c, generator=g)), (1 + 0.1 * torch.randn(c, generator=g))
    cos, sin = (t.to(dev()) for t in rope_tables(GRID, L, hd))
    wqd, wkd = wq.to(dev()), wk.to(dev())
    ref = {(t, r): rope_ref(x.float(), w, hd, r) for t, x, w in (("q", q, wq), ("k", k, wk)) for r in (True, False)}
    want = lambda t, r: (chunk(ref[t, r][0]), chunk(ref[t, r][1]))       # noqa: E731
    qkv0 = torch.cat([chunk(q), chunk(k), chunk(v)], 1).to(dev())
    rope = dict(rope_cos=cos, rope_sin=sin, tokens_per_batch=LC, token_offset=TOK0, head_dim=hd)

    qkv = qkv0.clone()
    H.rmsnorm_rope(qkv[:, :c], wqd, qkv[:, c:2 * c], wkd, **rope)
    close(qkv[:, :c], *want("q", True), msg="q, in place")
    close(qkv[:, c:2 * c], *want("k", True), msg="k, in place")
    assert torch.equal(qkv[:, 2 * c:], qkv0[:, 2 * c:]), "v was touched"

    qkv = qkv0.clone()
    obuf, qo = padded(B * LC, c, 8, BF, SENT)
    H.rmsnorm_rope(qkv[:, :c], wqd, **rope, q_out=qo)
    close(qo, *want("q", True), msg="q alone, out of place")
    keeps(obuf, c, SENT, "q alone")
    assert torch.equal(qkv, qkv0), "the input was written"

    obuf, qo = padded(B * LC, c, 8, BF, SENT)
    kbuf, ko = padded(B * LC, c, 24, BF, SENT)
    H.rmsnorm_rope(qkv[:, :c], wqd, qkv[:, c:2 * c], wkd, q_out=qo, k_out=ko)
    close(qo, *want("q", False), msg="q, no rope, out of place")
    close(ko, *want("k", False), msg="k, no rope, out of place")
    keeps(obuf, c, SENT, "q no rope")
    keeps(kbuf, c, SENT, "k no rope")
    assert torch.equal(qkv, qkv0), "the input was written"

    H.rmsnorm_rope(qkv[:, :c], wqd)
    close(qkv[:, :c], *want("q", False), msg="q alone, no rope, in place")


def scatter_expect(dst_numel, vals, base, ld_out, out_bs, cb, bs):
    """The cells flexam_hip.h's address formula names: (m, col) -> base + (m // LC) out_bs + (m % LC) ld_out + (col // cb) bs
    + col % cb, as flat indices [M, C] of the destination buffer."""
    m = torch.arange(vals.shape[0])[:, None]
    col = torch.arange(vals.shape[1])[None]
    idx = base + (m // LC) * out_bs + (m % LC) * ld_out + (col // cb) * bs + col % cb
    assert int(idx.max()) < dst_numel
    return idx


@pytest.mark.parametrize("layout", ["a2a-sp2", "a2a-sp3", "a2a-sp4", "half-head-blocks"])
def test_rmsnorm_rope_scatter_against_float64(H, layout):
    """flexam_rmsnorm_rope_scatter, rmsnorm_rope_kernel<3, true> (C = 3072, head_dim 128), against the float64 oracle of the whole
    sequences (not against the in-place kernel): the all-to-all send layout [B, sp, lc, 3G] for sp = 2, 3, 4 (G = C / sp: 12, 8, 6
    heads per rank), and a gapped layout whose column block is half a head (64 columns: the kernel only needs C % col_block == 0 and
    col_block % 8 == 0) with q absent.  Every destination cell the address formula does not name keeps its sentinel; v is copied
    bit for bit."""
    from flexam_amd.rope import rope_tables
    c, hd = 3072, 128
    g = torch.Generator().manual_seed(len(layout) * 31)
    q = (torch.randn(B, L, c, generator=g, dtype=F64) * 1.5).to(BF)
    k = torch.randn(B, L, c, generator=g, dtype=F64).to(BF)
    v = torch.randn(B, L, c, generator=g, dtype=F64).to(BF)
    wq, wk = (1 + 0.1 * torch.randn(c, generator=g)), (1 + 0.1 * torch.randn(c, generator=g))
    cos, sin = (t.to(dev()) for t in rope_tables(GRID, L, hd))
    qkv = torch.cat([chunk(q), chunk(k), chunk(v)], 1).to(dev())
    rope = dict(rope_cos=cos, rope_sin=sin, tokens_per_batch=LC, token_offset=TOK0, head_dim=hd)
    if layout.startswith("a2a"):
        sp = int(layout[-1])
        G = c // sp
        ld_out, cb, bs = 3 * G, G, LC * 3 * G
        out_bs = sp * bs
        dst = torch.full((B * out_bs,), SENT, dtype=BF, device=dev())
        H.rmsnorm_rope_scatter(qkv[:, :c], wq.to(dev()), qkv[:, c:2 * c], wk.to(dev()), qkv[:, 2 * c:], dst, dst[G:], dst[2 * G:],
                               ld_out=ld_out, out_bs=out_bs, col_block=cb, block_stride=bs, **rope)
        parts = (("q", 0, wq), ("k", G, wk), ("v", 2 * G, None))
    else:
        cb, bs = 64, 72                                     # a 64-column block every 72 elements
        ld_out = (c // cb) * bs + 8
        out_bs = LC * ld_out + 16
        dst = torch.full((2 * (B * out_bs + 8),), SENT, dtype=BF, device=dev())
        vo = B * out_bs + 8
        H.rmsnorm_rope_scatter(None, None, qkv[:, c:2 * c], wk.to(dev()), qkv[:, 2 * c:], None, dst, dst[vo:], ld_out=ld_out,
                               out_bs=out_bs, col_block=cb, block_stride=bs, **rope)
        parts = (("k", 0, wk), ("v", vo, None))
    got = dst.cpu()
    named = torch.zeros(got.numel(), dtype=torch.bool)
    for t, base, w in parts:
        src = {"q": q, "k": k, "v": v}[t]
        idx = scatter_expect(got.numel(), chunk(src), base, ld_out, out_bs, cb, bs)
        assert not bool(named[idx].any()), "two tensors map to one cell"
        named[idx] = True
        if w is None:
            assert torch.equal(got[idx], chunk(src)), f"{layout}: v copy"
        else:
            want, slack = rope_ref(src.float(), w, hd, True)
            close(got[idx], chunk(want), chunk(slack), msg=f"{layout}: {t}")
    assert torch.equal(got[~named], torch.full((int((~named).sum()),), SENT, dtype=BF)), f"{layout}: an unnamed cell was written"


# ----------------------------------------------------------------------------- gate_residual
@pytest.mark.parametrize("c,m", [(3072, 37), (1032, 29), (3072, 2912)])
def test_gate_residual_every_row_form(H, c, m):
    """flexam_gate_residual (one instance; the grid-stride loop runs several rounds at M = 2912, C = 3072, past 4096 x 256 vectors):
    x += y * gate[row] with the gate row from row_index (a permutation of a table of M rows), from m // rows_per_batch, and with
    gate = None; x and y are strided views (y a column slice of a [M, 3C] bf16 buffer).  Integer x, y in multiples of 1/2 and gates in
    {0, +-1/4, +-1/2, +-1, +-2}: every product and sum is exact, so the result is held to torch.equal."""
    g = torch.Generator().manual_seed(c + m)
    x0 = torch.randint(-64, 65, (m, c), generator=g).float()
    y = (torch.randint(-16, 17, (m, 3 * c), generator=g).float() / 2).to(BF)
    gates = torch.tensor([0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    tab = gates[torch.randint(0, 9, (m, c), generator=g)]
    perm = torch.randperm(m, generator=g).to(torch.int32)
    yd, tabd = y.to(dev()), tab.to(dev())
    yv = yd[:, c:2 * c]
    yf = y[:, c:2 * c].float()
    rpb = 10
    cases = [("row_index", dict(gate=tabd, row_index=perm.to(dev())), tab[perm.long()]),
             ("rows_per_batch", dict(gate=tabd, rows_per_batch=rpb), tab[torch.arange(m) // rpb]),
             ("no gate", dict(), torch.ones(m, c))]
    for what, kw, gate in cases:
        xbuf, xd = padded(m, c, 4, F32, -7.0)
        xd.copy_(x0)
        H.gate_residual(xd, yv, **kw)
        assert torch.equal(xd.cpu(), x0 + yf * gate), f"gate_residual C={c} M={m} {what}"
        keeps(xbuf, c, -7.0, f"gate_residual {what}")


# ----------------------------------------------------------------------------- small_linear
def small_linear_ref(x, w, b, silu):
    """float64 silu?(x) @ w^T + b and the slack: (K / 64 + 16) fp32 ulps of sum_k |t_k w_nk| + |b_n| (the per-lane partial sums run
    K / 256 x 4 terms, then a 64-lane tree; SiLU's exp and division add a few ulps of each term)."""
    t = x.double()
    if silu:
        t = F.silu(t)
    y = t @ w.double().t() + (b.double() if b is not None else 0.0)
    mag = t.abs() @ w.double().abs().t() + (b.double().abs() if b is not None else 0.0)
    return y, (x.shape[1] / 64 + 16) * 2.0 ** -24 * mag + 1e-30


@pytest.mark.parametrize("m", [1, 8, 9, 32])
@pytest.mark.parametrize("wdt", [F32, BF], ids=["f32w", "bf16w"])
def test_small_linear_both_instances(H, m, wdt):
    """flexam_small_linear_f32: M = 1, 8 take small_linear_kernel<WT, 8, 1> (one output per wave), M = 9, 32 take <WT, 32, 4> (four
    outputs per wave) -- both edges of each.  K = 256, 260 (the lanes' last k step is partial) and 3072; N = 771 and 13 (not multiples
    of 4 or 16: the last wave's outputs past N read the clamped row N - 1 and are not stored); with and without bias and SiLU; x a
    strided view, out a strided view whose pad keeps its sentinel.  For M > 8, every output equals the <WT, 8, 1> instance's on the
    same row bit for bit (a row's embedding does not depend on how many rows share the launch)."""
    g = torch.Generator().manual_seed(m * 10 + (wdt == BF))
    combos = [(True, True), (False, True), (True, False), (False, False)]
    for i, (k, n) in enumerate([(256, 771), (260, 13), (3072, 771), (260, 771)]):
        for bias, silu in combos[i:] + combos[:i]:
            x = torch.randn(m, k, generator=g) * 2
            w = (torch.randn(n, k, generator=g) / math.sqrt(k)).to(wdt)
            b = torch.randn(n, generator=g) if bias else None
            _, xd = padded(m, k, 4, F32, math.nan)
            xd.copy_(x)
            obuf, out = padded(m, n, 3, F32, -7.0)
            wd, bd = w.to(dev()), (b.to(dev()) if bias else None)
            H.small_linear(xd, wd, bd, silu_in=silu, out=out)
            want, slack = small_linear_ref(x, w, b, silu)
            what = f"small_linear M={m} K={k} N={n} bias={bias} silu={silu}"
            close(out, want, slack, ulps=0.0, msg=what)
            keeps(obuf, n, -7.0, what)
            if m > 8:
                narrow = torch.cat([H.small_linear(xd[r:r + 8], wd, bd, silu_in=silu) for r in range(0, m, 8)])
                assert torch.equal(out, narrow), f"{what}: the 32-row instance differs from the 8-row one"


def test_small_linear_time_mlp_shapes(H):
    """The time-embedding MLP's shapes (FX.py:928-944): 256 -> 3072 with SiLU out (the next layer's silu_in) and 3072 -> 18432
    (the 6 x 3072 projection), bf16 weights, M = 2 and M = 17 timesteps -- both instances at the model's K and N."""
    g = torch.Generator().manual_seed(44)
    w1, b1 = (torch.randn(3072, 256, generator=g) / 16).to(BF), torch.randn(3072, generator=g) * 0.1
    w2, b2 = (torch.randn(18432, 3072, generator=g) / 55).to(BF), torch.randn(18432, generator=g) * 0.1
    w1d, b1d, w2d, b2d = w1.to(dev()), b1.to(dev()), w2.to(dev()), b2.to(dev())
    for m in (2, 17):
        x = torch.randn(m, 256, generator=g) * 3
        h = H.small_linear(x.to(dev()), w1d, b1d)
        want, slack = small_linear_ref(x, w1, b1, False)
        close(h, want, slack, ulps=0.0, msg=f"time MLP 256->3072 M={m}")
        e = H.small_linear(h, w2d, b2d, silu_in=True)
        want, slack = small_linear_ref(h.cpu(), w2, b2, True)
        close(e, want, slack, ulps=0.0, msg=f"time MLP 3072->18432 M={m}")


# ----------------------------------------------------------------------------- patchify / unpatchify
def patch_ref(src):
    """[C, F, H, W] -> [(f, h/2, w/2), c*4 + ph*2 + pw] (FX.py:624-625, 676; odd H / W drop their last row / column)."""
    c, f, h, w = src.shape
    s = src[:, :, :h // 2 * 2, :w // 2 * 2].reshape(c, f, h // 2, 2, w // 2, 2)
    return s.permute(1, 2, 4, 0, 3, 5).reshape(f * (h // 2) * (w // 2), c * 4)


@pytest.mark.parametrize("sdt", [F32, BF], ids=["f32src", "bf16src"])
@pytest.mark.parametrize("c,f,h,w,col0,row0", [(16, 2, 8, 12, 0, 0), (48, 3, 10, 14, 40, 7), (5, 2, 9, 13, 8, 3)])
def test_patchify_into_a_larger_destination(H, sdt, c, f, h, w, col0, row0):
    """flexam_patchify, patchify_kernel<float> / <bf16>: written at column col0, row row0 of a wider, taller bf16 destination whose
    other cells keep their sentinel; odd H / W drop the last row / column.  Bit-exact (a cast to bf16 is one rounding)."""
    g = torch.Generator().manual_seed(c * f + h + w)
    src = (torch.randn(c, f, h, w, generator=g) * 3).to(sdt)
    want = patch_ref(src).to(BF)
    rows, cols = want.shape
    dst = torch.full((row0 + rows + 2, col0 + cols + 16), SENT, dtype=BF, device=dev())
    H.patchify(src.to(dev()), dst, col0=col0, row0=row0)
    expect = torch.full(dst.shape, SENT, dtype=BF)
    expect[row0:row0 + rows, col0:col0 + cols] = want
    assert torch.equal(dst.cpu(), expect)


@pytest.mark.parametrize("odt", [F32, BF], ids=["f32out", "bf16out"])
def test_unpatchify_strided_tokens(H, odt):
    """flexam_unpatchify, unpatchify_kernel<float> / <bf16>: token rows from tok0 = 5 of a buffer with row pitch 4C + 12; bit-exact
    against oracle.dit.unpatchify (then one rounding to bf16)."""
    g = torch.Generator().manual_seed(61)
    c, f, h, w, tok0 = 48, 3, 8, 12, 5
    n = f * (h // 2) * (w // 2)
    tb = torch.randn(tok0 + n, 4 * c + 12, generator=g) * 5
    got = H.unpatchify(tb.to(dev())[:, :4 * c], tok0, c, f, h, w, dtype=odt)
    want = O.unpatchify(tb[tok0:, :4 * c], (f, h // 2, w // 2), (1, 2, 2), c).to(odt)
    assert got.dtype == odt and torch.equal(got.cpu(), want)


# ----------------------------------------------------------------------------- sampler-step helpers
def cfg_ref(tu, tc, tok0, g, c, f, h, w):
    vu = O.unpatchify(tu[tok0:].double(), (f, h // 2, w // 2), (1, 2, 2), c)
    if tc is None:
        return vu, vu.abs()
    vc = O.unpatchify(tc[tok0:].double(), (f, h // 2, w // 2), (1, 2, 2), c)
    return vu + g * (vc - vu), vu.abs() + g * (vc - vu).abs()


@pytest.mark.parametrize("w", [168, 172], ids=["tiled-W168", "gather-lds-limit-W172"])
def test_cfg_step_at_the_lds_limit(H, w):
    """flexam_cfg_euler_blend / flexam_cfg_velocity with C = 48 and 16-byte aligned token rows: at W = 168 the [W/2][4C+1] fp32 tile
    is 64,848 B and cfg_euler_blend_tiled_kernel runs; at W = 172 it would be 66,392 B > 64 KiB, so the launcher takes the gather
    form cfg_euler_blend_kernel although the rows are aligned.  Both against float64, within a few fp32 ulps of the magnitudes."""
    g = torch.Generator().manual_seed(w)
    c, f, h, tok0, gd, dt = 48, 2, 4, 3, 5.5, -0.0371
    n = f * (h // 2) * (w // 2)
    tu, tc = torch.randn(tok0 + n, 4 * c, generator=g), torch.randn(tok0 + n, 4 * c, generator=g)
    lat, known = torch.randn(c, f, h, w, generator=g), torch.randn(c, f, h, w, generator=g)
    mask = torch.rand(f, h, w, generator=g)
    mask[0, 0] = 0
    mask[1, 1] = 1
    v, vmag = cfg_ref(tu, tc, tok0, gd, c, f, h, w)
    for cond in (True, False):
        vv, vm = (v, vmag) if cond else cfg_ref(tu, None, tok0, gd, c, f, h, w)
        vel = torch.full((c, f, h, w), math.nan, device=dev())
        H.cfg_velocity(tu.to(dev()), tc.to(dev()) if cond else None, tok0, gd, vel)
        close(vel, vv, 2.0 ** -21 * vm + 1e-30, ulps=0.0, msg=f"cfg_velocity W={w} cfg={cond}")
        ld = lat.clone().to(dev())
        H.cfg_euler_blend(tu.to(dev()), tc.to(dev()) if cond else None, tok0, gd, dt, ld, known.to(dev()), mask.to(dev()))
        x = lat.double() + dt * vv
        want = (1 - mask.double()) * known.double() + mask.double() * x
        mag = known.double().abs() + lat.double().abs() + abs(dt) * vm
        close(ld, want, 2.0 ** -21 * mag + 1e-30, ulps=0.0, msg=f"cfg_euler_blend W={w} cfg={cond}")


def exact_vals(g, n, lim=64):
    """fp32 values that are integers / 4: with power-of-two coefficients every product and sum below is exact."""
    return torch.randint(-lim * 4, lim * 4 + 1, (n,), generator=g).float() / 4


GRID_ELEMS = 4 * 4096 * 256          # elements one pass of lincomb / axpby's capped grid (4096 x 256 threads, 4 floats each) covers


@pytest.mark.parametrize("n", [4, 4 * 1001, GRID_ELEMS + 4], ids=["n4", "n4004", "grid+4"])
def test_lincomb_every_term_count_and_alias(H, n):
    """flexam_lincomb_f32 (lincomb_kernel) with 1..8 terms, out a fresh buffer, out aliasing the FIRST term and out aliasing the LAST
    term; n = 4, an odd multiple of 4 (4004), and one vector past a full pass of the capped grid (the grid-stride loop's second
    round).  Exact data and power-of-two coefficients: bit-exact against float64."""
    g = torch.Generator().manual_seed(n % 997)
    coefs = [0.5, -2.0, 1.0, 0.25, -1.0, 4.0, -0.125, 2.0]
    xs = [exact_vals(g, n) for _ in range(8)]
    xd = [x.to(dev()) for x in xs]
    for t in range(1, 9):
        want = sum(coefs[i] * xs[i].double() for i in range(t)).float()
        out = torch.full((n,), math.nan, device=dev())
        H.lincomb(out, [(coefs[i], xd[i]) for i in range(t)])
        assert torch.equal(out.cpu(), want), f"lincomb {t} terms"
        for alias in ({0, t - 1} if n < 10 ** 6 or t == 8 else {t - 1}):
            terms = [(coefs[i], xd[i].clone() if i == alias else xd[i]) for i in range(t)]
            H.lincomb(terms[alias][1], terms)
            assert torch.equal(terms[alias][1].cpu(), want), f"lincomb {t} terms, out = term {alias}"


@pytest.mark.parametrize("n", [4, GRID_ELEMS + 4], ids=["n4", "grid+4"])
def test_axpby_and_mask_blend_exact(H, n):
    """flexam_axpby_f32 (axpby_kernel): y = a x + b y with b = 0, with a = 0 and with both nonzero; flexam_mask_blend_f32 with masks
    in {0, 1/4, 1/2, 1}.  Exact data: bit-exact against float64."""
    g = torch.Generator().manual_seed(n % 991)
    x, y = exact_vals(g, n), exact_vals(g, n)
    xd = x.to(dev())
    for a, b in ((2.0, 0.0), (0.0, -0.5), (0.25, 4.0), (-1.0, 1.0)):
        yd = y.to(dev())
        H.axpby(yd, a, xd, b)
        assert torch.equal(yd.cpu(), (a * x.double() + b * y.double()).float()), f"axpby a={a} b={b}"
    c = 3
    fhw = max(n // c // 4 * 4, 4)
    xs, kn = exact_vals(g, c * fhw).view(c, fhw), exact_vals(g, c * fhw).view(c, fhw)
    mk = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (fhw,), generator=g)]
    xm = xs.to(dev())
    H.mask_blend(xm, kn.to(dev()), mk.to(dev()))
    assert torch.equal(xm.cpu(), ((1 - mk.double()) * kn.double() + mk.double() * xs.double()).float()), "mask_blend"


# ----------------------------------------------------------------------------- checksum
def device_bytes(t):
    return t.contiguous().cpu().view(-1).view(U8).numpy().tobytes()


def test_checksum_matches_the_restatement_bit_for_bit(H):
    """flexam_checksum (checksum_kernel) against tests/checksum_restatement.py on byte buffers of 1, 3, 4, 5, 4097 and 2^20 + 3 bytes
    (a tail of 0..3 bytes after the words; the large one runs the grid-stride loop), on bf16, fp32 and int64 tensors, and
    flexam_amd.hip.checksums of several tensors against separate checksum calls."""
    g = torch.Generator().manual_seed(71)
    store = torch.randint(0, 256, ((1 << 20) + 64,), generator=g, dtype=torch.int32).to(U8).to(dev())
    for n in (1, 3, 4, 5, 4097, (1 << 20) + 3):
        t = store[:n]                                      # 16-byte aligned base: the kernel needs 4
        assert H.checksum(t) == CR.checksum(device_bytes(t)), f"{n} bytes"
    ts = [torch.randn(7, 33, generator=g).to(BF).to(dev()), torch.randn(1001, generator=g).to(dev()),
          torch.randint(-2 ** 62, 2 ** 62, (77,), generator=g, dtype=torch.int64).to(dev()), store[:9]]
    for t in ts:
        assert H.checksum(t) == CR.checksum(device_bytes(t)), str(t.dtype)
    assert H.checksums(ts) == [H.checksum(t) for t in ts]


def test_checksum_sensitivity(H):
    """What the conditioning cache relies on (wan_transformer3d_FlexAM.py:598-614): any one of 64 sampled flipped bits changes the
    sum, two distinct words swapped change it, and a buffer with one more zero byte differs from the buffer."""
    g = torch.Generator().manual_seed(72)
    buf = torch.randint(0, 256, (4100,), generator=g, dtype=torch.int32).to(U8).to(dev())
    base = H.checksum(buf[:4097])
    for bit in torch.randperm(4097 * 8, generator=g)[:64].tolist():
        b = buf[:4097].clone()
        b[bit // 8] ^= 1 << (bit % 8)
        assert H.checksum(b) != base, f"bit {bit}"
    words = buf[:4096].view(torch.int32).clone()
    assert words[3] != words[900]
    words[3], words[900] = words[900].clone(), words[3].clone()
    sw = torch.cat([words.view(U8), buf[4096:4097]])
    assert H.checksum(sw) != base
    z = buf[:4098].clone()
    z[4097] = 0
    assert H.checksum(z) != base
