"""Every instance of the fp8 GEMM (csrc/gemm_fp8.hip: gemm_fp8_kernel<EPI, MT>, EPI in {NONE, GELU, GATE_RESIDUAL, GELU_Q} x MT in 4..7,
each with its interior and its bounds-checked boundary path) and the row quantiser, against restatements of their arithmetic.

Operands are small integers (exact in e4m3) with power-of-two scales and bias on a 1/4 grid, so the pre-epilogue value
y = acc sa sw + b is exact in float32 and:
  NONE           out = bf16(y), bit for bit;
  GATE_RESIDUAL  x = fp32(x0 + bf16(y) g), bit for bit (one rounding of an exact value), with the gate taken per row (gate_row), per
                 batch of rows (rows_per_batch) or not at all;
  GELU           out within 1 bf16 ulp of bf16(gelu_tanh(y)) evaluated in float64 (where |gelu(y)| < 2^-100, i.e. y < -10, the device's
                 exp2 may overflow to a signed zero: both sides must be below that);
  GELU_Q         byte = e4m3(fp32(gelu64(y)) / so) with power-of-two row scales so; the neighbouring code is accepted only where that
                 value lies within 2^-20 + 2^-22 |t| (relative) of the midpoint between the two codes, t = y (a + b y^2) the exponent
                 of the device's gelu_tanh (csrc/common.h): float32 rounding of t moves its exp2 by |t| 2^-23 ln 2 relative.
Views are slices of wider buffers whose margins (and the pad columns right of N) hold sentinels that must survive.
The quantiser: s = fp32(amax fp32(1/448)) (1 for a zero row), inv = fp32(1 / s), byte = e4m3(fp32(x inv)) -- scales and bytes exact."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp8_restatement as R  # noqa: E402
from gemm_checks import _bf16_ulp, _gelu64, _margins_untouched, _strided, dev  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GA, GB = -2.302208198, -0.1029432396          # gelu_tanh's exp2 exponent t = y (GA + GB y^2)


@pytest.fixture(scope="module")
def H():
    from flexam_amd import hip
    hip.device_check()
    return hip


def _e4m3_bytes(x_int):
    return x_int.float().to(torch.float8_e4m3fn).view(torch.uint8)


def _case(m, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-2, 3, (m, k), generator=g)
    w = torch.randint(-2, 3, (n, k), generator=g)
    sa = torch.pow(2.0, torch.randint(-4, 0, (m,), generator=g).float())
    sw = torch.pow(2.0, torch.randint(-3, 1, (n,), generator=g).float()) * (2.0 if k <= 128 else 1.0 if k <= 384 else 0.25)
    b = torch.randint(-8, 9, (n,), generator=g).float() / 4
    return a, w, sa, sw, b, g


def _shapes(mt):
    bm = 32 * mt
    return [(3 * bm + 17, 388, 128), (2 * bm - 5, 388, 384), (bm + 40, 644, 3072), (30 * bm + 5, 2180, 128)]      # last: 279 tiles > 256 CUs


@pytest.mark.parametrize("shape_i", range(4))
@pytest.mark.parametrize("mt", [4, 5, 6, 7])
def test_every_fp8_gemm_instance_is_exact(H, mt, shape_i, monkeypatch):
    monkeypatch.setenv("FLEXAM_GEMM_MT", str(mt))
    m, n, k = _shapes(mt)[shape_i]
    a, w, sa, sw, b, g = _case(m, n, k, 1000 * mt + shape_i)
    # operands: slices of wider buffers whose margins hold 0x7F (e4m3 NaN: a stray read would poison the product)
    abuf, a8 = _strided(m, k, k + 64, torch.uint8, 0x7F)
    wbuf, w8 = _strided(n, k, k + 32, torch.uint8, 0x7F)
    a8.copy_(_e4m3_bytes(a).to(dev()))
    w8.copy_(_e4m3_bytes(w).to(dev()))
    sa_d, sw_d = sa.to(dev()), sw.to(dev())
    bias = None if shape_i == 1 else b.to(dev())
    acc = a.to(dev()).double() @ w.to(dev()).double().t()
    y = acc * sa_d.double()[:, None] * sw_d.double()[None, :] + (0.0 if bias is None else bias.double())
    assert bool((y.float().double() == y).all())                          # exact in float32
    ld_c = (n + 40 + 7) // 8 * 8

    # NONE
    cbuf, c = _strided(m, n, ld_c, BF, 1234.0, c0=8)
    H.gemm_fp8(a8, sa_d, w8, sw_d, bias, out=c)
    assert torch.equal(c.float(), y.float().to(BF).float()), "EPI_NONE differs from bf16(y)"
    assert _margins_untouched(cbuf, m, n, 1234.0, c0=8)

    # GELU
    cbuf, c = _strided(m, n, ld_c, BF, 1234.0, c0=8)
    H.gemm_fp8(a8, sa_d, w8, sw_d, bias, out=c, epilogue=H.EPI_GELU_TANH)
    want = _gelu64(y).float().to(BF).double()
    got = c.double()
    tiny = want.abs() < 2.0 ** -100
    bad = ((got - want).abs() > _bf16_ulp(want)) & ~(tiny & (got.abs() < 2.0 ** -100))
    assert not bad.any(), f"EPI_GELU: {int(bad.sum())} outputs more than 1 bf16 ulp from gelu64; first y = {float(y[bad][0])}"
    assert _margins_untouched(cbuf, m, n, 1234.0, c0=8)

    # GATE_RESIDUAL: no gate, a gate row per output row, a gate row per batch of rows
    nb = 3
    gate = (torch.randint(-4, 5, (nb, n), generator=g).float() / 2).to(dev())
    rows = torch.randint(0, nb, (m,), generator=g, dtype=torch.int32).to(dev())
    rpb = -(-m // nb)
    x0 = torch.randint(-5, 6, (m, n), generator=g).float().to(dev())
    ybf = y.float().to(BF).double()
    ld_x = (n + 40 + 3) // 4 * 4
    for form in ("none", "gate_row", "rows_per_batch"):
        xbuf, x = _strided(m, n, ld_x, torch.float32, -7.5, c0=4)
        x.copy_(x0)
        if form == "none":
            H.gemm_fp8_gate_residual(a8, sa_d, w8, sw_d, bias, x)
            want = x0.double() + ybf
        elif form == "gate_row":
            H.gemm_fp8_gate_residual(a8, sa_d, w8, sw_d, bias, x, gate, rows)
            want = x0.double() + ybf * gate.double()[rows.long()]
        else:
            H.gemm_fp8_gate_residual(a8, sa_d, w8, sw_d, bias, x, gate, None, rows_per_batch=rpb)
            want = x0.double() + ybf * gate.double()[torch.arange(m, device=dev()) // rpb]
        assert torch.equal(x, want.float()), f"EPI_GATE_RESIDUAL ({form}) differs from fp32(x0 + bf16(y) g)"
        assert _margins_untouched(xbuf, m, n, -7.5, c0=4)

    # GELU_Q: power-of-two output row scales that keep every value inside e4m3's range
    so = torch.pow(2.0, torch.ceil(torch.log2(y.abs().amax(dim=1).cpu().float().clamp_min(1.0) / 448.0)) +
                   torch.randint(0, 3, (m,), generator=g).float()).to(dev())
    ld_q = (n + 48 + 15) // 16 * 16
    qbuf, q = _strided(m, n, ld_q, torch.uint8, 0x5A)
    H.gemm_fp8_gelu_q(a8, sa_d, w8, sw_d, bias, so, q)
    val = (_gelu64(y).float().double() / so.double()[:, None]).float()
    want_c = R.e4m3_code(val.cpu())
    got_c = q.cpu()
    diff = got_c != want_c
    if diff.any():
        v = val.cpu().double()[diff]
        gv, wv = R.e4m3_value(got_c[diff]), R.e4m3_value(want_c[diff])
        t = y.cpu()[diff] * (GA + GB * y.cpu()[diff] ** 2)
        tol = 2.0 ** -20 + 2.0 ** -22 * t.abs()
        adjacent = ((got_c[diff].long() & 127) - (want_c[diff].long() & 127)).abs() == 1
        same_sign = (got_c[diff] & 128) == (want_c[diff] & 128)
        near_mid = (v - (gv + wv) / 2).abs() <= tol * v.abs()
        ok = adjacent & same_sign & near_mid
        print(f"MT={mt} {m}x{n}x{k} GELU_Q: {int(diff.sum())} neighbouring codes at midpoints")
        assert bool(ok.all()), (f"EPI_GELU_Q: {int((~ok).sum())} bytes differ from e4m3(gelu64(y) / so); first: value {float(v[~ok][0])}, "
                                f"got {float(gv[~ok][0])}, want {float(wv[~ok][0])}")
    assert _margins_untouched(qbuf, m, n, 0x5A)


# ----------------------------------------------------------------------------- the row quantiser
def _quantise_restated(x):
    """x [M, K] bf16 (CPU) -> (codes uint8 [M, K], s float32 [M]) by the kernel's float32 arithmetic."""
    xf = x.float()
    amax = xf.abs().amax(dim=1)
    s = torch.where(amax > 0, amax * torch.tensor(1.0 / 448.0, dtype=torch.float32), torch.ones_like(amax))
    inv = torch.ones_like(s) / s
    return R.e4m3_code(xf * inv[:, None]), s


@pytest.mark.parametrize("m,k", [(37, 8), (301, 520), (260, 3072), (70, 14336), (262200, 8)])
def test_quantize_rows_fp8_is_exact(H, m, k):
    g = torch.Generator().manual_seed(m + k)
    x = torch.randn(m, k, generator=g) * torch.pow(2.0, torch.randint(-20, 12, (m, 1), generator=g).float())
    sub = torch.rand(m, k, generator=g) < 0.3                        # entries 2^-12 .. 2^-21 of the row maximum: e4m3 subnormals and zeros
    x = torch.where(sub, x * torch.pow(2.0, -torch.randint(12, 22, (m, k), generator=g).float()), x)
    x[min(5, m - 1)] = 0.0                                          # an all-zero row: scale 1
    x[min(6, m - 1), 0] = 448.0                                     # s = fp32(448 fp32(1/448))
    x = x.to(BF)
    want_q, want_s = _quantise_restated(x)
    xbuf, xv = _strided(m, k, k + 8, BF, 3.0, c0=8)
    xv.copy_(x.to(dev()))
    qbuf, qv = _strided(m, k, k + 16, torch.uint8, 0xA5)
    s = torch.full((m,), -1.0, device=dev())
    H.quantize_rows_fp8(xv, qv, s)
    assert torch.equal(s.cpu(), want_s), "row scales differ from fp32(amax * fp32(1/448))"
    got = qv.cpu()
    bad = got != want_q
    if bad.any():
        i = bad.nonzero()[0].tolist()
        xi = float(x[i[0], i[1]])
        raise AssertionError(f"{int(bad.sum())} bytes differ from e4m3(fp32(x * fp32(1/s))); first at {i}: x {xi}, "
                             f"x * inv {float(x.float()[i[0], i[1]] / want_s[i[0]])}, got {int(got[i[0], i[1]])}, want {int(want_q[i[0], i[1]])}")
    assert _margins_untouched(qbuf, m, k, 0xA5)
    sub_codes = (want_q & 127) < 8
    print(f"M={m} K={k}: {int((sub_codes & (want_q & 127 > 0)).sum())} subnormal codes, {int((want_q & 127 == 0).sum())} zeros")
