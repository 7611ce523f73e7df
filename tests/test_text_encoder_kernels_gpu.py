"""GPU: the umT5 encoder's own kernels (csrc/text_encoder.hip) called directly at umT5-XXL's sizes (oracle/t5.py: dim 4096, ffn 10240,
64 heads, text length <= 512), against float64 restatements of T5LayerNorm, the biased masked softmax and the gate product
(wan_text_encoder.py:44-56, 91-103, 125-126).  test_text_encoder_gpu.py reaches them only through the whole encoder at hidden width
128 / 256 and rel-RMS 2e-2.  Tolerances as test_dit_row_kernels_gpu.py: 1 bf16 ulp plus the fp32 rounding that enters, a few fp32 ulps
for fp32 outputs, bit-exact for the product."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = 12352.0


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def H():
    from flexam_amd import hip
    hip.device_check()
    return hip


def close(got, want, slack, ulps=1.0, msg=""):
    got, want = got.double().cpu(), want.double().cpu()
    err = (got - want).abs()
    tol = ulps * 2.0 ** -8 * want.abs() + slack
    bad = ~(err <= tol)
    assert not bool(bad.any()), f"{msg}: {int(bad.sum())}/{bad.numel()} off, worst err {float(err.nan_to_num(math.inf).max()):.4g}"


def test_t5_norm_at_xxl_width(H):
    """flexam_t5_norm at C = 4096, t5_norm_kernel<float> and <bf16>, from a strided x (row pitch 4100) into strided outputs whose pads
    keep their sentinel: w * x * rsqrt(mean(x^2) + eps) in float64.  fp32 output within 2^-19 relative (the row sum of 4096 squares and
    rsqrtf); bf16 output within 1 bf16 ulp plus that."""
    g = torch.Generator().manual_seed(81)
    m, c, eps = 67, 4096, 1e-6
    x = torch.randn(m, c, generator=g) * 3 + 0.25
    x[5] *= 1e-3                                          # a row where eps matters: mean(x^2) ~ 1e-5
    w = 1 + 0.3 * torch.randn(c, generator=g)
    xb = torch.full((m, c + 4), math.nan, device=dev())
    xb[:, :c] = x.to(dev())
    x64 = x.double()
    want = w.double() * x64 * (x64.pow(2).mean(1, keepdim=True) + eps).rsqrt()
    for dt, pad in ((F32, 4), (BF, 8)):
        ob = torch.full((m, c + pad), SENT, dtype=dt, device=dev())
        H.t5_norm(xb[:, :c], w.to(dev()), ob[:, :c], eps=eps)
        close(ob[:, :c], want, 2.0 ** -19 * want.abs() + 1e-30, ulps=1.0 if dt == BF else 0.0, msg=f"t5_norm {dt}")
        assert bool((ob[:, c:] == SENT).all()), "t5_norm wrote past the row"


def softmax_ref(s, scale, bias, key_mask):
    """float64 softmax(scale * s + bias) over the keys with key_mask != 0 (T5Attention, wan_text_encoder.py:91-103); a row with every
    key masked is uniform, as the reference's finfo.min fill (:98) makes it."""
    z = s.double() * scale + (bias.double() if bias is not None else 0.0)
    if key_mask is not None:
        if not bool(key_mask.bool().any()):
            return torch.full(z.shape, 1.0 / z.shape[1], dtype=F64)
        z = z.masked_fill(key_mask[None] == 0, -math.inf)
    return torch.softmax(z, dim=1)


def run_softmax(H, s, n, scale, bias, mask, npad):
    m = s.shape[0]
    ob = torch.full((m, npad + 8), SENT, dtype=BF, device=dev())
    H.softmax_bias_rows(s.to(dev()), ob[:, :npad], n, scale, bias.to(dev()) if bias is not None else None,
                        mask.to(dev()) if mask is not None else None)
    got = ob.cpu()
    assert bool((got[:, npad:] == SENT).all()), "softmax_bias_rows wrote past Npad"
    assert bool((got[:, n:npad] == 0).all()), "the padding columns n .. Npad are not exactly zero"
    return got[:, :n]


@pytest.mark.parametrize("n,m", [(1, 64), (9, 640), (512, 64 * 512)], ids=["N1", "N9", "N512-64heads"])
def test_softmax_bias_rows_at_the_text_length(H, n, m):
    """flexam_softmax_bias_rows (softmax_bias_kernel): N = 1, 9 and 512 keys (512 with 64 heads x 512 query rows, the XXL encoder's
    launch) into Npad = N rounded up to 64 (+64 when already a multiple) columns of a wider bf16 buffer, with and without the
    relative-position bias and the key mask, scale 0.125 and 1.  Probabilities within 1 bf16 ulp plus 2^-18 relative (the fp32 exp),
    the padding columns exactly 0."""
    g = torch.Generator().manual_seed(n)
    npad = (n + 63) // 64 * 64 + (64 if n % 64 == 0 else 0)
    s = torch.randn(m, n, generator=g) * 4
    bias = torch.randn(m, n, generator=g) * 2
    mask = torch.ones(n)
    if n > 1:
        mask[n - max(1, n // 5):] = 0                         # right padding of the prompt
        mask[1] = 0
    for scale, b, k in ((0.125, bias, mask), (1.0, None, None), (1.0, bias, None), (0.125, None, mask)):
        if n == 512 and b is None and k is None:
            continue                                          # the big shape once with bias and mask, once with the mask alone
        got = run_softmax(H, s, n, scale, b, k, npad)
        want = softmax_ref(s, scale, b, k)
        close(got, want, 2.0 ** -18 * want + 1e-30, msg=f"softmax N={n} scale={scale} bias={b is not None} mask={k is not None}")


def test_softmax_bias_rows_fully_masked_row_is_uniform(H):
    """A row whose keys are all masked: the reference's finfo.min fill swamps every score, so its softmax is uniform over the N keys
    (1/N each).  Before, the kernel took exp(-inf - -inf) and wrote NaN.  N = 1, 9, 512, with and without bias."""
    g = torch.Generator().manual_seed(83)
    for n in (1, 9, 512):
        npad = (n + 63) // 64 * 64
        s = torch.randn(33, n, generator=g) * 4
        for b in (None, torch.randn(33, n, generator=g)):
            got = run_softmax(H, s, n, 0.5, b, torch.zeros(n), npad)
            assert torch.equal(got, torch.full((33, n), 1.0 / n).to(BF)), f"fully masked row, N={n}"


def test_mul_bf16_at_the_ffn_width(H):
    """flexam_mul_bf16 (mul_bf16_kernel) over 512 x 10240 elements, the XXL FFN's gate product: bit-exact against torch's bf16
    multiply (one rounding of the exact fp32 product), with signed zeros and products that overflow bf16 mixed in."""
    g = torch.Generator().manual_seed(84)
    n = 512 * 10240
    a = (torch.randn(n, generator=g) * 4).to(BF)
    b = (torch.randn(n, generator=g) * 4).to(BF)
    a[:6] = torch.tensor([0.0, -0.0, 3e38, -3e38, 1e30, 7.0]).to(BF)
    b[:6] = torch.tensor([-5.0, 2.0, 2.0, 4.0, -1e10, -0.0]).to(BF)
    out = H.mul_bf16(a.to(dev()), b.to(dev()))
    want = (a.float() * b.float()).to(BF)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))
