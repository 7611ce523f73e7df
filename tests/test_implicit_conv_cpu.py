"""CPU: the packed weight and the offset table of every implicit-GEMM convolution agree, block by block.

Each class is built on the CPU with small integer weights, and the GEMM it would launch is restated in float64 from the header's words
(include/flexam_hip.h, flexam_gemm_bf16):  A[m, kb*64 + j] = buf[m*lda + a_koff[kb] + j],  C = A . W^T + bias.  The interior positions
must equal torch's convolution EXACTLY (integers: every sum is exact), against the references tests/test_vae_conv_layouts_gpu.py uses:
causal front padding, ZeroPad2d((0,1,0,1)) + stride 2, nearest-2x + 3x3.  One case per form, the smallest that reaches it; the causal
ones run as chunks of 1, 2, 2 frames with RING = 1, so the history ring wraps after every chunk.  Every address the restated GEMM forms
must lie inside the image's allocation, which checks the guards as well."""
import pytest
import torch
import torch.nn.functional as F

from flexam_amd import hip
from flexam_amd import wan_vae3_8 as V
from flexam_amd.dit_engine import _conv_cl
from flexam_amd.implicit_conv import GuardedImage, reach

BF, F64 = torch.bfloat16, torch.float64
CPU = torch.device("cpu")
CO, H, W = 8, 3, 4
CHUNKS = (1, 2, 2)


def _gemm(a, w, bias=None, out=None, epilogue=0, out_dtype=None, a_koff=None, m=None, k=None):
    """hip.gemm restated: `a` is a 2-D view into its allocation; with a_koff only its base address and row stride count."""
    rows = a.shape[0] if m is None else m
    if a_koff is None:
        A = a[:rows].to(F64)
    else:
        buf = torch.empty(0, dtype=a.dtype).set_(a.untyped_storage())
        idx = (a.storage_offset() + torch.arange(rows)[:, None, None] * a.stride(0) + a_koff[None, :, None] + torch.arange(64)[None, None, :])
        assert int(idx.min()) >= 0 and int(idx.max()) < buf.numel(), "the GEMM would read outside the image's allocation"
        A = buf[idx.reshape(rows, -1)].to(F64)
    assert A.shape[1] == w.shape[1] == (w.shape[1] if k is None else k)
    c = A @ w.to(F64).T + (0 if bias is None else bias.to(F64))
    return c if out is None else out.copy_(c)


def _tapsum(y, t, h, w, kt, co, bias, out):
    """hip.tapsum_cl restated: out[(t,h,w), o] = bias[o] + sum over taps of y[(t + dt, h + dh - 1, w + dw - 1), tap * co + o]."""
    yv = y.to(F64).view(kt - 1 + t, h + 2, w + 2, kt * 9, co)
    acc = bias.to(F64).expand(t, h, w, co).clone()
    for dt in range(kt):
        for dh in range(3):
            for dw in range(3):
                acc += yv[dt:dt + t, dh:dh + h, dw:dw + w, (dt * 3 + dh) * 3 + dw]
    out.view(t, h + 2, w + 2, co)[:, 1:-1, 1:-1] = acc
    return out


@pytest.fixture(autouse=True)
def restated(monkeypatch):
    monkeypatch.setattr(hip, "gemm", _gemm)
    monkeypatch.setattr(hip, "tapsum_cl", _tapsum)
    monkeypatch.setattr(V._CausalImage, "RING", 1)


def _ints(g, *shape):
    return torch.randint(-2, 3, shape, generator=g).to(F64)


def _put(img, x, t0=0):
    """x [C, t, h, w] -> interior of frames t0 .. t0 + t of the channels-last image, channels [0, C)."""
    c, t = x.shape[:2]
    img[t0:t0 + t, 1:-1, 1:-1, :c] = x.permute(1, 2, 3, 0).to(BF)


def _interior(rows, t, h, w):
    """GEMM rows of the padded (t, h + 2, w + 2) positions -> [Cout, t, h, w] of the interior, float64."""
    return rows.reshape(t, h + 2, w + 2, -1)[:, 1:-1, 1:-1].permute(3, 0, 1, 2).to(F64)


def _differ(got, want):
    return int((got != want).sum())


def _causal(x, wt, b):
    """CausalConv3d over all frames joined: zero front padding of kt - 1 frames, 'same' spatial padding."""
    kt, kh, kw = wt.shape[2:]
    return F.conv3d(F.pad(x[None], (kw // 2, kw // 2, kh // 2, kh // 2, kt - 1, 0)), wt, b)[0]


def _run_causal(cls, ci, k, g, co=CO, spoil=None):
    """Chunk by chunk through cls.run (which rolls the window); -> outputs that differ from the convolution over all frames joined."""
    wt, b = _ints(g, co, ci, *k), _ints(g, co)
    conv = cls(wt, b, CPU, t_cap=max(CHUNKS))
    x = _ints(g, ci, sum(CHUNKS), H, W)
    want = _causal(x, wt, b)
    bad, f0 = 0, 0
    for t in CHUNKS:
        _put(conv.image(H, W), x[:, f0:f0 + t], conv.hist)
        if spoil is not None and f0 == 0:
            spoil(conv)
        bad += _differ(_interior(conv.run(t, H, W), t, H, W), want[:, f0:f0 + t])
        f0 += t
    return bad


CAUSAL = [(V._Conv, 128, (3, 3, 3), CO), (V._Conv, 12, (3, 3, 3), CO), (V._Conv, 160, (3, 3, 3), CO), (V._Conv, 64, (3, 1, 1), CO),
          (V._ConvFold, 64, (3, 3, 3), 12)]


@pytest.mark.parametrize("cls,ci,k,co", CAUSAL, ids=["conv-128", "conv-runpacked-12", "conv-runpacked-160", "conv-3x1x1", "fold-64-12"])
def test_causal_conv_weight_and_offsets_agree(cls, ci, k, co):
    """_Conv in the (dt, dh, channel block, dw, 64) order with two channel blocks, run-packed (1 and 8 K blocks per image row, the last
    one reaching into the next pixel against zero weights), (3,1,1); _ConvFold's product rows followed by the restated tap sum."""
    assert _run_causal(cls, ci, k, torch.Generator().manual_seed(ci), co=co) == 0


def test_swapped_offsets_are_seen():
    """Negative control: two entries of one offset table exchanged (taps dw = 0 and dw = 1 of the first image row, same channel block)
    while the weight stays as packed -- the comparison above must fail, or it could not see an order mismatch."""
    def spoil(conv):
        k = conv.a_koff.clone()
        k[0], k[1] = conv.a_koff[1], conv.a_koff[0]
        conv.a_koff = k
    assert _run_causal(V._Conv, 128, (3, 3, 3), torch.Generator().manual_seed(128), spoil=spoil) > 0


def test_pointwise_conv_through_a_plain_image():
    """The engines' 1x1x1 convs: _Conv's packed weight over a padded image of Cp channels, no offset table."""
    g, t, ci = torch.Generator().manual_seed(1), 2, 96
    wt, b = _ints(g, CO, ci, 1, 1, 1), _ints(g, CO)
    sc = V._Conv(wt, b, CPU, t_cap=t)
    xb = GuardedImage(t, H, W, sc.cp, CPU, 0, 0)
    x = _ints(g, ci, t, H, W)
    _put(xb.img, x)
    assert _differ(_interior(hip.gemm(xb.mat, sc.weight, sc.bias), t, H, W), F.conv3d(x[None], wt, b)[0]) == 0


def test_space_to_depth_conv_weight_and_offsets_agree():
    """_ConvS2D: ZeroPad2d((0, 1, 0, 1)) + Conv2d(3x3, stride 2); sub-pixel (a, b) in channel group a * 2 + b of Cs."""
    g, t, ci = torch.Generator().manual_seed(2), 2, 64
    wt, b = _ints(g, CO, ci, 3, 3), _ints(g, CO)
    ds = V._ConvS2D(wt, b, CPU, t_cap=t)
    x = _ints(g, ci, t, 2 * H, 2 * W)
    sub = x.view(ci, t, H, 2, W, 2).permute(1, 2, 4, 3, 5, 0).reshape(t, H, W, 4, ci)
    ds.image(H, W).view(t, H + 2, W + 2, 4, ds.cs)[:, 1:-1, 1:-1, :, :ci] = sub.to(BF)
    want = F.conv2d(F.pad(x.permute(1, 0, 2, 3), (0, 1, 0, 1)), wt, b, stride=2).permute(1, 0, 2, 3)
    assert _differ(_interior(ds.run(t, H, W), t, H, W), want) == 0


def test_phase_upsample_conv_weight_and_offsets_agree():
    """_ConvUp2x: nearest-exact 2x upsample + Conv2d(3x3, padding 1) as four 2x2 phase convolutions of summed taps."""
    g, t, ci = torch.Generator().manual_seed(3), 2, 64
    wt, b = _ints(g, CO, ci, 3, 3), _ints(g, CO)
    rs = V._ConvUp2x(wt, b, CPU, t_cap=t)
    x = _ints(g, ci, t, H, W)
    _put(rs.image(H, W), x)
    ph = rs.run(t, H, W)
    up = F.interpolate(x.permute(1, 0, 2, 3), scale_factor=2.0, mode="nearest-exact")
    want = F.conv2d(up, wt, b, padding=1).permute(1, 0, 2, 3)                # [Cout, t, 2h, 2w]
    for a in range(2):
        for c in range(2):
            assert _differ(_interior(ph[a * 2 + c], t, H, W), want[:, :, a::2, c::2]) == 0, f"phase ({a}, {c})"


def test_cnn_block_conv_weight_and_offsets_agree():
    """The DiT cnn-block's (1,3,3) convolution in its tap-major order (dh, dw, channel block), cp = 192 (three channel blocks)."""
    g, t, ci, cp = torch.Generator().manual_seed(4), 2, 160, 192
    wt, b = _ints(g, CO, ci, 1, 3, 3), _ints(g, CO)
    conv = _conv_cl(wt, b, CPU)
    img = GuardedImage(t, H, W, cp, CPU, reach(W, cp), reach(W, cp))
    x = _ints(g, ci, t, H, W)
    _put(img.img, x)
    conv.at(H + 2, W + 2, cp)
    assert _differ(_interior(conv.launch(img.mat, t * (H + 2) * (W + 2)), t, H, W), F.conv3d(x[None], wt, b, padding=(0, 1, 1))[0]) == 0
