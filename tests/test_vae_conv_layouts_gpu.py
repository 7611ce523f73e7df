"""GPU: every convolution layout the Wan2.2 VAE builds, at the model's true widths, EXACT against torch.

The layer list is encoder_param_shapes() + decoder_param_shapes() at their defaults (encoder 160 / 320 / 640 channels, decoder
1024 / 512 / 256), one case per distinct (class, Cin, Cout, kernel), each built with the class the engines pick and run on its own:
_Conv (3x3x3 and (3,1,1), run-packed when Cin % 64 != 0), _ConvS2D (encoder resample), _ConvUp2x (decoder resample), _ConvFold (decoder
head) and the plain GEMM over a padded image (1x1x1 shortcuts).  The whole-VAE tests only bound these to 40 dB, under which one wrong
tap of one layer can hide.  Here weights, biases and activations are small integers, so every fp32 sum is exact whatever the tile or
split-K plan: an fp32 output equals the float64 torch convolution bit for bit, a bf16 output equals it rounded once, and the fused
residual adds that bf16 value to x."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def dev():
    return torch.device("cuda:0")


def _layers():
    """{(kind, Cin, Cout, kernel): first parameter name} of every convolution the engines run at the true widths."""
    from flexam_amd.wan_vae3_8 import decoder_param_shapes, encoder_param_shapes
    out = {}
    for side, shapes in (("encoder", encoder_param_shapes()), ("decoder", decoder_param_shapes())):
        for key, shape in shapes.items():
            if not key.endswith(".weight"):
                continue
            name, (co, ci, *k) = key[:-len(".weight")], shape
            k = tuple(k)
            if k == (1, 1):
                continue                              # the middle attention's to_qkv / proj: GEMMs on compact rows, no image
            if name == "conv1":
                continue                              # folded into the encoder head's weights, never run on its own
            if name.endswith("resample.1"):
                kind = "s2d" if side == "encoder" else "up2x"
            elif name == "decoder.head.2":
                kind = "fold"
            elif name.endswith("time_conv"):
                kind = "time_stride2" if side == "encoder" else "conv"
            elif k == (1, 1, 1):
                kind = "gemm1x1"
            else:
                kind = "conv"
            out.setdefault((kind, ci, co, k), name)
    return out


LAYERS = sorted(_layers())


def _id(layer):
    kind, ci, co, k = layer
    return f"{kind}-{ci}-{co}-{'x'.join(map(str, k))}"


def _ints(g, *shape):
    return torch.randint(-2, 3, shape, generator=g).to(F64)


def _put(img, x, t0=0):
    """x [C, t, h, w] -> interior of frames t0 .. t0 + t of the channels-last image, channels [0, C)."""
    c, t = x.shape[:2]
    img[t0:t0 + t, 1:-1, 1:-1, :c] = x.permute(1, 2, 3, 0).to(BF).to(img.device)


def _interior(rows, t, h, w):
    """GEMM rows of the padded (t, h + 2, w + 2) positions -> [Cout, t, h, w] of the interior, on the host."""
    return rows.reshape(t, h + 2, w + 2, -1)[:, 1:-1, 1:-1].permute(3, 0, 1, 2).cpu()


def _exact_bound(terms):
    """|product| <= 8 * 2 (summed Up2x taps) and at most `terms` of them: every partial sum is an integer fp32 holds."""
    assert terms * 16 < 2 ** 24


def _check(got, want, what):
    """got from the GPU (fp32 or bf16), want the float64 result: equal after one rounding to got's dtype."""
    ref = want.to(F32).to(got.dtype)
    bad = int((got != ref).sum())
    assert bad == 0, f"{what}: {bad} of {got.numel()} outputs differ, max |diff| {float((got.double() - ref.double()).abs().max()):.4g}"


def _causal(x, wt, b):
    """CausalConv3d over all frames joined: zero front padding of kt - 1 frames, 'same' spatial padding."""
    kt, kh, kw = wt.shape[2:]
    return F.conv3d(F.pad(x[None], (kw // 2, kw // 2, kh // 2, kh // 2, kt - 1, 0)), wt, b)[0]


def _size(ci, co):
    return (4, 6) if max(ci, co) >= 512 else (6, 10)


def _run_layer(kind, ci, co, k, h, w, g, chunks=None):
    """Build the layer with integer weights, run it chunk by chunk and compare every output with the float64 reference."""
    from flexam_amd import hip
    from flexam_amd import wan_vae3_8 as V
    wt, b = _ints(g, co, ci, *k), _ints(g, co)
    if kind in ("conv", "fold"):
        # causal: chunks of 1, 2, 2 frames (ring forced to wrap after every chunk by the caller), the outputs cycling through the three
        # epilogues the engines use: fp32 rows, bf16 rows (the first conv of a residual block), x += bf16(conv) (its second conv)
        chunks = chunks or (1, 2, 2)
        conv = (V._ConvFold if kind == "fold" else V._Conv)(wt, b, dev(), t_cap=max(chunks))
        _exact_bound(conv.weight.shape[1] * (27 if kind == "fold" else 1))
        x = _ints(g, ci, sum(chunks), h, w)
        want = _causal(x, wt, b)
        f0 = 0
        for i, t in enumerate(chunks):
            _put(conv.image(h, w), x[:, f0:f0 + t], conv.hist)
            ref = want[:, f0:f0 + t]
            mode = 0 if kind == "fold" else i % 3
            what = f"{kind} {ci}->{co} {k}, chunk {i} ({t} frames)"
            if mode < 2:
                out = conv.run(t, h, w, out_dtype=(F32, BF)[mode])
                _check(_interior(out, t, h, w), ref, what + (", fp32", ", bf16")[mode])
            else:
                x0 = _ints(g, t * (h + 2) * (w + 2), co).to(F32).to(dev())
                xr = x0.clone()
                conv.run(t, h, w, residual_into=xr)
                want_r = _interior(x0, t, h, w) + ref.to(F32).to(BF).to(F32)
                _check(_interior(xr, t, h, w), want_r, what + ", residual")
            f0 += t
    elif kind == "time_stride2":
        # Resample downsample3d's time conv (VAE.py:162-174): the first 1-frame chunk is only cached, every later chunk of 4 frames
        # gives 2 frames of a stride-2 (3,1,1) conv over [last cached frame | chunk]
        chunks = (1, 4, 4)
        conv = V._Conv(wt, b, dev(), t_cap=4)
        _exact_bound(conv.weight.shape[1])
        x = _ints(g, ci, sum(chunks), h, w)
        want = F.conv3d(x[None], wt, b, stride=(2, 1, 1))[0]                    # frames (0,1,2), (2,3,4), ...: 4 outputs
        f0, j0 = 0, 0
        for i, t in enumerate(chunks):
            _put(conv.image(h, w), x[:, f0:f0 + t], conv.hist)
            if i == 0:
                conv.roll(t)
            else:
                od = (F32, BF)[i - 1]
                out = conv.run_time_stride2(t, h, w, out_dtype=od)
                _check(_interior(out, t // 2, h, w), want[:, j0:j0 + t // 2], f"time conv {ci}->{co} stride 2, chunk {i}, {od}")
                j0 += t // 2
            f0 += t
    elif kind == "s2d":
        # ZeroPad2d((0, 1, 0, 1)) + Conv2d(3x3, stride 2) over a space-to-depth image: sub-pixel (a, b) in channel group a * 2 + b of Cs
        t, h2, w2 = 2, h, w
        ds = V._ConvS2D(wt, b, dev(), t_cap=t)
        _exact_bound(ds.weight.shape[1])
        x = _ints(g, ci, t, 2 * h2, 2 * w2)
        img = ds.image(h2, w2)
        sub = x.view(ci, t, h2, 2, w2, 2).permute(1, 2, 4, 3, 5, 0).reshape(t, h2, w2, 4, ci)
        img.view(t, h2 + 2, w2 + 2, 4, ds.cs)[:, 1:-1, 1:-1, :, :ci] = sub.to(BF).to(dev())
        frames = x.permute(1, 0, 2, 3)
        want = F.conv2d(F.pad(frames, (0, 1, 0, 1)), wt, b, stride=2).permute(1, 0, 2, 3)
        for od in (F32, BF):
            _check(_interior(ds.run(t, h2, w2, out_dtype=od), t, h2, w2), want, f"s2d {ci}->{co}, {od}")
        x0 = _ints(g, t * (h2 + 2) * (w2 + 2), co).to(F32).to(dev())
        xr = x0.clone()
        ds.run(t, h2, w2, residual_into=xr)
        _check(_interior(xr, t, h2, w2), _interior(x0, t, h2, w2) + want.to(F32).to(BF).to(F32), f"s2d {ci}->{co}, residual")
    elif kind == "up2x":
        # nearest-exact 2x upsample + Conv2d(3x3, padding 1) as four 2x2 phase convolutions of the low-resolution frames
        t = 2
        rs = V._ConvUp2x(wt, b, dev(), t_cap=t)
        _exact_bound(rs.weights[0].shape[1])
        x = _ints(g, ci, t, h, w)
        _put(rs.image(h, w), x)
        ph = rs.run(t, h, w)
        up = F.interpolate(x.permute(1, 0, 2, 3), scale_factor=2.0, mode="nearest-exact")
        want = F.conv2d(up, wt, b, padding=1).permute(1, 0, 2, 3)                # [Cout, t, 2h, 2w]
        for a in range(2):
            for c in range(2):
                _check(_interior(ph[a * 2 + c], t, h, w), want[:, :, a::2, c::2], f"up2x {ci}->{co}, phase ({a}, {c})")
    elif kind == "gemm1x1":
        # the engines' 1x1x1 convs: one plain GEMM over the padded image of Cp channels (_Conv's packed weight, no tap table)
        t = 2
        sc = V._Conv(wt, b, dev(), t_cap=t)
        xb = torch.zeros(t, h + 2, w + 2, sc.cp, device=dev(), dtype=BF)
        x = _ints(g, ci, t, h, w)
        _put(xb, x)
        want = F.conv3d(x[None], wt, b)[0]
        for od in (F32, BF):
            out = hip.gemm(xb.view(-1, sc.cp), sc.weight, sc.bias, out_dtype=od)
            _check(_interior(out, t, h, w), want, f"1x1x1 {ci}->{co}, {od}")
    else:
        raise AssertionError(kind)


def test_layer_list_covers_every_layout():
    """The cases below are the engines' layouts at true widths: the run-packed Cin = 12 / 48 / 160 (1 / 3 / 8 K blocks per image row),
    5 / 10 / 16 channel blocks of the plain K order, Cs = 192 padding of the 160-channel S2D, N = 2048 time conv, folded head at 256."""
    keys = set(LAYERS)
    assert ("conv", 160, 160, (3, 3, 3)) in keys and ("conv", 12, 160, (3, 3, 3)) in keys and ("conv", 48, 1024, (3, 3, 3)) in keys
    assert ("conv", 320, 320, (3, 3, 3)) in keys and ("conv", 640, 640, (3, 3, 3)) in keys and ("conv", 1024, 1024, (3, 3, 3)) in keys
    assert ("s2d", 160, 160, (3, 3)) in keys and ("up2x", 1024, 1024, (3, 3)) in keys and ("up2x", 512, 512, (3, 3)) in keys
    assert ("conv", 1024, 2048, (3, 1, 1)) in keys and ("time_stride2", 640, 640, (3, 1, 1)) in keys
    assert ("fold", 256, 12, (3, 3, 3)) in keys and ("conv", 640, 96, (3, 3, 3)) in keys
    assert {co for kind, ci, co, k in keys if kind == "conv"} >= {96, 160, 320, 640, 1024, 2048}


@pytest.mark.parametrize("layer", LAYERS, ids=[_id(x) for x in LAYERS])
def test_vae_conv_layout_is_exact(layer, monkeypatch):
    """One layer of the engines at its true width; causal convs across three chunks with the history ring wrapping after every one
    (RING = 1), compared with one convolution over all frames joined."""
    from flexam_amd import wan_vae3_8 as V
    monkeypatch.setattr(V._CausalImage, "RING", 1)
    kind, ci, co, k = layer
    h, w = _size(ci, co)
    _run_layer(kind, ci, co, k, h, w, torch.Generator().manual_seed(ci * 7919 + co * 31 + len(k)))


WIDE = [("conv", 160, 160, (3, 3, 3), 8, 112), ("s2d", 160, 160, (3, 3), 8, 112), ("up2x", 512, 512, (3, 3), 4, 56),
        ("fold", 256, 12, (3, 3, 3), 8, 112), ("gemm1x1", 160, 320, (1, 1, 1), 8, 112)]


@pytest.mark.parametrize("kind,ci,co,k,h,w", WIDE, ids=[c[0] for c in WIDE])
def test_vae_conv_layout_wide_row_is_exact(kind, ci, co, k, h, w, monkeypatch):
    """One long-row case per class (112-position rows, as in the 64 x 112 stage of a 512 x 896 clip): thousands of GEMM rows, so the
    persistent grid runs many tiles and a tail, with the run-packed 160-channel taps reaching across tile edges."""
    from flexam_amd import wan_vae3_8 as V
    monkeypatch.setattr(V._CausalImage, "RING", 1)
    _run_layer(kind, ci, co, k, h, w, torch.Generator().manual_seed(ci + co + h * w), chunks=(1, 2))
