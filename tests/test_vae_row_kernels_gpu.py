"""GPU: the VAE's one-pass row kernels (csrc/vae.hip) at the channel counts and row lengths the model runs, in every dispatch form,
against float64 torch formulas.  tests/test_conv_helpers_gpu.py checks them at C <= 64 and W <= 12, where the vector prep runs only with
one slab, the scalar prep not at all, AvgDown3D only at 8 / 16 channels, and no row kernel loops over several positions per thread
(row_grid does that once W * C / 4 > 2048, on every real VAE row).  Tolerances are that file's: one bf16 rounding for bf16 outputs,
exact for casts, 1e-6 for fp32 in-place adds (1e-5 for the AvgDown3D mean)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def dev():
    return torch.device("cuda:0")


def bf16_close(got, want, atol=1e-3):
    got, want = got.double().cpu(), want.double()
    tol = 2.0 ** -8 * want.abs() + atol
    assert bool(((got - want).abs() <= tol).all()), f"max err {(got - want).abs().max():.4g}"


def padded_rows(x, ld=None):
    """[C, T, H, W] -> rows [(t, hp, wp), ld] with zero borders (and zero columns [C, ld))."""
    c, t, h, w = x.shape
    p = torch.zeros(t, h + 2, w + 2, ld or c, dtype=x.dtype)
    p[:, 1:-1, 1:-1, :c] = x.permute(1, 2, 3, 0)
    return p.view(-1, ld or c)


def interior(img, t0, t, c):
    """[frames, hp, wp, Cp] image -> [C, t, h, w] of frames t0 .. t0 + t, on the host."""
    return img[t0:t0 + t, 1:-1, 1:-1, :c].permute(3, 0, 1, 2).cpu()


def assert_zero_outside(img, t0, t, c):
    """Everything of the image but the interior channels [0, c) of frames t0 .. t0 + t is still zero."""
    m = torch.ones(img.shape, dtype=torch.bool, device=img.device)
    m[t0:t0 + t, 1:-1, 1:-1, :c] = False
    assert int(torch.count_nonzero(img[m])) == 0, "a border pixel, history frame or pad channel was written"


# ----------------------------------------------------------------------------- vae_prep_cl
def prep_form(src, C, dst, gamma):
    """The form flexam_vae_prep_cl dispatches to (csrc/vae.hip, same conditions)."""
    ld, cp = src.stride(0), dst.shape[-1]
    g16 = gamma is None or gamma.data_ptr() % 16 == 0
    vec = C % 4 == 0 and C <= 1024 and ld % 4 == 0 and cp % 4 == 0 and src.data_ptr() % 16 == 0 and dst.data_ptr() % 8 == 0 and g16
    if vec and src.dtype == BF and C <= 256 and C % 8 == 0 and ld % 8 == 0 and cp % 8 == 0 and dst.data_ptr() % 16 == 0 and g16:
        return "span"
    return f"vector{(C + 255) // 256}" if vec else "scalar"


# (dtype, C, Cp, W, misaligned source, form): W >= 64 and not a multiple of 32; every form, NSLAB 1-4 for fp32 and 2-4 for bf16
PREP = [(BF, 160, 160, 70, False, "span"), (BF, 256, 256, 100, False, "span"),
        (F32, 160, 192, 100, False, "vector1"), (F32, 320, 320, 70, False, "vector2"), (F32, 640, 704, 70, False, "vector3"),
        (F32, 1024, 1024, 66, False, "vector4"),
        (BF, 320, 384, 70, False, "vector2"), (BF, 512, 512, 70, False, "vector2"), (BF, 640, 640, 66, False, "vector3"),
        (BF, 1024, 1088, 66, False, "vector4"),
        (F32, 1280, 1280, 66, False, "scalar"), (BF, 160, 192, 70, True, "scalar")]


@pytest.mark.parametrize("dtype,c,cp,w,misaligned,form", PREP, ids=[f"{p[-1]}-{str(p[0])[6:]}-{p[1]}" for p in PREP])
def test_vae_prep_every_form_at_vae_widths(dtype, c, cp, w, misaligned, form):
    """Modes 0 (cast), 1 (RMS_norm) and 2 (RMS_norm + SiLU) into a padded image behind 2 history frames and into compact rows."""
    from flexam_amd import hip as H
    g = torch.Generator().manual_seed(c + w)
    t, h, t0 = 2, 3, 2
    x = (torch.randn(c, t, h, w, generator=g, dtype=F64) * 2 + 0.5).to(dtype)
    rows = padded_rows(x)
    if misaligned:                                  # a source view 2 bytes past a 16-byte boundary
        buf = torch.zeros(rows.numel() + 8, dtype=dtype, device=dev())
        src = buf[1:1 + rows.numel()].view(rows.shape)
        src.copy_(rows)
    else:
        src = rows.to(dev())
    gamma = (1 + 0.2 * torch.randn(c, generator=g, dtype=F64)).to(F32)
    gd = gamma.to(dev())
    xd = x.to(F64)
    nrm = F.normalize(xd, dim=0) * math.sqrt(c) * gamma.to(F64).view(c, 1, 1, 1)
    wants = {0: xd, 1: nrm, 2: F.silu(nrm)}
    img = torch.zeros(t0 + t, h + 2, w + 2, cp, dtype=BF, device=dev())
    comp = torch.zeros(t * h * w, cp, dtype=BF, device=dev())
    assert prep_form(src, c, img, gd) == form and prep_form(src, c, comp, gd) == form
    for mode in (0, 1, 2):
        img.zero_()
        H.vae_prep_cl(src, c, t, h, w, img, mode=mode, gamma=gd if mode else None, t0=t0)
        got = interior(img, t0, t, c)
        if mode == 0:
            assert torch.equal(got, x.to(BF)), f"mode 0 ({form}): not the bf16 cast"
        else:
            bf16_close(got, wants[mode])
        assert_zero_outside(img, t0, t, c)
        comp.zero_()
        H.vae_prep_cl(src, c, t, h, w, comp, mode=mode, gamma=gd if mode else None, compact=True)
        got = comp.view(t, h, w, cp)[..., :c].permute(3, 0, 1, 2).cpu()
        if mode == 0:
            assert torch.equal(got, x.to(BF))
        else:
            bf16_close(got, wants[mode])
        assert int(torch.count_nonzero(comp[:, c:])) == 0


# ----------------------------------------------------------------------------- encoder helpers
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c,cs", [(160, 192), (320, 320), (640, 640)])
def test_space_to_depth_at_encoder_widths(c, cs, dtype):
    """The stride-2 convolutions' input: 160 channels in 192-channel groups (pad channels stay zero), 320 and 640 unpadded; long rows."""
    from flexam_amd import hip as H
    g = torch.Generator().manual_seed(c)
    t, h, w = 2, 4, 128
    x = torch.randn(c, t, h, w, generator=g).to(dtype)
    s2d = torch.zeros(t, h // 2 + 2, w // 2 + 2, 4 * cs, dtype=BF, device=dev())
    H.space_to_depth_cl(padded_rows(x).to(dev()), c, t, h, w, s2d, cs)
    grp = s2d.view(t, h // 2 + 2, w // 2 + 2, 4, cs)
    for a in range(2):
        for b in range(2):
            got = grp[:, 1:-1, 1:-1, a * 2 + b, :c].permute(3, 0, 1, 2).cpu()
            assert torch.equal(got, x[:, :, a::2, b::2].to(BF)), f"sub-pixel ({a}, {b})"
    m = torch.ones(grp.shape, dtype=torch.bool, device=dev())
    m[:, 1:-1, 1:-1, :, :c] = False
    assert int(torch.count_nonzero(grp[m])) == 0


# (Ci, Co, ft, fs, Ti): the encoder's AvgDown3D shortcuts, odd frame counts where ft = 2 (one zero frame in front)
AVG = [(160, 160, 1, 2, 3, "same"), (160, 320, 2, 2, 3, "general"), (160, 320, 2, 2, 4, "general"), (320, 640, 2, 2, 1, "general"),
       (320, 640, 2, 2, 5, "general"), (640, 640, 1, 1, 2, "same")]


@pytest.mark.parametrize("ci,co,ft,fs,ti,form", AVG, ids=[f"{a[0]}-{a[1]}-ft{a[2]}-fs{a[3]}-ti{a[4]}" for a in AVG])
def test_avgdown_add_both_forms_at_encoder_widths(ci, co, ft, fs, ti, form):
    from flexam_amd import hip as H
    from oracle import vae as OV
    g = torch.Generator().manual_seed(ci + co + ti)
    ho, wo = 3, 64
    xin = torch.randn(ci, ti, ho * fs, wo * fs, generator=g).double()
    want = OV.avg_down3d(xin[None], co, ft, fs)[0]                                  # [co, to, ho, wo]
    to = want.shape[1]
    base = torch.randn(co, to, ho, wo, generator=g).double()
    xm, xi = padded_rows(base.float()).to(dev()), padded_rows(xin.float()).to(dev())
    same = ci == co and co % 4 == 0 and xm.stride(0) % 4 == 0 and xi.stride(0) % 4 == 0 and xm.data_ptr() % 16 == 0 and xi.data_ptr() % 16 == 0
    assert ("same" if same else "general") == form                                  # the dispatcher's test in flexam_avgdown_add_cl
    H.avgdown_add_cl(xm, co, to, ho, wo, xi, ci, ti, ft, fs)
    got = xm.view(to, ho + 2, wo + 2, co)[:, 1:-1, 1:-1].permute(3, 0, 1, 2).cpu()
    torch.testing.assert_close(got.double(), base + want, rtol=1e-5, atol=1e-5)
    rows = xm.view(to, ho + 2, wo + 2, co)
    assert float(rows[:, 0].abs().max()) == 0 and float(rows[:, :, -1].abs().max()) == 0     # border rows untouched


# ----------------------------------------------------------------------------- decoder helpers
def dupup_ref(xin, co, ft, first):
    """DupUp3D (VAE.py:375-417) of x_in [Ci, T, H, W] -> [Co, T ft (- (ft - 1) on the first chunk), 2H, 2W]."""
    ci, t, h, w = xin.shape
    rep = co * ft * 4 // ci
    d = xin[None].repeat_interleave(rep, dim=1).view(1, co, ft, 2, 2, t, h, w).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(co, t * ft, 2 * h, 2 * w)
    return d[:, ft - 1:] if first else d


# (Ci, Co, ft): decoder stage 0 / 1 (1024 -> 1024, temporal) and stage 2 (x_in 1024 -> 512, spatial only)
DUP = [(1024, 1024, 2), (1024, 512, 1)]


@pytest.mark.parametrize("ci,co,ft", DUP, ids=[f"{d[0]}-{d[1]}-ft{d[2]}" for d in DUP])
def test_decoder_upsample_helpers_at_decoder_widths(ci, co, ft):
    """upsample2x_cl and deinterleave_cl from the time conv's [rows, 2 Co] (bf16) or the main rows (fp32), then phase_dupup_cl and
    dupup_add_cl with the DupUp3D shortcut, first chunk (frame dropped) and a regular one."""
    from flexam_amd import hip as H
    g = torch.Generator().manual_seed(ci + co)
    t, h, w = 2, 3, 64
    # upsample2x: interleave (time conv output, 2 Co wide, bf16 like the engine's) when ft = 2, plain fp32 rows otherwise
    cw = co * ft
    x = torch.randn(cw, t, h, w, generator=g)
    src = padded_rows(x.to(BF) if ft == 2 else x).to(dev())
    up = torch.zeros(t * ft, 2 * h + 2, 2 * w + 2, co, dtype=BF, device=dev())
    H.upsample2x_cl(src, co, t, h, w, up, interleave=ft == 2)
    frames = torch.stack((x[:co], x[co:]), dim=2).reshape(co, 2 * t, h, w) if ft == 2 else x
    want = frames.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    assert torch.equal(interior(up, 0, t * ft, co), want.to(BF))
    assert_zero_outside(up, 0, t * ft, co)
    # deinterleave: frame 2t + s = channels [s Co, (s + 1) Co) of frame t, at the input resolution
    y = torch.randn(2 * co, t, h, w, generator=g)
    for dt in (BF, F32):
        img = torch.zeros(2 * t, h + 2, w + 2, co + 64, dtype=BF, device=dev())
        H.deinterleave_cl(padded_rows(y.to(dt)).to(dev()), co, t, h, w, img)
        want = torch.stack((y[:co], y[co:]), dim=2).reshape(co, 2 * t, h, w)
        assert torch.equal(interior(img, 0, 2 * t, co), want.to(dt).to(BF))
        assert_zero_outside(img, 0, 2 * t, co)
    # phase_dupup (written) and dupup_add (accumulated): DupUp3D of x_in at 2x the resolution
    for first in (True, False):
        t_in = 1 if first else t
        to = t_in * ft - (ft - 1 if first else 0)
        xin = torch.randn(ci, t_in, h, w, generator=g)
        d = dupup_ref(xin.double(), co, ft, first)
        ph = torch.randn(4, co, to, h, w, generator=g)
        ph_rows = torch.stack([padded_rows(ph[i]) for i in range(4)]).to(dev())
        out = torch.full((to * (2 * h + 2) * (2 * w + 2), co), float("nan"), device=dev())
        H.phase_dupup_cl(ph_rows, out, co, to, 2 * h, 2 * w, padded_rows(xin).to(dev()), ci, ft, (ft - 1) if first else 0)
        inter = torch.zeros(co, to, 2 * h, 2 * w, dtype=F64)
        for a in range(2):
            for b in range(2):
                inter[:, :, a::2, b::2] = ph[a * 2 + b].double()
        got = out.view(to, 2 * h + 2, 2 * w + 2, co)[:, 1:-1, 1:-1].permute(3, 0, 1, 2).cpu()
        torch.testing.assert_close(got.double(), inter + d, rtol=1e-6, atol=1e-6)
        main = torch.randn(co, to, 2 * h, 2 * w, generator=g)
        mrows = padded_rows(main).to(dev())
        H.dupup_add_cl(mrows, co, to, 2 * h, 2 * w, padded_rows(xin).to(dev()), ci, ft, (ft - 1) if first else 0)
        got = mrows.view(to, 2 * h + 2, 2 * w + 2, co)[:, 1:-1, 1:-1].permute(3, 0, 1, 2).cpu()
        torch.testing.assert_close(got.double(), main.double() + d, rtol=1e-6, atol=1e-6)


def test_tapsum_of_the_decoder_head_on_a_full_width_row():
    """The folded head's gather at Co = 12 on a 448-pixel row (the 256 x 448 head stage), with two history frames."""
    from flexam_amd import hip as H
    g = torch.Generator().manual_seed(12)
    cin, co, kt, t, h, w = 8, 12, 3, 2, 2, 448
    xs = torch.randn(cin, kt - 1 + t, h, w, generator=g, dtype=F64)
    wt = torch.randn(co, cin, kt, 3, 3, generator=g, dtype=F64) / math.sqrt(cin * 27)
    b = torch.randn(co, generator=g, dtype=F64)
    wf = wt.permute(2, 3, 4, 0, 1).reshape(kt * 9 * co, cin)
    yrows = (padded_rows(xs) @ wf.t()).float()
    out = torch.zeros(t * (h + 2) * (w + 2), co, device=dev())
    H.tapsum_cl(yrows.to(dev()), t, h, w, kt, co, b.float().to(dev()), out)
    want = F.conv3d(F.pad(xs[None], (1, 1, 1, 1, 0, 0)), wt, b)[0]                 # [co, t, h, w]
    got = out.view(t, h + 2, w + 2, co)[:, 1:-1, 1:-1].permute(3, 0, 1, 2).cpu()
    torch.testing.assert_close(got.double(), want, rtol=1e-4, atol=1e-4)
    assert float(out.view(t, h + 2, w + 2, co)[:, 0].abs().max()) == 0


# the middle attention: c = 640 (encoder) / 1024 (decoder), n = h w positions per frame (24 and 450: a partial 64-column tail)
ATT = [(640, 4, 6), (1024, 4, 6), (640, 15, 30), (1024, 16, 28)]


@pytest.mark.parametrize("c,h,w", ATT, ids=[f"c{a[0]}-n{a[1] * a[2]}" for a in ATT])
def test_attention_softmax_and_scatter_add_at_middle_sizes(c, h, w):
    """softmax_rows over the first n of n4 = round_up(n, 4) score columns into [n, round_up(n, 64)] bf16 (zero tail), and the
    projection's compact rows added back into the padded fp32 residual rows (VAE.py:243-282 around the three GEMMs)."""
    from flexam_amd import hip as H
    g = torch.Generator().manual_seed(c + h * w)
    n = h * w
    n4, kp = (n + 3) // 4 * 4, (n + 63) // 64 * 64
    s = torch.randn(n, n4, generator=g) * 3
    p = torch.full((n, kp), float("nan"), dtype=BF, device=dev())
    H.softmax_rows(s.to(dev()), c ** -0.5, p, n)
    bf16_close(p[:, :n], torch.softmax(s[:, :n].double() * c ** -0.5, dim=1), atol=1e-4)
    assert int(torch.count_nonzero(p[:, n:])) == 0
    x = torch.randn(c, 1, h, w, generator=g)
    y = torch.randn(n, c, generator=g).to(BF)
    xr = padded_rows(x).to(dev())
    H.scatter_add_cl(xr, y.to(dev()), c, 1, h, w)
    got = xr.view(1, h + 2, w + 2, c)[:, 1:-1, 1:-1].permute(3, 0, 1, 2).cpu()
    torch.testing.assert_close(got.double(), x.double() + y.double().view(1, h, w, c).permute(3, 0, 1, 2), rtol=1e-6, atol=1e-6)
    assert float(xr.view(1, h + 2, w + 2, c)[:, 0].abs().max()) == 0


def test_pack_affine_latent_into_the_decoder_input_image():
    """Every decode starts here: z [48, T, H, W] * std + mean -> the conv2 image interior, 48 of 64 channels (pad stays zero)."""
    from flexam_amd import hip as H
    from flexam_amd.wan_vae3_8 import LATENT_MEAN, LATENT_STD
    g = torch.Generator().manual_seed(48)
    c, cp, t, h, w = 48, 64, 3, 5, 70
    z = torch.randn(c, t, h, w, generator=g)
    std, mean = torch.tensor(LATENT_STD), torch.tensor(LATENT_MEAN)
    img = torch.zeros(t, h + 2, w + 2, cp, dtype=BF, device=dev())
    H.pack_affine_cl(z.to(dev()), std.to(dev()), mean.to(dev()), img)
    want = z.double() * std.double().view(c, 1, 1, 1) + mean.double().view(c, 1, 1, 1)
    bf16_close(interior(img, 0, t, c), want)
    assert_zero_outside(img, 0, t, c)
