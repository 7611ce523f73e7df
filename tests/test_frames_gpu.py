"""GPU: flexam_amd.frames (csrc/frames.hip) through the C ABI -- the resize against torch's CPU `F.interpolate` on the same inputs
within accumulation rounding, the byte conversion bit for bit against the numpy chain, the two reference functions against their
arithmetic written out with torch on the CPU, and the argument errors."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frames_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in R.SHAPES]


def _check(got, want, tol, what):
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape, what
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"{what}: max error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol, what


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_resize_equals_torch_cpu(shape, antialias):
    """T = 5, C = 3; uint8 and float32 sources, both input layouts, both output layouts.  uint8 `thwc` at the odd widths 53, 59 and 47
    are the alignment cases: rows of 3 W bytes."""
    from flexam_amd import resize_frames
    (h, w), size = shape
    tol = R.tolerance(h, w, *size, antialias)
    for dtype in ("u8", "f32"):
        x = R.case(h, w, dtype)
        want = R.reference(h, w, *size, antialias, dtype)
        thwc = torch.from_numpy(x.copy())
        _check(resize_frames(thwc, size, antialias, "thwc", "tchw"), want, tol, f"{dtype} thwc->tchw")
        _check(resize_frames(thwc, size, antialias, "thwc", "cthw"), want.transpose(1, 0, 2, 3), tol, f"{dtype} thwc->cthw")
        tchw = thwc.permute(0, 3, 1, 2).contiguous()
        _check(resize_frames(tchw, size, antialias, "tchw", "cthw"), want.transpose(1, 0, 2, 3), tol, f"{dtype} tchw->cthw")
        _check(resize_frames(x.copy(), size, antialias, "thwc", "tchw"), want, tol, f"{dtype} numpy")
        if (h, w) == size:
            assert np.array_equal(resize_frames(thwc, size, antialias).cpu().numpy(), want), "the identity resize must be exact"


@pytest.mark.parametrize("antialias", [False, True])
def test_resize_epilogue_and_input_forms(antialias):
    """`mul` / `div` / `add`, C = 1, one frame, a sliced source, a source on the GPU, an `out` view.  Tolerance of the scaled result: the
    resize tolerance times |mul / div| plus one rounding (2^-24 relative) per closing step on results up to `peak`."""
    from flexam_amd import resize_frames
    (h, w), size = R.SHAPES[0]
    x = torch.from_numpy(R.case(h, w, "u8").copy())
    want = R.reference(h, w, *size, antialias, "u8").astype(np.float64)
    tol = R.tolerance(h, w, *size, antialias)
    step = 2.0 ** -24
    _check(resize_frames(x, size, antialias, mul=2.0 / 255.0, add=-1.0), want * (2.0 / 255.0) - 1.0, tol * 2 / 255 + 3 * step * 2, "* 2 / 255 - 1")
    _check(resize_frames(x, size, antialias, div=255.0), want / 255.0, tol / 255 + 2 * step, "/ 255")
    _check(resize_frames(x.to(DEV), size, antialias), want, tol, "source on the GPU")
    _check(resize_frames(x[:1], size, antialias), want[:1], tol, "one frame")
    _check(resize_frames(x[..., 1:2], size, antialias), want[:, 1:2], tol, "C = 1, sliced channels")
    _check(resize_frames(x.to(DEV)[..., 1:2], size, antialias), want[:, 1:2], tol, "C = 1, sliced on the GPU")
    sl = x[1:4, 3:30, 5:46]                                                   # frames, rows and columns sliced: non-contiguous
    ws = F.interpolate(sl.permute(0, 3, 1, 2).float(), size=size, mode="bilinear", align_corners=False, antialias=antialias).numpy()
    for src in (sl, sl.to(DEV), x.to(DEV)[1:4, 3:30, 5:46]):
        _check(resize_frames(src, size, antialias), ws, R.tolerance(27, 41, *size, antialias), "sliced source")
    buf = torch.zeros(7, 3, *size, device=DEV)
    resize_frames(x, size, antialias, out=buf[1:6])
    _check(buf[1:6], want, tol, "out view")
    assert not buf[0].any() and not buf[6].any()
    x5 = torch.from_numpy(R.case(h, w, "f32", 2, 5).copy())                    # five channels: two register blocks
    w5 = F.interpolate(x5.permute(0, 3, 1, 2), size=size, mode="bilinear", align_corners=False, antialias=antialias).numpy()
    _check(resize_frames(x5, size, antialias), w5, tol, "C = 5")


def test_resize_many_rows_loops_over_the_grid():
    """More output rows than the grid's y limit holds at four rows a workgroup (T * oh > 4 * 65535): the row loop."""
    from flexam_amd import resize_frames
    x = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (2, 70000, 3, 1), dtype=np.uint8))
    size = (140000, 2)
    want = F.interpolate(x.permute(0, 3, 1, 2).float(), size=size, mode="bilinear", align_corners=False, antialias=False).numpy()
    _check(resize_frames(x, size, False), want, 255 * 2.0 ** -24 * (2 * 2 + 4), "280000 rows")      # two taps an axis


@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", [(3, 5, 17, 23), (3, 4, 16, 32)], ids=["odd-rows", "dwords"])
def test_to_bytes_bit_exact(shape, bf16, signed):
    from flexam_amd import frames_to_bytes
    x = torch.from_numpy(R.bytes_case(shape))
    if not signed:
        x = x / 2 + 0.5
    x.view(-1)[::97] = float("nan")
    x.view(-1)[5], x.view(-1)[6] = float("inf"), float("-inf")
    if bf16:
        x = x.bfloat16()
    want = R.to_bytes(x.float().numpy(), signed)
    for src in (x.to(DEV), x, x.unsqueeze(0).to(DEV)):
        got = frames_to_bytes(src, signed=signed)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (shape[1], shape[2], shape[3], 3)
        assert np.array_equal(got.cpu().numpy(), want)
    one = frames_to_bytes(x[:1].to(DEV), signed=signed)                        # one channel: the general kernel
    assert np.array_equal(one.cpu().numpy(), want[..., :1])


def _reference_branch(video, video_length, size, restore):
    """utils.py:424-438, 447-449 written out."""
    v = F.interpolate(video.permute(0, 3, 1, 2), size=size, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).cpu().numpy()
    if restore:
        v = v * 255
    v = torch.from_numpy(np.array(v))[:video_length]
    v = v.permute([3, 0, 1, 2]).unsqueeze(0) / 255
    mask = torch.zeros_like(v[:, :1])
    mask[:, :, :] = 255
    return v, mask


@pytest.mark.parametrize("restore", [False, True])
def test_get_video_to_video_latent(restore):
    from flexam_amd import get_video_to_video_latent, resize_frames
    (h, w), size = R.SHAPES[2]
    peak = 1.0 if restore else 255.0                                           # a ComfyUI IMAGE in [0, 1] is what if_restore_255 is for
    video = torch.from_numpy(R.case(h, w, "f32", 7).copy()) * (peak / 255.0)
    want, want_mask = _reference_branch(video, 5, size, restore)
    got, mask, ref, clip = get_video_to_video_latent(video, 5, size, if_restore_255=restore)
    assert ref is None and clip is None and tuple(got.shape) == (1, 3, 5, *size)
    assert mask.is_cuda and torch.equal(mask.cpu(), want_mask)
    tol = R.tolerance(h, w, *size, False, peak) * (255.0 if restore else 1.0) / 255.0 + 2 * 2.0 ** -24
    _check(got, want.numpy(), tol, f"if_restore_255={restore}")
    # the closing steps are the reference's roundings, bit for bit, on the kernel's own resized values: with if_restore_255 that is
    # (y * 255) / 255 in float32, which is not y everywhere
    y = resize_frames(video[:5], size, False, "thwc", "cthw").cpu().numpy()[None]
    chain = (y * np.float32(255.0)) / np.float32(255.0) if restore else y / np.float32(255.0)
    assert np.array_equal(got.cpu().numpy(), chain)
    if restore:
        assert not np.array_equal(chain, y), "the case must tell the chain from the unscaled input"


def test_mask_video_feeds_the_refinement_like_the_host_resize():
    """get_maskvideo_to_video_latent -> generate_mask_fg_tracking_for_validation gives the mask of the host-resized frames (torch CPU,
    antialias).  Condition on the input: no channel mean of the host-resized frames within the resize tolerance of the 0.5 threshold."""
    from flexam_amd import generate_mask_fg_tracking_for_validation as fg
    from flexam_amd import get_maskvideo_to_video_latent
    video = R.blob_mask_video(9, 135, 240)
    size = (64, 112)
    host = F.interpolate(torch.from_numpy(video).permute(0, 3, 1, 2).float(), size=size, mode="bilinear", align_corners=False, antialias=True)
    tol = R.tolerance(135, 240, *size, True)
    assert float((host.mean(dim=1) - 0.5).abs().min()) > 2 * tol
    dev = get_maskvideo_to_video_latent(video, 9, size)
    _check(dev, host.numpy(), tol, "mask frames")
    want = fg(host, blur_radius=5, dilation_pixels=6)
    got = fg(dev, blur_radius=5, dilation_pixels=6)
    assert want[1:].any() and torch.equal(got, want)
    # the frame-count rule: 3 frames for 5 -> all resized, the last repeated; 9 for 5 -> the first five
    short = get_maskvideo_to_video_latent(video[4:7], 5, size)
    assert tuple(short.shape) == (5, 3, 64, 112) and torch.equal(short[:3], dev[4:7]) and torch.equal(short[3], dev[6]) and torch.equal(short[4], dev[6])
    assert torch.equal(get_maskvideo_to_video_latent(torch.from_numpy(video), 5, size), dev[:5])


def test_argument_errors():
    from flexam_amd import frames as FR
    from flexam_amd import hip as H
    lib = H.lib()
    src = torch.zeros(1, 1, 8, 8, device=DEV)
    dst = torch.zeros(1, 1, 4, 4, device=DEV)
    yt, xt = FR._table(8, 4, True, torch.device(DEV)), FR._table(8, 4, True, torch.device(DEV))
    p = (yt[0].data_ptr(), yt[1].data_ptr(), yt[1].shape[1], xt[0].data_ptr(), xt[1].data_ptr(), xt[1].shape[1])

    def call(s=src.data_ptr(), d=dst.data_ptr(), T=1, C=1, oh=4, tab=p, div=1.0):
        return lib.flexam_frames_resize(s, 0, 64, 64, 8, 1, T, C, 8, 8, d, 16, 16, 4, oh, 4, *tab, 1.0, div, 0.0, None)
    assert call(s=None) == -1 and b"null pointer" in lib.flexam_last_error()
    assert call(d=None) == -1
    assert call(tab=(None,) + p[1:]) == -1
    assert call(T=0) == -2 and b"T=0" in lib.flexam_last_error()
    assert call(oh=0) == -2
    assert call(tab=p[:2] + (H.FRAMES_MAX_TAPS + 1,) + p[3:]) == -2 and b"tap table" in lib.flexam_last_error()
    assert call(tab=p[:5] + (9,)) == -2 and b"tap count over" in lib.flexam_last_error()
    assert call(tab=p[:2] + (0,) + p[3:]) == -2
    assert call(div=0.0) == -1
    assert call() == 0
    out = torch.zeros(2, 4, 4, 3, dtype=torch.uint8, device=DEV)
    clip = torch.zeros(3, 2, 4, 4, device=DEV)
    assert lib.flexam_frames_to_bytes(None, 0, 3, 2, 4, 4, 1, out.data_ptr(), None) == -1 and b"null pointer" in lib.flexam_last_error()
    assert lib.flexam_frames_to_bytes(clip.data_ptr(), 0, 3, 0, 4, 4, 1, out.data_ptr(), None) == -2
    assert lib.flexam_frames_to_bytes(clip.data_ptr(), 0, 5, 2, 4, 4, 1, out.data_ptr(), None) == -2 and b"C=5" in lib.flexam_last_error()
    # the wrappers check what the C side cannot
    with pytest.raises(RuntimeError, match="GPU view"):
        H.frames_resize(src.cpu(), dst, yt, xt)
    with pytest.raises(RuntimeError, match="contiguous columns"):
        H.frames_resize(src, torch.zeros(1, 1, 4, 8, device=DEV)[..., ::2], yt, xt)
    with pytest.raises(RuntimeError, match="tap index"):
        H.frames_resize(src, dst, FR._table(8, 5, True, torch.device(DEV)), xt)
    with pytest.raises(RuntimeError, match="taps per output"):
        H.frames_resize(src[:, :, :2], dst, yt, xt)                             # a table with more taps than the axis has samples
    with pytest.raises(RuntimeError, match="contiguous float32 or bf16"):
        H.frames_to_bytes(clip.permute(0, 1, 3, 2))
    with pytest.raises(RuntimeError, match="out must be"):
        H.frames_to_bytes(clip, out=out[:1])
