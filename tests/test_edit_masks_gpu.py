"""GPU: demo.py's foreground / background edit masks (flexam_amd/edit_masks.py, csrc/edit_mask.hip) against the numpy restatement of
tests/edit_mask_restatement.py -- bit for bit.  No SciPy or OpenCV here."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_mask_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fg(frames, **kw):
    from flexam_amd import generate_mask_fg_tracking_for_validation
    return generate_mask_fg_tracking_for_validation(frames, **kw)


def _video(planes):
    """[F-1] list of bool [H, W] -> [F, 1, H, W] float32 (0 / 1) with an empty frame 0 in front."""
    v = np.stack([np.zeros_like(planes[0])] + list(planes)).astype(np.float32)
    return torch.from_numpy(v[:, None])


def _frames_for_stages():
    rng = np.random.default_rng(11)
    out = []
    for p in (0.02, 0.2, 0.5, 0.8, 0.97):
        out.append(rng.random((37, 53)) < p)
    cb = (np.add.outer(np.arange(24), np.arange(31)) % 2).astype(bool)
    out.append(cb)
    lines = np.zeros((40, 45), bool)
    lines[3, 2:40] = True
    lines[5:38, 7] = True
    lines[np.arange(30) + 6, np.arange(30) + 10] = True
    lines[10:30, 44] = True
    out.append(lines)
    border = np.zeros((29, 33), bool)
    border[0, :] = border[:, 0] = border[-1, 10:20] = border[5:9, -1] = True
    out.append(border)
    for h, w in ((5, 5), (5, 9), (7, 6), (13, 5)):
        out.append(rng.random((h, w)) < 0.4)
    out.append(np.ones((21, 17), bool))
    return out


@pytest.mark.parametrize("blur_radius", [15, 7, 40])
def test_blur_and_threshold_bit_exact(blur_radius):
    from flexam_amd import edit_masks as E
    from flexam_amd import hip
    w = torch.from_numpy(E.gaussian_weights(blur_radius)).to(DEV)
    for i, b in enumerate(_frames_for_stages()):
        got = hip.edit_mask_blur(torch.from_numpy(np.stack([b, ~b]).astype(np.uint8)).to(DEV), w).cpu().numpy()
        for k, frame in enumerate((b, ~b)):
            want = R.gaussian_blur(frame.astype(np.float32), blur_radius / 6.0) > 0.5
            assert np.array_equal(got[k].astype(bool), want), (i, k, blur_radius)


def test_hull_fill_exact():
    planes = []
    a = np.zeros((60, 70), bool)
    yy, xx = np.mgrid[0:60, 0:70]
    ring = ((yy - 30) ** 2 + (xx - 30) ** 2 < 25 ** 2) & ((yy - 30) ** 2 + (xx - 30) ** 2 >= 15 ** 2)
    a |= ring
    a[27:33, 28:32] = True                               # a component nested in the ring's hole
    a[2:5, 60:69] = True
    a[50, 55:66] = True                                  # collinear: one row
    a[40:55, 68] = True                                  # collinear: one column
    a[np.arange(8) + 45, np.arange(8) + 2] = True        # collinear: a diagonal
    a[20, 62] = True                                     # a 1-pixel component
    a[0, 40:46] = a[1, 38:41] = True                     # touching the top border
    a[57:60, 0:3] = True                                 # bottom-left corner
    a[30:36, 67:70] = True                               # right border
    a[10, 0], a[12, 1], a[11, 2] = True, True, True      # left border, 8-connected by corners
    planes.append(a)
    rng = np.random.default_rng(5)
    for p in (0.05, 0.15, 0.3):
        planes.append(rng.random((41, 57)) < p)
    planes.append((np.add.outer(np.arange(16), np.arange(19)) % 2).astype(bool))
    planes.append(np.ones((9, 11), bool))
    for plane in planes:
        got = _fg(_video([plane]), blur_radius=0, dilation_pixels=0)[1, 0].cpu().numpy()
        assert np.array_equal(got.astype(bool), R.hull_fill(plane))


@pytest.mark.parametrize("r", [1, 2, 7, 30])
def test_dilation_exact(r):
    rng = np.random.default_rng(r)
    planes = [rng.random((64, 80)) < 0.01, np.zeros((64, 80), bool)]
    planes[1][30:34, 0:5] = True
    planes[1][0:3, 70:80] = True
    planes[1][60:64, 40:45] = True
    v = _video(planes)
    filled = _fg(v, blur_radius=0, dilation_pixels=0).cpu().numpy()[:, 0].astype(bool)
    got = _fg(v, blur_radius=0, dilation_pixels=r).cpu().numpy()[:, 0].astype(bool)
    el = R.ellipse_element(r)
    for f in (1, 2):
        want = np.zeros_like(filled[f])
        H, W = want.shape
        for y, x in zip(*np.nonzero(filled[f])):                          # brute force: stamp the element on every set pixel
            y0, y1, x0, x1 = max(0, y - r), min(H, y + r + 1), max(0, x - r), min(W, x + r + 1)
            want[y0:y1, x0:x1] |= el[y0 - y + r:y1 - y + r, x0 - x + r:x1 - x + r]
        assert np.array_equal(got[f], want), (r, f)


def test_end_to_end_full_size_defaults():
    """97 x 512 x 896 at default arguments.  The restatement takes 0.1-0.4 s a frame on the host, so it checks a spread of 16 of the 96
    refined frames, the last one included; the GPU result must also repeat bit for bit."""
    video = torch.from_numpy(R.blob_video(97, 512, 896, seed=5))
    got = _fg(video.to(DEV))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (97, 1, 512, 896) and got.is_cuda
    assert not got[0].any() and set(torch.unique(got).tolist()) <= {0, 1}
    assert torch.equal(got, _fg(video.to(DEV))), "two runs differ"
    grey = video.mean(dim=1).numpy()
    frames = sorted(set(np.linspace(1, 96, 16).round().astype(int).tolist()))
    assert 96 in frames
    g = got.cpu().numpy()[:, 0]
    for f in frames:
        assert np.array_equal(g[f], R.refine_frame(grey[f])), f
    # the same clip in another form: CPU input, 0/1 scale, one channel
    assert torch.equal(_fg((video[:, :1] / 255.0).contiguous()), got)


def test_input_forms_and_small_cases():
    rng = np.random.default_rng(9)
    planes = [(rng.random((48, 64)) < 0.004) for _ in range(3)]
    for p in planes:
        p[10:30, 20:40] = True
    one = _video(planes)                                    # [4, 1, H, W] in 0 / 1
    three = (one.repeat(1, 3, 1, 1) * 255.0)                 # 3 channels in 0-255
    want = _fg(one.to(DEV), dilation_pixels=5)
    assert torch.equal(want, _fg(three, dilation_pixels=5)) and torch.equal(want, _fg(three.to(DEV), dilation_pixels=5))
    for f, p in enumerate(planes, start=1):
        assert np.array_equal(want[f, 0].cpu().numpy(), R.refine_frame(p.astype(np.float32), dilation_pixels=5))
    # 0-255: any non-black pixel counts (thresholds are > 0.5 on the scale that arrives)
    assert torch.equal(_fg(one * 1.2, dilation_pixels=5), want)
    single = _fg(one[:1], dilation_pixels=5)
    assert tuple(single.shape) == (1, 1, 48, 64) and single.dtype == torch.uint8 and single.is_cuda and not single.any()


def test_background_mask_follows_demo():
    rng = np.random.default_rng(4)
    from flexam_amd import generate_mask_bg_tracking_for_validation as bg
    for scale, c in ((255.0, 3), (1.0, 3), (255.0, 1)):
        x = torch.from_numpy((rng.random((5, c, 20, 24)) * scale).astype(np.float32))
        got = bg(x)
        assert got.dtype == torch.float32 and tuple(got.shape) == (5, 1, 20, 24) and got.is_cuda
        want = torch.zeros(5, 1, 20, 24)
        for f in range(1, 5):                                 # demo.py:113-124, restated
            g = x[f].mean(dim=0, keepdim=True) if c > 1 else x[f]
            n = g / 255.0 if g.max() > 1.0 else g
            want[f] = (n < 0.5).float()
        assert torch.equal(got.cpu(), want)
    assert not bg(torch.ones(1, 3, 4, 4) * 255).any()


def test_demo_form_feeds_mask_video_unchanged():
    """demo.py:389: (m * 255).unsqueeze(0).permute(0, 2, 1, 3, 4) as mask_video gives the mask_pixels / mask latents of the float mask."""
    from flexam_amd.pipeline_wan2_2_fun_control_FlexAM import Wan2_2FunControlPipeline_FlexAM as P
    from flexam_amd.pipeline_wan2_2_fun_control_FlexAM import prepare_masks
    video = torch.from_numpy(R.blob_video(9, 64, 96, seed=2))
    m = _fg(video, dilation_pixels=6)
    demo = (m * 255).unsqueeze(0).permute(0, 2, 1, 3, 4)
    assert demo.dtype == torch.uint8
    flt = m.float().unsqueeze(0).permute(0, 2, 1, 3, 4)
    a, b = P._preprocess(demo, 64, 96, mask=True), P._preprocess(flt, 64, 96, mask=True)
    assert torch.equal(a, b) and a.any()
    for u, v in zip(prepare_masks(a, (1, 48, 3, 8, 12)), prepare_masks(b, (1, 48, 3, 8, 12))):
        assert (torch.equal(u, v) if torch.is_tensor(u) else u == v)


def test_argument_errors():
    from flexam_amd import hip as H
    b = torch.zeros(2, 8, 8, dtype=torch.uint8, device=DEV)
    w = torch.ones(1, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="uint8 frames"):
        H.edit_mask_blur(b.float(), w)
    with pytest.raises(RuntimeError, match="float64"):
        H.edit_mask_blur(b, w.float())
    with pytest.raises(RuntimeError, match="frames up to"):
        H.edit_mask_hull(torch.zeros(1, 4097, 4, dtype=torch.uint8, device=DEV))
    runs, nruns = H.edit_mask_hull(b)
    hw = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="ceil"):
        H.edit_mask_dilate(runs, nruns, 10, hw)
    with pytest.raises(RuntimeError, match="nruns"):
        H.edit_mask_dilate(runs, nruns[:1], 8, hw)
    lib = H.lib()
    assert lib.flexam_edit_mask_blur(None, 1, 8, 8, None, 0, None, None, None) == -1
    assert b"null pointer" in lib.flexam_last_error()
    assert lib.flexam_edit_mask_dilate(runs.data_ptr(), nruns.data_ptr(), 2, 8, 8, hw.data_ptr(), -1, b.data_ptr(), None) == -2
    assert b"radius" in lib.flexam_last_error()
    assert lib.flexam_edit_mask_hull(b.data_ptr(), 2, 8, 8, runs.data_ptr(), nruns.data_ptr(), runs.data_ptr(), 0, None) == -2
    assert torch.equal(H.edit_mask_dilate(runs, nruns, 8, hw), b)
