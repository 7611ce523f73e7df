"""CPU: the host side of flexam_amd.frames -- the resize tables against torch's CPU `F.interpolate`, the to-bytes chain against the
reference's torch / numpy chain, the mask video's frame-count rule, the refusals, the lazy exports.  No GPU, no kernel call."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frames_restatement as R  # noqa: E402


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_tables_in_float64_equal_torch_cpu_interpolate(shape, antialias):
    """The float32 tables applied in float64 against F.interpolate on float32 data uniform in [0, 255]: accumulation rounding only.  A
    shape over the tolerance means the table's float32 arithmetic is not torch's (a float64 `scale` misses 135x240 -> 64x112 by 3.2e-3)."""
    (h, w), (oh, ow) = shape
    x = torch.from_numpy(R.case(h, w, "f32").copy()).permute(0, 3, 1, 2)
    got = R.apply_tables(x.numpy(), (oh, ow), antialias)
    want = R.reference(h, w, oh, ow, antialias, "f32")
    err, tol = float(np.abs(got - want).max()), R.tolerance(h, w, oh, ow, antialias)
    print(f"{shape} antialias={antialias}: max |table - torch| = {err:.3e}, tolerance {tol:.3e}")
    if (h, w) == (oh, ow):
        assert np.array_equal(got, x.numpy()), "the identity resize must be exact"
    assert err <= tol


def test_table_shapes_and_padding():
    from flexam_amd.frames import resize_tables
    for n_in, n_out, aa in ((135, 64, True), (16, 32, True), (16, 32, False), (1, 4, False), (1, 4, True), (9, 1, True), (9, 1, False)):
        first, count, w = resize_tables(n_in, n_out, aa)
        assert first.shape == count.shape == (n_out,) and w.shape == (n_out, count.max()) and w.dtype == np.float32
        assert (first >= 0).all() and (count >= 1).all() and (first + count <= n_in).all()
        assert np.allclose(w.sum(axis=1), 1.0, atol=1e-6)
        assert all(not w[i, count[i]:].any() for i in range(n_out))
    with pytest.raises(ValueError):
        resize_tables(0, 4, True)


def _torch_chain(x, signed):
    """decode_latents (`(x / 2 + 0.5).clamp(0, 1)`, `.cpu().float()`) -> save_videos_grid(rescale=False) (`(x * 255).numpy().astype(np.uint8)`)."""
    v = (x.float() / 2 + 0.5).clamp(0, 1) if signed else x.float().clamp(0, 1)
    return (v.permute(1, 2, 3, 0) * 255).numpy().astype(np.uint8)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("signed", [True, False])
def test_to_bytes_restatement_is_the_reference_chain(signed, bf16):
    x = torch.from_numpy(R.bytes_case((3, 5, 17, 23)))
    if not signed:
        x = x / 2 + 0.5                                       # about [-0.15, 1.15]: the clamp still works on both ends
    if bf16:
        x = x.bfloat16()
    got = R.to_bytes(x.float().numpy(), signed)
    assert np.array_equal(got, _torch_chain(x, signed))
    assert got.min() == 0 and got.max() == 255


def test_to_bytes_at_the_edges():
    k = np.arange(256, dtype=np.float32)
    x = (k / np.float32(255.0))[None, None, None, :]
    assert np.array_equal(R.to_bytes(x, signed=False), _torch_chain(torch.from_numpy(x), False))
    e = np.array([-1.0, 1.0, -3.0, 3.0, np.inf, -np.inf, np.nan, -0.0], np.float32)[None, None, None, :]
    assert R.to_bytes(e, signed=True).reshape(-1).tolist() == [0, 255, 0, 255, 255, 0, 0, 127]


def test_mask_frame_plan():
    from flexam_amd.frames import mask_frame_plan
    assert mask_frame_plan(3, 5) == (3, 2)                    # all three resized, the last repeated twice
    assert mask_frame_plan(9, 5) == (5, 0)                    # the first five
    assert mask_frame_plan(5, 5) == (5, 0)
    with pytest.raises(ValueError):
        mask_frame_plan(0, 5)


def test_refusals_without_a_gpu():
    from flexam_amd import frames as FR
    with pytest.raises(NotImplementedError, match="decord"):
        FR.get_maskvideo_to_video_latent("mask.mp4", 5, (16, 32))
    assert FR.get_maskvideo_to_video_latent(None, 5, (16, 32)) is None
    with pytest.raises(NotImplementedError, match="cv2"):
        FR.get_video_to_video_latent("clip.mp4", 5, (16, 32))
    x = torch.zeros(2, 8, 8, 3)
    with pytest.raises(NotImplementedError, match="PIL"):
        FR.get_video_to_video_latent(x, 5, (16, 32), validation_video_mask="m.png")
    with pytest.raises(NotImplementedError, match="PIL"):
        FR.get_video_to_video_latent(x, 5, (16, 32), ref_image="r.png")
    with pytest.raises(NotImplementedError, match="tensor branch"):
        FR.get_video_to_video_latent(x.to(torch.uint8), 5, (16, 32))
    assert FR.get_video_to_video_latent(None, 5, (16, 32)) == (None, None, None, None)
    with pytest.raises(TypeError, match="uint8 or float32"):
        FR.resize_frames(torch.zeros(2, 8, 8, 3, dtype=torch.float64), (4, 4), True)
    with pytest.raises(ValueError, match="layout"):
        FR.resize_frames(x, (4, 4), True, layout_in="hwc")
    with pytest.raises(ValueError, match="one clip"):
        FR.frames_to_bytes(torch.zeros(2, 3, 4, 8, 8))


def test_no_cpu_path():
    """Frames on the CPU are uploaded, never resized there: without a GPU the call fails instead of falling back to torch."""
    from flexam_amd import frames as FR
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises((RuntimeError, AssertionError)):
        FR.resize_frames(torch.zeros(2, 8, 8, 3), (4, 4), True)


def test_public_names_are_exported_lazily():
    import flexam_amd
    from flexam_amd import frames as FR
    for name in ("resize_tables", "resize_frames", "frames_to_bytes", "get_maskvideo_to_video_latent", "get_video_to_video_latent"):
        assert getattr(flexam_amd, name) is getattr(FR, name) and name in flexam_amd.__all__


def test_entry_points_are_declared_and_built():
    from flexam_amd import abi, build, hip
    assert "frames.hip" in build.SOURCES
    for name in ("flexam_frames_resize", "flexam_frames_to_bytes"):
        assert name in hip._SIGNATURES and name in hip._REPLAYABLE
        assert len(hip._SIGNATURES[name][0]) <= abi.CONSTANTS["FLEXAM_REPLAY_MAX_ARGS"]
