"""Pixels across the boundary, on the GPU: decoded frames in (resize + convert), finished clip out (bytes).  csrc/frames.hip.

The reference does this work on the host, frame by frame:
  * FlexAM/utils/utils.py:473-517 `get_maskvideo_to_video_latent` -- decoded mask frames `.float()`, torchvision `resize` per frame
    (bilinear, antialiased for float tensors); demo.py:380-384, comfyui/wan2_2_fun_flexam/nodes.py:546-555;
  * utils.py:424-438, 447-449 the tensor branch of `get_video_to_video_latent` -- `F.interpolate(bilinear, align_corners=False)`,
    `.cpu().numpy()`, `* 255`, `/ 255`, a permute; nodes.py:560, 586-591;
  * utils.py:59-88 `save_videos_grid` behind `decode_latents` -- `x / 2 + 0.5`, clamp, `* 255`, `astype(np.uint8)`.
Here the frames are uploaded as they are (uint8 stays uint8), one kernel resizes, converts and writes the layout the next stage takes,
and the clip leaves the device as bytes.  The tap tables of the resize are built on the host in float32, step for step as torch's
float path builds them (`resize_tables`), and cached per (n_in, n_out, antialias, device).

Out of scope: cv2's fixed-point `resize` and PIL's `Image.resize` (the file-path branches, `get_image_latent`), video decoding and
mp4 writing, `color_transfer`.
"""
import numpy as np
import torch

from . import hip

__all__ = ["resize_tables", "resize_frames", "frames_to_bytes", "get_maskvideo_to_video_latent", "get_video_to_video_latent"]

_TABLES = {}
_F32, _F64 = np.float32, np.float64


def resize_tables(n_in: int, n_out: int, antialias: bool):
    """One axis of `F.interpolate(x.float(), mode="bilinear", align_corners=False, antialias=antialias)`, n_in -> n_out samples, as
    torch's CPU float path computes it (ATen UpSample.h `area_pixel_compute_source_index` / `guard_index_and_lambda`; UpSampleKernel.cpp
    `_compute_indices_min_size_weights_aa`), every operation in the width it has there.  Returns (first [n_out] int32, count [n_out]
    int32, weights [n_out, K] float32): output i = sum_j weights[i, j] * in[first[i] + j] over j < count[i]; K = count.max(), the
    rest of a row is 0.  first[i] + count[i] <= n_in always."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize_tables: sizes must be positive, got {n_in} -> {n_out}")
    scale = _F32(n_in) / _F32(n_out)
    i = np.arange(n_out, dtype=np.int64)
    if not antialias:
        if n_in == n_out:                                        # torch copies the index: weights 1 and 0
            return i.astype(np.int32), np.ones(n_out, np.int32), np.ones((n_out, 1), _F32)
        s = np.maximum((_F64(scale) * (i.astype(_F64) + 0.5) - 0.5).astype(_F32), _F32(0.0))      # one rounding: torch's build contracts it to an fma
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        lam = np.minimum(np.maximum(s - i0.astype(_F32), _F32(0.0)), _F32(1.0)).astype(_F32)
        two = i0 < n_in - 1                                      # at the last sample both of torch's taps read it: one tap, w0 + w1
        w = np.zeros((n_out, 2), _F32)
        w[:, 0] = np.where(two, _F32(1.0) - lam, (_F32(1.0) - lam) + lam)
        w[:, 1] = np.where(two, lam, _F32(0.0))
        count = np.where(two, 2, 1).astype(np.int32)
        k = int(count.max())
        return i0.astype(np.int32), count, np.ascontiguousarray(w[:, :k])
    support = scale if scale >= 1.0 else _F32(1.0)
    inv = _F32(_F64(1.0) / _F64(scale)) if scale >= 1.0 else _F32(1.0)
    center = (_F64(scale) * (i.astype(_F64) + 0.5)).astype(_F32)             # the product is formed in double and rounded once
    lo = np.maximum(((center - support).astype(_F64) + 0.5).astype(np.int64), 0)
    hi = np.minimum(((center + support).astype(_F64) + 0.5).astype(np.int64), n_in)
    count = np.maximum(hi - lo, 0)
    k = int(count.max())
    j = lo[:, None] + np.arange(k, dtype=np.int64)[None, :]
    x = (((j.astype(_F32) - center[:, None]).astype(_F64) + 0.5) * _F64(inv)).astype(_F32)
    w = np.where(np.arange(k)[None, :] < count[:, None], np.maximum(_F32(1.0) - np.abs(x), _F32(0.0)), _F32(0.0)).astype(_F32)
    total = np.zeros(n_out, _F32)
    for t in range(k):                                           # torch adds the taps up one by one in float32
        total = (total + w[:, t]).astype(_F32)
    w = np.where(total[:, None] != 0, w / np.where(total == 0, _F32(1.0), total)[:, None], w).astype(_F32)
    return lo.astype(np.int32), count.astype(np.int32), np.ascontiguousarray(w)


def _device(x, device):
    if device is not None:
        d = torch.device(device)
        return d if d.index is not None else torch.device(d.type, torch.cuda.current_device())
    if torch.is_tensor(x) and x.is_cuda:
        return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _table(n_in, n_out, antialias, device):
    """(index [n_out, 2] int32 = (first, count), weights [n_out, K] float32) on `device`."""
    key = (int(n_in), int(n_out), bool(antialias), str(device))
    if key not in _TABLES:
        first, count, w = resize_tables(n_in, n_out, antialias)
        _TABLES[key] = (torch.from_numpy(np.stack([first, count], axis=1).copy()).to(device), torch.from_numpy(w).to(device))
    return _TABLES[key]


def _as_frames(frames, what):
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(frames)
    if not torch.is_tensor(frames) or frames.dim() != 4:
        raise TypeError(f"{what}: a 4-D torch tensor or numpy array of frames is required")
    if frames.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"{what}: uint8 or float32 frames required, got {frames.dtype}")
    return frames


def resize_frames(frames, size, antialias, layout_in="thwc", layout_out="tchw", mul=1.0, add=0.0, device=None, div=1.0, out=None):
    """`F.interpolate(frames.float(), size=size, mode="bilinear", align_corners=False, antialias=antialias)` over a stack of frames,
    then `y * mul / div + add` (three roundings, each step skipped at its neutral value; `/ 255` is a division, not a product with
    a rounded reciprocal).  frames: torch tensor or numpy array, uint8 or float32, on the CPU or the GPU, any strides, [T, H, W, C]
    (layout_in "thwc") or [T, C, H, W] ("tchw"); a uint8 source is widened exactly, never rounded back.  Result: float32 on the GPU,
    [T, C, oh, ow] (layout_out "tchw") or [C, T, oh, ow] ("cthw"); `out`: such a buffer (or a view with a contiguous last axis)."""
    frames = _as_frames(frames, "resize_frames")
    if layout_in not in ("thwc", "tchw") or layout_out not in ("tchw", "cthw"):
        raise ValueError(f"resize_frames: layout_in 'thwc' | 'tchw' and layout_out 'tchw' | 'cthw', got {layout_in!r}, {layout_out!r}")
    oh, ow = int(size[0]), int(size[1])
    dev = _device(frames, device)
    with torch.cuda.device(dev):
        src = frames.to(dev)
        src = src.permute(0, 3, 1, 2) if layout_in == "thwc" else src            # a (t, c, y, x) view, whatever the memory order
        T, C, H, W = src.shape
        shape = (T, C, oh, ow) if layout_out == "tchw" else (C, T, oh, ow)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        elif tuple(out.shape) != shape or out.device != dev:
            raise RuntimeError(f"resize_frames: out must be {shape} on {dev}, got {tuple(out.shape)} on {out.device}")
        dst = out if layout_out == "tchw" else out.permute(1, 0, 2, 3)
        hip.frames_resize(src, dst, _table(H, oh, antialias, dev), _table(W, ow, antialias, dev), mul=mul, div=div, add=add)
    return out


def frames_to_bytes(video, signed=True, device=None):
    """The clip as bytes: video [3, F, H, W] or [1, 3, F, H, W] (float32 or bfloat16; any channel count up to 4) -> uint8 [F, H, W, 3]
    on the GPU.  signed=True is the reference's `decode_latents` -> `save_videos_grid(rescale=False)` for one clip, bit for bit: in
    float32 `x / 2`, `+ 0.5`, clamp to [0, 1], `* 255`, each rounded on its own, then truncation toward zero (`astype(np.uint8)`).
    signed=False takes a clip already in [0, 1] (the pipeline's `.videos`): clamp, `* 255`, truncation.  NaN gives 0: this library's
    choice (the clamp here drops a NaN to 0; the reference keeps it through `clamp` and leaves the byte to numpy's cast, which yields
    0 on x86).  -inf gives 0, +inf 255.  `make_grid` over one image is that image, so no grid is built."""
    if isinstance(video, np.ndarray):
        video = torch.from_numpy(video)
    if not torch.is_tensor(video) or video.dim() not in (4, 5) or (video.dim() == 5 and video.shape[0] != 1):
        raise ValueError("frames_to_bytes: one clip [C, F, H, W] or [1, C, F, H, W] is required (no grid is built)")
    if video.dim() == 5:
        video = video[0]
    dev = _device(video, device)
    with torch.cuda.device(dev):
        return hip.frames_to_bytes(video.to(dev).contiguous(), signed=signed)


def mask_frame_plan(n_frames: int, video_length: int):
    """utils.py:482-515's frame-count rule: (frames that are resized, copies of the last resized frame appended)."""
    n_frames, video_length = int(n_frames), int(video_length)
    if n_frames < 1 or video_length < 1:
        raise ValueError(f"mask video of {n_frames} frames for video_length {video_length}")
    if n_frames < video_length:
        return n_frames, video_length - n_frames
    return video_length, 0


def get_maskvideo_to_video_latent(mask_frames, video_length, sample_size, fps=None, validation_video_mask=None, ref_image=None, device=None):
    """utils.py:473-517 with the decoded frames in place of `mask_path`: mask_frames [N, H, W, C] (uint8 as a decoder gives them, or
    float32; torch or numpy, CPU or GPU) -> [video_length, C, h, w] float32 on the 0-255 scale, on the GPU -- what
    `generate_mask_fg_tracking_for_validation` takes.  Fewer than video_length frames: all are resized and the last resized frame is
    repeated; otherwise the first video_length are used.  The resize is torchvision's for float tensors: bilinear, antialiased.
    `fps`, `validation_video_mask` and `ref_image` are unused, as in the reference.  None (no mask video) gives None."""
    if mask_frames is None:
        return None
    if isinstance(mask_frames, (str, bytes)) or hasattr(mask_frames, "__fspath__"):
        raise NotImplementedError("get_maskvideo_to_video_latent: reading a mask video file needs decord, which this build does not "
                                  "have; pass the decoded frames [N, H, W, C]")
    frames = _as_frames(mask_frames, "get_maskvideo_to_video_latent")
    used, repeat = mask_frame_plan(frames.shape[0], video_length)
    dev = _device(frames, device)
    h, w = int(sample_size[0]), int(sample_size[1])
    out = torch.empty((used + repeat, frames.shape[3], h, w), dtype=torch.float32, device=dev)
    resize_frames(frames[:used], (h, w), True, "thwc", "tchw", device=dev, out=out[:used])
    if repeat:
        out[used:] = out[used - 1]
    return out


def get_video_to_video_latent(input_video, video_length, sample_size, fps=None, validation_video_mask=None, ref_image=None,
                              if_restore_255=False, device=None):
    """The tensor branch of utils.py:399-470 (:424-438, :447-449): input_video [T, H, W, 3] float32 (a ComfyUI IMAGE) ->
    (input_video [1, 3, T', h, w] = resized / 255, input_video_mask [1, 1, T', h, w] = 255, None, None) on the GPU, T' = min(T,
    video_length).  The resize is plain bilinear (no antialias), as there.  With if_restore_255 the reference multiplies by 255 in
    float32 and divides by 255 afterwards: both roundings are made here too, so the result is that chain's, not the resized input."""
    if input_video is None:
        return None, None, None, None
    if isinstance(input_video, (str, bytes)) or hasattr(input_video, "__fspath__"):
        raise NotImplementedError("get_video_to_video_latent: the file-path branch is cv2's VideoCapture + fixed-point resize, which "
                                  "this build does not have; pass the frames as a tensor [T, H, W, 3]")
    if validation_video_mask is not None or ref_image is not None:
        raise NotImplementedError("get_video_to_video_latent: validation_video_mask / ref_image are PIL file paths (Image.open + "
                                  "Image.resize), which this build does not restate")
    if not torch.is_tensor(input_video) or input_video.dim() != 4 or input_video.dtype != torch.float32:
        raise NotImplementedError("get_video_to_video_latent: only the tensor branch is implemented: a float32 tensor [T, H, W, C]")
    dev = _device(input_video, device)
    h, w = int(sample_size[0]), int(sample_size[1])
    clip = resize_frames(input_video[:video_length], (h, w), False, "thwc", "cthw", mul=255.0 if if_restore_255 else 1.0, div=255.0,
                         device=dev).unsqueeze(0)
    mask = torch.full((1, 1) + tuple(clip.shape[2:]), 255.0, dtype=torch.float32, device=dev)
    return clip, mask, None, None
