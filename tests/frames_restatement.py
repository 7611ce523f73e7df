"""Restatements for flexam_amd.frames, shared by tests/test_frames_cpu.py and tests/test_frames_gpu.py: the resize tables applied in
float64, torch's CPU `F.interpolate` as the reference (computed once per case), the tolerance that separates the two, the to-bytes
chain in numpy float32, and a synthetic 0 / 255 blob mask video."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

# (H, W) -> (oh, ow): mostly non-integer scales, both directions, an identity, odd widths (53, 59, 47: unaligned uint8 [T, H, W, 3] rows)
SHAPES = [((37, 53), (16, 32)), ((16, 24), (32, 48)), ((38, 59), (16, 32)), ((33, 47), (33, 47)), ((135, 240), (64, 112)),
          ((90, 130), (16, 32)), ((7, 9), (16, 32))]


def dense(n_in, n_out, antialias):
    """The axis table as a float64 matrix [n_out, n_in], and its largest tap count."""
    from flexam_amd.frames import resize_tables
    first, count, w = resize_tables(n_in, n_out, antialias)
    assert first.dtype == np.int32 and count.dtype == np.int32 and w.dtype == np.float32 and w.shape == (n_out, count.max())
    m = np.zeros((n_out, n_in))
    for i in range(n_out):
        assert count[i] >= 1 and first[i] >= 0 and first[i] + count[i] <= n_in and not w[i, count[i]:].any()
        m[i, first[i]:first[i] + count[i]] = w[i, :count[i]]
    return m, int(count.max())


def tolerance(h, w, oh, ow, antialias, peak=255.0):
    """Accumulation rounding only: one rounding per multiply-add of the taps_y * taps_x products plus the weight normalisation, on data
    up to `peak`: peak * 2^-24 * (taps_y * taps_x + 4), tap counts read from the tables."""
    return peak * 2.0 ** -24 * (dense(h, oh, antialias)[1] * dense(w, ow, antialias)[1] + 4)


def apply_tables(x, size, antialias):
    """x [T, C, H, W] -> float64 [T, C, oh, ow] through the tables."""
    return dense(x.shape[2], size[0], antialias)[0] @ np.asarray(x, np.float64) @ dense(x.shape[3], size[1], antialias)[0].T


@functools.lru_cache(maxsize=None)
def case(h, w, dtype="u8", t=5, c=3, seed=0):
    """Seeded frames [T, H, W, C] (numpy, read-only): uint8, or float32 uniform in [0, 255]."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    x = rng.integers(0, 256, (t, h, w, c), dtype=np.uint8) if dtype == "u8" else (rng.random((t, h, w, c)) * 255).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(h, w, oh, ow, antialias, dtype="u8", t=5, c=3, seed=0):
    """torch's CPU F.interpolate of case(...).float(): [T, C, oh, ow] float32 (numpy, read-only)."""
    x = torch.from_numpy(case(h, w, dtype, t, c, seed).copy()).permute(0, 3, 1, 2).float()
    y = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False, antialias=antialias).numpy()
    y.setflags(write=False)
    return y


def to_bytes(x, signed=True):
    """decode_latents -> save_videos_grid(rescale=False) for one clip in numpy float32: x [C, T, H, W] float32 -> uint8 [T, H, W, C]."""
    x = np.asarray(x, np.float32)
    if signed:
        x = x / np.float32(2.0) + np.float32(0.5)
    x = np.where(np.isnan(x), np.float32(0.0), np.minimum(np.maximum(x, np.float32(0.0)), np.float32(1.0)))     # NaN -> 0: the library's choice
    return np.ascontiguousarray((x * np.float32(255.0)).astype(np.uint8).transpose(1, 2, 3, 0))


def bytes_case(shape, seed=0):
    """A clip [C, T, H, W] float32 in about [-1.3, 1.3] with the awkward values planted: +-1 and beyond, exact multiples of 1 / 255 on both
    scales, their float32 neighbours, zeros."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.3, 1.3, shape).astype(np.float32)
    flat = x.reshape(-1)
    k = np.arange(256, dtype=np.float32)
    special = np.concatenate([[-1.0, 1.0, -1.5, 2.0, 0.0, -0.0, 0.5, -0.5], k / np.float32(255.0), k / np.float32(255.0) * 2 - 1,
                              np.nextafter(k / np.float32(255.0), np.float32(2.0)), np.nextafter(k / np.float32(255.0), np.float32(-2.0)),
                              np.nextafter(k / np.float32(255.0) * 2 - 1, np.float32(2.0))]).astype(np.float32)
    pos = rng.choice(flat.size, special.size, replace=False)
    flat[pos] = special
    return x


def blob_mask_video(frames=9, h=135, w=240, seed=3):
    """A 0 / 255 mask video [frames, H, W, 3] uint8: frame 0 empty, then a disc and a box that move."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = rng.uniform(50, 85), rng.uniform(80, 160)
    v = np.zeros((frames, h, w, 3), np.uint8)
    for f in range(1, frames):
        disc = (yy - (cy + 1.5 * f)) ** 2 + (xx - (cx + 2.5 * f)) ** 2 < 24.0 ** 2
        box = (abs(yy - 30 - f) < 9) & (abs(xx - 40 - 2 * f) < 14)
        v[f][disc | box] = 255
    return v
