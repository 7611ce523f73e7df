"""The masks of demo.py's `foreground_edit` / `background_edit` branch (demo.py:33-126, run at :380-389 on the decoded mask video
before the pipeline call), on the GPU.

`generate_mask_fg_tracking_for_validation` refines every frame after frame 0 through csrc/edit_mask.hip: channel mean and `> 0.5`
(torch, on the device), scipy's Gaussian blur and `> 0.5` (bit-exact), the union of the filled convex hulls of the 8-connected
components (cv2.findContours RETR_EXTERNAL + convexHull + fillPoly), and a dilation with cv2's MORPH_ELLIPSE element of size
(2 dilation_pixels + 1)^2.  `generate_mask_bg_tracking_for_validation` is a few tensor ops.  Both keep the reference's names and
arguments and add `device`; the result stays on the GPU.
"""
import numpy as np
import torch

from . import hip

_TABLES = {}


def gaussian_weights(blur_radius) -> np.ndarray:
    """scipy.ndimage.gaussian_filter's kernel for sigma = blur_radius / 6 (truncate 4): its normalised weights from the centre outwards."""
    sigma = blur_radius / 6.0
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return phi[radius:].copy()


def ellipse_half_widths(r: int) -> np.ndarray:
    """Row half widths of cv2.getStructuringElement(MORPH_ELLIPSE, (2r+1, 2r+1)) for |dy| = 0 .. r: cvRound(r sqrt((r^2 - dy^2) / r^2)),
    the quotient taken as OpenCV does, times 1 / r^2; cvRound rounds halves to even."""
    dy = np.arange(r + 1)
    return np.rint(r * np.sqrt((r * r - dy * dy) * (1.0 / (r * r)))).astype(np.int32)


def _table(kind, arg, device):
    key = (kind, arg, str(device))
    if key not in _TABLES:
        if kind == "blur":
            _TABLES[key] = torch.from_numpy(gaussian_weights(arg)).to(device)
        else:
            _TABLES[key] = torch.from_numpy(ellipse_half_widths(arg) if arg > 0 else np.zeros(1, np.int32)).to(device)
    return _TABLES[key]


def _device(x, device):
    if device is not None:
        return torch.device(device)
    return x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())


def generate_mask_fg_tracking_for_validation(mask_video_input, blur_radius: int = 15, dilation_pixels: int = 200, device=None):
    """demo.py:33-96.  mask_video_input [F, C, H, W] float (CPU or GPU; thresholds are `> 0.5` on whatever scale arrives, so with the
    demo's 0-255 frames every non-black pixel counts) -> uint8 {0, 1} [F, 1, H, W] on the GPU.  Frame 0 is all zeros and is not
    processed.  Per later frame: grey = channel mean > 0.5; Gaussian blur with sigma = blur_radius / 6 and > 0.5 again (skipped when
    blur_radius <= 0); the filled convex hull of every 8-connected component whose pixel centres are not collinear; dilation by the
    elliptical element of radius dilation_pixels (skipped when dilation_pixels <= 0)."""
    dev = _device(mask_video_input, device)
    f, _, h, w = mask_video_input.shape
    out = torch.zeros((f, 1, h, w), dtype=torch.uint8, device=dev)
    if f == 1:
        return out
    with torch.cuda.device(dev):
        x = mask_video_input[1:].to(dev)
        binary = (x.mean(dim=1) > 0.5).to(torch.uint8)
        if blur_radius > 0:
            binary = hip.edit_mask_blur(binary, _table("blur", blur_radius, dev))
        runs, nruns = hip.edit_mask_hull(binary)
        radius = max(int(dilation_pixels), 0)
        hip.edit_mask_dilate(runs, nruns, w, _table("ellipse", radius, dev), out=out[1:, 0])
    return out


def generate_mask_bg_tracking_for_validation(mask_video_input, device=None):
    """demo.py:98-126 (not nodes.py:73-160's variant, which returns uint8, tests `<= 0.5` and does not normalise).  [F, C, H, W] ->
    float32 [F, 1, H, W] on the GPU: frame 0 is zeros; every later frame is its channel mean, divided by 255 when its maximum is > 1,
    then `< 0.5` (1 = a black pixel).  Device tensor ops only, no host synchronisation."""
    dev = _device(mask_video_input, device)
    f, _, h, w = mask_video_input.shape
    mask = torch.zeros((f, 1, h, w), dtype=torch.float32, device=dev)
    if f > 1:
        grey = mask_video_input[1:].to(dev).mean(dim=1, keepdim=True)
        peak = grey.amax(dim=(1, 2, 3), keepdim=True)
        mask[1:] = (torch.where(peak > 1.0, grey / 255.0, grey) < 0.5).float()
    return mask
