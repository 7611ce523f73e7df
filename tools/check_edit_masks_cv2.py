"""Compares flexam_amd's foreground-edit masks with the SciPy / OpenCV call sequence of demo.py's generate_mask_fg_tracking_for_validation,
for anyone who has both installed (the tests hold the GPU result to a numpy restatement; this is the one check against cv2 itself).

The sequence, per frame after frame 0: channel mean, `> 0.5`; scipy.ndimage.gaussian_filter(sigma = blur_radius / 6), `> 0.5`;
cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE), cv2.convexHull + cv2.fillPoly for every contour of >= 3 points; cv2.dilate with
the MORPH_ELLIPSE element of size (2 dilation_pixels + 1)^2; `> 127`.  Prints the differing pixels per frame; the expected
differences are confined to hull edges where a line passes exactly half way between two pixels ("Foreground-edit masks").

    python tools/check_edit_masks_cv2.py [--frames 9] [--height 512] [--width 896] [--blur 15] [--dilate 200] [--seed 5]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cv2_masks(video, blur_radius, dilation_pixels):
    import cv2
    import numpy as np
    from scipy.ndimage import gaussian_filter
    grey = video.mean(axis=1)
    out = np.zeros((video.shape[0], video.shape[2], video.shape[3]), np.uint8)
    for i in range(1, video.shape[0]):
        m = (grey[i] > 0.5).astype(np.uint8) * 255
        if blur_radius > 0:
            m = (gaussian_filter(m.astype(np.float32) / 255.0, sigma=blur_radius / 6.0) > 0.5).astype(np.uint8) * 255
        contours, _ = cv2.findContours(m, cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE)
        filled = np.zeros_like(m)
        for c in contours:
            if len(c) >= 3:
                cv2.fillPoly(filled, [cv2.convexHull(c)], 255)
        if dilation_pixels > 0:
            k = cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (2 * dilation_pixels + 1, 2 * dilation_pixels + 1))
            filled = cv2.dilate(filled, k, iterations=1)
        out[i] = (filled > 127).astype(np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=9)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=896)
    ap.add_argument("--blur", type=int, default=15)
    ap.add_argument("--dilate", type=int, default=200)
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    try:
        import cv2  # noqa: F401
        import scipy.ndimage  # noqa: F401
    except ImportError as e:
        raise SystemExit(f"check_edit_masks_cv2: OpenCV and SciPy are needed for this comparison ({e}); nothing compared")
    import numpy as np
    import torch
    import edit_mask_restatement as R
    from flexam_amd import generate_mask_fg_tracking_for_validation as fg
    video = R.blob_video(args.frames, args.height, args.width, seed=args.seed)
    want = cv2_masks(video, args.blur, args.dilate)
    got = fg(torch.from_numpy(video), blur_radius=args.blur, dilation_pixels=args.dilate).cpu().numpy()[:, 0]
    total = 0
    for i in range(args.frames):
        d = int(np.count_nonzero(got[i] != want[i]))
        total += d
        print(f"frame {i}: {d} differing pixels (GPU {int(got[i].sum())} set, cv2 {int(want[i].sum())} set)")
    print(f"total differing pixels: {total}")


if __name__ == "__main__":
    main()
