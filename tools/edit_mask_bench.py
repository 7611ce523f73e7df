"""Times the foreground-edit mask refinement (flexam_amd.edit_masks.generate_mask_fg_tracking_for_validation) on the GPU at default
arguments (blur_radius 15, dilation_pixels 200) on seeded moving-blob mask videos of 49 x 512 x 896 (demo.py's default length) and
97 x 512 x 896, with the input already on the device.  Warm-up first; each timing ends in a device synchronise; best of N.

Also times the numpy restatement of tests/edit_mask_restatement.py on a few frames on the host: a restatement written for the tests,
NOT the reference (scipy + OpenCV), whose cost is not measured here.

    python tools/edit_mask_bench.py [--repeats 20] [--out profiles/edit_mask_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-frames", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import edit_mask_restatement as R
    from flexam_amd import generate_mask_fg_tracking_for_validation as fg
    if not torch.cuda.is_available():
        raise SystemExit("edit_mask_bench: no GPU (this measures the GPU path; there is nothing to fall back to)")
    rec = {"device": torch.cuda.get_device_name(0), "args": "blur_radius=15 dilation_pixels=200", "gpu": {}}
    for frames in (49, 97):
        video = torch.from_numpy(R.blob_video(frames, 512, 896, seed=5)).cuda()
        for _ in range(3):
            fg(video)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fg(video)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        rec["gpu"][f"{frames}x512x896"] = {"best_ms": round(1e3 * min(times), 3), "median_ms": round(1e3 * float(np.median(times)), 3),
                                           "repeats": args.repeats}
    grey = R.blob_video(4, 512, 896, seed=5).mean(axis=1)
    t0 = time.perf_counter()
    for f in range(1, 1 + args.host_frames):
        R.refine_frame(grey[1 + (f - 1) % 3])
    rec["numpy_restatement_per_frame_s"] = round((time.perf_counter() - t0) / args.host_frames, 3)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
