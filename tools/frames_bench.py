"""Times flexam_amd.frames against the host path it replaces, written with torch on the CPU, on the same box (one run):
  (a) 97 x 1080 x 1920 x 3 uint8 mask frames -> 512 x 896, antialiased, upload included  vs  `.float()` + per-frame antialiased resize;
  (b) one 97 x 512 x 896 x 3 float32 stream through get_video_to_video_latent's tensor branch (to 480 x 832, if_restore_255)  vs  the
      reference's F.interpolate / .numpy() / * 255 / / 255 / permute;
  (c) [3, 97, 512, 896] float32 -> bytes + the 134 MB device-to-host copy  vs  the 534 MB float32 copy + host `* 255` / astype.
Also the two kernels alone (inputs on the device) with their achieved GB/s (bytes read + written once / time), to put beside the
plain-copy rate the row kernels are compared with.  Warm-up first; each timing ends in a device synchronise; best of N.
The host side runs on `--threads` torch threads (default 16); the record states them and the box's CPU count.

    python tools/frames_bench.py [--repeats 5] [--threads 16] [--only a|b|c] [--out profiles/frames_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best(fn, repeats, sync):
    fn()
    sync()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        times.append(time.perf_counter() - t0)
    return round(1e3 * min(times), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--only", default="abc")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from flexam_amd import frames as FR
    if not torch.cuda.is_available():
        raise SystemExit("frames_bench: no GPU (this measures the GPU path; there is nothing to fall back to)")
    torch.set_num_threads(args.threads)
    sync, nosync = torch.cuda.synchronize, (lambda: None)
    rec = {"device": torch.cuda.get_device_name(0), "nproc": os.cpu_count(), "host_threads": torch.get_num_threads(), "unit": "ms, best of N"}
    g = torch.Generator().manual_seed(0)
    if "a" in args.only:
        mask = (torch.rand(97, 1080, 1920, 1, generator=g) > 0.7).to(torch.uint8).mul_(255).expand(-1, -1, -1, 3).contiguous()

        def host_a():
            x = mask.float().permute(0, 3, 1, 2).contiguous()
            return torch.stack([F.interpolate(f[None], size=(512, 896), mode="bilinear", align_corners=False, antialias=True)[0] for f in x])
        dev = mask.cuda()
        t_k = best(lambda: FR.resize_frames(dev, (512, 896), True), args.repeats, sync)
        nbytes = mask.numel() + 97 * 3 * 512 * 896 * 4
        rec["a_mask_frames_1080p_to_512x896"] = {
            "gpu_with_upload": best(lambda: FR.get_maskvideo_to_video_latent(mask, 97, (512, 896)), args.repeats, sync),
            "gpu_kernel_only": t_k, "kernel_GBps": round(nbytes / t_k / 1e6, 1), "host": best(host_a, args.host_repeats, nosync)}
        del dev, mask
    if "b" in args.only:
        stream = torch.rand(97, 512, 896, 3, generator=g)

        def host_b():
            v = F.interpolate(stream.permute(0, 3, 1, 2), size=(480, 832), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
            v = v.cpu().numpy() * 255
            return torch.from_numpy(np.array(v))[:97].permute([3, 0, 1, 2]).unsqueeze(0) / 255
        rec["b_stream_512x896_to_480x832"] = {
            "gpu_with_upload": best(lambda: FR.get_video_to_video_latent(stream, 97, (480, 832), if_restore_255=True), args.repeats, sync),
            "host": best(host_b, args.host_repeats, nosync)}
        del stream
    if "c" in args.only:
        clip = torch.rand(3, 97, 512, 896, generator=g).mul_(2).sub_(1).cuda()

        def host_c():
            v = (clip / 2 + 0.5).clamp(0, 1).cpu().float()
            return [(f.permute(1, 2, 0) * 255).numpy().astype(np.uint8) for f in v.permute(1, 0, 2, 3)]
        t_k = best(lambda: FR.frames_to_bytes(clip), args.repeats, sync)
        rec["c_clip_3x97x512x896_to_bytes"] = {
            "gpu_with_download": best(lambda: FR.frames_to_bytes(clip).cpu(), args.repeats, sync), "gpu_kernel_only": t_k,
            "kernel_GBps": round(clip.numel() * 5 / t_k / 1e6, 1), "host_with_fp32_download": best(host_c, args.host_repeats, sync)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
