"""Dev tool: the conditioning rasteriser at the clip's size (97 x 512 x 896, a 4-pixel grid of tracked points): wall time of
visualize_tracking_DELTA (host colour tables + HIP) and of its two kernels alone.  usage: raster_bench.py [grid_step]

raster_bench.py --dense [--baseline FILE] [--out JSON]: the device-resident path.  Tracks from moge_tracks at 97 x 512 x 896 (every valid
pixel a point, ~413 000 per frame) and the 4-pixel grid (28 672), both handed over as the float32 tensor on the GPU; the six videos,
best of 3 after a warm-up, host clock around a device synchronise; the selection kernels alone.  --baseline: another copy of
flexam_amd/conditioning_raster.py (the previous commit's, say) timed on the same tensors in the same process."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from flexam_amd import conditioning_raster as P
from flexam_amd import hip as H


def dense(argv):
    import argparse, importlib.util, json
    ap = argparse.ArgumentParser()
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "raster_colors_bench.json"))
    args = ap.parse_args(argv)
    from flexam_amd import CameraMotionGenerator, moge_tracks
    dev = torch.device("cuda:0")
    T, Hh, W = 97, 512, 896
    g = torch.Generator().manual_seed(5)
    v, u = torch.meshgrid((torch.arange(Hh) + 0.5) / Hh, (torch.arange(W) + 0.5) / W, indexing="ij")
    z = 2.0 + 0.8 * torch.sin(3 * u) + 0.5 * v + 0.3 * torch.rand(Hh, W, generator=g)
    pm = torch.stack([(u - 0.5) / 0.9 * z, (v - 0.5) / 1.35 * z, z], -1).float()
    valid = torch.rand(Hh, W, generator=g) > 0.1
    cam = CameraMotionGenerator("rot y 25", frame_num=T, H=Hh, W=W, device=dev)
    cam.set_intr(torch.tensor([[0.9, 0.0, 0.5], [0.0, 1.35, 0.5], [0.0, 0.0, 1.0]]))
    poses = cam.get_default_motion()
    grid = torch.zeros(Hh, W, dtype=torch.bool)
    grid[2::4, 2::4] = True
    impls = {"this": P}
    if args.baseline:
        spec = importlib.util.spec_from_file_location("flexam_amd.conditioning_raster_baseline", args.baseline)
        impls["baseline"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(impls["baseline"])
    rec = {"device": torch.cuda.get_device_name(0), "clip": [T, Hh, W], "timing": "best of 3 after one warm-up, perf_counter around torch.cuda.synchronize"}
    for case, mask in (("dense", valid), ("grid4", grid)):
        tracks, vis = moge_tracks(pm.to(dev), mask.to(dev), cam, poses, Hh, W)
        rec[case] = {"points_per_frame": tracks.shape[1]}
        for name, impl in impls.items():
            times = []
            for it in range(4):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                out = impl.visualize_tracking_DELTA(tracks, vis, False, 4, Hh, W, 4)
                torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
                del out
            rec[case][name + "_s"] = [round(t, 5) for t in times[1:]]
            rec[case][name + "_best_s"] = round(min(times[1:]), 5)
            print(f"{case} ({tracks.shape[1]} points x {T} frames), {name}: six videos in {min(times[1:]) * 1e3:.1f} ms (3 runs: {rec[case][name + '_s']})", flush=True)
        if case == "dense":
            n = tracks.shape[1]
            ranks1 = torch.tensor([[int(0.02 * T * n), int(0.02 * T * n) + 1, int(0.98 * T * n), int(0.98 * T * n) + 1]], device=dev)
            ranksT = torch.tensor([[int(0.02 * n), int(0.02 * n) + 1, int(0.98 * n), int(0.98 * n) + 1]] * T, device=dev)
            d_vis = torch.from_numpy(vis).to(dev)
            sel = {}
            for what, fn, passes in (("whole_clip_inverse_depth_4_ranks", lambda: H.select_ranks(tracks, 2, 1, T * n, ranks1, None, True), 4),
                                     ("per_frame_depth_masked_4_ranks", lambda: H.select_ranks(tracks, 2, T, n, ranksT, d_vis, False), 4),
                                     ("whole_clip_count_only", lambda: H.select_ranks(tracks, 2, 1, T * n, None, None, True), 1)):
                fn(); torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(5): fn()
                torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 5
                sel[what] = {"ms": round(dt * 1e3, 4), "passes": passes, "values_GB_per_s": round(passes * T * n * 4 / dt / 1e9, 1),
                             "touched_GB_per_s": round(passes * T * n * 12 / dt / 1e9, 1)}
                print(f"select {what}: {dt * 1e3:.3f} ms, {sel[what]['values_GB_per_s']} GB/s of values ({sel[what]['touched_GB_per_s']} GB/s of the [T, N, 3] lines they sit in)", flush=True)
            rec["selection"] = sel
        del tracks
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if "--dense" in sys.argv:
    dense(sys.argv[1:])
    sys.exit(0)

step = int(sys.argv[1]) if len(sys.argv) > 1 else 4
t_n, h, w = 97, 512, 896
rng = np.random.default_rng(0)
ys, xs = np.meshgrid(np.arange(step // 2, h, step), np.arange(step // 2, w, step), indexing="ij")
base = np.stack([xs.ravel(), ys.ravel()], -1).astype(np.float32)
n = base.shape[0]
pts = np.zeros((t_n, n, 3), np.float32)
drift = rng.normal(0, 0.6, (n, 2)).astype(np.float32)
for t in range(t_n):
    pts[t, :, :2] = base + drift * t
pts[:, :, 2] = rng.uniform(0.5, 9, (t_n, n))
vis = rng.random((t_n, n)) > 0.05
dev = "cuda:0"
for it in range(3):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    tr, cos, dep = P.visualize_tracking_DELTA(pts, vis, False, 4, h, w, 4, device=dev)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print(f"visualize_tracking_DELTA: {n} points x {t_n} frames -> 6 videos [1, 3, {t_n}, {h}, {w}]: {dt:.3f} s", flush=True)
d_pts, d_vis = torch.from_numpy(pts).to(dev), torch.from_numpy(vis).to(dev)
colors = torch.randint(0, 256, (n, 3), dtype=torch.uint8, device=dev)
keys = H.raster_keys(d_pts, d_vis, h, w, 2, 0)
out = torch.empty(3, t_n, h, w, device=dev)
for name, fn, nbytes in (("raster_keys", lambda: H.raster_keys(d_pts, d_vis, h, w, 2, 0, keys=keys), t_n * h * w * 8),
                         ("raster_resolve (float planes)", lambda: H.raster_resolve(keys, colors, out_f32=out), t_n * h * w * (8 + 12))):
    fn(); torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(10): fn()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 10
    print(f"{name}: {dt * 1e3:.3f} ms  ({nbytes / dt / 1e9:.0f} GB/s of key / output bytes)")
t0 = time.perf_counter(); P._depth_colors(pts, vis); t1 = time.perf_counter(); P._tracking_colors(pts[0], h, w); t2 = time.perf_counter()
enc = P.apply_cosine_positional_encoding(torch.from_numpy(pts), h, w, 4); t3 = time.perf_counter()
print(f"host: depth colours {t1 - t0:.3f} s, tracking colours {t2 - t1:.4f} s, cosine encodings (CPU tensors) {t3 - t2:.3f} s")
