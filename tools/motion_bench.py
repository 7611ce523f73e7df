"""Times the edit tracks of flexam_amd.motion on the GPU against the same chains written the way the reference writes them.

  moge   moge_tracks at 97 x 512 x 896 ("rot y 25", object motion "left" in a 300 x 500 mask; inputs already on the device) against
         this tool's restatement of demo.py:222-266 in torch ops on the SAME GPU: the map repeated T times, apply_motion's per-frame
         boolean-index loop (pipelines.py:1014-1023), w2s_moge's cat / bmm / permute (:512-530), the download to the host, the numpy
         scaling and mask gather of convert_moge_to_delta_format (:1269-1289), and the upload the rasteriser then does.
  delta  the DELTA / VGGT chain at 97 x 4900 points: s2w_vggt -> w2s_vggt -> apply_motion, against s2w / w2s in their host numpy form
         (:356-510, written out here) followed by apply_motion's torch loop on the GPU (:1027-1038).
The restatements are this tool's own (the reference is not importable); each timing ends in a device synchronise; best of N after
warm-up.  One JSON record; nothing is promised in advance, the record states both numbers and their ratio.

    python tools/motion_bench.py [--repeats 10] [--out profiles/motion_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best(fn, repeats, sync):
    for _ in range(2):
        fn()
    sync()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        times.append(time.perf_counter() - t0)
    return round(1e3 * min(times), 3), round(1e3 * sorted(times)[len(times) // 2], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from flexam_amd import CameraMotionGenerator, ObjectMotionGenerator, moge_tracks
    from flexam_amd.motion import _moge_motion_rows, object_motion_matrices
    if not torch.cuda.is_available():
        raise SystemExit("motion_bench: no GPU (this measures the GPU path; there is nothing to fall back to)")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    rec = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats}

    # ------------------------------------------------------------------ MoGe route
    T, H, W = 97, 512, 896
    g = torch.Generator().manual_seed(5)
    v, u = torch.meshgrid((torch.arange(H) + 0.5) / H, (torch.arange(W) + 0.5) / W, indexing="ij")
    z = 2.0 + 0.8 * torch.sin(3 * u) + 0.5 * v + 0.3 * torch.rand(H, W, generator=g)
    pm = torch.stack([(u - 0.5) / 0.9 * z, (v - 0.5) / 1.35 * z, z], -1).float()
    valid = torch.rand(H, W, generator=g) > 0.1
    pm[~valid] = float("nan")
    obj = torch.zeros(H, W, dtype=torch.bool)
    obj[100:400, 200:700] = True
    intr = torch.tensor([[0.9, 0.0, 0.5], [0.0, 1.35, 0.5], [0.0, 0.0, 1.0]])
    cam = CameraMotionGenerator("rot y 25", frame_num=T, H=H, W=W, device=dev)
    cam.set_intr(intr)
    poses = cam.get_default_motion()
    pm_d, valid_d, obj_d, poses_d, intr_d = pm.to(dev), valid.to(dev), obj.to(dev), poses.to(dev), intr.to(dev)

    def hip_moge():
        return moge_tracks(pm_d, valid_d, cam, poses, H, W, object_mask=obj_d, object_motion="left", distance=50)[0]

    def torch_moge():
        tracks = pm_d.unsqueeze(0).repeat(T, 1, 1, 1)
        sel = ~torch.any(torch.isnan(tracks[0]), dim=2) & obj_d
        center = tracks[0][sel].reshape(-1, 3).mean(dim=0)
        motions = object_motion_matrices(center.cpu(), "left", 50, T).to(dev)
        mod = tracks.clone().reshape(T, -1, 3)
        flat = sel.reshape([-1])
        for f in range(T):
            m = motions[f].clone()
            m[0, 3] /= W
            m[1, 3] /= H
            p = mod[f, flat]
            mod[f, flat] = torch.matmul(torch.cat([p, torch.ones_like(p[:, :1])], dim=1), m.T)[:, :3]
        ones = torch.ones((T, H * W, 1), device=dev, dtype=mod.dtype)
        cam_h = torch.bmm(poses_d, torch.cat([mod, ones], dim=-1).permute(0, 2, 1))
        cam_p = cam_h[:, :3, :].permute(0, 2, 1)
        img = torch.bmm(cam_p, intr_d.unsqueeze(0).repeat(T, 1, 1).permute(0, 2, 1))
        uvd = torch.cat([img[:, :, :2] / img[:, :, 2:3], cam_p[:, :, 2:3]], dim=-1)
        host = uvd.reshape(T, H, W, 3).cpu().numpy()
        px = host.copy()
        px[:, :, :, 0] *= W
        px[:, :, :, 1] *= H
        kept = px.reshape(T, H * W, 3)[:, valid.numpy().flatten(), :]
        return torch.from_numpy(kept).float().to(dev)

    a, b = hip_moge(), torch_moge()
    sync()
    err = float((a - b).abs().max())
    hb, hm = best(hip_moge, args.repeats, sync)
    tb, tm = best(torch_moge, max(3, args.repeats // 3), sync)
    rec["moge_97x512x896"] = {"hip_best_ms": hb, "hip_median_ms": hm, "torch_restatement_best_ms": tb, "torch_restatement_median_ms": tm,
                              "ratio": round(tb / hb, 2), "points_per_frame": int(valid.sum()), "max_abs_difference": err,
                              "output_bytes": int(a.numel() * 4)}
    del a, b

    # ------------------------------------------------------------------ DELTA / VGGT route
    N, Hs, Ws = 4900, 480, 720
    rng = np.random.default_rng(9)
    uvz = np.stack([rng.uniform(0, Ws, (T, N)), rng.uniform(0, Hs, (T, N)), rng.uniform(0.8, 4, (T, N))], -1).astype(np.float32)
    ext = np.tile(np.eye(4, dtype=np.float32)[:3], (1, T, 1, 1))
    ext[0, :, 0, 3] = np.linspace(0, 0.2, T)
    itr = np.tile(np.array([[600.0, 0, Ws / 2], [0, 600.0, Hs / 2], [0, 0, 1]], np.float32), (1, T, 1, 1))
    ext_t, itr_t = torch.from_numpy(ext), torch.from_numpy(itr)
    cam2 = CameraMotionGenerator("rot y 10", frame_num=T, H=Hs, W=Ws, device=dev)
    poses2 = cam2.get_default_motion()
    mask = torch.zeros(Hs, Ws, dtype=torch.bool)
    mask[100:300, 200:500] = True
    tracks_d, mask_d = torch.from_numpy(uvz).to(dev), mask.to(dev)
    gen = ObjectMotionGenerator(device=dev)

    def hip_delta():
        world = cam2.s2w_vggt(tracks_d, ext_t, itr_t)
        screen = cam2.w2s_vggt(world, ext_t, itr_t, poses2, override_extrinsics=False)
        return gen.apply_motion(screen, mask_d, "left", 50, num_frames=T, tracking_method="DELTA")

    def host_delta():
        pts = tracks_d.detach().cpu().numpy()
        e, k = ext[0], itr[0]
        world = np.zeros_like(pts)
        ok = pts[..., 2] > 0
        uv1 = np.concatenate([pts[..., :2], np.ones((T, N, 1))], axis=-1)
        for i in range(T):
            kinv, rinv = np.linalg.inv(k[i]), np.linalg.inv(e[i, :, :3])
            idx = np.where(ok[i])[0]
            if len(idx):
                world[i, idx] = ((uv1[i, idx] @ kinv.T) * pts[i, idx, 2][:, None] - e[i, :, 3]) @ rinv.T
        cp = poses2.numpy().copy()
        cp[:, :3, 3] = cp[:, :3, 3] / 5.0
        for i in range(T):
            m = np.eye(4)
            m[:3, :] = e[i]
            cp[i] = np.matmul(cp[i], m)
        c = np.matmul(np.concatenate([world, np.ones([T, N, 1])], axis=-1), np.transpose(cp, (0, 2, 1)))[..., :3]
        depth = c[..., 2:3]
        good = depth[..., 0] > 0
        px = np.matmul(c / (depth + 1e-10), np.transpose(k, (0, 2, 1)))
        res = np.concatenate([px[..., 0:1], px[..., 1:2], depth], axis=-1)
        res[~good] = 0
        tr = torch.from_numpy(res).to(dev).float()
        xy = tr[0][:, :2].round().long()
        xy[:, 0].clamp_(0, Ws - 1)
        xy[:, 1].clamp_(0, Hs - 1)
        inside = mask_d[xy[:, 1], xy[:, 0]]
        motions = object_motion_matrices(tr[0, inside].mean(dim=0).cpu(), "left", 50, T).to(dev)
        out = tr.clone()
        for f in range(T):
            p = out[f, inside]
            out[f, inside] = torch.matmul(torch.cat([p, torch.ones_like(p[:, :1])], dim=1), motions[f].T)[:, :3]
        return out

    a, b = hip_delta(), host_delta()
    sync()
    err = float((a - b).abs().max())
    hb, hm = best(hip_delta, args.repeats, sync)
    tb, tm = best(host_delta, args.repeats, sync)
    rec["delta_97x4900"] = {"hip_best_ms": hb, "hip_median_ms": hm, "host_numpy_restatement_best_ms": tb, "host_numpy_restatement_median_ms": tm,
                            "ratio": round(tb / hb, 2), "max_abs_difference": err}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
