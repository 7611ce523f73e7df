"""Writes tests/golden/g15_motion_*.safetensors: what the REFERENCE's CameraMotionGenerator, ObjectMotionGenerator and
convert_moge_to_delta_format (pipelines.py:195-850, 852-1038, 1255-1291) compute on the CPU for small seeded inputs, and for two
end-to-end cases the six conditioning videos the reference's own rasteriser draws from the reference's own edited tracks.

The classes are cut out of the reference's pipelines.py BY NAME with `ast` at run time and executed (the technique of
oracle/ref_raster.py, which supplies the rasteriser end): the reference's code runs, nothing of it is stored here.  Needs the
reference checkout (FLEXAM_REFERENCE_ROOT, as oracle/ref_raster.py reads it); never imported by flexam_amd, bench.py or the tests.

Before anything is written the script asserts, on the CPU, that the reference's float32 results are inside the bounds the tests
hold the HIP kernels to (tests/motion_restatement.py), and filters the end-to-end inputs so that no projected coordinate is within
64 bounds of an integer (or of the frame tests 0, W, H) and no two points whose squares can share a pixel are closer in depth than
that: truncation and depth order cannot flip, so the videos must agree bit for bit.

    python tools/make_golden_motion.py
"""
import ast
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import motion_restatement as MR          # noqa: E402
from oracle import ref_raster            # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
T, MH, MW, N = 9, 32, 48, 400
OBJECT_MOTION_NAMES = ("up down left right front back up_left up_right down_left down_left2 down_right up_front up_back down_front down_back "
                       "left_front left_back right_front right_back up_left_front up_left_back up_right_front up_right_back down_left_front "
                       "down_left_back down_right_front down_right_back rot rot_ccw pitch_up pitch_down roll_left roll_right").split()
CAMERA_MOTIONS = ("trans 0.1 -0.2 0.5", "rot y 25", "rot x -10 2 6", "rot z 7 6 2", "spiral 1.5", "spiral 2 1 7",
                  "trans 0 0 0.5 0 4; rot x 25 0 4; trans 0.1 0 0 4 8", "rot y 12; spiral 1 0 8; trans -0.3 0.1 0.2 3 5")


class _Recorder:
    """`torch` as the reference sees it, with the arguments of torch.stack kept: apply_motion stacks its motion matrices."""

    def __init__(self):
        self.stacked = []

    def __getattr__(self, name):
        if name == "stack":
            def stack(seq, *a, **k):
                out = torch.stack(seq, *a, **k)
                self.stacked.append(out)
                return out
            return stack
        return getattr(torch, name)


def load_reference():
    src = open(ref_raster.SOURCE).read()
    tree = ast.parse(src)
    classes = {n.name: n for n in tree.body if isinstance(n, ast.ClassDef)}
    convert = next(n for n in classes["FlexAMPipeline"].body if isinstance(n, ast.FunctionDef) and n.name == "convert_moge_to_delta_format")
    holder = ast.ClassDef(name="_Convert", bases=[], keywords=[], body=[convert], decorator_list=[])
    if hasattr(holder, "type_params"):
        holder.type_params = []
    mod = ast.Module(body=[classes["CameraMotionGenerator"], classes["ObjectMotionGenerator"], holder], type_ignores=[])
    ast.fix_missing_locations(mod)
    rec = _Recorder()
    ns = {"np": np, "torch": rec, "math": math, "os": os, "print": lambda *a, **k: None}
    exec(compile(mod, ref_raster.SOURCE, "exec"), ns)
    return ns["CameraMotionGenerator"], ns["ObjectMotionGenerator"], ns["_Convert"]().convert_moge_to_delta_format, rec


def moge_inputs(rng):
    """A 32 x 48 MoGe-like point map (camera-space points whose projection through `intr` fills the unit square), NaN where invalid,
    a few points at and behind z = 0, the validity mask and an object mask."""
    intr = torch.tensor([[0.9, 0.0, 0.5], [0.0, 1.35, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float32)
    v, u = np.meshgrid((np.arange(MH) + rng.uniform(0.2, 0.8, MH)) / MH, (np.arange(MW) + rng.uniform(0.2, 0.8, MW)) / MW, indexing="ij")
    z = 2.0 + 0.8 * np.sin(3 * u) + 0.5 * v + rng.uniform(0, 0.3, (MH, MW))
    pm = np.stack([(u - 0.5) / 0.9 * z, (v - 0.5) / 1.35 * z, z], -1).astype(np.float32)
    valid = rng.random((MH, MW)) > 0.12
    pm[~valid] = np.nan
    odd = rng.choice(np.flatnonzero(valid.reshape(-1)), 12, replace=False)
    pm.reshape(-1, 3)[odd[:6], 2] = 0.0                       # z == 0
    pm.reshape(-1, 3)[odd[6:], 2] *= -1.0                     # z < 0: behind the camera
    obj = np.zeros((MH, MW), bool)
    obj[8:24, 14:34] = True                                   # covers NaN points too: they must not be selected
    return torch.from_numpy(pm), torch.from_numpy(valid), torch.from_numpy(obj), intr


def moge_exact(pm, obj, motion_name, distance, poses, intr, c_used):
    """float64 restatement of apply_motion("moge") -> w2s_moge -> x * W, y * H on the full map: (value, bound) [T, H W, 3], flags."""
    p0 = pm.reshape(-1, 3)
    flags = obj.reshape(-1) & ~torch.isnan(p0).any(dim=1)
    p = p0.double()[None].repeat(T, 1, 1)
    b = torch.zeros_like(p)
    if motion_name is not None:
        A, col_err = MR.exact_object_motion(MR.motion_about_origin(motion_name, distance, T), MR.exact_center(p0, flags), c_used, (MH, MW))
        p, b = MR.affine32(A, p, b, col_err, flags)
    moved = (p, b)
    p, b = MR.project32(poses.double()[:, :3, :], intr.double(), p, b)
    return moved, (p, b), MR.scale32(p, b, MW, MH), flags


def safe_points(val, bound, half, height, width, vis=None):
    """[N] bool: points that, in every frame, keep 64 bounds between (u, v) and the nearest integer (which covers the frame tests) and,
    against every point whose square can share a pixel with theirs, in depth.  Greedy: a point in conflict is dropped."""
    val, bound = np.asarray(val, np.float64), np.asarray(bound, np.float64)
    finite = np.isfinite(val).all(-1)
    with np.errstate(invalid="ignore"):
        frac = np.abs(val[..., :2] - np.rint(val[..., :2]))
        keep = (finite & (frac > 64 * bound[..., :2]).all(-1)).all(0)
    reach = 2 * max(half, 2) + 2                               # the cosine videos draw +-2 whatever point_wise is
    for t in range(val.shape[0]):
        idx = np.flatnonzero(keep if vis is None else keep & vis[t])
        order = idx[np.argsort(val[t, idx, 2], kind="stable")]
        for a, i in enumerate(order):
            if not keep[i]:
                continue
            for j in order[a + 1:]:
                if val[t, j, 2] - val[t, i, 2] > 64 * (bound[t, j, 2] + bound[t, i, 2]) + 1e-300:
                    break
                if keep[j] and abs(val[t, j, 0] - val[t, i, 0]) <= reach and abs(val[t, j, 1] - val[t, i, 1]) <= reach:
                    keep[j] = False
    return keep


def videos_u8(raster, tracks, vis, point_wise, height, width):
    """The reference's six conditioning videos as bytes [6, T, H, W, 3] (tracking, cos levels 0..3, depth); the float videos are
    byte / 255 exactly (pipelines.py:1658-1660)."""
    import contextlib
    import io
    pts = tracks.detach().cpu().numpy() if isinstance(tracks, torch.Tensor) else np.asarray(tracks)
    vis = np.asarray(vis)
    with contextlib.redirect_stdout(io.StringIO()):
        tracking = np.stack(raster.fun_visualize_tracking_with_depth(torch.from_numpy(pts), torch.from_numpy(vis), height, width,
                                                                     point_wise=point_wise, mask_video=None, generate_type="full_edit"))
        enc = raster.apply_cosine_positional_encoding(torch.from_numpy(pts), height, width, 4)
        cos = raster._visualize_cosine_encoded_tracking(enc, pts, vis, height, width, False, mask_video=None, generate_type="full_edit")
        dep = raster._visualize_depth_tracking(torch.from_numpy(pts), vis, height, width, point_wise, False, mask_video=None, generate_type="full_edit")
    out = [torch.from_numpy(tracking)]
    for v in [cos[i] for i in range(4)] + [dep]:
        u8 = torch.round(v[0] * 255).to(torch.uint8)
        assert torch.equal(u8.float() / 255, v[0].float()), "a reference video is not byte / 255"
        out.append(u8.permute(1, 2, 3, 0).contiguous())
    return torch.stack(out)


def main():
    from safetensors.torch import save_file
    torch.set_num_threads(1)
    Cam, Obj, convert, rec = load_reference()
    rng = np.random.default_rng(15)

    # ---------------------------------------------------------------- host matrices
    out = {}
    for i, s in enumerate(CAMERA_MOTIONS):
        out[f"camera.{i}"] = Cam(s, frame_num=T, H=MH, W=MW, device="cpu").get_default_motion()
        assert out[f"camera.{i}"].dtype == torch.float32
    cam = Cam("rot y 5", frame_num=T, H=MH, W=MW, device="cpu")
    out["intr_default"] = cam.intr.clone()
    out["rot_x"], out["rot_y"], out["rot_z"] = cam.rot_poses(33.0, "x"), cam.rot_poses(-12.5, "y"), cam.rot_poses(190.0, "z")
    out["trans"] = cam.trans_poses(1.0, -2.0, 0.3)
    out["spiral"] = cam.spiral_poses(2.0)
    ext = rng.normal(size=(12, 3, 4))
    out["cameras_ext"] = torch.from_numpy(ext)
    out["cameras_long"] = cam.convert_cameras_to_poses([None] * 12, ext.tolist())
    out["cameras_short"] = cam.convert_cameras_to_poses([None] * 4, ext[:4].tolist())

    # ---------------------------------------------------------------- DELTA route, float32
    tracks = np.stack([rng.uniform(-3, MW + 3, (T, N)), rng.uniform(-3, MH + 3, (T, N)), rng.uniform(0.5, 5, (T, N))], -1).astype(np.float32)
    tracks[0, :40, 0] = np.arange(40) * 0.5 + 10.0                 # exact halves: round-half-even decides
    tracks[0, 40:80, 1] = np.arange(40) * 0.5 + 5.0
    tracks = torch.from_numpy(tracks)
    mask = torch.zeros(MH, MW, dtype=torch.bool)
    mask[6:22, 10:30] = True
    mask[0, :] = True
    gen = Obj(device="cpu")
    flags = gen._get_points_in_mask(tracks, mask)
    center = tracks[0, flags].mean(dim=0)
    d = {"tracks": tracks, "mask": mask, "flags": flags, "center": center, "empty_mask": torch.zeros(MH, MW, dtype=torch.bool)}
    mats = []
    for name in OBJECT_MOTION_NAMES:
        rec.stacked.clear()
        moved = gen.apply_motion(tracks, mask, name, 50, num_frames=T, tracking_method="DELTA")
        mats.append(rec.stacked[-1])
        c_star = MR.exact_center(tracks[0], flags)
        A, col_err = MR.exact_object_motion(MR.motion_about_origin(name, 50, T), c_star, center)
        val, bound = MR.affine32(A, tracks.double(), torch.zeros(T, N, 3, dtype=torch.float64), col_err, flags)
        ok, worst = MR.close32(moved, val, bound)
        assert ok, (name, worst)
        if name in ("left", "rot", "pitch_up", "up_left_front"):
            d[f"moved.{name}"] = moved
    out["object_matrices"] = torch.stack(mats)
    out["object_center"] = center
    assert torch.equal(gen.apply_motion(tracks, d["empty_mask"], "rot", 50, num_frames=T, tracking_method="DELTA"), tracks)
    n_sel = int(flags.sum())
    assert (center.double() - MR.exact_center(tracks[0], flags)).abs().max() <= (n_sel - 1) * MR.U32 * tracks[0, flags].double().abs().mean(0).max()
    save_file({k: v.contiguous() for k, v in out.items()}, os.path.join(GOLDEN, "g15_motion_host.safetensors"))
    save_file({k: v.contiguous() for k, v in d.items()}, os.path.join(GOLDEN, "g15_motion_delta.safetensors"))

    # ---------------------------------------------------------------- MoGe route, float32, + end to end
    pm, valid, obj, intr = moge_inputs(rng)
    cam = Cam("rot y 14; trans 0.05 -0.02 -0.3", frame_num=T, H=MH, W=MW, device="cpu")
    cam.set_intr(intr)
    poses = cam.get_default_motion()
    maps = pm.unsqueeze(0).repeat(T, 1, 1, 1)
    moved = Obj(device="cpu").apply_motion(maps, obj, "rot", 50, num_frames=T, tracking_method="moge")
    screen = cam.w2s_moge(moved.reshape(T, MH * MW, 3), poses)
    p0 = pm.reshape(-1, 3)
    sel = obj.reshape(-1) & ~torch.isnan(p0).any(dim=1)
    c_used = p0[sel].mean(dim=0)
    (mv, mb), (sv, sb), (pv, pb), flags_m = moge_exact(pm, obj, "rot", 50, poses, intr, c_used)
    assert torch.equal(flags_m, sel)
    for name, got, val, bound in (("apply_motion", moved.reshape(T, -1, 3), mv, mb), ("w2s_moge", screen, sv, sb)):
        ok, worst = MR.close32(got, val, bound)
        assert ok, (name, worst)
    assert bool((sv[:, valid.reshape(-1), 2] < 0).any()), "no point behind the moved camera"
    keep = safe_points(pv.numpy(), pb.numpy(), 1, MH, MW) & valid.reshape(-1).numpy()
    valid_e2e = torch.from_numpy(keep.reshape(MH, MW))
    delta, vis = convert(screen.reshape(T, MH, MW, 3).numpy(), valid.numpy(), MH, MW)
    ok, worst = MR.close32(delta, pv[:, valid.reshape(-1)], pb[:, valid.reshape(-1)])
    assert ok, ("convert", worst)
    delta_e2e, vis_e2e = convert(screen.reshape(T, MH, MW, 3).numpy(), valid_e2e.numpy(), MH, MW)
    raster = ref_raster.load()
    m = {"point_map": pm, "valid_mask": valid, "valid_mask_e2e": valid_e2e, "object_mask": obj, "intr": intr, "poses": poses,
         "center": c_used, "moved": moved, "screen": screen, "delta": delta,
         "empty_object_mask": torch.zeros(MH, MW, dtype=torch.bool),
         "videos_e2e": videos_u8(raster, delta_e2e, vis_e2e, 2, MH, MW)}
    assert torch.equal(Obj(device="cpu").apply_motion(maps, m["empty_object_mask"], "left", 50, num_frames=T, tracking_method="moge").isnan(), maps.isnan())
    save_file({k: v.contiguous() for k, v in m.items()}, os.path.join(GOLDEN, "g15_motion_moge.safetensors"))

    # ---------------------------------------------------------------- VGGT route, float64, + end to end
    ang = np.linspace(0, 0.2, T)
    ext = np.zeros((1, T, 3, 4), np.float32)
    for t in range(T):
        c, s = math.cos(ang[t]), math.sin(ang[t])
        ext[0, t, :, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.array([[1, 0, 0], [0, math.cos(0.05 * t), -math.sin(0.05 * t)], [0, math.sin(0.05 * t), math.cos(0.05 * t)]])
        ext[0, t, :, 3] = [0.02 * t, -0.01 * t, 0.03 * t]
    itr = np.tile(np.array([[40.0, 0, MW / 2], [0, 40.0, MH / 2], [0, 0, 1]], np.float32), (1, T, 1, 1))
    itr[0, :, 0, 0] += np.linspace(0, 1, T, dtype=np.float32)
    ext_t, itr_t = torch.from_numpy(ext), torch.from_numpy(itr)
    cam = Cam("rot y 160 0 8; trans 0.3 0.1 -0.5", frame_num=T, H=MH, W=MW, device="cpu")
    cam.set_intr(itr_t)
    cam.set_extr(ext_t)
    poses = cam.get_default_motion()
    uvz = np.stack([rng.uniform(-2, MW + 2, (T, N)), rng.uniform(-2, MH + 2, (T, N)), rng.uniform(0.8, 4, (T, N))], -1)
    uvz[:, :10, 2] = 0.0
    uvz[:, 10:20, 2] *= -1
    g = {"tracks64": torch.from_numpy(uvz), "tracks32": torch.from_numpy(uvz.astype(np.float32)), "extrinsics": ext_t, "intrinsics": itr_t, "poses": poses}
    kinv, rinv, tvec, _, _ = MR.vggt_host_matrices(ext_t, itr_t)
    for tag, src in (("64", g["tracks64"]), ("32", g["tracks32"])):
        world = cam.s2w_vggt(src, ext_t, itr_t)
        assert world.dtype == src.numpy().dtype
        val, bound, ok_in = MR.unproject64(src.numpy(), kinv, rinv, tvec)
        ok, worst = MR.close64(world, val, bound, MR.U32 * np.abs(val) if tag == "32" else None)
        assert ok and (world[~ok_in] == 0).all(), ("s2w", tag, worst)
        g[f"world{tag}"] = torch.from_numpy(world)
    behind = False
    for tag, kw in (("none", dict(poses=None)), ("override", dict(poses=poses, override_extrinsics=True)), ("ontop", dict(poses=poses, override_extrinsics=False))):
        for w in ("64", "32"):
            res = cam.w2s_vggt(g[f"world{w}"], ext_t, itr_t, **kw)
            _, _, _, pose, intr64 = MR.vggt_host_matrices(ext_t, itr_t, kw.get("poses"), kw.get("override_extrinsics", True))
            val, bound, ok_out, depth = MR.project64(g[f"world{w}"].numpy(), pose, intr64)
            ok, worst = MR.close64(res.numpy(), val, bound)
            assert ok and torch.equal(torch.from_numpy(ok_out), res[..., 2] > 0) and (res.numpy()[~ok_out] == 0).all(), ("w2s", tag, w, worst)
            behind |= bool((~ok_out & (g[f"world{w}"].numpy() != 0).any(-1)).any())
            if w == "64" or tag == "ontop":                   # the float32-input variant is kept for one case only (file size)
                g[f"screen.{tag}.{w}"] = res
    assert behind, "no point behind the moved camera"
    # end to end: a gentle motion (the points stay in front), float64 tracks, visibility, override_extrinsics=False, point_wise 4
    cam2 = Cam("rot y 8; trans 0.05 0 0.1", frame_num=T, H=MH, W=MW, device="cpu")
    poses2 = cam2.get_default_motion()
    world = cam2.s2w_vggt(g["tracks64"], ext_t, itr_t)
    res = cam2.w2s_vggt(world, ext_t, itr_t, poses2, override_extrinsics=False)
    _, _, _, pose, intr64 = MR.vggt_host_matrices(ext_t, itr_t, poses2, False)
    val, bound, _, _ = MR.project64(world, pose, intr64)
    vis = rng.random((T, N)) > 0.1
    keep = safe_points(val.astype(np.float64), np.maximum(bound.astype(np.float64), 1e-14), 2, MH, MW, vis) & (uvz[0, :, 2] > 0)
    g["e2e_keep"] = torch.from_numpy(keep)
    g["e2e_vis"] = torch.from_numpy(vis[:, keep])
    g["e2e_poses"] = poses2
    res_keep = cam2.w2s_vggt(cam2.s2w_vggt(g["tracks64"][:, keep], ext_t, itr_t), ext_t, itr_t, poses2, override_extrinsics=False)
    assert torch.equal(res_keep, res[:, keep])
    g["videos_e2e"] = videos_u8(raster, res_keep, vis[:, keep], 4, MH, MW)
    save_file({k: v.contiguous() for k, v in g.items()}, os.path.join(GOLDEN, "g15_motion_vggt.safetensors"))
    for f in ("host", "delta", "moge", "vggt"):
        p = os.path.join(GOLDEN, f"g15_motion_{f}.safetensors")
        print(p, os.path.getsize(p), "bytes")
        assert os.path.getsize(p) < (1 << 20)


if __name__ == "__main__":
    main()
