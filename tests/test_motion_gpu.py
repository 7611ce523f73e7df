"""GPU: flexam_amd.motion through the C ABI (csrc/motion.hip) against the reference's CPU results (tests/golden/g15_motion_*.safetensors,
tools/make_golden_motion.py) and against exact restatements with derived forward error bounds (tests/motion_restatement.py).

Selection flags, compaction and the six end-to-end conditioning videos are bit-exact; float32 and float64 transforms are held to
|hip - exact| <= 2 B with B the first-order bound of the chain (the same inequality the reference's own results satisfy:
tests/test_motion_cpu.py, and the generator asserts it before writing); the centre to one float32 ulp of the float64 mean."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
T, MH, MW = 9, 32, 48


def dev():
    return torch.device("cuda:0")


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


# ----------------------------------------------------------------------------- flags, compaction, centre
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 458752])
@pytest.mark.parametrize("kind", ["none", "all", "random"])
def test_compaction_equals_nonzero(n, kind):
    from flexam_amd import hip as H
    g = torch.Generator().manual_seed(n)
    mask = {"none": torch.zeros(n, dtype=torch.bool), "all": torch.ones(n, dtype=torch.bool), "random": torch.rand(n, generator=g) > 0.37}[kind].to(dev())
    index, count = H.motion_compact(mask)
    want = torch.nonzero(mask).flatten().to(torch.int32)
    assert int(count.item()) == want.numel() and torch.equal(index[:want.numel()], want)


def test_selection_flags_equal_the_reference(golden):
    from flexam_amd import ObjectMotionGenerator
    from flexam_amd import hip as H
    d, m = golden("g15_motion_delta"), golden("g15_motion_moge")
    gen = ObjectMotionGenerator(device=dev())
    flags = gen._get_points_in_mask(d["tracks"], d["mask"])
    assert flags.dtype == torch.bool and torch.equal(flags.cpu(), d["flags"])          # 80 first-frame coordinates sit on exact halves
    assert not bool(gen._get_points_in_mask(d["tracks"], d["empty_mask"]).any())
    p0 = m["point_map"].reshape(-1, 3)
    want = m["object_mask"].reshape(-1) & ~torch.isnan(p0).any(dim=1)
    got, _ = H.motion_select_map(p0.to(dev()), m["object_mask"].reshape(-1).to(dev()))
    assert torch.equal(got.cpu(), want) and bool((m["object_mask"].reshape(-1) & ~want).any())     # the mask covers NaN points; they are not selected


@pytest.mark.parametrize("n", [1, 65, 4097, 458752])
def test_centre_is_the_correctly_rounded_mean_and_reproducible(n):
    from flexam_amd import hip as H
    from flexam_amd.motion import _center
    g = torch.Generator().manual_seed(100 + n)
    pts = (torch.rand(n, 3, generator=g) * torch.tensor([4.0, 2.0, 9.0]) + torch.tensor([-2.0, 100.0, 0.5])).to(dev())
    mask = (torch.rand(n, generator=g) > 0.3).to(dev()) if n > 1 else torch.ones(1, dtype=torch.bool, device=dev())
    flags, sums = H.motion_select_map(pts, mask)
    exact = pts.double().cpu()[mask.cpu()].mean(dim=0).numpy()
    c = _center(sums).numpy()
    assert int(sums[3].item()) == int(mask.sum().item())
    assert (np.abs(c.astype(np.float64) - exact) <= ulp32(exact)).all(), (c, exact)
    flags2, sums2 = H.motion_select_map(pts, mask)
    assert torch.equal(sums, sums2) and torch.equal(flags, flags2)


def test_reference_centre_and_hip_centre_are_both_tied_to_the_exact_mean(golden):
    import motion_restatement as MR
    from flexam_amd import hip as H
    from flexam_amd.motion import _center
    d = golden("g15_motion_delta")
    flags, sums = H.motion_select_pixels(d["tracks"][0].contiguous().to(dev()), d["mask"].to(dev()))
    exact = MR.exact_center(d["tracks"][0], d["flags"]).numpy()
    n = int(d["flags"].sum())
    assert (np.abs(_center(sums).numpy().astype(np.float64) - exact) <= ulp32(exact)).all()
    lim = (n - 1) * MR.U32 * d["tracks"][0, d["flags"]].double().abs().mean(0).numpy()
    assert (np.abs(d["center"].numpy().astype(np.float64) - exact) <= lim).all()


# ----------------------------------------------------------------------------- float32 transforms
def _hip_center(points0, mask_flat=None, mask_hw=None):
    from flexam_amd import hip as H
    from flexam_amd.motion import _center
    p = points0.contiguous().to(dev())
    _, sums = H.motion_select_map(p, mask_flat.to(dev())) if mask_flat is not None else H.motion_select_pixels(p, mask_hw.to(dev()))
    return _center(sums)


@pytest.mark.parametrize("name", ["left", "rot", "pitch_up", "up_left_front"])
def test_apply_motion_delta_within_the_derived_bound(golden, name):
    import motion_restatement as MR
    from flexam_amd import ObjectMotionGenerator
    d = golden("g15_motion_delta")
    tracks, flags = d["tracks"], d["flags"]
    got = ObjectMotionGenerator(device=dev()).apply_motion(tracks, d["mask"], name, 50, num_frames=T, tracking_method="DELTA")
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == tracks.shape
    c_star = MR.exact_center(tracks[0], flags)
    m = MR.motion_about_origin(name, 50, T)
    for what, res, c_used in (("hip", got.cpu(), _hip_center(tracks[0], mask_hw=d["mask"])), ("reference", d[f"moved.{name}"], d["center"])):
        A, col_err = MR.exact_object_motion(m, c_star, c_used)
        val, bound = MR.affine32(A, tracks.double(), val_like(tracks), col_err, flags)
        ok, worst = MR.close32(res, val, bound)
        print(f"apply_motion DELTA {name} {what}: worst |err| / (2 B) = {worst:.3f}")
        assert ok, (what, worst)
    assert torch.equal(got.cpu()[:, ~flags], tracks[:, ~flags])                         # unselected points are untouched


def val_like(t):
    return torch.zeros(t.shape, dtype=torch.float64)


def test_empty_mask_moves_nothing(golden):
    from flexam_amd import ObjectMotionGenerator
    d, m = golden("g15_motion_delta"), golden("g15_motion_moge")
    gen = ObjectMotionGenerator(device=dev())
    got = gen.apply_motion(d["tracks"], d["empty_mask"], "rot", 50, num_frames=T, tracking_method="DELTA")
    assert torch.equal(got.cpu(), d["tracks"])
    maps = m["point_map"].unsqueeze(0).repeat(T, 1, 1, 1)
    got = gen.apply_motion(maps, m["empty_object_mask"], "left", 50, num_frames=T, tracking_method="moge").cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(maps)) and torch.equal(torch.nan_to_num(got), torch.nan_to_num(maps))


def _moge_exact(m, c_used, with_motion=True):
    import motion_restatement as MR
    pm, obj = m["point_map"], m["object_mask"]
    p0 = pm.reshape(-1, 3)
    flags = obj.reshape(-1) & ~torch.isnan(p0).any(dim=1)
    p = p0.double()[None].repeat(T, 1, 1)
    b = torch.zeros_like(p)
    if with_motion:
        A, col_err = MR.exact_object_motion(MR.motion_about_origin("rot", 50, T), MR.exact_center(p0, flags), c_used, (MH, MW))
        p, b = MR.affine32(A, p, b, col_err, flags)
    moved = (p, b)
    screen = MR.project32(m["poses"].double()[:, :3, :], m["intr"].double(), p, b)
    return moved, screen, MR.scale32(screen[0], screen[1], MW, MH)


def test_moge_route_stages_within_the_derived_bound_and_fused_equal_to_their_composition(golden):
    import motion_restatement as MR
    from flexam_amd import CameraMotionGenerator, ObjectMotionGenerator, convert_moge_to_delta_format, moge_tracks
    m = golden("g15_motion_moge")
    pm, valid = m["point_map"], m["valid_mask"]
    cam = CameraMotionGenerator("rot y 14; trans 0.05 -0.02 -0.3", frame_num=T, H=MH, W=MW, device=dev())
    cam.set_intr(m["intr"])
    poses = cam.get_default_motion()
    assert torch.equal(poses, m["poses"])
    maps = pm.to(dev()).unsqueeze(0).expand(T, MH, MW, 3)           # a stride-0 view: read as one map
    moved = ObjectMotionGenerator(device=dev()).apply_motion(maps, m["object_mask"], "rot", 50, num_frames=T, tracking_method="moge")
    moved_rep = ObjectMotionGenerator(device=dev()).apply_motion(pm.unsqueeze(0).repeat(T, 1, 1, 1), m["object_mask"], "rot", 50, num_frames=T,
                                                                tracking_method="moge")
    assert moved.shape == (T, MH, MW, 3) and torch.equal(moved.view(torch.int32), moved_rep.view(torch.int32))
    screen = cam.w2s_moge(moved.reshape(T, MH * MW, 3), poses)
    delta, vis = convert_moge_to_delta_format(screen.reshape(T, MH, MW, 3), valid, MH, MW, device=dev())
    n = int(valid.sum())
    assert delta.shape == (T, n, 3) and vis.shape == (T, n) and vis.dtype == bool and vis.all()
    c_hip = _hip_center(pm.reshape(-1, 3), mask_flat=m["object_mask"].reshape(-1))
    keep = valid.reshape(-1)
    for what, res, c_used in (("hip", (moved.cpu(), screen.cpu(), delta.cpu()), c_hip), ("reference", (m["moved"], m["screen"], m["delta"]), m["center"])):
        (mv, mb), (sv, sb), (pv, pb) = _moge_exact(m, c_used)
        for stage, got, val, bound in (("apply_motion", res[0].reshape(T, -1, 3), mv, mb), ("w2s_moge", res[1], sv, sb),
                                       ("convert_moge_to_delta_format", res[2], pv[:, keep], pb[:, keep])):
            ok, worst = MR.close32(got, val, bound)
            print(f"moge {stage} {what}: worst |err| / (2 B) = {worst:.3f}")
            assert ok, (what, stage, worst)
    fused, vis2 = moge_tracks(pm, valid, cam, poses, MH, MW, object_mask=m["object_mask"], object_motion="rot", distance=50)
    assert torch.equal(fused.view(torch.int32), delta.view(torch.int32)) and np.array_equal(vis, vis2)
    # without object motion: camera only
    plain, _ = moge_tracks(pm, valid, cam, poses, MH, MW)
    sep, _ = convert_moge_to_delta_format(cam.w2s_moge(pm.reshape(1, -1, 3).repeat(T, 1, 1), poses).reshape(T, MH, MW, 3), valid, MH, MW, device=dev())
    assert torch.equal(plain.view(torch.int32), sep.view(torch.int32))
    (_, _), (_, _), (pv, pb) = _moge_exact(m, None, with_motion=False)
    ok, worst = MR.close32(plain.cpu(), pv[:, keep], pb[:, keep])
    assert ok, worst


# ----------------------------------------------------------------------------- float64 transforms
def test_vggt_route_within_the_derived_bound(golden):
    import motion_restatement as MR
    from flexam_amd import CameraMotionGenerator
    g = golden("g15_motion_vggt")
    ext, itr, poses = g["extrinsics"], g["intrinsics"], g["poses"]
    cam = CameraMotionGenerator("rot y 160 0 8; trans 0.3 0.1 -0.5", frame_num=T, H=MH, W=MW, device=dev())
    assert torch.equal(cam.get_default_motion(), poses)
    kinv, rinv, tvec, _, _ = MR.vggt_host_matrices(ext, itr)
    for tag in ("64", "32"):
        src = g[f"tracks{tag}"]
        world = cam.s2w_vggt(src, ext, itr)
        assert world.is_cuda and world.dtype == src.dtype                  # the dtype of `points`: float32 in, computed in double, rounded once
        val, bound, valid_in = MR.unproject64(src.numpy(), kinv, rinv, tvec)
        extra = MR.U32 * np.abs(val) if tag == "32" else None
        for what, res in (("hip", world.cpu().numpy()), ("reference", g[f"world{tag}"].numpy())):
            ok, worst = MR.close64(res, val, bound, extra)
            print(f"s2w_vggt float{tag} {what}: worst |err| / limit = {worst:.3f}")
            assert ok and (res[~valid_in] == 0).all(), (what, tag, worst)
        assert (~valid_in).any()
    for tag, kw in (("none", dict(poses=None)), ("override", dict(poses=poses, override_extrinsics=True)), ("ontop", dict(poses=poses, override_extrinsics=False))):
        for w in ("64", "32"):
            if f"screen.{tag}.{w}" not in g:
                continue
            world = g[f"world{w}"]
            got = cam.w2s_vggt(world, ext, itr, **kw)
            assert got.is_cuda and got.dtype == torch.float64
            _, _, _, pose, intr64 = MR.vggt_host_matrices(ext, itr, kw.get("poses"), kw.get("override_extrinsics", True))
            val, bound, valid_out, _ = MR.project64(world.numpy(), pose, intr64)
            ref = g[f"screen.{tag}.{w}"]
            for what, res in (("hip", got.cpu()), ("reference", ref)):
                ok, worst = MR.close64(res.numpy(), val, bound)
                print(f"w2s_vggt {tag} float{w} {what}: worst |err| / (2 B) = {worst:.3f}")
                assert ok and (res.numpy()[~valid_out] == 0).all(), (what, tag, w, worst)
            assert torch.equal(got.cpu()[..., 2] > 0, ref[..., 2] > 0)      # validity flags identical to the reference's


# ----------------------------------------------------------------------------- end to end: edited tracks -> six videos, bit-identical
def _videos(tracks, vis, point_wise):
    from flexam_amd import visualize_tracking_DELTA
    tr, cos, dep = visualize_tracking_DELTA(tracks, vis_mask=vis, point_wise=point_wise, height=MH, width=MW, cos_level=4, device=dev(),
                                            generator=np.random.RandomState(0))
    return [tr] + [cos[i] for i in range(4)] + [dep]


def _assert_videos(got, want_u8):
    for k, v in enumerate(got):
        want = (want_u8[k].float() / 255).permute(3, 0, 1, 2).unsqueeze(0)
        assert torch.equal(v.cpu(), want), f"video {k}: {int((v.cpu() != want).sum())} values differ"


def test_end_to_end_moge_route_videos_are_bit_identical_to_the_reference(golden):
    from flexam_amd import CameraMotionGenerator, moge_tracks
    m = golden("g15_motion_moge")
    cam = CameraMotionGenerator("rot y 14; trans 0.05 -0.02 -0.3", frame_num=T, H=MH, W=MW, device=dev())
    cam.set_intr(m["intr"])
    tracks, vis = moge_tracks(m["point_map"], m["valid_mask_e2e"], cam, cam.get_default_motion(), MH, MW, object_mask=m["object_mask"],
                              object_motion="rot", distance=50)
    _assert_videos(_videos(tracks, vis, 2), m["videos_e2e"])


def test_end_to_end_vggt_route_videos_are_bit_identical_to_the_reference(golden):
    from flexam_amd import CameraMotionGenerator
    g = golden("g15_motion_vggt")
    cam = CameraMotionGenerator("rot y 8; trans 0.05 0 0.1", frame_num=T, H=MH, W=MW, device=dev())
    poses = cam.get_default_motion()
    assert torch.equal(poses, g["e2e_poses"])
    src = g["tracks64"][:, g["e2e_keep"]]
    tracks = cam.w2s_vggt(cam.s2w_vggt(src, g["extrinsics"], g["intrinsics"]), g["extrinsics"], g["intrinsics"], poses, override_extrinsics=False)
    _assert_videos(_videos(tracks, g["e2e_vis"].numpy(), 4), g["videos_e2e"])


# ----------------------------------------------------------------------------- full size
def test_moge_tracks_full_size_against_the_float64_restatement_and_twice_equal():
    """97 x 512 x 896: T N 3 = 133 M elements (index arithmetic past 2^31 bytes), the broadcast-source path, a rotation and an object
    motion.  The float64 restatement runs in torch on the GPU, a few frames at a time."""
    import motion_restatement as MR
    from flexam_amd import CameraMotionGenerator, moge_tracks
    from flexam_amd import hip as H
    from flexam_amd.motion import _center
    Tn, Hn, Wn = 97, 512, 896
    g = torch.Generator().manual_seed(5)
    v, u = torch.meshgrid((torch.arange(Hn) + 0.5) / Hn, (torch.arange(Wn) + 0.5) / Wn, indexing="ij")
    z = 2.0 + 0.8 * torch.sin(3 * u) + 0.5 * v + 0.3 * torch.rand(Hn, Wn, generator=g)
    pm = torch.stack([(u - 0.5) / 0.9 * z, (v - 0.5) / 1.35 * z, z], -1).float()
    valid = torch.rand(Hn, Wn, generator=g) > 0.1
    pm[~valid] = float("nan")
    obj = torch.zeros(Hn, Wn, dtype=torch.bool)
    obj[100:400, 200:700] = True
    intr = torch.tensor([[0.9, 0.0, 0.5], [0.0, 1.35, 0.5], [0.0, 0.0, 1.0]])
    cam = CameraMotionGenerator("rot y 25", frame_num=Tn, H=Hn, W=Wn, device=dev())
    cam.set_intr(intr)
    poses = cam.get_default_motion()
    pm_d, valid_d, obj_d = pm.to(dev()), valid.to(dev()), obj.to(dev())
    out, vis = moge_tracks(pm_d, valid_d, cam, poses, Hn, Wn, object_mask=obj_d, object_motion="left", distance=50)
    n = int(valid.sum())
    assert out.shape == (Tn, n, 3) and vis.shape == (Tn, n)
    again, _ = moge_tracks(pm_d, valid_d, cam, poses, Hn, Wn, object_mask=obj_d, object_motion="left", distance=50)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    del again
    p0 = pm_d.reshape(-1, 3)
    flags, sums = H.motion_select_map(p0, obj_d.reshape(-1))
    assert torch.equal(flags, obj_d.reshape(-1) & ~torch.isnan(p0).any(dim=1))
    c_used = _center(sums).to(dev())
    c_star = MR.exact_center(p0, flags)
    m = MR.motion_about_origin("left", 50, Tn).to(dev())
    A, col_err = MR.exact_object_motion(m, c_star, c_used, (Hn, Wn))
    keep = valid_d.reshape(-1)
    P, K = poses.double()[:, :3, :].to(dev()), intr.double().to(dev())
    worst = 0.0
    for t0 in range(0, Tn, 8):
        t1 = min(Tn, t0 + 8)
        p = p0.double()[None].expand(t1 - t0, -1, -1)
        val, b = MR.affine32(A[t0:t1], p, torch.zeros_like(p), col_err[t0:t1], flags)
        val, b = MR.project32(P[t0:t1], K, val, b)
        val, b = MR.scale32(val, b, Wn, Hn)
        ok, w = MR.close32(out[t0:t1], val[:, keep], b[:, keep])
        worst = max(worst, w)
        assert ok, (t0, w)
        del val, b, p
    print(f"moge_tracks 97 x 512 x 896: worst |err| / (2 B) = {worst:.3f}")


# ----------------------------------------------------------------------------- argument errors through the ABI
def test_motion_argument_errors_return_codes_without_a_launch():
    import ctypes
    from flexam_amd import hip as H
    from flexam_amd.abi import CONSTANTS as C
    lib = H.lib()
    E_ARG, E_SHAPE = C["FLEXAM_E_ARG"], C["FLEXAM_E_SHAPE"]
    pts = torch.zeros(2048, 3, device=dev())
    mask = torch.ones(2048, dtype=torch.uint8, device=dev())
    flags = torch.zeros(2048, dtype=torch.uint8, device=dev())
    ws = torch.zeros(64, dtype=torch.float64, device=dev())
    idx = torch.zeros(2048, dtype=torch.int32, device=dev())
    out = torch.zeros(2, 2048, 3, device=dev())
    mats = torch.zeros(2, 3, 4, device=dev())
    d64 = torch.zeros(2, 2048, 3, dtype=torch.float64, device=dev())
    m64 = torch.zeros(2, 12, dtype=torch.float64, device=dev())
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    err = lambda: lib.flexam_last_error().decode()
    assert lib.flexam_motion_select_map(None, 2048, p(mask), p(flags), p(ws), 512, p(ws), None) == E_ARG and "null" in err()
    assert lib.flexam_motion_select_map(p(pts), 0, p(mask), p(flags), p(ws), 512, p(ws), None) == E_SHAPE
    assert lib.flexam_motion_select_map(p(pts), 2048, p(mask), p(flags), p(ws), 63, p(ws), None) == E_ARG and "workspace" in err()
    assert lib.flexam_motion_select_map(p(pts), 2048, p(mask), p(flags), off(ws, 4), 256, p(ws), None) == E_ARG and "alignment" in err()
    assert lib.flexam_motion_select_pixels(p(pts), 2048, p(mask), 0, 8, p(flags), p(ws), 512, p(ws), None) == E_SHAPE
    assert lib.flexam_motion_compact(p(mask), 2048, None, p(idx), p(idx), 64, None) == E_ARG
    assert lib.flexam_motion_compact(p(mask), 2048, p(idx), p(idx), p(idx), 4, None) == E_ARG and "workspace" in err()
    assert lib.flexam_motion_compact(p(mask), 0, p(idx), p(idx), p(idx), 64, None) == E_SHAPE
    assert lib.flexam_motion_compact(p(mask), 2048, off(idx, 2), p(idx), p(idx), 64, None) == E_ARG
    f = ctypes.c_float
    assert lib.flexam_motion_transform_f32(None, 0, 2, 2048, None, None, None, None, f(1), f(1), None, 2048, p(out), None) == E_ARG
    assert lib.flexam_motion_transform_f32(p(pts), 0, 2, 2048, None, None, p(mats), None, f(1), f(1), None, 2048, p(out), None) == E_ARG     # pose without intr
    assert lib.flexam_motion_transform_f32(p(pts), 0, 2, 2048, p(flags), None, None, None, f(1), f(1), None, 2048, p(out), None) == E_ARG    # flags without motion
    assert lib.flexam_motion_transform_f32(p(pts), 0, 0, 2048, None, None, None, None, f(1), f(1), None, 2048, p(out), None) == E_SHAPE
    assert lib.flexam_motion_transform_f32(p(pts), 0, 2, 2048, None, None, None, None, f(1), f(1), None, 100, p(out), None) == E_SHAPE       # M != N without an index
    assert lib.flexam_motion_transform_f32(p(pts), 0, 2, 2048, None, None, None, None, f(1), f(1), p(idx), 4096, p(out), None) == E_SHAPE    # M > N
    assert lib.flexam_motion_transform_f32(p(pts), 5, 2, 2048, None, None, None, None, f(1), f(1), None, 2048, p(out), None) == E_SHAPE      # frame stride < 3 N
    assert lib.flexam_motion_transform_f32(off(pts, 2), 0, 2, 2048, None, None, None, None, f(1), f(1), None, 2048, p(out), None) == E_ARG
    assert lib.flexam_motion_unproject_f64(p(d64), 0, 2, 2048, None, p(m64), p(m64), p(d64), None) == E_ARG
    assert lib.flexam_motion_unproject_f64(off(d64, 4), 0, 2, 2048, p(m64), p(m64), p(m64), p(d64), None) == E_ARG and "misaligned" in err()
    assert lib.flexam_motion_unproject_f64(p(d64), 0, 2, 0, p(m64), p(m64), p(m64), p(d64), None) == E_SHAPE
    assert lib.flexam_motion_project_f64(p(d64), 0, 2, 2048, p(m64), None, p(d64), None) == E_ARG
    assert lib.flexam_motion_project_f64(p(d64), 0, 0, 2048, p(m64), p(m64), p(d64), None) == E_SHAPE
    assert lib.flexam_motion_project_f64(p(d64), 0, 2, 2048, p(m64), off(m64, 4), p(d64), None) == E_ARG
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and float(d64.abs().sum()) == 0.0              # nothing was launched
    with pytest.raises(RuntimeError, match="not on a GPU"):
        H.motion_compact(torch.ones(8, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="frames"):
        H.motion_transform(torch.zeros(3, 8, 3, device=dev()), 2)
    with pytest.raises(ValueError, match="num_frames"):
        from flexam_amd import ObjectMotionGenerator
        ObjectMotionGenerator(device=dev()).apply_motion(torch.zeros(4, 8, 3), torch.ones(4, 4, dtype=torch.bool), "left", 50, num_frames=9)
