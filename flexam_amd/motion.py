"""Edit tracks: camera motion and object motion on the 3-D tracks, the step between the tracker and the conditioning rasteriser.

Mirrors, under their own names, the reference's

  CameraMotionGenerator          pipelines.py:195-850     `--camera_motion "rot y 25"`: poses, and the tracks seen through them
  ObjectMotionGenerator          pipelines.py:852-1038    `--object_motion left`: the masked points moved rigidly about their centre
  convert_moge_to_delta_format   pipelines.py:1255-1291   MoGe point maps -> the rasteriser's [T, N, 3] pixel tracks

and adds `moge_tracks`, demo.py:222-266 as one launch chain that never builds the [T, H, W, 3] copies of the first frame's point map.

Split of the work: everything O(T) -- parsing the motion string, the [T, 4, 4] pose and motion matrices, the 3x3 inverses -- is torch /
numpy on the HOST in the reference's dtypes (the matrices a CPU run of the reference makes, bit for bit; pose tables are therefore
host tensors here, whatever `device` is); everything per point is csrc/motion.hip and stays on the GPU.  There is no CPU path for the
tracks: without the HIP library `flexam_amd.hip` raises.

Kept reference behaviours: a motion segment with start_frame == end_frame raises ZeroDivisionError; w2s_vggt divides the pose
translations by 5; apply_motion on MoGe maps divides the x / y translation by W / H; _get_points_in_mask rounds halves to even.
Differences: `num_frames` must equal the number of frames of the tracks (the reference indexes past its motion table or leaves the
later frames unmoved); tracks come back as GPU tensors where the reference returns numpy arrays / CPU tensors; set_intr does not
print.  Refused (NotImplementedError): the `path` camera motion, process_pose_file, process_video_file (un-vendored Pi3 code)."""
import math

import numpy as np
import torch

from . import hip


def _device(device):
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"flexam_amd.motion: tracks are computed on a GPU, not on '{device}' (there is no CPU path)")
    return device


def _host_tensor(x):
    return x.detach().cpu() if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))


def _host_array(x):
    """numpy view of camera matrices, the leading batch dimension of [B, T, r, c] dropped (pipelines.py:371-381)."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
        if x.ndim == 4:
            x = x[0]
    return x


def _rows3(mats, device, dtype):
    """[T, 4, 4] or [T, 3, 4] host matrices -> their first three rows, contiguous, on the device."""
    return _host_tensor(mats)[:, :3, :].to(dtype).contiguous().to(device)


def _segment(params, fixed, frame_num, usage):
    """Frame range of one motion clause: `fixed` words, optionally followed by <start_frame> <end_frame> (clamped, ordered)."""
    if len(params) not in (fixed, fixed + 2):
        raise ValueError(usage)
    start, end = 0, frame_num - 1
    if len(params) == fixed + 2:
        start = max(0, min(frame_num - 1, int(params[fixed])))
        end = max(0, min(frame_num - 1, int(params[fixed + 1])))
        if start > end:
            start, end = end, start
    return start, end


class CameraMotionGenerator:
    """pipelines.py:195-850.  `device` is where the projected tracks live (None = the current GPU)."""

    def __init__(self, motion_type, frame_num=49, H=480, W=720, fx=None, fy=None, fov=55, device=None, pose_file=None):
        self.motion_type = motion_type
        self.frame_num = frame_num
        self.fov = fov
        self.device = device
        self.W = W
        self.H = H
        self.pose_file = pose_file
        if not fx or not fy:
            fx = fy = (W / 2) / math.tan(math.radians(fov) / 2)
        self.intr = torch.tensor([[0, 0, W / 2], [0, 0, H / 2], [0, 0, 1]], dtype=torch.float32)
        self.intr[0, 0] = fx
        self.intr[1, 1] = fy
        self.extr = torch.eye(4)

    # ------------------------------------------------------------------ host: O(T) matrices
    def set_intr(self, K):
        self.intr = _host_tensor(K)

    def set_extr(self, extr):
        self.extr = _host_tensor(extr)

    def process_pose_file(self, *args, **kwargs):
        raise NotImplementedError("process_pose_file (pipelines.py:219-258) feeds the `path` motion only, which is not part of this build")

    def process_video_file(self, *args, **kwargs):
        raise NotImplementedError("process_video_file (pipelines.py:260-321) runs the Pi3 model of an un-vendored submodule")

    def convert_cameras_to_poses(self, intrinsic_list, extrinsic_list):
        """pipelines.py:323-354: 3x4 extrinsics -> [frame_num, 4, 4] float32, the last pose repeated or the list cut to frame_num."""
        poses = []
        for _, extrinsic in zip(intrinsic_list, extrinsic_list):
            pose = np.eye(4)
            pose[:3, :4] = np.array(extrinsic)
            poses.append(pose)
        arr = np.array(poses)
        if len(poses) < self.frame_num:
            arr = np.concatenate([arr, arr[-1:].repeat(self.frame_num - len(poses), axis=0)], axis=0)
        elif len(poses) > self.frame_num:
            arr = arr[:self.frame_num]
        return torch.from_numpy(arr).float()

    def rot_poses(self, angle, axis='y'):
        """pipelines.py:543-581: one [4, 4] float32 rotation by `angle` degrees."""
        rad = torch.tensor(math.radians(angle))
        c, s = torch.cos(rad), torch.sin(rad)
        if axis not in ('x', 'y', 'z'):
            raise ValueError("Invalid axis value. Choose 'x', 'y', or 'z'.")
        i, j = {'x': (1, 2), 'y': (2, 0), 'z': (0, 1)}[axis]
        m = torch.eye(4, dtype=torch.float32)
        m[i, i] = c
        m[i, j] = -s
        m[j, i] = s
        m[j, j] = c
        return m

    def trans_poses(self, dx, dy, dz):
        """pipelines.py:583-604: [frame_num, 4, 4], frame i translated by i / (frame_num - 1) of (dx, dy, dz)."""
        mats = torch.eye(4).unsqueeze(0).repeat(self.frame_num, 1, 1)
        steps = torch.arange(self.frame_num, dtype=torch.float64)
        for row, d in enumerate((dx, dy, dz)):
            mats[:, row, 3] = (steps * (d / (self.frame_num - 1))).float()       # i * delta in double, rounded on assignment
        return mats

    def _look_at(self, camera_position, target_position):
        direction = target_position - camera_position
        direction /= np.linalg.norm(direction)
        right = np.cross(np.array([0, 1, 0]), direction)
        right /= np.linalg.norm(right)
        return np.linalg.inv(np.vstack([right, np.cross(direction, right), direction]))

    def spiral_poses(self, radius, forward_ratio=0.5, backward_ratio=0.5, rotation_times=0.1, look_at_times=0.5):
        """pipelines.py:620-659: [frame_num, 4, 4] float64, the camera on a flattened spiral looking at (0, 0, radius * look_at_times)."""
        t = np.linspace(0, 1, self.frame_num)
        r = np.sin(np.pi * t) * radius * rotation_times
        theta = 2 * np.pi * t
        y = r * np.cos(theta) * 0.15
        x = r * np.sin(theta) * 0.5
        z = -r
        z[z < 0] *= forward_ratio
        z[z > 0] *= backward_ratio
        target = np.array([0, 0, radius * look_at_times])
        poses = np.zeros((self.frame_num, 4, 4))
        for k, pos in enumerate(np.vstack([x, y, z]).T):
            m = np.eye(4)
            m[:3, :3] = self._look_at(pos, target)
            m[:3, 3] = pos
            poses[k] = m
        return torch.from_numpy(poses)

    def get_default_motion(self):
        """pipelines.py:661-850: "trans <dx> <dy> <dz> [start end]; rot <axis> <angle> [start end]; spiral <radius> [start end]" ->
        [frame_num, 4, 4] float32, the clauses multiplied up in order; frames past a clause's end keep its last matrix."""
        if not isinstance(self.motion_type, str):
            raise ValueError(f'camera_motion must be a string, but got {type(self.motion_type)}')
        n = self.frame_num
        final = torch.eye(4).unsqueeze(0).repeat(n, 1, 1)
        for clause in (s.strip() for s in self.motion_type.split(';')):
            params = clause.lower().split()
            if not params:
                continue
            kind = params[0]
            if kind == 'trans':
                start, end = _segment(params, 4, n, f"trans motion requires 3 or 5 parameters: 'trans <dx> <dy> <dz>' or "
                                                    f"'trans <dx> <dy> <dz> <start_frame> <end_frame>', got: {clause}")
                vec = torch.tensor([float(p) for p in params[1:4]])
                frame = lambda t, cur: cur[:3, 3].copy_(vec * t)
            elif kind == 'rot':
                start, end = _segment(params, 3, n, f"rot motion requires 2 or 4 parameters: 'rot <axis> <angle>' or "
                                                    f"'rot <axis> <angle> <start_frame> <end_frame>', got: {clause}")
                axis = params[1]
                if axis not in ('x', 'y', 'z'):
                    raise ValueError(f"Invalid rotation axis '{axis}', must be 'x', 'y' or 'z'")
                angle = float(params[2])
                frame = lambda t, cur: cur.copy_(self.rot_poses(angle * t, axis))
            elif kind == 'spiral':
                start, end = _segment(params, 2, n, f"spiral motion requires 1 or 3 parameters: 'spiral <radius>' or "
                                                    f"'spiral <radius> <start_frame> <end_frame>', got: {clause}")
                spiral = self.spiral_poses(float(params[1]))
                frame = lambda t, cur: cur.copy_(spiral[int(t * (len(spiral) - 1))])
            elif kind == 'path':
                raise NotImplementedError("camera motion 'path' (pipelines.py:792-845) inverts its poses with se3_inverse of the un-vendored Pi3 "
                                          "submodule: not part of this build; pass explicit poses (convert_cameras_to_poses)")
            else:
                raise ValueError(f'camera_motion type must be in [trans, spiral, rot, path], but got {kind}')
            current = torch.eye(4).unsqueeze(0).repeat(n, 1, 1)
            for f in range(start, n):
                if f <= end:
                    frame((f - start) / (end - start), current[f])       # start == end: ZeroDivisionError, as the reference
                else:
                    current[f] = current[end]
            final = torch.matmul(final, current)
        return final

    # ------------------------------------------------------------------ GPU: per-point work
    def w2s_moge(self, pts, poses):
        """pipelines.py:512-530: world points [T, N, 3] -> (u, v, depth) through poses [T, 4, 4] and self.intr, float32 on the GPU."""
        poses = _host_tensor(poses)
        assert poses.shape[0] == self.frame_num
        dev = _device(self.device)
        pts = torch.as_tensor(pts).to(dev).float().contiguous()
        with torch.cuda.device(dev):
            return hip.motion_transform(pts, pts.shape[0], pose=_rows3(poses, dev, torch.float32),
                                        intr=self.intr.to(torch.float32).contiguous().to(dev))

    def s2w_vggt(self, points, extrinsics, intrinsics):
        """pipelines.py:356-417: (u, v, z) tracks [T, N, 3] -> world points, in double, returned in the dtype of `points` on the GPU.
        Points with z <= 0 give zeros.  The 3x3 inverses are numpy's, in the dtype the matrices arrive in."""
        dev = _device(self.device)
        extrinsics, intrinsics = _host_array(extrinsics), _host_array(intrinsics)
        points = torch.as_tensor(points).to(dev)
        if points.dtype != torch.float32:
            points = points.double()
        T = points.shape[0]
        kinv = np.stack([np.linalg.inv(intrinsics[i]) for i in range(T)]).astype(np.float64)
        rinv = np.stack([np.linalg.inv(extrinsics[i, :, :3]) for i in range(T)]).astype(np.float64)
        tvec = np.ascontiguousarray(extrinsics[:T, :, 3], dtype=np.float64)
        with torch.cuda.device(dev):
            return hip.motion_unproject(points.contiguous(), torch.from_numpy(kinv).to(dev), torch.from_numpy(rinv).to(dev),
                                        torch.from_numpy(tvec).to(dev))

    def w2s_vggt(self, world_points, extrinsics, intrinsics, poses=None, override_extrinsics=True):
        """pipelines.py:419-510: world points [T, N, 3] -> (u, v, depth) float64 on the GPU through `poses` (translations / 5; on top of
        the extrinsics when override_extrinsics is False) or, without poses, the first frame's extrinsics.  depth <= 0 gives zeros."""
        dev = _device(self.device)
        extrinsics, intrinsics = _host_array(extrinsics), _host_array(intrinsics)
        world_points = torch.as_tensor(world_points).to(dev)
        if world_points.dtype != torch.float32:
            world_points = world_points.double()
        T = world_points.shape[0]
        if poses is None:
            first = np.eye(4)
            first[:3, :3] = extrinsics[0, :, :3]
            first[:3, 3] = extrinsics[0, :, 3]
            camera_poses = np.tile(first[np.newaxis, :, :], (T, 1, 1))
        else:
            given = poses.cpu().numpy() if isinstance(poses, torch.Tensor) else poses
            camera_poses = given.copy()
            camera_poses[:, :3, 3] = given[:, :3, 3] / 5.0
            if not override_extrinsics:
                for i in range(T):
                    ext = np.eye(4)
                    ext[:3, :3] = extrinsics[i, :, :3]
                    ext[:3, 3] = extrinsics[i, :, 3]
                    camera_poses[i] = np.matmul(camera_poses[i], ext)            # rounded to the poses' dtype, as the reference
        pose = np.ascontiguousarray(camera_poses[:T, :3, :], dtype=np.float64)
        intr = np.ascontiguousarray(intrinsics[:T], dtype=np.float64)
        with torch.cuda.device(dev):
            return hip.motion_project(world_points.contiguous(), torch.from_numpy(pose).to(dev), torch.from_numpy(intr).to(dev))


_S2, _S3 = math.sqrt(2), math.sqrt(3)
# pipelines.py:884-928: name -> ('trans', direction, divisor) or (rotation kind, plane (i, j), sign of the entry [i, j])
OBJECT_MOTIONS = {
    'up': ('trans', (0, -1, 0), None), 'down': ('trans', (0, 1, 0), None), 'left': ('trans', (-1, 0, 0), None),
    'right': ('trans', (1, 0, 0), None), 'front': ('trans', (0, 0, 1), None), 'back': ('trans', (0, 0, -1), None),
    'up_left': ('trans', (-1, -1, 0), _S2), 'up_right': ('trans', (1, -1, 0), _S2), 'down_left': ('trans', (-1, 1, 0), _S2),
    'down_left2': ('trans', (-1, 0.5, 0), _S2), 'down_right': ('trans', (1, 1, 0), _S2),
    'up_front': ('trans', (0, -1, 1), _S2), 'up_back': ('trans', (0, -1, -1), _S2), 'down_front': ('trans', (0, 1, 1), _S2),
    'down_back': ('trans', (0, 1, -1), _S2), 'left_front': ('trans', (-1, 0, 1), _S2), 'left_back': ('trans', (-1, 0, -1), _S2),
    'right_front': ('trans', (1, 0, 1), _S2), 'right_back': ('trans', (1, 0, -1), _S2),
    'up_left_front': ('trans', (-1, -1, 1), _S3), 'up_left_back': ('trans', (-1, -1, -1), _S3), 'up_right_front': ('trans', (1, -1, 1), _S3),
    'up_right_back': ('trans', (1, -1, -1), _S3), 'down_left_front': ('trans', (-1, 1, 1), _S3), 'down_left_back': ('trans', (-1, 1, -1), _S3),
    'down_right_front': ('trans', (1, 1, 1), _S3), 'down_right_back': ('trans', (1, 1, -1), _S3),
    'rot': ('rot', (0, 2), 1), 'rot_ccw': ('rot', (0, 2), -1), 'pitch_up': ('rot', (1, 2), -1), 'pitch_down': ('rot', (1, 2), 1),
    'roll_left': ('rot', (0, 1), -1), 'roll_right': ('rot', (0, 1), 1),
}


def object_motion_matrices(center, motion_type, distance, num_frames):
    """pipelines.py:930-1008 on the host: [num_frames, 4, 4] float32, frame f = translate(center) . M(f / (num_frames - 1)) .
    translate(-center) with M a translation of t * distance along the named direction or a rotation by t * distance degrees."""
    if motion_type not in OBJECT_MOTIONS:
        raise ValueError(f"unknown motion type: {motion_type}")
    kind, spec, extra = OBJECT_MOTIONS[motion_type]
    center = torch.as_tensor(center, dtype=torch.float32).cpu()
    if kind == 'trans':
        base = torch.tensor(spec)
        if extra is not None:
            base = base / extra
        base = base * distance
    motions = []
    for f in range(num_frames):
        t = f / (num_frames - 1)
        about = torch.eye(4)
        about[:3, 3] = -center
        m = torch.eye(4)
        if kind == 'trans':
            m[:3, 3] = base * t
        else:
            rad = torch.deg2rad(torch.tensor(distance * t))
            c, s = torch.cos(rad), torch.sin(rad)
            (i, j) = spec
            m[i, i] = c
            m[i, j] = s if extra > 0 else -s
            m[j, i] = -s if extra > 0 else s
            m[j, j] = c
        about = m @ about
        about[:3, 3] += center
        motions.append(about)
    return torch.stack(motions)


def _center(sums):
    """float32 centre of the selected points from the kernel's double sums; no point selected: NaN, as the mean of nothing."""
    s = sums.cpu()
    return (s[:3] / s[3]).to(torch.float32)


def _moge_motion_rows(center, motion_type, distance, num_frames, H, W, device):
    motions = object_motion_matrices(center, motion_type, distance, num_frames)
    if W > 1:                                          # pipelines.py:1016-1019: the maps are in normalised image units
        motions[:, 0, 3] /= W
        motions[:, 1, 3] /= H
    return _rows3(motions, device, torch.float32)


class ObjectMotionGenerator:
    """pipelines.py:852-1038."""

    def __init__(self, device=None):
        self.device = device
        self.num_frames = 49

    def _get_points_in_mask(self, pred_tracks, mask):
        """pipelines.py:857-876: [N] bool, the mask [H, W] at the first frame's (x, y), rounded half to even and clamped."""
        dev = _device(self.device)
        first = torch.as_tensor(pred_tracks)[0].to(dev).float().contiguous()
        with torch.cuda.device(dev):
            return hip.motion_select_pixels(first, torch.as_tensor(mask).to(dev).bool().contiguous())[0]

    def apply_motion(self, pred_tracks, mask, motion_type, distance, num_frames=49, tracking_method="DELTA"):
        """pipelines.py:878-1038.  DELTA: pred_tracks [T, N, 3] pixel tracks; "moge": [T, H, W, 3] point maps (an expanded view of one
        map, stride 0 over T, is read as one map).  Returns the moved tracks, same shape, float32 on the GPU."""
        if motion_type not in OBJECT_MOTIONS:
            raise ValueError(f"unknown motion type: {motion_type}")
        self.num_frames = num_frames
        dev = _device(self.device)
        tracks = torch.as_tensor(pred_tracks).to(dev).float()
        if tracks.shape[0] != num_frames:
            raise ValueError(f"apply_motion: {tracks.shape[0]} frames of tracks for num_frames = {num_frames}")
        mask = torch.as_tensor(mask).to(dev).bool().contiguous()
        with torch.cuda.device(dev):
            if tracking_method == "moge":
                T, H, W, _ = tracks.shape
                first = tracks[0].contiguous().reshape(-1, 3)
                flags, sums = hip.motion_select_map(first, mask.reshape(-1))
                rows = _moge_motion_rows(_center(sums), motion_type, distance, num_frames, H, W, dev)
                src = first if tracks.stride(0) == 0 else tracks.contiguous().reshape(T, -1, 3)
                return hip.motion_transform(src, T, flags=flags, motion=rows).reshape(T, H, W, 3)
            tracks = tracks.contiguous()
            flags, sums = hip.motion_select_pixels(tracks[0], mask)
            rows = _rows3(object_motion_matrices(_center(sums), motion_type, distance, num_frames), dev, torch.float32)
            return hip.motion_transform(tracks, tracks.shape[0], flags=flags, motion=rows)


def convert_moge_to_delta_format(moge_points, mask, height, width, device=None):
    """pipelines.py:1255-1291: point maps [T, H, W, 3] in normalised image units, mask [H, W] bool -> (tracks [T, N, 3] float32 on the GPU
    with x * width, y * height, the masked positions in row-major order; visibility [T, N] numpy bool, all True)."""
    dev = _device(device)
    pts = torch.as_tensor(moge_points).to(dev).float().contiguous()
    T, H, W, _ = pts.shape
    with torch.cuda.device(dev):
        index, count = hip.motion_compact(torch.as_tensor(mask).to(dev).bool().reshape(-1).contiguous())
        n = int(count.item())
        out = hip.motion_transform(pts.reshape(T, H * W, 3), T, scale=(width, height), index=index, count=n)
    return out, np.ones((T, n), dtype=bool)


def moge_tracks(point_map, valid_mask, cam, poses, height, width, object_mask=None, object_motion=None, distance=50, device=None):
    """demo.py:222-266 in one launch chain: the first frame's point map [H, W, 3] and MoGe's validity mask [H, W], optionally moved by
    `object_motion` inside `object_mask` [H, W], seen through `poses` [T, 4, 4] and cam.intr, scaled to pixels and gathered by the
    validity mask -- exactly what ObjectMotionGenerator.apply_motion(map repeated T times, tracking_method="moge"), cam.w2s_moge and
    convert_moge_to_delta_format return one after the other, without their [T, H, W, 3] intermediates."""
    dev = _device(device if device is not None else cam.device)
    poses = _host_tensor(poses)
    T = poses.shape[0]
    assert T == cam.frame_num
    pm = torch.as_tensor(point_map).to(dev).float().contiguous()
    H, W, _ = pm.shape
    pm = pm.reshape(-1, 3)
    with torch.cuda.device(dev):
        flags = rows = None
        if object_motion:
            if object_mask is None:
                raise ValueError("Object motion specified but no mask provided")
            if object_motion not in OBJECT_MOTIONS:
                raise ValueError(f"unknown motion type: {object_motion}")
            flags, sums = hip.motion_select_map(pm, torch.as_tensor(object_mask).to(dev).bool().reshape(-1).contiguous())
            rows = _moge_motion_rows(_center(sums), object_motion, distance, T, H, W, dev)
        index, count = hip.motion_compact(torch.as_tensor(valid_mask).to(dev).bool().reshape(-1).contiguous())
        n = int(count.item())
        out = hip.motion_transform(pm, T, flags=flags, motion=rows, pose=_rows3(poses, dev, torch.float32),
                                   intr=cam.intr.to(torch.float32).contiguous().to(dev), scale=(width, height), index=index, count=n)
    return out, np.ones((T, n), dtype=bool)
