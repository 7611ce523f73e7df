"""CPU: the host half of flexam_amd.motion -- pose tables and object-motion matrices -- against what the reference's
CameraMotionGenerator / ObjectMotionGenerator compute on the CPU (tests/golden/g15_motion_host.safetensors, written by
tools/make_golden_motion.py), bit for bit: the module makes them with the reference's own torch / numpy calls in its dtypes.  Also the
refusals and the reference behaviours that are kept on purpose."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

T, MH, MW = 9, 32, 48
CAMERA_MOTIONS = ("trans 0.1 -0.2 0.5", "rot y 25", "rot x -10 2 6", "rot z 7 6 2", "spiral 1.5", "spiral 2 1 7",
                  "trans 0 0 0.5 0 4; rot x 25 0 4; trans 0.1 0 0 4 8", "rot y 12; spiral 1 0 8; trans -0.3 0.1 0.2 3 5")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def cam(motion="rot y 5", **kw):
    from flexam_amd import CameraMotionGenerator
    return CameraMotionGenerator(motion, frame_num=T, H=MH, W=MW, **kw)


@pytest.mark.parametrize("i", range(len(CAMERA_MOTIONS)))
def test_get_default_motion_equals_the_reference_bit_for_bit(golden, i):
    got = cam(CAMERA_MOTIONS[i]).get_default_motion()
    assert got.dtype == torch.float32                              # float32 even when a spiral contributes float64 poses
    assert same_bits(got, golden("g15_motion_host")[f"camera.{i}"])


def test_pose_builders_equal_the_reference_bit_for_bit(golden):
    g = golden("g15_motion_host")
    c = cam()
    assert same_bits(c.intr, g["intr_default"])
    assert same_bits(c.rot_poses(33.0, "x"), g["rot_x"]) and same_bits(c.rot_poses(-12.5, "y"), g["rot_y"]) and same_bits(c.rot_poses(190.0, "z"), g["rot_z"])
    assert same_bits(c.trans_poses(1.0, -2.0, 0.3), g["trans"])
    assert same_bits(c.spiral_poses(2.0), g["spiral"]) and g["spiral"].dtype == torch.float64
    ext = g["cameras_ext"].numpy().tolist()
    assert same_bits(c.convert_cameras_to_poses([None] * 12, ext), g["cameras_long"])
    assert same_bits(c.convert_cameras_to_poses([None] * 4, ext[:4]), g["cameras_short"])


def test_object_motion_matrices_of_all_33_names_equal_the_reference_bit_for_bit(golden):
    from flexam_amd.motion import OBJECT_MOTIONS, object_motion_matrices
    g = golden("g15_motion_host")
    names = list(OBJECT_MOTIONS)
    assert len(names) == 33 and g["object_matrices"].shape == (33, T, 4, 4)
    for k, name in enumerate(names):                                # the fixture is in the table's order
        assert same_bits(object_motion_matrices(g["object_center"], name, 50, T), g["object_matrices"][k]), name


def test_refusals_and_kept_error_behaviours():
    from flexam_amd import ObjectMotionGenerator
    from flexam_amd.motion import object_motion_matrices
    with pytest.raises(NotImplementedError, match="792"):
        cam("path").get_default_motion()
    with pytest.raises(NotImplementedError, match="260"):
        cam().process_video_file("clip.mp4")
    with pytest.raises(NotImplementedError, match="219"):
        cam().process_pose_file("poses.txt")
    import flexam_amd
    assert not hasattr(flexam_amd, "FirstFrameRepainter")
    for motion in ("rot y 10 4 4", "trans 1 0 0 3 3", "spiral 1 8 8"):          # start_frame == end_frame
        with pytest.raises(ZeroDivisionError):
            cam(motion).get_default_motion()
    for motion, msg in (("zoom 3", "must be in"), ("rot w 10", "Invalid rotation axis"), ("trans 1 2", "trans motion requires"),
                        ("rot y", "rot motion requires"), ("spiral", "spiral motion requires")):
        with pytest.raises(ValueError, match=msg):
            cam(motion).get_default_motion()
    with pytest.raises(ValueError, match="must be a string"):
        cam(None).get_default_motion()
    with pytest.raises(ValueError, match="unknown motion type"):
        object_motion_matrices(torch.zeros(3), "sideways", 50, T)
    with pytest.raises(ValueError, match="unknown motion type"):
        ObjectMotionGenerator(device="cpu").apply_motion(torch.zeros(T, 4, 3), torch.zeros(4, 4, dtype=torch.bool), "sideways", 50, num_frames=T)
    # frames before a segment keep the identity, frames after it its last matrix; swapped bounds are reordered
    m = cam("trans 0 0 1 6 2").get_default_motion()
    assert torch.equal(m[0], torch.eye(4)) and torch.equal(m[1], torch.eye(4)) and torch.equal(m[6], m[8]) and m[6, 2, 3] == 1.0


def test_no_selected_point_gives_a_nan_centre_like_the_mean_of_nothing():
    from flexam_amd.motion import _center
    c = _center(torch.zeros(4, dtype=torch.float64))
    assert c.dtype == torch.float32 and bool(torch.isnan(c).all())
    c = _center(torch.tensor([3.0, -6.0, 1.5, 3.0], dtype=torch.float64))
    assert torch.equal(c, torch.tensor([1.0, -2.0, 0.5]))


def test_tracks_have_no_cpu_path():
    from flexam_amd import ObjectMotionGenerator, convert_moge_to_delta_format
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises((RuntimeError, AssertionError)):
        ObjectMotionGenerator(device="cpu").apply_motion(torch.zeros(T, 4, 3), torch.ones(4, 4, dtype=torch.bool), "left", 50, num_frames=T)
    with pytest.raises((RuntimeError, AssertionError)):
        convert_moge_to_delta_format(np.zeros((T, 4, 4, 3), np.float32), np.ones((4, 4), bool), 4, 4, device="cpu")
    with pytest.raises((RuntimeError, AssertionError)):
        cam(device="cpu").w2s_moge(torch.zeros(T, 4, 3), torch.eye(4).repeat(T, 1, 1))


def test_restatement_bounds_hold_for_the_reference_float32_results(golden):
    """The bound the GPU tests use is honest: the reference's own float32 outputs (any BLAS order) satisfy it too."""
    import motion_restatement as MR
    g = golden("g15_motion_delta")
    tracks, flags = g["tracks"], g["flags"]
    c_star = MR.exact_center(tracks[0], flags)
    n = int(flags.sum())
    assert float((g["center"].double() - c_star).abs().max()) <= (n - 1) * MR.U32 * float(tracks[0, flags].double().abs().mean(0).max())
    for name in ("left", "rot", "pitch_up", "up_left_front"):
        A, col_err = MR.exact_object_motion(MR.motion_about_origin(name, 50, T), c_star, g["center"])
        val, bound = MR.affine32(A, tracks.double(), torch.zeros_like(tracks, dtype=torch.float64), col_err, flags)
        ok, worst = MR.close32(g[f"moved.{name}"], val, bound)
        assert ok, (name, worst)
