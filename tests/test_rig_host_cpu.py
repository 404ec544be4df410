"""Host side of the camera-rig calls, on NumPy inputs without a device: grouping by slot with the order within a slot kept,
slot tables, optics records, union of dirty windows, refusals -- and the condition the GPU order test relies on (the oracle
itself gives another map when a slot's cameras are applied in reverse)."""
import ctypes

import numpy as np
import pytest

from vlfm_amd.synthetic import camera_intrinsics, pose_to_tf


def test_group_rig_keeps_the_order_within_a_slot_under_any_interleaving():
    from vlfm_amd.mapping.value_map import group_rig

    rng = np.random.default_rng(0)
    for _ in range(200):
        n_envs = int(rng.integers(1, 20))
        env = rng.integers(0, n_envs, size=int(rng.integers(1, 60)))
        order, slots = group_rig(env, n_envs)
        assert sorted(order.tolist()) == list(range(len(env)))
        assert slots.dtype == np.int32 and slots.shape == (len(np.unique(env)), 2)
        assert int(slots[:, 1].sum()) == len(env) and (slots[:, 1] > 0).all()
        assert np.array_equal(slots[:, 0], np.concatenate([[0], np.cumsum(slots[:, 1])[:-1]]))
        for first, count in slots:
            members = order[first:first + count]
            assert len(set(env[members].tolist())) == 1                    # one slot per table row
            assert np.array_equal(members, np.sort(members))                # ... in the order the caller listed them
            assert np.array_equal(members, np.nonzero(env == env[members[0]])[0])
    order, slots = group_rig([3, 1, 3, 1, 0], 4)
    assert order.tolist() == [4, 1, 3, 0, 2] and slots.tolist() == [[0, 1], [1, 2], [3, 2]]


def test_group_rig_refuses_slots_out_of_range():
    from vlfm_amd.mapping.value_map import group_rig

    for bad in ([0, 4], [-1, 0]):
        with pytest.raises(AssertionError, match="out of range"):
            group_rig(bad, 4)


def test_optics_records_and_struct_layout():
    from vlfm_amd import _lib
    from vlfm_amd.mapping.value_map import VM_OPTICS_DTYPE, per_observation, rig_optics

    assert VM_OPTICS_DTYPE.itemsize == ctypes.sizeof(_lib.VmOptics) == 48
    for name, _ in _lib.VmOptics._fields_:
        assert VM_OPTICS_DTYPE.fields[name][1] == getattr(_lib.VmOptics, name).offset, name
    asked = []

    def lookup(fov, max_depth):
        asked.append((fov, max_depth))
        T = 2 * int(max_depth * 20) + 1
        return 1000 + T, 2000 + T, 3000 + T, 4000 + int(fov * 100), T

    op = rig_optics(0.5, [5.0, 2.5, 5.0, 5.0], [1.2, 1.0, 1.2, 1.0], 4, lookup)
    assert sorted(asked) == [(1.0, 2.5), (1.0, 5.0), (1.2, 5.0)]             # one lookup per camera model
    assert op["template_size"].tolist() == [201, 101, 201, 201]
    assert op["d_template_bits"].tolist() == [2201, 2101, 2201, 2201] and op["d_tan"].tolist() == [4120, 4100, 4120, 4100]
    assert op["depth_scale"].tolist() == [4.5, 2.0, 4.5, 4.5] and (op["depth_offset"] == np.float32(0.5)).all()
    # f32(max - min) with the difference taken in f64, as the single-camera entry point computes it
    op = rig_optics(0.1, 0.3, 1.0, 1, lookup)
    assert op["depth_scale"][0] == np.float32(0.3 - 0.1)
    assert per_observation(2.0, 3).tolist() == [2.0, 2.0, 2.0]
    with pytest.raises(AssertionError):
        per_observation([1.0, 2.0], 3)


def test_mixed_image_shapes_are_refused():
    from vlfm_amd.mapping.value_map import stack_rig_frames

    a, b = np.zeros((480, 640), np.float32), np.zeros((480, 320), np.float32)
    assert stack_rig_frames([a, a]).shape == (2, 480, 640)
    with pytest.raises(ValueError, match="share the image shape"):
        stack_rig_frames([a, b])


def test_rig_dirty_windows_are_the_union_over_a_slots_cameras():
    from vlfm_amd.mapping.obstacle_map import ObstacleMapBatch

    S, ppm = 1000, 20
    tf = np.stack([pose_to_tf(1.0, 2.0, 0.3), pose_to_tf(-3.0, 0.5, 1.0), pose_to_tf(1.5, 2.5, -2.0), pose_to_tf(24.0, 0.0, 0.0)])
    env = np.array([2, 0, 2, 1])
    reach = np.array([100.2, 60.0, 50.0, 80.0])
    slots, win = ObstacleMapBatch.rig_windows(env, tf, reach, S, ppm)
    assert slots.tolist() == [0, 1, 2]
    # one camera: its own window (cell +- (ceil(reach) + 2)); (x -> row, y -> S - col)
    assert win[0].tolist() == [440 - 62, 440 + 62, 490 - 62, 490 + 62]
    assert win[1].tolist() == [0, S - 1, 0, S - 1]                        # leaves the map: the whole map
    r0, r2 = 103, 52
    rows = [520 - r0, 520 + r0, 530 - r2, 530 + r2]
    cols = [S - 540 - r0, S - 540 + r0, S - 550 - r2, S - 550 + r2]
    assert win[2].tolist() == [min(rows), max(rows), min(cols), max(cols)]


def test_camera_rig_pose_composition():
    from vlfm_amd.harness import Camera, CameraRig

    _, _, hfov = camera_intrinsics(640)
    rig = CameraRig([Camera(yaw=0.0), Camera(yaw=0.61, forward=0.2, left=-0.1, up=0.3, max_depth=2.5, value=False),
                     Camera(yaw=-0.61, hfov=1.0, obstacle=False)])
    assert rig.obstacle_ids == [0, 1] and rig.value_ids == [0, 2] and len(rig) == 3
    x, y, yaw = 1.5, -2.0, 0.8
    robot = pose_to_tf(x, y, yaw)
    tfs = rig.camera_tfs(robot)
    assert tfs.shape == (3, 4, 4)
    assert np.array_equal(tfs[0], robot)
    c, s = np.cos(yaw), np.sin(yaw)
    want = pose_to_tf(x + 0.2 * c - (-0.1) * s, y + 0.2 * s + (-0.1) * c, yaw + 0.61, z=robot[2, 3] + 0.3)
    assert np.allclose(tfs[1], want, atol=1e-12) and np.array_equal(tfs[1][3], [0, 0, 0, 1])
    assert np.allclose(np.arctan2(tfs[2][1, 0], tfs[2][0, 0]), yaw - 0.61)
    batch = rig.camera_tfs(np.stack([robot, pose_to_tf(0, 0, 0)]))
    assert batch.shape == (2, 3, 4, 4) and np.array_equal(batch[0], tfs)
    with pytest.raises(ValueError):
        CameraRig([Camera(obstacle=False, value=False)])
    with pytest.raises(ValueError):
        CameraRig([Camera(value=False)])     # nothing feeds the value map


def test_the_order_generator_makes_order_matter_on_the_oracle():
    """The condition tests/test_rig_gpu.py::test_order_within_a_slot_is_honoured stands on, checked without a device: in weighted
    mode every generated case gives another map when the cameras of a step are applied in reverse."""
    import test_rig_gpu as t

    for case, steps in t.order_cases():
        fwd, rev = t.oracle_forward_and_reversed(steps)
        differ = int((np.asarray(fwd._value_map) != np.asarray(rev._value_map)).sum())
        assert differ > 100, (case, differ)
