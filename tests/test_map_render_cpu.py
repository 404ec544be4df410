"""The map renderer's yardsticks on the CPU: the inferno table embedded in csrc/map_render.hip, the test-side cv2 stand-ins,
and the NumPy renderer (tests/map_render_ref.py) against the REFERENCE'S OWN ValueMap.visualize / ObstacleMap.visualize
(imported through oracle/ref_shim.py with the stand-ins planted; replayed from tests/golden/ref_map_render_*.json.gz where
the reference tree is absent) on seeded random map states."""
import types

import numpy as np
import pytest

import map_render_ref as R
from golden_util import ReferenceRecord, same
from oracle import cv as ocv


def test_inferno_lut_in_the_kernel_source_is_opencv_table():
    pytest.importorskip("matplotlib")
    want = R.matplotlib_lut()
    assert np.array_equal(R.hip_lut(), want)
    assert np.array_equal(R.lut(), want)
    assert R.hip_lut()[0].tolist() == [4, 0, 0] and R.hip_lut()[255].tolist() == [164, 255, 252]


def test_line_standin_is_the_facade_polyline_and_the_shifted_thick_line():
    rng = np.random.default_rng(5)
    for _ in range(200):
        S = int(rng.integers(5, 60))
        p0, p1 = rng.integers(-20, S + 20, 2), rng.integers(-20, S + 20, 2)
        t = int(rng.integers(2, 6))
        a = R.line(np.zeros((S, S), np.uint8), tuple(p0), tuple(p1), 7, t)
        b = ocv.polylines(np.zeros((S, S), np.uint8), np.array([[p0, p1]], np.int32), False, 7, t)
        assert np.array_equal(a, b)
        c = np.zeros((S, S), np.uint8)     # the Python ThickLine on 16.16 points (the circle outline's path) agrees
        R._thick_line16(c, (int(p0[0]) << 16, int(p0[1]) << 16), (int(p1[0]) << 16, int(p1[1]) << 16), t, 3)
        assert np.array_equal(c * 7, b), (S, p0, p1, t)


@pytest.mark.parametrize("thickness", [2, 3, 1, 0, -1])
def test_circle_outlines_are_symmetric_and_clip_without_wrapping(thickness):
    """(Thick outlines go through Line2, which clips its end points before stepping: near the border they are not the
    crop of the unclipped circle, but nothing wraps to the far side.)"""
    for r in (0, 1, 2, 5, 9, 17, 30):
        m = R.circle_mask((101, 101), (50, 50), r, thickness)
        assert m.sum() > 0
        if thickness <= 1:
            assert np.array_equal(m, m[::-1]) and np.array_equal(m, m[:, ::-1]) and np.array_equal(m, m.T)
        else:
            ys, xs = np.nonzero(m)
            assert abs(ys.mean() - 50) <= 0.5 and abs(xs.mean() - 50) <= 0.5
            assert ys.max() - 50 <= r + thickness and 50 - ys.min() <= r + thickness
        for cx, cy in ((2, 50), (98, 3), (-3, 40), (50, 104), (0, 0)):
            small = R.circle_mask((101, 101), (cx, cy), r, thickness)
            ys, xs = np.nonzero(small)
            reach = r + max(thickness, 1)
            assert (np.abs(ys - cy) <= reach).all() and (np.abs(xs - cx) <= reach).all(), (r, cx, cy)
            if thickness <= 1:   # per-point clipping: exactly the crop of the unclipped circle
                big = R.circle_mask((301, 301), (cx + 100, cy + 100), r, thickness)[100:201, 100:201]
                assert np.array_equal(small, big), (r, cx, cy)


def _reference(rec):
    from oracle import ref_shim

    vm, om, _, _ = ref_shim.reference_modules()
    import cv2

    if getattr(cv2, "__vlfm_standin__", False):   # VLFM_REAL_CV2=1: the real OpenCV draws the reference's images
        R.plant(cv2)
    return vm, om


@pytest.mark.parametrize("seed", range(16))
def test_numpy_renderer_equals_reference_value_map_visualize(seed):
    st = R.random_value_state(seed)
    rec = ReferenceRecord(f"map_render_value_{seed}")
    S = st["size"]

    def theirs():
        vm, _ = _reference(rec)
        m = vm.ValueMap(st["channels"], size=S, use_max_confidence=st["value"].dtype == np.float32)
        m._value_map = st["value"].copy()
        for p in st["positions"]:
            m.update_agent_traj(p, st["yaw"])
        om = None if st["explored"] is None else types.SimpleNamespace(explored_area=st["explored"].astype(np.uint8))
        return m.visualize(st["markers"], reduce_fn=st["reduce_fn"], obstacle_map=om)

    want = rec(theirs)
    got = R.render_value(st["reduce_fn"](st["value"]), st["explored"], st["positions"], st["yaw"],
                         R.pixel_markers(st["markers"], S))
    assert got.dtype == np.uint8 and got.shape == (S, S, 3)
    assert same(want, got), seed
    rec.close()


@pytest.mark.parametrize("seed", range(8))
def test_numpy_renderer_equals_reference_obstacle_map_visualize(seed):
    st = R.random_obstacle_state(seed)
    rec = ReferenceRecord(f"map_render_obstacle_{seed}")
    S = st["size"]

    def theirs():
        _, om = _reference(rec)
        m = om.ObstacleMap(min_height=0.61, max_height=0.88, agent_radius=0.18, size=S)
        m._map = st["obstacle"].copy()
        m._navigable_map = st["navigable"].astype(np.uint8)
        m.explored_area = st["explored"].astype(np.uint8)
        m._frontiers_px = st["frontiers"].copy()
        for p in st["positions"]:
            m.update_agent_traj(p, st["yaw"])
        return m.visualize()

    want = rec(theirs)
    got = R.render_obstacle(st["obstacle"], st["navigable"], st["explored"], st["frontiers"], st["positions"], st["yaw"])
    assert same(want, got), seed
    rec.close()


def test_incremental_reference_trajectory_equals_drawing_once():
    """The reference's cached path mask (traj_visualizer.py:41-58) is the union of its segments: visualize() called every
    step and once at the end give the same image -- what lets the device plane grow by the new segments only."""
    st = R.random_value_state(9)
    rec = ReferenceRecord("map_render_incremental")

    def theirs():
        vm, _ = _reference(rec)
        a = vm.ValueMap(1, size=st["size"])
        b = vm.ValueMap(1, size=st["size"])
        a._value_map = b._value_map = st["value"][..., :1].astype(np.float32)
        for p in st["positions"]:
            a.update_agent_traj(p, st["yaw"])
            b.update_agent_traj(p, st["yaw"])
            a.visualize()
        return a.visualize(), b.visualize()

    x, y = rec(theirs)
    if isinstance(x, np.ndarray):
        assert np.array_equal(x, y)
    else:
        assert x.digest == y.digest
    rec.close()


@pytest.mark.parametrize("use_max_confidence", [False, True])
def test_reference_session_images_recorded_and_equal_to_the_numpy_renderer(use_max_confidence):
    """The reference's own ValueMap / ObstacleMap through update_map, update_agent_traj, visualize() every step and a
    reset() between two episodes: their images are recorded (tests/test_map_render_gpu.py replays them against the device
    drop-ins) and equal the NumPy renderer fed the reference's own snapshots."""
    rec = ReferenceRecord(f"map_render_session_{int(use_max_confidence)}")
    if not rec.live:
        for _ in range(sum(R.SESSION_STEPS)):   # replay: the recorded images are there for the GPU test
            rec(lambda: None)
        rec.close()
        return
    vm_mod, om_mod = _reference(rec)
    vm, om = vm_mod.ValueMap(1, use_max_confidence=use_max_confidence), om_mod.ObstacleMap(**R.SESSION_KW)

    def step(k):
        mk = R.frontier_markers(om.frontiers)
        v, o = rec(lambda: (vm.visualize(mk, obstacle_map=om), om.visualize()))
        want_v = R.render_value(np.max(vm._value_map, axis=-1), om.explored_area, vm._camera_positions,
                                vm._last_camera_yaw, R.pixel_markers(mk, vm.size))
        want_o = R.render_obstacle(om._map, om._navigable_map, om.explored_area, om._frontiers_px, om._camera_positions,
                                   om._last_camera_yaw)
        assert np.array_equal(v, want_v) and np.array_equal(o, want_o), k

    R.run_session(vm, om, step)
    rec.close()
