"""Objects in the rooms world, host side (no GPU): the NumPy renderer that states the ray caster's arithmetic contract
(synthetic.render_objects_numpy), the layouts, the kinematics' extra boxes, and the harness's pure host rules."""
import numpy as np
import pytest

from vlfm_amd import synthetic as S
from world_object_cases import A, B, EDGES, poses, render


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------------------------------------------------ NumPy renderer
@pytest.mark.parametrize("H,W", [(480, 640), (50, 70)], ids=["640x480", "70x50"])
def test_without_objects_it_is_the_wall_renderer(H, W):
    for (x, y, k) in poses()[:20]:                                     # every 25th pose of the tour
        d, ids = render((x, y, k), [], H, W)
        want = S.depth_from_profile(S.wall_profile(x, y, k, W), H)
        assert d.dtype == np.float32 and np.array_equal(_bits(d), _bits(want))
        assert ids.dtype == np.uint8 and not ids.any()


def test_pinned_scene():
    """The figures of a restatement of the contract made outside this repository: 640 x 480, default optics, from (0, 0)."""
    d, ids = render((0.0, 0.0, 0), [A, B], 480, 640)
    st = S.object_stats_numpy(ids)
    assert st.dtype == np.int32 and st.shape == (S.WORLD_MAX_OBJECTS, 5)
    assert st[0].tolist() == [13485, 277, 363, 237, 391]
    assert st[1].tolist() == [8880, 199, 255, 190, 346]
    assert all(row.tolist() == [0, 640, -1, 480, -1] for row in st[2:])
    assert np.array_equal(np.unique(d[ids == 1]), np.array([np.float32(np.float64(2.25 - 0.5) / 4.5)]))
    assert np.float32(0.3888889) == d[300, 300]
    d1, ids1 = render((0.0, 0.0, 1), [A, B], 480, 640)
    assert S.object_stats_numpy(ids1)[0].tolist() == [20710, 491, 605, 236, 427]
    # the object pixels are nearer than the walls-only frame, every other pixel is that frame's
    walls = render((0.0, 0.0, 0), [], 480, 640)[0]
    assert (d[ids > 0] < walls[ids > 0]).all() and np.array_equal(_bits(d[ids == 0]), _bits(walls[ids == 0]))


def _scene(name, H=480, W=640):
    pose, boxes = EDGES[name]
    d, ids = render(pose, boxes, H, W)
    return pose, boxes, d, ids, render(pose, [], H, W)[0]


@pytest.mark.parametrize("name", ["behind_wall", "camera_inside", "beyond_range"])
def test_invisible_objects(name):
    """Behind a wall; around the camera (transparent, like a wall box around it); beyond max_depth (normalises to 1.0 like the
    far wall behind it, and a tie goes to the wall)."""
    _, _, d, ids, walls = _scene(name)
    assert not ids.any() and np.array_equal(_bits(d), _bits(walls))


def test_beyond_range_scene_is_what_it_says():
    (x, y, k), boxes = EDGES["beyond_range"]
    assert S.wall_profile(x, y, k)[320] > boxes[0][0] - x > S.MAX_DEPTH      # nothing in front of it on the centre column


def test_pillar_hides_exactly_its_columns():
    (x, y, k), boxes, d, ids, _ = _scene("behind_pillar")
    cols = np.flatnonzero((ids == 1).any(axis=0))
    near = np.flatnonzero(S.wall_profile(x, y, k) < boxes[0][0] - x)           # columns with a wall nearer than the object: the pillar
    lo, hi = cols.min(), cols.max()
    hidden = near[(near > lo) & (near < hi)]
    assert len(hidden) > 50 and hidden.min() > lo + 10 and hidden.max() < hi - 10     # the pillar stands in the middle of it
    assert sorted(set(range(lo, hi + 1)) - set(cols.tolist())) == hidden.tolist()
    # the same rows in every visible column of one distance... and none in a hidden one
    assert not (ids[:, hidden] != 0).any()


def test_low_near_object_shares_the_column_with_the_tall_far_one():
    _, _, d, ids, _ = _scene("low_before_tall")
    col = ids[:, 320]
    far, near = np.flatnonzero(col == 1), np.flatnonzero(col == 2)
    assert len(far) and len(near) and far.max() < near.min()                  # the tall one shows above the low one
    assert np.array_equal(np.flatnonzero(col), np.arange(far.min(), near.max() + 1))   # and nothing between them
    assert d[near[0], 320] < d[far[0], 320]


def test_hanging_object_rows_are_above_the_horizon():
    (x, y, k), boxes, d, ids, _ = _scene("hanging")
    rows = np.flatnonzero(ids[:, 320] == 1)
    fx, t = S.camera_intrinsics(640)[0], boxes[0][0] - x
    assert rows.min() - 240 == int(np.ceil((S.CAMERA_HEIGHT - 1.5) * fx / t)) < 0
    assert rows.max() - 240 == int(np.floor((S.CAMERA_HEIGHT - 1.0) * fx / t)) < 0


def test_identical_objects_the_lower_index_wins():
    _, _, d, ids, _ = _scene("identical")
    st = S.object_stats_numpy(ids)
    assert st[0].tolist() == [13485, 277, 363, 237, 391] and st[1].tolist() == [0, 640, -1, 480, -1]
    assert np.array_equal(_bits(d), _bits(render((0.0, 0.0, 0), [A], 480, 640)[0]))


# ------------------------------------------------------------------------------------------------------------ layout
def test_spots_and_sizes():
    from vlfm_amd.harness import TARGETS

    assert len(S.OBJECT_SPOTS) >= 12 and len(set(S.OBJECT_SPOTS)) == len(S.OBJECT_SPOTS)
    assert all(not S._blocked(x, y, 0.65) for (x, y) in S.OBJECT_SPOTS)
    hall = [p for p in S.OBJECT_SPOTS if max(abs(p[0]), abs(p[1])) < 4.0]
    assert 4 <= len(hall) <= len(S.OBJECT_SPOTS) - 6                           # spread over the hall and the ring
    assert list(S.OBJECT_SIZES) == TARGETS
    for hx, hy, z0, z1 in S.OBJECT_SIZES.values():
        assert 0 < hx <= 0.5 and 0 < hy <= 0.5 and z0 == 0.0 and 0.7 <= z1 <= 1.5


def test_layout_is_deterministic_and_keeps_its_distance():
    from vlfm_amd.harness import TARGETS

    seen = set()
    for env_id in range(14):
        for episode in range(6):
            robot = S.OBJECT_SPOTS[(env_id + 3 * episode) % len(S.OBJECT_SPOTS)]        # the worst case: standing on a spot
            lay = S.object_layout(env_id, episode, robot)
            assert lay == S.object_layout(env_id, episode, np.array(robot))
            (tc, tb), (dc, db) = lay
            assert tc == TARGETS[env_id % len(TARGETS)] and dc != tc and dc in TARGETS
            centres = [((b[0] + b[2]) / 2, (b[1] + b[3]) / 2) for b in (tb, db)]
            spots = [min(S.OBJECT_SPOTS, key=lambda p: np.hypot(p[0] - c[0], p[1] - c[1])) for c in centres]
            assert all(np.hypot(p[0] - c[0], p[1] - c[1]) < 1e-9 for p, c in zip(spots, centres)) and spots[0] != spots[1]
            assert all(np.hypot(c[0] - robot[0], c[1] - robot[1]) > 1.5 for c in centres)
            assert tb == S.object_box(tc, *spots[0])
            seen.add(spots[0])
    assert len(seen) >= 10                                                       # the hash spreads the targets over the spots


# ------------------------------------------------------------------------------------------------------------ kinematics
def test_step_poses_extra_boxes():
    xy, k = np.array([[0.0, 0.0], [0.0, 0.0], [-3.0, -3.0]]), np.array([0, 0, 0])
    fwd = np.full(3, S.ACTION_FORWARD)
    box = np.array([0.44, -0.25, 0.94, 0.25])                  # 0.19 m ahead of where a step forward ends: inside the margin
    extra = np.full((3, 2, 4), np.nan)
    extra[0, 1] = box
    extra[2, 0] = box                                          # far from robot 2
    got_xy, got_k, hit = S.step_poses(xy, k, fwd, extra)
    assert hit.tolist() == [True, False, False]
    assert got_xy[0].tolist() == [0.0, 0.0] and got_xy[1].tolist() == [0.25, 0.0] and got_xy[2].tolist() == [-2.75, -3.0]
    extra[0, 1, 0] = 0.46                                      # 0.21 m: outside the margin
    assert not S.step_poses(xy, k, fwd, extra)[2].any()
    # turns are never refused; None is the function as it was
    assert not S.step_poses(xy, k, np.full(3, S.ACTION_TURN_LEFT), np.tile(box, (3, 1, 1)))[2].any()
    a = np.array([S.ACTION_FORWARD, S.ACTION_TURN_RIGHT, S.ACTION_STOP])
    for x, y in zip(S.step_poses(xy, k, a), S.step_poses(xy, k, a, None)):
        assert np.array_equal(x, y)
    for x, y in zip(S.step_poses(xy, k, a), S.step_poses(xy, k, a, np.full((3, 8, 4), np.nan))):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError):
        S.step_poses(xy, k, a, np.zeros((2, 8, 4)))


# ------------------------------------------------------------------------------------------------------------ harness rules
def test_sightings_from_stats_thresholds():
    from vlfm_amd.harness import sightings_from_stats

    st = np.tile(np.array([0, 640, -1, 480, -1], np.int32), (2, 8, 1))
    st[0, 0] = (199, 10, 40, 100, 120)          # min_pixels - 1: faint
    st[0, 1] = (200, 277, 363, 237, 391)        # min_pixels: confident
    st[1, 0] = (49, 1, 2, 3, 4)                 # min_pixels / 4 - 1: not seen
    st[1, 2] = (50, 5, 5, 0, 49)                # min_pixels / 4: faint
    got = sightings_from_stats(st, [["chair", "tv"], ["bed", "tv", "couch"]], 200, 0.9, 0.35)
    assert got == [(0, "chair", 0.35, (25.5, 110.5, 15.5, 10.5), 0), (0, "tv", 0.9, (320.5, 314.5, 43.5, 77.5), 1),
                   (1, "couch", 0.35, (5.5, 25.0, 0.5, 25.0), 2)]
    # the box is the visible bounding box: its corners are cmin, cmax + 1, rmin, rmax + 1
    cx, cy, ax, ay = got[1][3]
    assert (cx - ax, cx + ax, cy - ay, cy + ay) == (277, 364, 237, 392)


def test_success_is_measured_to_the_footprint_rectangle():
    from vlfm_amd.harness import objectnav_outcome

    box = np.array(A[:4])
    assert S.rect_distance((2.5, 0.0), box) == 0.0 and S.rect_distance((1.25, 0.0), box) == 1.0
    assert S.rect_distance((2.5, 1.0), box) == 0.75 and abs(S.rect_distance((1.95, 0.65), box) - 0.5) < 1e-12
    kw = dict(steps_done=40, max_steps=500, target_box=box, success_distance=1.0)
    assert objectnav_outcome(True, True, False, robot_xy=(1.25, 0.0), **kw) == "success"          # exactly at the distance
    assert objectnav_outcome(True, True, False, robot_xy=(1.24, 0.0), **kw) == "wrong_stop"
    assert objectnav_outcome(True, True, False, robot_xy=(1.5, 0.9), **kw) == "success"           # corner: hypot(0.75, 0.65) < 1
    assert objectnav_outcome(True, True, False, robot_xy=(1.45, 1.0), **kw) == "wrong_stop"       # hypot(0.8, 0.75) > 1
    assert objectnav_outcome(True, False, True, robot_xy=(2.0, 0.0), **kw) == "no_frontier"
    assert objectnav_outcome(False, True, False, robot_xy=(2.0, 0.0), **kw) is None
    kw["steps_done"] = 500
    assert objectnav_outcome(False, False, False, robot_xy=(9.0, 9.0), **kw) == "timeout"
    assert objectnav_outcome(True, True, False, robot_xy=(2.0, 0.0), **kw) == "success"            # a stop on the last step counts
    kw["target_box"] = None
    assert objectnav_outcome(True, True, False, robot_xy=(2.0, 0.0), **kw) == "wrong_stop"


def test_constructor_refuses_before_the_device_is_touched(monkeypatch):
    from vlfm_amd import harness
    from vlfm_amd.harness import BatchedEpisodes, Camera, CameraRig, ScriptedSightings, WorldObjects

    def no_device(_):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(harness, "require_gpu", no_device)
    ok = dict(use_blip2=False, select_frontiers=True)
    with pytest.raises(ValueError, match="closed_loop"):
        BatchedEpisodes(2, world_objects=WorldObjects(), **ok)
    with pytest.raises(ValueError, match="sightings"):
        BatchedEpisodes(2, world_objects=WorldObjects(), closed_loop=True, sightings=ScriptedSightings(), **ok)
    with pytest.raises(ValueError, match="rig"):
        BatchedEpisodes(2, world_objects=WorldObjects(), closed_loop=True, rig=CameraRig([Camera()]), **ok)
    with pytest.raises(AssertionError, match="device was asked"):
        BatchedEpisodes(2, world_objects=WorldObjects(), closed_loop=True, **ok)
    wo = WorldObjects()
    assert (wo.min_pixels, wo.confidence, wo.faint_confidence, wo.success_distance, wo.max_episode_steps) == \
        (200, 0.9, 0.35, 1.0, 500) and wo.layout is S.object_layout
