"""Procedural worlds on the host: the generator (synthetic.ProceduralWorlds) is deterministic and its worlds have the properties
the harness relies on; the host statements with ``boxes=BOXES`` are their defaults; the argument checks need no device."""
import functools

import numpy as np
import pytest

from vlfm_amd import synthetic as S

ENVS, EPISODES = range(48), range(2)


@functools.lru_cache(maxsize=None)
def _world(e, k, seed=0):
    w = S.ProceduralWorlds(seed).world(e, k)
    for a in (w.boxes, w.start_xy, w.spots, w.doors):
        a.setflags(write=False)
    return w


def _bytes(w):
    return w.boxes.tobytes() + w.start_xy.tobytes() + bytes([w.start_k]) + w.spots.tobytes()


def test_deterministic_and_distinct():
    for (e, k) in [(0, 0), (5, 1), (47, 0)]:
        assert _bytes(S.ProceduralWorlds(0).world(e, k)) == _bytes(S.ProceduralWorlds(0).world(e, k))
    a = _world(3, 0)
    for other in (_world(4, 0), _world(3, 1), _world(3, 0, seed=1)):
        assert a.boxes.shape != other.boxes.shape or not np.array_equal(a.boxes, other.boxes)
    # 96 worlds, 96 different floor plans
    assert len({_world(e, k).boxes.tobytes() for e in ENVS for k in EPISODES}) == len(ENVS) * len(EPISODES)
    # every coordinate is a multiple of 0.05 m: an integer number of units divided by 20
    for arr in (a.boxes, a.spots, a.start_xy):
        assert np.array_equal(np.round(arr * 20.0) / 20.0, arr)
    assert a.boxes.dtype == np.float64 and a.boxes.shape[1] == 4 and 0 <= a.start_k < 12


@pytest.mark.parametrize("k", EPISODES)
def test_properties(k):
    classes = list(S.OBJECT_SIZES)
    for e in ENVS:
        w = _world(e, k)
        assert len(w.boxes) <= S.WORLD_MAX_BOXES                                            # 1
        assert min(S.rect_distance(w.start_xy, b) for b in w.boxes) >= 0.5                  # 2
        assert len(w.spots) >= 12                                                           # 3
        rects = S.inflated_rects(boxes=w.boxes)                                             # 4: walls only, STEP_MARGIN
        nodes, dist = S.geodesic_field_numpy(rects, [w.start_xy])
        d = S.geodesic_query_numpy(rects, [w.start_xy], nodes, dist, w.spots)
        assert np.isfinite(d).all(), (e, k)
        assert not S.rects_abut(rects, rects).any(), (e, k)                                 # 5: walls against walls ...
        objs = S.inflated_rects([S.object_box(c, x, y) for (x, y) in w.spots for c in classes], boxes=np.zeros((0, 4)))
        assert len(objs) == len(classes) * len(w.spots)
        assert not S.rects_abut(objs, rects).any(), (e, k)                                  # ... and against every object
        # what the spots promise: 0.65 m to every box, 1.6 m to every doorway centre (exact in the generator's integer units of
        # 0.05 m; the doubles carry the rounding of a few operations on coordinates below 10)
        assert min(S.rect_distance(p, b) for p in w.spots for b in w.boxes) >= 0.65 - 1e-12
        if len(w.doors):
            assert np.hypot(*(w.spots[:, None] - w.doors[None]).transpose(2, 0, 1)).min() >= 1.6 - 1e-12


def test_rects_abut():
    a = [(0.0, 0.0, 1.0, 1.0)]
    assert S.rects_abut(a, [(1.0, 0.5, 2.0, 3.0)]).all() and S.rects_abut(a, [(-1.0, 1.0, 0.5, 2.0)]).all()
    assert not S.rects_abut(a, [(1.0, 1.0, 2.0, 2.0)]).any()          # corner to corner: no shared edge
    assert not S.rects_abut(a, [(0.5, 0.5, 2.0, 2.0)]).any()          # overlapping
    assert not S.rects_abut(a, [(1.0 + 1e-12, 0.0, 2.0, 1.0)]).any()  # a slit of positive width


@pytest.mark.parametrize("k", EPISODES)
def test_reachable_with_objects(k):
    worlds = S.ProceduralWorlds(0)
    classes = list(S.OBJECT_SIZES)
    for e in ENVS:
        w = _world(e, k)
        lay = worlds.layout(e, k, w.start_xy)
        assert lay == worlds.layout(e, k, w.start_xy) and len(lay) == 2
        (tc, tb), (dc, db) = lay
        assert tc == classes[e % 6] and dc != tc
        centres = [((b[0] + b[2]) / 2, (b[1] + b[3]) / 2) for b in (tb, db)]
        spots = {tuple(p) for p in w.spots.tolist()}
        for c in centres:
            assert min(np.hypot(c[0] - s[0], c[1] - s[1]) for s in spots) < 1e-9          # on the world's own spots
            assert np.hypot(c[0] - w.start_xy[0], c[1] - w.start_xy[1]) > S.OBJECT_START_CLEARANCE - 1e-9
        assert np.hypot(centres[0][0] - centres[1][0], centres[0][1] - centres[1][1]) > 1.5 - 1e-9
        rects = S.inflated_rects([tb, db], boxes=w.boxes)
        src = S.goal_viewpoints(tb, rects, 1.0)
        assert len(src) > 0, (e, k)
        nodes, dist = S.geodesic_field_numpy(rects, src)
        assert np.isfinite(S.geodesic_query_numpy(rects, src, nodes, dist, [w.start_xy])[0]), (e, k)


def test_defaults_are_unchanged():
    rng = np.random.Generator(np.random.PCG64(5))
    poses = S.integrate(S.plan_actions(200))[::13]
    for (x, y, k) in poses:
        assert np.array_equal(S.wall_profile(x, y, k, 64, boxes=S.BOXES).view(np.int32), S.wall_profile(x, y, k, 64).view(np.int32))
        for m in (0.2, 0.3, 0.65):
            assert S._blocked(x, y, m, boxes=S.BOXES) == S._blocked(x, y, m)
    objs = [(2.25, -0.25, 2.75, 0.25, 0.0, 0.9), (3.2, 0.6, 3.6, 1.0, 0.0, 1.3)]
    for (x, y, k) in poses[:4]:
        c, s = S.HEADINGS[k]
        args = (x, y, c, s, 0.88, S.camera_intrinsics(40)[0], 0.5, 5.0, 24, 40, objs)
        a, b = S.render_objects_numpy(*args), S.render_objects_numpy(*args, boxes=S.BOXES)
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])
    # a world without boxes: floor only
    assert np.isinf(S.wall_profile(0.0, 0.0, 0, 16, boxes=np.zeros((0, 4)))).all()
    # step_poses: 1000 random lattice poses and actions
    E = 1000
    tour = S.integrate(S.plan_actions(S.ROOMS_STEPS))
    pick = rng.integers(0, len(tour), E)
    xy = np.array([tour[i][:2] for i in pick], np.float64)
    k = rng.integers(0, 12, E)
    acts = rng.integers(0, 4, E)
    extra = np.full((E, 2, 4), np.nan)
    extra[::3, 0] = np.concatenate([xy[::3] + 0.1, xy[::3] + 0.6], axis=1)
    want = S.step_poses(xy, k, acts, extra)
    assert want[2].sum() > 20 and (acts == S.ACTION_FORWARD).sum() - want[2].sum() > 20
    B = len(S.BOXES)
    got = S.step_poses(xy, k, acts, extra, boxes=np.broadcast_to(S.BOXES, (E, B, 4)))
    padded = np.full((E, S.WORLD_MAX_BOXES, 4), np.nan)
    padded[:, :B] = S.BOXES
    for g in (got, S.step_poses(xy, k, acts, extra, boxes=padded)):
        assert g[0].tobytes() == want[0].tobytes() and np.array_equal(g[1], want[1]) and np.array_equal(g[2], want[2])
    # per-robot walls really are per robot: robot 0 in an empty world walks through what refuses robot 1
    two = np.array([xy[np.flatnonzero(want[2])[0]]] * 2)
    kk = np.array([k[np.flatnonzero(want[2])[0]]] * 2)
    walls = np.stack([np.full((B, 4), np.nan), S.BOXES])
    assert S.step_poses(two, kk, [S.ACTION_FORWARD] * 2, boxes=walls)[2].tolist() == [False, True]
    with pytest.raises(ValueError):
        S.step_poses(xy, k, acts, boxes=S.BOXES)


def test_argument_checks():
    from vlfm_amd.harness import BatchedEpisodes, CameraRig, Camera, ScriptedSightings, WorldTable

    worlds = S.ProceduralWorlds(3)
    # refused before the device is touched: none of these needs a GPU
    with pytest.raises(ValueError, match="closed_loop"):
        BatchedEpisodes(2, use_blip2=False, select_frontiers=True, worlds=worlds)
    with pytest.raises(ValueError, match="rig"):
        BatchedEpisodes(2, use_blip2=False, select_frontiers=True, closed_loop=True, worlds=worlds, rig=CameraRig([Camera()]))
    with pytest.raises(ValueError, match="sightings"):
        BatchedEpisodes(2, use_blip2=False, select_frontiers=True, closed_loop=True, worlds=worlds, sightings=ScriptedSightings())
    table = WorldTable(3, "cpu", max_boxes=5)
    assert table.boxes.shape == (3, 5, 4) and np.isnan(table.boxes).all() and table.counts.tolist() == [0, 0, 0]
    table.assign([2, 0], [S.BOXES[:5], S.BOXES[5:7]])
    assert table.counts.tolist() == [2, 0, 5] and np.array_equal(table.world(2), S.BOXES[:5])
    assert np.array_equal(table.boxes[0, :2], S.BOXES[5:7]) and np.isnan(table.boxes[0, 2:]).all() and np.isnan(table.boxes[1]).all()
    assert np.array_equal(table.d_boxes.numpy(), table.boxes, equal_nan=True) and table.d_counts.tolist() == [2, 0, 5]
    with pytest.raises(ValueError, match="boxes"):
        table.assign([1], [S.BOXES[:6]])
    for rows, boxes in (([3], [S.BOXES[:1]]), ([0, 0], [S.BOXES[:1]] * 2), ([0], []), ([1], [[[0.0, 0.0, np.nan, 1.0]]])):
        with pytest.raises(ValueError):
            table.assign(rows, boxes)
    assert table.counts.tolist() == [2, 0, 5]           # a refused assignment changes nothing
