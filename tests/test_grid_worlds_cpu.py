"""Grid worlds on the host (vlfm_amd/synthetic.py): a GridPlan IS the box world of its occupied cells.  The grid walk
(grid_profile_numpy), the near-cell move test (step_poses(grids=...)) and the constructors are held against the box statements
run on grid_boxes(plan); every comparison is == on the bits."""
import functools

import numpy as np
import pytest

from vlfm_amd import synthetic as S

W = 70
FX = S.camera_intrinsics(W)[0]


def _brute(x, y, c, s, plan, fx=FX, width=W):
    """f64 [W]: the slab test of wall_profile over the cell boxes, BEFORE the rounding to f32."""
    b = S.grid_boxes(plan)
    m = -(np.arange(width, dtype=np.float64) - width // 2) / fx
    dx, dy = (c - s * m)[:, None], (s + c * m)[:, None]
    dx = np.where(np.abs(dx) < 1e-12, 1e-12, dx)
    dy = np.where(np.abs(dy) < 1e-12, 1e-12, dy)
    tx0, tx1 = (b[None, :, 0] - x) / dx, (b[None, :, 2] - x) / dx
    ty0, ty1 = (b[None, :, 1] - y) / dy, (b[None, :, 3] - y) / dy
    tmin = np.maximum(np.minimum(tx0, tx1), np.minimum(ty0, ty1))
    tmax = np.minimum(np.maximum(tx0, tx1), np.maximum(ty0, ty1))
    hit = (tmax >= np.maximum(tmin, 0.0)) & (tmin > 0.0)
    return np.where(hit, tmin, np.inf).min(axis=1, initial=np.inf)


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _edges(kind, n, first):
    i = np.arange(n + 1, dtype=np.float64)
    return first + 0.05 * i if kind == "sum" else (i + round(first * 20)) / 20.0


@functools.lru_cache(maxsize=None)
def _random_plan(density, kind, seed=5):
    rng = np.random.default_rng(seed)
    occ = rng.random((40, 48)) < density
    occ[20, 24] = True                                  # the cell [0, 0.05] x [0, 0.05]: a camera stands inside it below
    return S.GridPlan(occ, _edges(kind, 48, -1.2), _edges(kind, 40, -1.0))


def _poses(rng):
    lattice = [(0.25 * a, 0.25 * b) for a in range(-5, 6) for b in range(-4, 5)][::7]         # on cell edges and corners
    return lattice + [(3.0, 0.5), (-2.0, -3.0), (0.02, 0.03)] + [tuple(p) for p in rng.uniform(-1.3, 1.3, size=(6, 2))]


@pytest.mark.parametrize("kind", ["sum", "div"])
@pytest.mark.parametrize("density", [0.03, 0.15])
def test_the_walk_is_the_brute_force(density, kind):
    plan = _random_plan(density, kind)
    assert plan.nx == 48 and plan.ny == 40 and plan.occ.any()
    rng = np.random.default_rng(17)
    finite = steps = 0
    for (x, y) in _poses(rng):
        for (c, s) in S.HEADINGS:
            got, n = S.grid_profile_numpy(x, y, c, s, FX, W, plan, return_steps=True)
            want = _brute(x, y, c, s, plan)
            assert _same(got, want), (x, y, c, s, np.flatnonzero(got != want)[:5])
            assert n.max() <= plan.nx + plan.ny + 2
            finite += int(np.isfinite(want).sum())
            steps += int(n.sum())
    assert finite > 1000 and steps > finite


def test_the_inside_camera_sees_through_its_cell_and_the_outside_one_sees_the_grid():
    plan = _random_plan(0.15, "div")
    assert S.grid_blocked(plan, 0.02, 0.03, 0.0)
    inside = S.grid_profile_numpy(0.02, 0.03, 1.0, 0.0, FX, W, plan)
    assert (inside > 0.03).all() and np.isfinite(inside).any()
    assert np.isfinite(S.grid_profile_numpy(3.0, 0.5, -1.0, 0.0, FX, W, plan)).any()          # from outside, looking at it
    assert np.isinf(S.grid_profile_numpy(3.0, 0.5, 1.0, 0.0, FX, W, plan)).all()              # looking away


@pytest.mark.parametrize("name", ["1x1", "1x7", "7x1", "empty", "full"])
def test_degenerate_grids(name):
    occ = {"1x1": np.ones((1, 1), bool), "1x7": np.array([[1, 0, 0, 1, 0, 1, 1]], bool), "7x1": np.array([[1, 0, 1, 1, 0, 0, 1]], bool).T,
           "empty": np.zeros((6, 5), bool), "full": np.ones((6, 5), bool)}[name]
    plan = S.GridPlan.uniform(occ, 4, -1, -1)
    for (x, y) in [(0.0, 0.0), (-0.25, -0.25), (-0.125, -0.1), (0.3, 0.3), (-2.0, 0.1), (0.1, 2.5), (5.0, 5.0)]:
        for (c, s) in S.HEADINGS:
            assert _same(S.grid_profile_numpy(x, y, c, s, FX, W, plan), _brute(x, y, c, s, plan)), (name, x, y, c, s)
    if name == "empty":
        assert len(S.grid_boxes(plan)) == 0 and np.isinf(S.grid_profile_numpy(0.0, 0.0, 1.0, 0.0, FX, W, plan)).all()


@pytest.mark.parametrize("env", [0, 1, 2, 3])
def test_a_rasterised_procedural_world_is_its_box_world(env):
    world = S.ProceduralWorlds(0).world(env, 0)
    plan = S.GridPlan.from_boxes(world.boxes)
    assert (plan.nx, plan.ny) == (400, 400) and plan.xs[0] == -10.0 and plan.xs[-1] == 10.0
    Wd, H = 64, 12
    fx = S.camera_intrinsics(Wd)[0]
    none = np.zeros((0, 4))
    views = [(world.start_xy, world.start_k)] + [(world.spots[n], (3 * n + env) % 12) for n in range(5)]
    for (x, y), k in views:
        c, s = S.HEADINGS[k]
        assert np.array_equal(S.wall_profile(x, y, k, Wd, boxes=none, grid=plan).view(np.int32),
                              S.wall_profile(x, y, k, Wd, boxes=world.boxes).view(np.int32))
        assert _same(S.grid_profile_numpy(x, y, c, s, fx, Wd, plan), _brute(x, y, c, s, plan, fx, Wd))
        box6 = [S.object_box("chair", x + 1.0 * c, y + 1.0 * s)]
        a = S.render_objects_numpy(x, y, c, s, S.CAMERA_HEIGHT, fx, S.MIN_DEPTH, S.MAX_DEPTH, H, Wd, box6, boxes=none, grid=plan)
        b = S.render_objects_numpy(x, y, c, s, S.CAMERA_HEIGHT, fx, S.MIN_DEPTH, S.MAX_DEPTH, H, Wd, box6, boxes=world.boxes)
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])


def test_boxes_and_a_grid_take_the_f64_minimum():
    plan = _random_plan(0.03, "div")
    boxes = np.array([(0.5, -0.4, 0.7, 0.6), (-1.0, 0.8, 0.4, 0.9)])
    both = np.concatenate([boxes, S.grid_boxes(plan)])
    for k in range(12):
        assert np.array_equal(S.wall_profile(0.1, 0.1, k, W, boxes=boxes, grid=plan).view(np.int32),
                              S.wall_profile(0.1, 0.1, k, W, boxes=both).view(np.int32))
    assert S._blocked(0.45, 0.0, 0.1, boxes=boxes, grid=plan) and S._blocked(0.02, 0.03, 0.0, boxes=np.zeros((0, 4)), grid=plan)


def test_step_poses_on_grids_is_step_poses_on_the_cell_boxes():
    rng = np.random.default_rng(3)
    plans = [_random_plan(0.03, "div"), _random_plan(0.15, "sum"), None]
    cells = [np.zeros((0, 4)) if p is None else S.grid_boxes(p) for p in plans]
    n = 1000
    xy = 0.25 * rng.integers(-6, 7, size=(n, 2)).astype(np.float64)
    xy[::5] += rng.uniform(-0.2, 0.2, size=(len(xy[::5]), 2))
    k = rng.integers(0, 12, size=n)
    acts = rng.integers(0, 4, size=n)
    which = rng.integers(0, 3, size=n)
    pad = max(len(b) for b in cells)
    boxes = np.full((n, pad, 4), np.nan)
    for e in range(n):
        boxes[e, :len(cells[which[e]])] = cells[which[e]]
    empty = np.full((n, 1, 4), np.nan)
    got = S.step_poses(xy, k, acts, boxes=empty, grids=[plans[w] for w in which])
    want = S.step_poses(xy, k, acts, boxes=boxes)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert 50 < want[2].sum() < (acts == S.ACTION_FORWARD).sum()
    with pytest.raises(ValueError):
        S.step_poses(xy, k, acts, grids=[None])
    # the margin's closed comparisons, on the edge itself: a cell [0.5, 0.75]^2, a robot that lands exactly STEP_MARGIN away
    one = S.GridPlan.uniform(np.ones((1, 1), bool), 4, 2, 2)
    for x in (0.5 - S.STEP_MARGIN, np.nextafter(0.5 - S.STEP_MARGIN, -1.0)):
        assert S.grid_blocked(one, x, 0.6) == S._blocked(x, 0.6, S.STEP_MARGIN, boxes=S.grid_boxes(one))
    assert S.grid_blocked(one, 0.5 - S.STEP_MARGIN, 0.6) and not S.grid_blocked(one, np.nextafter(0.5 - S.STEP_MARGIN, -1.0), 0.6)


def test_from_image_orientation_and_threshold():
    img = np.array([[0, 255, 255, 255, 127],
                    [255, 255, 128, 255, 255],
                    [255, 10, 255, 255, 255]], np.uint8)
    plan = S.GridPlan.from_image(img, 2, -1, 3)
    assert plan.occ.shape == (3, 5) and np.array_equal(plan.xs, [-0.5, 0.0, 0.5, 1.0, 1.5, 2.0]) and np.array_equal(plan.ys, [1.5, 2.0, 2.5, 3.0])
    assert np.array_equal(np.argwhere(plan.occ), [[0, 1], [2, 0], [2, 4]])        # row 0 of the image is the highest y; 128 is free
    assert S.GridPlan.from_image(img, 2, -1, 3, occupied_below=129).occ[1, 2]
    assert np.array_equal(S.grid_boxes(plan), [(0.0, 1.5, 0.5, 2.0), (-0.5, 2.5, 0.0, 3.0), (1.5, 2.5, 2.0, 3.0)])
    assert np.array_equal(plan.packed_rows(), [[2], [0], [17]]) and plan.packed_rows(2).shape == (3, 2)
    wide = S.GridPlan.uniform(np.arange(70)[None, :] % 3 == 0, 20, 0, 0)
    assert wide.packed_rows().shape == (1, 3) and wide.packed_rows()[0, 1] == sum(1 << (i - 32) for i in range(32, 64) if i % 3 == 0)


def test_from_image_opens_a_file(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    img = np.array([[0, 255, 255, 255, 127], [255, 255, 128, 255, 255], [255, 10, 255, 255, 255]], np.uint8)
    path = tmp_path / "plan.png"
    Image.fromarray(np.stack([img] * 3, axis=-1)).save(path)                  # an RGB file: taken as greyscale
    assert np.array_equal(S.GridPlan.from_image(str(path), 2, -1, 3).occ, S.GridPlan.from_image(img, 2, -1, 3).occ)


def test_refusals():
    ok = np.zeros((2, 3), bool)
    S.GridPlan(ok, [0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 2.0])
    for occ, xs, ys in [(ok, [0.0, 1.0, 2.0], [0.0, 1.0, 2.0]),                       # one edge short
                        (ok, [0.0, 1.0, 1.0, 3.0], [0.0, 1.0, 2.0]),                  # not strictly increasing
                        (ok, [0.0, 2.0, 1.0, 3.0], [0.0, 1.0, 2.0]),
                        (ok, [0.0, 1.0, 1.0005, 3.0], [0.0, 1.0, 2.0]),               # a cell below 1 mm
                        (ok, [0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 10001.0]),              # beyond 1e4 m
                        (ok, [0.0, 1.0, 2.0, np.nan], [0.0, 1.0, 2.0]),
                        (np.zeros((0, 3), bool), [0.0, 1.0, 2.0, 3.0], [0.0]),
                        (np.zeros((1, 1025), bool), np.arange(1026.0), [0.0, 1.0]),
                        (np.zeros((1025, 1), bool), [0.0, 1.0], np.arange(1026.0)),
                        (np.zeros(3, bool), [0.0, 1.0, 2.0, 3.0], [0.0, 1.0]),
                        (np.zeros((2, 3)), [0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 2.0])]:   # floats are not truth values
        with pytest.raises(ValueError):
            S.GridPlan(occ, xs, ys)
    S.GridPlan(np.zeros((1, 1024), bool), np.arange(1025.0), [0.0, 1.0])
    with pytest.raises(ValueError):
        S.GridPlan.from_boxes([(0.0, 0.0, 0.33, 1.0)])                                # off the lattice
    with pytest.raises(ValueError):
        S.GridPlan.from_boxes(np.zeros((0, 4)))
    with pytest.raises(ValueError):
        S.GridPlan.from_boxes([(0.0, 0.0, 60.0, 1.0)])                                # 1200 cells at 20 per metre
    with pytest.raises(ValueError):
        S.GridPlan.uniform(ok, 2.5, 0, 0)
    with pytest.raises(ValueError):
        S.GridPlan.from_image(np.zeros((2, 2), np.float32), 2, 0, 0)
    with pytest.raises(ValueError):
        S.GridWorlds([])
    with pytest.raises(ValueError):
        S.GridWorlds([S.GridPlan.uniform(ok, 2, 0, 0)], starts=[])
    assert not S.GridPlan.uniform(ok, 2, 0, 0).occ.flags.writeable


@functools.lru_cache(maxsize=None)
def _two_plans():
    """Two 12 m x 10 m plans at 10 cells per metre, neither a set of lattice boxes: a ring wall with a diagonal partition that
    leaves a gap, round pillars; the second one mirrored with other pillars."""
    out = []
    for flip in (False, True):
        jj, ii = np.mgrid[0:100, 0:120]
        occ = (ii < 3) | (ii >= 117) | (jj < 3) | (jj >= 97)
        occ |= (np.abs(ii - jj - 10) <= 1) & ((jj < 40) | (jj > 58))               # a diagonal wall with a doorway
        for (ci, cj, r) in ((30, 70, 5), (85, 30, 6), (90, 75, 4)) if not flip else ((25, 75, 6), (80, 20, 4), (95, 60, 5)):
            occ |= (ii - ci) ** 2 + (jj - cj) ** 2 <= r * r
        out.append(S.GridPlan.uniform(occ[:, ::-1] if flip else occ, 10, -60, -50))
    return tuple(out)


def test_grid_spots_are_clear_and_reachable():
    plan = _two_plans()[0]
    spots = S.grid_spots(plan)
    assert len(spots) >= 12 and np.array_equal(spots, S.grid_spots(plan))
    assert np.array_equal(spots * 4, np.rint(spots * 4))                                      # on the 0.25 m lattice
    order = [tuple(p) for p in spots.tolist()]
    assert order == sorted(order)
    boxes = S.grid_boxes(plan)
    for p in spots:
        assert min(S.rect_distance(p, b) for b in boxes) >= 0.65
    # reachable: a walk over free lattice points from the first spot gets to every other one
    free = {(a, b) for a in range(-24, 25) for b in range(-20, 21) if not S._blocked(0.25 * a, 0.25 * b, S.STEP_MARGIN, boxes=boxes)}
    seen, todo = set(), [tuple(int(v) for v in np.rint(spots[0] * 4))]
    while todo:
        p = todo.pop()
        if p in seen or p not in free:
            continue
        seen.add(p)
        todo += [(p[0] + 1, p[1]), (p[0] - 1, p[1]), (p[0], p[1] + 1), (p[0], p[1] - 1)]
    assert all(tuple(int(v) for v in np.rint(p * 4)) in seen for p in spots)
    # a walled-off pocket: its clear points are dropped when the fill starts outside it, and are all there is from inside
    occ = np.zeros((80, 80), bool)
    occ[[0, -1], :] = occ[:, [0, -1]] = True
    occ[:, 40:42] = True
    split = S.GridPlan.uniform(occ, 10, -40, -40)
    left, right = S.grid_spots(split, start=(-2.0, 0.0)), S.grid_spots(split, start=(2.0, 0.0))
    assert len(left) and len(right) and (left[:, 0] < 0).all() and (right[:, 0] > 0).all()
    with pytest.raises(ValueError):
        S.grid_spots(split, start=(0.1, 0.0))


def test_grid_worlds_are_a_pure_function_of_seed_env_and_episode():
    plans = _two_plans()
    a, b, other = S.GridWorlds(plans, seed=4), S.GridWorlds(plans, seed=4), S.GridWorlds(plans, seed=5)
    assert a.max_grid == (100, 120)
    keys = [(e, k) for e in range(6) for k in range(4)]
    for (e, k) in keys:
        u, v = a.world(e, k), b.world(e, k)
        assert u.grid is v.grid and u.grid in plans and len(u.boxes) == 0 and u.boxes.shape == (0, 4)
        assert np.array_equal(u.start_xy, v.start_xy) and u.start_k == v.start_k and np.array_equal(u.spots, v.spots)
        assert any(np.array_equal(u.start_xy, p) for p in u.spots) and 0 <= u.start_k < 12
        assert not S._blocked(u.start_xy[0], u.start_xy[1], S.STEP_MARGIN, boxes=np.zeros((0, 4)), grid=u.grid)
        lay = a.layout(e, k, u.start_xy)
        assert lay == b.layout(e, k, u.start_xy) and lay[0][0] == list(S.OBJECT_SIZES)[e % 6] and len(lay) == 2
        for _, box in lay:
            centre = (0.5 * (box[0] + box[2]), 0.5 * (box[1] + box[3]))
            assert np.hypot(centre[0] - u.start_xy[0], centre[1] - u.start_xy[1]) > S.OBJECT_START_CLEARANCE
    assert {a.plan_of(e, k) for (e, k) in keys} == {0, 1}
    assert len({(a.world(e, k).start_xy.tobytes(), a.world(e, k).start_k) for (e, k) in keys}) > 12
    assert any(a.plan_of(e, k) != other.plan_of(e, k) for (e, k) in keys)
    fixed = S.GridWorlds(plans, starts=[(0.0, -3.0, 2), (1.0, -3.0, 14)], spots=[[(0.0, 0.0)], [(1.0, 1.0)]])
    w = fixed.world(3, 1)
    n = fixed.plan_of(3, 1)
    assert np.array_equal(w.start_xy, [(0.0, -3.0), (1.0, -3.0)][n]) and w.start_k == 2 and np.array_equal(w.spots, [[(0.0, 0.0)], [(1.0, 1.0)]][n])
    assert S.ProceduralWorlds(0).world(0, 0).grid is None


def test_the_harness_refuses_what_grid_worlds_cannot_do():
    """Before any device is touched: colours are defined by box and face, the geodesic fields hold at most 141 rectangles."""
    from vlfm_amd.harness import BatchedEpisodes, WorldObjects

    worlds = S.GridWorlds(_two_plans())
    kw = dict(device="cuda:0", use_blip2=False, select_frontiers=True, closed_loop=True, worlds=worlds)
    with pytest.raises(ValueError, match="render_rgb"):
        BatchedEpisodes(2, render_rgb=True, **kw)
    with pytest.raises(ValueError, match="objectnav_metrics"):
        BatchedEpisodes(2, world_objects=WorldObjects(), objectnav_metrics=True, **kw)
    with pytest.raises(ValueError, match="closed_loop"):
        BatchedEpisodes(2, device="cuda:0", use_blip2=False, worlds=worlds)
