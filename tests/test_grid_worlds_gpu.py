"""-m gpu: grid worlds on the device (vlfm_worlds_raycast_grids through RoomsRenderer.cast_worlds and WorldTable(max_grid=...))
against the host statements, bit for bit, and BatchedEpisodes(worlds=GridWorlds(...))."""
import functools

import numpy as np
import pytest

from vlfm_amd import synthetic as S
from test_grid_worlds_cpu import _two_plans
from world_object_cases import ENV_OBJECTS, RING8, objects_array

pytestmark = pytest.mark.gpu

WORLD_OF = [3, 0, 2, 2, 1, 5, 4]
ENV_OF = [2, 0, 3, 3, 1, 2, 2]
MAX_GRID = (64, 70)
NONE = np.zeros((0, 4))


@functools.lru_cache(maxsize=None)
def _worlds():
    """Six worlds (boxes, plan): BOXES without a grid; grids of 1 x 1, 3 x 5, 33 x 70 (a row crosses 32-bit words) and, with 5
    boxes, 64 x 64 cells; an empty grid of 40 x 40.  (ny x nx.)"""
    rng = np.random.default_rng(23)
    g1 = S.GridPlan.uniform(np.ones((1, 1), bool), 2, 2, 2)                                    # the cell [1, 1.5]^2
    g2 = S.GridPlan.uniform(np.array([[1, 0, 0, 1, 0], [0, 0, 1, 0, 1], [1, 1, 0, 0, 1]], bool), 2, -2, 2)
    occ3 = rng.random((33, 70)) < 0.08
    occ3[16, 35] = True                                                                          # [0, 0.1]^2: camera 0 is in it
    occ3[:, 69] = True                                                                           # the last column: word 2, bit 5
    g3 = S.GridPlan.uniform(occ3, 10, -35, -16)
    occ4 = rng.random((64, 64)) < 0.05
    occ4[28:38, 30:40] = False
    g4 = S.GridPlan(occ4, -3.2 + 0.1 * np.arange(65), (np.arange(65) - 32) / 10.0)             # edges built two ways
    five = np.array([(1.0, 0.45, 1.2, 0.8), (-0.6, 0.9, 0.2, 1.0), (0.5, -0.7, 0.6, -0.5), (-3.0, -3.0, 3.0, -2.9), (0.8, 1.4, 0.9, 1.5)])
    g5 = S.GridPlan.uniform(np.zeros((40, 40), bool), 10, -20, -20)
    out = ((S.BOXES.copy(), None), (NONE, g1), (NONE, g2), (NONE, g3), (five, g4), (NONE, g5))
    assert len(out[0][0]) == 37 and [(p.ny, p.nx) for _, p in out[1:]] == [(1, 1), (3, 5), (33, 70), (64, 64), (40, 40)]
    return out


def _cameras():
    """7 cameras (tf, hfov, lo, hi): camera 0 inside an occupied cell, camera 2 on a cell corner, cameras 3 and 4 outside their
    grids; three with an arbitrary yaw, height, field of view and depth range."""
    tf = np.stack([S.tf_of(0.05, 0.05, 2), S.tf_of(0.0, 0.0, 0), S.tf_of(0.0, 1.5, 4), S.pose_to_tf(0.2, 0.4, 1.2, 1.1),
                   S.tf_of(-0.5, 0.0, 1), S.pose_to_tf(0.25, -0.5, -2.5, 0.5), S.pose_to_tf(0.3, 0.1, 1.0, 0.88)])
    hfov = np.deg2rad([79.0, 79.0, 79.0, 60.0, 79.0, 100.0, 42.0])
    lo = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.3, 0.05])
    hi = np.array([5.0, 5.0, 5.0, 2.5, 5.0, 3.5, 9.0])
    return tf, hfov, lo, hi


def _objects():
    """Four object rows; the last stands between the cells of the 3 x 5 grid, in front of cameras 2 and 3."""
    return [ENV_OBJECTS[0], ENV_OBJECTS[1], RING8, [(-0.3, 1.75, -0.1, 1.95, 0.0, 1.2), (0.3, 0.75, 0.45, 0.9, 0.0, 1.0)]]


def _table(device, worlds, tails="zeros", max_grid=MAX_GRID):
    """The table of ``worlds``; tails "ones": behind the wrapper's back every bit and every edge beyond each world's dims is set
    (bits to one, edges to 0.5: a wall everywhere, were it read)."""
    import torch

    from vlfm_amd.harness import WorldTable

    table = WorldTable(len(worlds), device, max_grid=max_grid)
    table.assign(np.arange(len(worlds)), [b for b, _ in worlds], [g for _, g in worlds])
    assert table.d_grid_dims.cpu().numpy().tolist() == [[0, 0] if g is None else [g.ny, g.nx] for _, g in worlds]
    if tails == "ones":
        ny, nx = max_grid
        bits = table.d_grid_bits.cpu().numpy().view(np.uint32).copy()
        edges = table.d_grid_edges.cpu().numpy().copy()
        for w, (_, g) in enumerate(worlds):
            inside = np.zeros((ny, table.grid_words * 32), bool)
            keep = np.zeros(nx + ny + 2, bool)
            if g is not None:
                inside[:g.ny, :g.nx] = True
                keep[:g.nx + 1] = keep[nx + 1:nx + 1 + g.ny + 1] = True
            fill = np.packbits(~inside, axis=1, bitorder="little").view("<u4").reshape(ny, table.grid_words)
            assert not (bits[w] & fill).any()                  # the wrapper left the tails zero
            bits[w] |= fill
            edges[w, ~keep] = 0.5
        table.d_grid_bits.copy_(torch.from_numpy(bits.view(np.int32)))
        table.d_grid_edges.copy_(torch.from_numpy(edges))
    return table


@functools.lru_cache(maxsize=None)
def _reference(H, W, with_objects=True):
    worlds = _worlds()
    tf, hfov, lo, hi = _cameras()
    objs = _objects()
    ref = [S.render_objects_numpy(t[0, 3], t[1, 3], t[0, 0], t[1, 0], t[2, 3], W / (2 * np.tan(f / 2)), a, b, H, W,
                                  objs[e] if with_objects else [], boxes=worlds[w][0], grid=worlds[w][1])
           for t, f, a, b, e, w in zip(tf, hfov, lo, hi, ENV_OF, WORLD_OF)]
    out = (np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]), np.stack([S.object_stats_numpy(r[1]) for r in ref]))
    for a in out:
        a.setflags(write=False)
    return out


def _bits(t):
    import torch

    return t.contiguous().view(torch.int32).cpu().numpy()


def _assert_equal(got, want):
    depth, ids, stats = got
    assert np.array_equal(stats.cpu().numpy(), want[2])
    assert np.array_equal(ids.cpu().numpy(), want[1])
    assert np.array_equal(_bits(depth), np.ascontiguousarray(want[0]).view(np.int32))


def _renderer(H, W, device):
    from vlfm_amd.harness import RoomsRenderer

    return RoomsRenderer([0], 500, H, W, device)


def test_the_scene_is_worth_its_name():
    """Host only: the grids show in the frames, the definition holds for them (the walk is the cell boxes), and the cameras
    stand where the docstring says."""
    worlds = _worlds()
    tf, hfov, lo, hi = _cameras()
    H, W = 36, 64
    want = _reference(H, W)
    assert len({w.tobytes() for w in want[0]}) == 7 and (want[2][:, :, 0].sum(axis=1) > 0).all()
    for cam, (t, f, a, b, e, w) in enumerate(zip(tf, hfov, lo, hi, ENV_OF, WORLD_OF)):
        boxes, g = worlds[w]
        args = (t[0, 3], t[1, 3], t[0, 0], t[1, 0], t[2, 3], W / (2 * np.tan(f / 2)), a, b, H, W, _objects()[e])
        if g is not None:
            cells = S.render_objects_numpy(*args, boxes=np.concatenate([boxes, S.grid_boxes(g)]))
            assert np.array_equal(cells[0].view(np.int32), want[0][cam].view(np.int32)) and np.array_equal(cells[1], want[1][cam])
        if g is not None and g.occ.any():
            bare = S.render_objects_numpy(*args, boxes=boxes)
            assert not np.array_equal(bare[0], want[0][cam]), cam
    assert S.grid_blocked(worlds[3][1], 0.05, 0.05, 0.0)                                   # camera 0: inside an occupied cell
    assert 0.0 in worlds[2][1].xs and 1.5 in worlds[2][1].ys                               # camera 2: on a corner
    assert tf[3][1, 3] < worlds[2][1].ys[0] and tf[4][0, 3] < worlds[1][1].xs[0]           # cameras 3, 4: outside


@pytest.mark.parametrize("tails", ["zeros", "ones"])
@pytest.mark.parametrize("H,W", [(50, 70), (36, 64)], ids=["70x50", "64x36"])
def test_raycast_with_objects_equals_the_numpy_renderer(gpu_device, H, W, tails):
    tf, hfov, lo, hi = _cameras()
    table = _table(gpu_device, _worlds(), tails)
    got = _renderer(H, W, gpu_device).cast_worlds(tf, table, WORLD_OF, objects_array(_objects()), ENV_OF, hfov, lo, hi)
    _assert_equal(got, _reference(H, W))


@pytest.mark.parametrize("tails", ["zeros", "ones"])
@pytest.mark.parametrize("H,W", [(50, 70), (36, 64)], ids=["70x50", "64x36"])
def test_raycast_walls_only_equals_the_numpy_renderer(gpu_device, H, W, tails):
    tf, hfov, lo, hi = _cameras()
    table = _table(gpu_device, _worlds(), tails)
    got = _renderer(H, W, gpu_device).cast_worlds(tf, table, WORLD_OF, hfov=hfov, min_depth=lo, max_depth=hi)
    assert got.shape == (7, H, W) and np.array_equal(_bits(got), _reference(H, W, False)[0].view(np.int32))


def test_raycast_at_640x480(gpu_device):
    tf, hfov, lo, hi = _cameras()
    r = _renderer(480, 640, gpu_device)
    table = _table(gpu_device, _worlds(), "ones")
    _assert_equal(r.cast_worlds(tf, table, WORLD_OF, objects_array(_objects()), ENV_OF, hfov, lo, hi), _reference(480, 640))
    walls = r.cast_worlds(tf, table, WORLD_OF, hfov=hfov, min_depth=lo, max_depth=hi)
    assert np.array_equal(_bits(walls), _reference(480, 640, False)[0].view(np.int32))


def test_lattice_poses_on_edges_and_corners(gpu_device):
    """Walls only, all 12 headings from lattice points of the 33 x 70 grid (0.1 m cells: every pose is on a corner) and of the
    64 x 64 grid with its boxes: wall_profile(boxes=, grid=)."""
    worlds = _worlds()
    H, W = 12, 70
    ps = [(0.5, 0.25, k) for k in range(12)] + [(-0.25, -0.5, k) for k in range(12)] + [(0.0, 0.0, k) for k in range(12)]
    world_of = [3] * 12 + [3] * 12 + [4] * 12
    want = np.stack([S.depth_from_profile(S.wall_profile(x, y, k, W, boxes=worlds[w][0], grid=worlds[w][1]), H)
                     for (x, y, k), w in zip(ps, world_of)])
    tf = np.stack([S.tf_of(x, y, k) for (x, y, k) in ps])
    got = _renderer(H, W, gpu_device).cast_worlds(tf, _table(gpu_device, worlds, "ones"), world_of)
    assert np.array_equal(_bits(got), want.view(np.int32)) and len({w.tobytes() for w in want}) == 36


def test_out_and_a_side_stream(gpu_device):
    import torch

    H, W = 36, 64
    tf, hfov, lo, hi = _cameras()
    want = _reference(H, W)
    r = _renderer(H, W, gpu_device)
    side = torch.cuda.Stream(gpu_device)
    out = torch.empty((7, H, W), dtype=torch.float32, device=gpu_device)
    big = torch.ones((64, 480, 640), dtype=torch.float32, device=gpu_device)
    objs = objects_array(_objects())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        table = _table(gpu_device, _worlds())           # the table is written on the side stream too
        for _ in range(20):
            big.mul_(1.0001)
        out.copy_(big[:7, :H, :W])                      # queued BEFORE the launch: must not land after it
        got = r.cast_worlds(tf, table, WORLD_OF, objs, ENV_OF, hfov, lo, hi, out=out)
        after = out.clone()
    side.synchronize()
    assert got[0].data_ptr() == out.data_ptr()
    _assert_equal((after, got[1], got[2]), want)
    _assert_equal(got, want)
    # a view 8 bytes into an allocation: the scalar store path
    odd = torch.full((2 + 7 * H * W,), -1.0, dtype=torch.float32, device=gpu_device)
    _assert_equal(r.cast_worlds(tf, table, WORLD_OF, objs, ENV_OF, hfov, lo, hi, out=odd[2:].view(7, H, W)), want)
    assert bool((odd[:2] == -1.0).all())


def test_refusals_leave_the_outputs_untouched(gpu_device):
    import torch

    from vlfm_amd import _lib as L
    from vlfm_amd.harness import WorldTable

    worlds = _worlds()
    tf, hfov, lo, hi = _cameras()
    H, W = 9, 18
    r = _renderer(H, W, gpu_device)
    table = _table(gpu_device, worlds)
    objs = objects_array(_objects())
    with pytest.raises(ValueError, match="colour"):
        r.cast_worlds_rgb(tf, table, WORLD_OF, objs, ENV_OF)
    for bad in ((1025, 4), (4, 1025), (0, 4)):
        with pytest.raises(ValueError):
            WorldTable(2, gpu_device, max_grid=bad)
    small = WorldTable(2, gpu_device, max_grid=(32, 69))
    with pytest.raises(ValueError):
        small.assign([0], [NONE], [worlds[3][1]])                       # 70 columns into 69
    with pytest.raises(ValueError):
        WorldTable(2, gpu_device).assign([0], [NONE], [worlds[1][1]])   # a table without grids
    with pytest.raises(ValueError):
        table.assign([0, 1], [NONE, NONE], [None])
    # the raw entry: one camera in world 2
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    f64 = dict(dtype=torch.float64, device=gpu_device)
    cam = torch.tensor([[0.0, 0.0, 0.0, 1.0, S.CAMERA_HEIGHT, S.camera_intrinsics(W)[0], S.MIN_DEPTH, S.MAX_DEPTH]], **f64)
    world_of = torch.full((1,), 2, dtype=torch.int32, device=gpu_device)
    env_of = torch.zeros(1, dtype=torch.int32, device=gpu_device)
    d_obj = torch.zeros((1, 8, 8), **f64)
    colours = torch.zeros(8, dtype=torch.int32, device=gpu_device)
    palette = torch.tensor(S.WORLD_PALETTE, dtype=torch.int32, device=gpu_device)
    depth = torch.full((1, H, W), -1.0, dtype=torch.float32, device=gpu_device)
    ids = torch.full((1, H, W), 9, dtype=torch.uint8, device=gpu_device)
    stats = torch.full((1, 8, 5), -7, dtype=torch.int32, device=gpu_device)
    rgb = torch.full((1, H, W, 3), 7, dtype=torch.uint8, device=gpu_device)

    def call(d_rgb=None, bits=table.d_grid_bits.data_ptr(), edges=table.d_grid_edges.data_ptr(), dims=table.d_grid_dims.data_ptr(),
             max_nx=MAX_GRID[1], max_ny=MAX_GRID[0], objects=True):
        o = objects or d_rgb is not None
        return lib.vlfm_worlds_raycast_grids(
            cam.data_ptr(), 1, table.d_boxes.data_ptr(), table.d_counts.data_ptr(), table.n_worlds, table.max_boxes,
            world_of.data_ptr(), d_obj.data_ptr() if o else None, env_of.data_ptr() if o else None, 1, H, W, depth.data_ptr(),
            ids.data_ptr() if o else None, stats.data_ptr() if o else None, colours.data_ptr() if d_rgb else None,
            palette.data_ptr() if d_rgb else None, d_rgb, bits, edges, dims, max_nx, max_ny, st)

    for kw in (dict(d_rgb=rgb.data_ptr()), dict(max_nx=1025), dict(max_ny=1025), dict(max_nx=0), dict(max_ny=0), dict(bits=None),
               dict(edges=None), dict(dims=None), dict(max_nx=1025, objects=False)):
        assert call(**kw) == L.VLFM_ERR_INVALID, kw
    torch.cuda.synchronize()
    assert bool((depth == -1.0).all()) and bool((ids == 9).all()) and bool((stats == -7).all()) and bool((rgb == 7).all())
    # the same call unrefused is the frame; without the three arrays it is vlfm_worlds_raycast: world 2 has no boxes
    assert call() == L.VLFM_OK, L.last_error()
    want = S.render_objects_numpy(0.0, 0.0, 0.0, 1.0, S.CAMERA_HEIGHT, S.camera_intrinsics(W)[0], S.MIN_DEPTH, S.MAX_DEPTH, H, W, [],
                                  boxes=NONE, grid=worlds[2][1])[0]
    assert np.array_equal(_bits(depth[0]), want.view(np.int32)) and bool((ids == 0).all())
    assert call(bits=None, edges=None, dims=None, max_nx=0, max_ny=0) == L.VLFM_OK, L.last_error()
    bare = S.render_objects_numpy(0.0, 0.0, 0.0, 1.0, S.CAMERA_HEIGHT, S.camera_intrinsics(W)[0], S.MIN_DEPTH, S.MAX_DEPTH, H, W, [],
                                  boxes=NONE)[0]
    assert np.array_equal(_bits(depth[0]), bare.view(np.int32)) and not np.array_equal(bare, want)
    assert lib.vlfm_abi_version() >= 25


def test_a_rasterised_procedural_world_is_its_box_world_from_the_same_launch(gpu_device):
    world = S.ProceduralWorlds(0).world(2, 0)
    plan = S.GridPlan.from_boxes(world.boxes)
    assert (plan.ny, plan.nx) == (400, 400)
    H, W = 36, 64
    views = [(world.start_xy, world.start_k)] + [(world.spots[n], (5 * n + 1) % 12) for n in range(5)]
    tf = np.stack([S.tf_of(x, y, k) for (x, y), k in views] * 2)
    world_of = [0] * 6 + [1] * 6
    c, s = S.HEADINGS[world.start_k]
    near = [S.object_box("chair", world.start_xy[0] + 1.0 * c, world.start_xy[1] + 1.0 * s)]
    table = _table(gpu_device, ((world.boxes, None), (NONE, plan)), "ones", max_grid=(400, 400))
    depth, ids, stats = _renderer(H, W, gpu_device).cast_worlds(tf, table, world_of, objects_array([near]), [0] * 12)
    d, i, st = _bits(depth), ids.cpu().numpy(), stats.cpu().numpy()
    assert np.array_equal(d[:6], d[6:]) and np.array_equal(i[:6], i[6:]) and np.array_equal(st[:6], st[6:])
    assert len({x.tobytes() for x in d[:6]}) == 6 and st[0, 0, 0] > 0
    (x, y), k = views[0]
    want = S.render_objects_numpy(x, y, c, s, S.CAMERA_HEIGHT, S.camera_intrinsics(W)[0], S.MIN_DEPTH, S.MAX_DEPTH, H, W, near,
                                  boxes=world.boxes)
    assert np.array_equal(d[6], want[0].view(np.int32)) and np.array_equal(i[6], want[1])


# ------------------------------------------------------------------------------------------------------------------- harness
E, STEPS = 4, 30


def _harness(device, **kw):
    from vlfm_amd.harness import BatchedEpisodes, WorldObjects

    return BatchedEpisodes(E, device=device, use_blip2=False, select_frontiers=True, closed_loop=True,
                           world_objects=WorldObjects(max_episode_steps=12), worlds=S.GridWorlds(_two_plans(), seed=3), **kw)


def _clear(h, e):
    x, y = h.live.xy[e]
    plan = h.live.table.grids[e]
    return plan is not None and not S.grid_blocked(plan, x, y, S.STEP_MARGIN) and \
        not S._blocked(x, y, S.STEP_MARGIN, boxes=S.grid_boxes(plan))


def test_harness_in_grid_worlds(gpu_device):
    import torch

    a, b = _harness(gpu_device), _harness(gpu_device)
    worlds = S.GridWorlds(_two_plans(), seed=3)
    fx = S.camera_intrinsics(a.W)[0]
    assert a.live.world_episode.tolist() == [0] * E and a.live.table.max_grid == (100, 120)
    for e in range(E):
        w = worlds.world(a.env_ids[e], 0)
        assert a.live.table.grids[e] is not None and np.array_equal(a.live.table.grids[e].occ, w.grid.occ)
        assert len(a.live.table.world(e)) == 0 and np.array_equal(a.live.xy[e], w.start_xy) and a.live.k[e] == w.start_k
    moved, lived_in = 0, set()
    for t in range(STEPS):
        before = [(a.live.xy[e].copy(), int(a.live.k[e]), a.live.table.grids[e], a.live.objects[e].copy(), int(a.live.world_episode[e]))
                  for e in range(E)]
        lived_in |= {_two_plans().index(x[2]) for x in before}
        a.step()
        b.step()
        assert np.array_equal(a.last_poses, b.last_poses) and np.array_equal(a.last_world_actions, b.last_world_actions)
        assert np.array_equal(a.live.xy, b.live.xy) and np.array_equal(a.live.k, b.live.k)
        if t in (0, 7, 29):
            torch.cuda.synchronize()
            assert np.array_equal(_bits(a.live.frames), _bits(b.live.frames))
            for e in (0, 3):
                (x, y), k, plan, objs, _ = before[e]
                c, s = S.HEADINGS[k]
                want = S.render_objects_numpy(x, y, c, s, S.CAMERA_HEIGHT, fx, S.MIN_DEPTH, S.MAX_DEPTH, a.H, a.W,
                                              objs[objs[:, 6] != 0.0, :6], boxes=NONE, grid=plan)
                assert np.array_equal(_bits(a.live.frames[e]), want[0].view(np.int32)), (t, e)
                assert np.array_equal(a.live.ids[e].cpu().numpy(), want[1]), (t, e)
        for e in range(E):
            assert _clear(a, e), (t, e)
            if a.live.world_episode[e] != before[e][4]:              # the episode ended: the NEXT world, from its start
                moved += 1
                w = worlds.world(a.env_ids[e], before[e][4] + 1)
                assert a.live.world_episode[e] == before[e][4] + 1 == a.live.ep_index[e] and a.last_episode_end[e]
                assert a.live.table.grids[e] is w.grid or np.array_equal(a.live.table.grids[e].occ, w.grid.occ)
                assert np.array_equal(a.live.xy[e], w.start_xy) and a.live.k[e] == w.start_k and not a.live.collided[e]
    assert moved >= 2 * E and lived_in == {0, 1}                # 30 steps, episodes of 12 at the most; both plans
    np.testing.assert_equal(a.live.stats, b.live.stats)
    np.testing.assert_equal(a.live.objectnav_stats, b.live.objectnav_stats)


def test_harness_with_the_map_planner(gpu_device):
    h = _harness(gpu_device, controller=S.MapPlannerController())
    for t in range(STEPS):
        h.step()
        for e in range(E):
            assert _clear(h, e), (t, e)
    ps = h.planner_stats
    assert np.array_equal(ps["plans"], ps["ok"] + ps["unreachable"] + ps["too_long"] + ps["invalid"])
    assert len(h.live.objectnav_stats["episode_outcome"]) >= 2 * E
