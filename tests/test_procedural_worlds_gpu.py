"""-m gpu: a world per camera / per field (vlfm_worlds_raycast, vlfm_geodesic_fields through RoomsRenderer.cast_worlds /
geodesic_fields_worlds and WorldTable) against the host statements, bit for bit, and BatchedEpisodes(worlds=...)."""
import functools

import numpy as np
import pytest

from vlfm_amd import synthetic as S
from world_object_cases import ENV_OBJECTS, objects_array, poses

pytestmark = pytest.mark.gpu

WORLD_OF = [3, 0, 2, 2, 1, 3, 0]
ENV_OF = [2, 0, 1, 0, 0, 2, 1]


@functools.lru_cache(maxsize=None)
def _worlds():
    """Four worlds with 0, 1, 37 (BOXES) and 64 boxes (a generated one, padded up with small pillars); read-only."""
    gen = S.ProceduralWorlds(0).world(7, 0)
    n = S.WORLD_MAX_BOXES - len(gen.boxes)
    assert n >= 0
    pad = np.array([(-9.0 + 0.3 * i, 9.0 - 0.05 * i, -8.9 + 0.3 * i, 9.1 - 0.05 * i) for i in range(n)]).reshape(-1, 4)
    out = (np.zeros((0, 4)), np.array([(1.0, -0.5, 1.5, 0.1)]), S.BOXES.copy(), np.concatenate([gen.boxes, pad]))
    assert [len(b) for b in out] == [0, 1, 37, 64]
    for b in out:
        b.setflags(write=False)
    return out, gen


def _cameras():
    """7 cameras (tf, hfov, lo, hi): lattice poses in their worlds; three of them with an arbitrary yaw, height, field of view
    and depth range."""
    gen = _worlds()[1]
    gx, gy = gen.start_xy
    tf = np.stack([S.tf_of(gx, gy, gen.start_k), S.tf_of(0.0, 0.0, 0), S.tf_of(0.5, -0.5, 4), S.pose_to_tf(0.2, 0.4, 0.2, 1.1),
                   S.tf_of(-0.5, 0.0, 0), S.pose_to_tf(gen.spots[3][0], gen.spots[3][1], -2.5, 0.5), S.pose_to_tf(0.3, 0.1, 1.0, 0.88)])
    hfov = np.deg2rad([79.0, 79.0, 79.0, 60.0, 79.0, 100.0, 42.0])
    lo = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.3, 0.05])
    hi = np.array([5.0, 5.0, 5.0, 2.5, 5.0, 3.5, 9.0])
    return tf, hfov, lo, hi


def _objects():
    """Three object rows: around the origin (ENV_OBJECTS[0]), the ring of 8, and in the generated world one object in front of
    its start pose and one in front of camera 5."""
    gen = _worlds()[1]
    c, s = S.HEADINGS[gen.start_k]
    x, y = gen.start_xy[0] + 1.0 * c, gen.start_xy[1] + 1.0 * s
    u, v = gen.spots[3][0] + 1.2 * np.cos(-2.5), gen.spots[3][1] + 1.2 * np.sin(-2.5)
    near = [(x - 0.2, y - 0.2, x + 0.2, y + 0.2, 0.0, 1.0), (u - 0.1, v - 0.1, u + 0.1, v + 0.1, 0.2, 1.4)]
    return [ENV_OBJECTS[0], ENV_OBJECTS[2], near]


def _poison(tf, world_of=WORLD_OF):
    """Per world a finite box 0.5 m in front of the first camera that stands in it: what the table tails are filled with."""
    out = np.zeros((4, 4))
    for w in range(4):
        t = tf[list(world_of).index(w)]
        x, y = t[0, 3] + 0.8 * t[0, 0], t[1, 3] + 0.8 * t[1, 0]
        out[w] = (x - 0.3, y - 0.3, x + 0.3, y + 0.3)
    return out


def _table(device, worlds, poison=None, max_boxes=S.WORLD_MAX_BOXES):
    import torch

    from vlfm_amd.harness import WorldTable

    table = WorldTable(len(worlds), device, max_boxes)
    table.assign(np.arange(len(worlds)), worlds)
    if poison is not None:                         # behind the wrapper's back: the rows beyond each count, on the device only
        d = table.d_boxes.cpu().numpy()
        for w, b in enumerate(worlds):
            d[w, len(b):] = poison[w]
        table.d_boxes.copy_(torch.from_numpy(d))
    return table


@functools.lru_cache(maxsize=None)
def _reference(H, W):
    worlds = _worlds()[0]
    tf, hfov, lo, hi = _cameras()
    objs = _objects()
    ref = [S.render_objects_numpy(t[0, 3], t[1, 3], t[0, 0], t[1, 0], t[2, 3], W / (2 * np.tan(f / 2)), a, b, H, W, objs[e],
                                  boxes=worlds[w]) for t, f, a, b, e, w in zip(tf, hfov, lo, hi, ENV_OF, WORLD_OF)]
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


@pytest.mark.parametrize("tails", ["nan", "box"])
@pytest.mark.parametrize("H,W", [(12, 20), (9, 18), (48, 64)], ids=["20x12", "18x9", "64x48"])
def test_raycast_equals_the_numpy_renderer(gpu_device, H, W, tails):
    worlds = _worlds()[0]
    tf, hfov, lo, hi = _cameras()
    want = _reference(H, W)
    assert (want[2][:, :, 0].sum(axis=1) > 0).all() and len({w.tobytes() for w in want[0]}) == 7      # every camera sees an object
    poison = _poison(tf)
    if tails == "box":      # the poison is worth its name: as a box of world 0 (empty) or 2 (BOXES) it would change the frame
        for cam in (1, 2):
            t, w = tf[cam], WORLD_OF[cam]
            seen = S.render_objects_numpy(t[0, 3], t[1, 3], t[0, 0], t[1, 0], t[2, 3], W / (2 * np.tan(hfov[cam] / 2)), lo[cam],
                                          hi[cam], H, W, [], boxes=np.concatenate([worlds[w], poison[w:w + 1]]))[0]
            bare = S.render_objects_numpy(t[0, 3], t[1, 3], t[0, 0], t[1, 0], t[2, 3], W / (2 * np.tan(hfov[cam] / 2)), lo[cam],
                                          hi[cam], H, W, [], boxes=worlds[w])[0]
            assert not np.array_equal(seen, bare)
    table = _table(gpu_device, worlds, poison if tails == "box" else None)
    got = _renderer(H, W, gpu_device).cast_worlds(tf, table, WORLD_OF, objects_array(_objects()), ENV_OF, hfov, lo, hi)
    _assert_equal(got, want)


def test_walls_only_on_lattice_poses(gpu_device):
    """objects=None: depth_from_profile(wall_profile(boxes=...)), the frames of cast_cameras."""
    worlds, gen = _worlds()
    H, W = 48, 64
    ps = [(gen.start_xy[0], gen.start_xy[1], k) for k in (0, 5, 9)] + [(gen.spots[2][0], gen.spots[2][1], 2)] + list(poses()[:3]) \
        + [(0.0, 0.0, 0), (-0.5, 0.0, 0)]
    world_of = [3, 3, 3, 3, 2, 2, 2, 0, 1]
    want = np.stack([S.depth_from_profile(S.wall_profile(x, y, k, W, boxes=worlds[w]), H) for (x, y, k), w in zip(ps, world_of)])
    tf = np.stack([S.tf_of(x, y, k) for (x, y, k) in ps])
    table = _table(gpu_device, worlds, _poison(tf, world_of))
    r = _renderer(H, W, gpu_device)
    got = r.cast_worlds(tf, table, world_of)
    assert got.shape == (9, H, W) and np.array_equal(_bits(got), want.view(np.int32))
    assert len({w.tobytes() for w in want}) == 9
    for bad in ([0] * 8, [0] * 8 + [4], [-1] + [0] * 8):
        with pytest.raises(ValueError):
            r.cast_worlds(tf, table, bad)
    assert r.cast_worlds(np.zeros((0, 4, 4)), table, []).shape == (0, H, W)


@pytest.mark.parametrize("H,W", [(48, 64), (9, 18)], ids=["64x48", "18x9"])
def test_a_row_of_BOXES_is_the_existing_entries(gpu_device, H, W):
    """The rooms-world methods and a table row that holds BOXES are one path now: both are held against the host statements
    of the rooms world (render_objects_numpy / object_stats_numpy with boxes=None; walls only: render_objects_numpy without objects)."""
    tf, hfov, lo, hi = _cameras()
    r = _renderer(H, W, gpu_device)
    table = _table(gpu_device, [_worlds()[0][1], S.BOXES])
    objs = _objects()
    ref = [S.render_objects_numpy(t[0, 3], t[1, 3], t[0, 0], t[1, 0], t[2, 3], W / (2 * np.tan(f / 2)), a, b, H, W, objs[e],
                                  boxes=None) for t, f, a, b, e in zip(tf, hfov, lo, hi, ENV_OF)]
    want = (np.stack([x[0] for x in ref]), np.stack([x[1] for x in ref]), np.stack([S.object_stats_numpy(x[1]) for x in ref]))
    assert (want[1] > 0).any()
    old = r.cast_cameras_objects(tf, objects_array(objs), ENV_OF, hfov, lo, hi)
    new = r.cast_worlds(tf, table, [1] * 7, objects_array(objs), ENV_OF, hfov, lo, hi)
    _assert_equal(old, want)
    _assert_equal(new, want)
    assert np.array_equal(_bits(new[0]), _bits(old[0])) and (new[1] == old[1]).all() and (new[2] == old[2]).all()
    walls = np.stack([S.render_objects_numpy(t[0, 3], t[1, 3], t[0, 0], t[1, 0], t[2, 3], W / (2 * np.tan(f / 2)), a, b, H, W, [])[0]
                      for t, f, a, b in zip(tf, hfov, lo, hi)]).view(np.int32)
    assert np.array_equal(_bits(r.cast_worlds(tf, table, [1] * 7, hfov=hfov, min_depth=lo, max_depth=hi)), walls)
    assert np.array_equal(_bits(r.cast_cameras(tf, hfov, lo, hi)), walls)


def test_lds_refusal_out_and_shapes(gpu_device):
    import torch

    tf, hfov, lo, hi = _cameras()
    worlds = _worlds()[0]
    r = _renderer(12, 20, gpu_device)
    objs = objects_array(_objects())
    big = _table(gpu_device, worlds, max_boxes=2100)                 # 2100 * 32 bytes of boxes alone: beyond 64 KB of LDS
    out = torch.full((7, 12, 20), -1.0, dtype=torch.float32, device=gpu_device)
    for kw in (dict(objects=objs, env_of=ENV_OF), dict()):
        with pytest.raises(RuntimeError, match="LDS"):
            r.cast_worlds(tf, big, WORLD_OF, out=out, **kw)
        torch.cuda.synchronize()
        assert bool((out == -1.0).all())
    # a roomier table than the default is the same picture; `out` is rendered into
    want = _reference(12, 20)
    got = r.cast_worlds(tf, _table(gpu_device, worlds, max_boxes=100), WORLD_OF, objs, ENV_OF, hfov, lo, hi, out=out)
    assert got[0].data_ptr() == out.data_ptr()
    _assert_equal(got, want)
    # a view 8 bytes into an allocation: the scalar store path
    odd = torch.full((2 + 7 * 12 * 20,), -1.0, dtype=torch.float32, device=gpu_device)
    _assert_equal(r.cast_worlds(tf, _table(gpu_device, worlds), WORLD_OF, objs, ENV_OF, hfov, lo, hi, out=odd[2:].view(7, 12, 20)), want)
    assert bool((odd[:2] == -1.0).all())
    for bad in (torch.empty((6, 12, 20), dtype=torch.float32, device=gpu_device),
                torch.empty((7, 12, 20), dtype=torch.float64, device=gpu_device)):
        with pytest.raises(ValueError):
            r.cast_worlds(tf, big, WORLD_OF, objs, ENV_OF, out=bad)
    with pytest.raises(ValueError):
        r.cast_worlds(tf, big, WORLD_OF, objs, [0, 1, 2, 3, 0, 0, 0])


def test_the_one_entry_refuses_colour_without_objects(gpu_device):
    """Raw calls of vlfm_worlds_raycast, one camera of 18x9 in a table of one world (BOXES): d_rgb without d_objects is refused
    by status with nothing written; the same call without d_rgb is the walls-only frame; n == 0 needs no pointer."""
    import torch

    from vlfm_amd import _lib as L

    lib, H, W = L.lib(), 9, 18
    st = torch.cuda.current_stream().cuda_stream
    f64 = dict(dtype=torch.float64, device=gpu_device)
    cam = torch.tensor([[0.0, 0.0, 1.0, 0.0, S.CAMERA_HEIGHT, S.camera_intrinsics(W)[0], S.MIN_DEPTH, S.MAX_DEPTH]], **f64)
    boxes = torch.tensor(np.asarray(S.BOXES, np.float64), **f64)
    counts = torch.tensor([len(S.BOXES)], dtype=torch.int32, device=gpu_device)
    world_of = torch.zeros(1, dtype=torch.int32, device=gpu_device)
    depth = torch.full((1, H, W), -1.0, dtype=torch.float32, device=gpu_device)
    rgb = torch.full((1, H, W, 3), 7, dtype=torch.uint8, device=gpu_device)

    def call(d_rgb):
        return lib.vlfm_worlds_raycast(cam.data_ptr(), 1, boxes.data_ptr(), counts.data_ptr(), 1, len(S.BOXES), world_of.data_ptr(),
                                       None, None, 0, H, W, depth.data_ptr(), None, None, None, None, d_rgb, st)

    assert call(rgb.data_ptr()) == L.VLFM_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((depth == -1.0).all()) and bool((rgb == 7).all())
    assert lib.vlfm_worlds_raycast(None, 0, None, None, 0, 0, None, None, None, 0, H, W, None, None, None, None, None, None,
                                   st) == L.VLFM_OK
    assert call(None) == L.VLFM_OK, L.last_error()
    want = S.depth_from_profile(S.wall_profile(0.0, 0.0, 0, W), H)
    assert np.array_equal(_bits(depth[0]), want.view(np.int32)) and bool((rgb == 7).all())


def test_launch_is_ordered_on_the_current_stream(gpu_device):
    """On a side stream, behind a chain of kernels that fills the output buffer on that stream first."""
    import torch

    H, W = 48, 64
    tf, hfov, lo, hi = _cameras()
    want = _reference(H, W)
    r = _renderer(H, W, gpu_device)
    side = torch.cuda.Stream(gpu_device)
    out = torch.empty((7, H, W), dtype=torch.float32, device=gpu_device)
    big = torch.ones((64, 480, 640), dtype=torch.float32, device=gpu_device)
    objs = objects_array(_objects())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        table = _table(gpu_device, _worlds()[0])        # the table is written on the side stream too
        for _ in range(20):
            big.mul_(1.0001)
        out.copy_(big[:7, :H, :W])                  # queued BEFORE the launch: must not land after it
        _, ids, stats = r.cast_worlds(tf, table, WORLD_OF, objs, ENV_OF, hfov, lo, hi, out=out)
        after = out.clone()
    side.synchronize()
    _assert_equal((after, ids, stats), want)
    _assert_equal((out, ids, stats), want)


# ------------------------------------------------------------------------------------------------------------------ geodesic
def _same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_geodesic_fields_of_three_worlds(gpu_device):
    worlds_all, gen = _worlds()
    small = np.array([(-3.0, -3.0, 3.0, -2.0), (-3.0, 2.0, 3.0, 3.0), (-3.0, -3.0, -2.0, 3.0), (2.0, -3.0, 3.0, 3.0),
                      (-0.5, -1.0, 0.5, 2.0)])
    worlds = [S.BOXES, worlds_all[3], small]                  # counts 37, 64, 5
    lay = S.ProceduralWorlds(0).layout(7, 0, gen.start_xy)
    objs = objects_array([[(-1.6, -1.6, -1.2, -1.2, 0.0, 1.0)], [b for _, b in S.object_layout(0, 0, (0.0, 0.0))], [b for _, b in lay]])
    objs[0, 3], objs[0, 0, 6] = objs[0, 0], 0.0             # a gap in the slots: the object stands in slot 3
    world_of = [2, 0, 1]
    targets = [objs[0, 3, :4], objs[1, 0, :4], objs[2, 0, :4]]
    table = _table(gpu_device, worlds, np.array([(0.0, 0.0, 1.0, 1.0)] * 3))
    rooms = _renderer(12, 20, gpu_device)
    h = rooms.geodesic_fields_worlds(table, world_of, objs, targets, 1.0)
    R = S.WORLD_MAX_BOXES + S.WORLD_MAX_OBJECTS
    assert h.n == 3 and h.rects.shape == (3, R, 4) and h.nodes.shape == (3, 4 * R, 2) and h.has_target.all()
    host = []
    for i, w in enumerate(world_of):
        rects = S.inflated_rects(objs[i], S.STEP_MARGIN, worlds[w])
        src = S.goal_viewpoints(targets[i], rects, 1.0)
        nodes, dist = S.geodesic_field_numpy(rects, src)
        host.append((rects, src, nodes, dist))
        assert h.counts[i].cpu().numpy().tolist() == [len(rects), len(nodes)] and len(rects) == len(worlds[w]) + 1 + (i > 0)
        assert int(h.source_counts[i]) == len(src) > 0 and _same_bits(h.sources[i, :len(src)].cpu().numpy(), src)
        g_rects, g_nodes, g_dist = (getattr(h, k)[i].cpu().numpy() for k in ("rects", "nodes", "dist"))
        assert _same_bits(g_rects[:len(rects)], rects) and _same_bits(g_nodes[:len(nodes)], nodes)
        assert np.array_equal(np.isinf(g_dist[:len(nodes)]), np.isinf(dist)) and _same_bits(g_dist[:len(nodes)], dist)
        assert not g_rects[len(rects):].any() and not g_nodes[len(nodes):].any() and np.isinf(g_dist[len(nodes):]).all()
        assert np.isfinite(dist).any()
    # 40 points, some inside rectangles, through the unchanged query
    rng = np.random.default_rng(11)
    pts = np.concatenate([[(0.0, 0.0), (0.0, 1.0), (-2.5, 0.0), gen.start_xy, (9.9, 9.9), (1.5, 0.5)],
                          0.25 * rng.integers(-38, 39, size=(34, 2))])
    field_of = np.arange(40) % 3
    want = np.array([S.geodesic_query_numpy(*host[f], [p])[0] for p, f in zip(pts, field_of)])
    got = rooms.geodesic_distances(h, field_of, pts).cpu().numpy()
    assert _same_bits(got, want) and np.isinf(want).any() and np.isfinite(want).sum() > 10
    # the row that holds BOXES is the existing entry's field
    old = rooms.geodesic_fields(objs[1:2], targets[1:2], 1.0)
    n_r, n_n = old.counts[0].cpu().numpy().tolist()
    assert h.counts[1].cpu().numpy().tolist() == [n_r, n_n]
    assert _same_bits(h.rects[1, :n_r].cpu().numpy(), old.rects[0, :n_r].cpu().numpy())
    assert _same_bits(h.nodes[1, :n_n].cpu().numpy(), old.nodes[0, :n_n].cpu().numpy())
    assert _same_bits(h.dist[1, :n_n].cpu().numpy(), old.dist[0, :n_n].cpu().numpy())
    assert _same_bits(rooms.geodesic_distances(old, np.zeros(40, np.int32), pts).cpu().numpy(),
                      rooms.geodesic_distances(h, np.ones(40, np.int32), pts).cpu().numpy())
    # a row replaced on the device; refusals
    h.assign([0], rooms.geodesic_fields_worlds(table, [1], objs[2:3], targets[2:3], 1.0))
    assert _same_bits(rooms.geodesic_distances(h, [0], [gen.start_xy]).cpu().numpy(),
                      S.geodesic_query_numpy(*host[2], [gen.start_xy]))
    for bad in ([0, 1], [0, 1, 3], [0, -1, 1]):
        with pytest.raises(ValueError):
            rooms.geodesic_fields_worlds(table, bad, objs, targets, 1.0)
    with pytest.raises(RuntimeError, match="LDS"):
        rooms.geodesic_fields_worlds(_table(gpu_device, [small], max_boxes=140), [0], objs[:1], targets[:1], 1.0)
    assert rooms.geodesic_fields_worlds(table, [], objs[:0], np.zeros((0, 4)), 1.0).n == 0


# ------------------------------------------------------------------------------------------------------------------- harness
E, STEPS = 4, 30


def _harness(device, **kw):
    from vlfm_amd.harness import BatchedEpisodes, WorldObjects

    return BatchedEpisodes(E, device=device, use_blip2=False, select_frontiers=True, closed_loop=True,
                           world_objects=WorldObjects(max_episode_steps=12), objectnav_metrics=True,
                           worlds=S.ProceduralWorlds(3), **kw)


def _host_geodesic(h, e):
    rects = S.inflated_rects(h.live.objects[e], S.STEP_MARGIN, h.live.table.world(e))
    box = h.live.objects[e, h.live.target_slot[e], :4]
    src = S.goal_viewpoints(box, rects, h.world_objects.success_distance)
    nodes, dist = S.geodesic_field_numpy(rects, src)
    return S.geodesic_query_numpy(rects, src, nodes, dist, [h.live.xy[e]])[0]


def test_harness_in_procedural_worlds(gpu_device):
    import torch

    a, b = _harness(gpu_device), _harness(gpu_device)
    worlds = S.ProceduralWorlds(3)
    fx = S.camera_intrinsics(a.W)[0]
    assert a.live.world_episode.tolist() == [0] * E and len({a.live.table.world(e).tobytes() for e in range(E)}) == E
    for e in range(E):
        w = worlds.world(a.env_ids[e], 0)
        assert np.array_equal(a.live.table.world(e), w.boxes) and np.array_equal(a.live.xy[e], w.start_xy) and a.live.k[e] == w.start_k
        assert (a.live.target_slot >= 0).all() and a.live.ep_geodesic[e] == _host_geodesic(a, e) and np.isfinite(a.live.ep_geodesic[e])
    moved = 0
    for t in range(STEPS):
        before = [(a.live.xy[e].copy(), int(a.live.k[e]), a.live.table.world(e), a.live.objects[e].copy(), int(a.live.world_episode[e]))
                  for e in range(E)]
        a.step()
        b.step()
        assert np.array_equal(a.last_poses, b.last_poses) and np.array_equal(a.last_world_actions, b.last_world_actions)
        assert np.array_equal(a.live.xy, b.live.xy) and np.array_equal(a.live.k, b.live.k)
        if t in (0, 7, 29):
            torch.cuda.synchronize()
            for e in (0, 3):
                (x, y), k, boxes, objs, _ = before[e]
                c, s = S.HEADINGS[k]
                want = S.render_objects_numpy(x, y, c, s, S.CAMERA_HEIGHT, fx, S.MIN_DEPTH, S.MAX_DEPTH, a.H, a.W,
                                              objs[objs[:, 6] != 0.0, :6], boxes=boxes)
                assert np.array_equal(_bits(a.live.frames[e]), want[0].view(np.int32)), (t, e)
                assert np.array_equal(a.live.ids[e].cpu().numpy(), want[1]), (t, e)
        for e in range(E):
            x, y = a.live.xy[e]
            assert not S._blocked(x, y, S.STEP_MARGIN, boxes=a.live.table.world(e)), (t, e)
            if a.live.world_episode[e] != before[e][4]:              # the episode ended: the NEXT world, from its start
                moved += 1
                w = worlds.world(a.env_ids[e], before[e][4] + 1)
                assert a.live.world_episode[e] == before[e][4] + 1 == a.live.ep_index[e] and a.last_episode_end[e]
                assert not np.array_equal(w.boxes, before[e][2]) and np.array_equal(a.live.table.world(e), w.boxes)
                assert np.array_equal(a.live.xy[e], w.start_xy) and a.live.k[e] == w.start_k and not a.live.collided[e]
                if before[e][4] == 0:
                    assert a.live.ep_geodesic[e] == _host_geodesic(a, e) and a.live.distance_to_goal[e] == a.live.ep_geodesic[e]
    assert moved >= 2 * E                                       # 30 steps, episodes of 12 at the most
    np.testing.assert_equal(a.live.stats, b.live.stats)
    np.testing.assert_equal(a.live.objectnav_stats, b.live.objectnav_stats)
    np.testing.assert_equal(a.live.objectnav_summary(), b.live.objectnav_summary())
    assert a.live.objectnav_summary()["episodes"] >= 2 * E


def test_harness_with_the_map_planner(gpu_device):
    h = _harness(gpu_device, controller=S.MapPlannerController())
    for _ in range(STEPS):
        h.step()
        for e in range(E):
            assert not S._blocked(h.live.xy[e][0], h.live.xy[e][1], S.STEP_MARGIN, boxes=h.live.table.world(e))
    ps = h.planner_stats
    assert np.array_equal(ps["plans"], ps["ok"] + ps["unreachable"] + ps["too_long"] + ps["invalid"])
    assert len(h.live.objectnav_stats["episode_outcome"]) >= 2 * E


@pytest.mark.parametrize("planner", [False, True], ids=["bang_bang", "planner"])
def test_worlds_without_objects_stay_in_episode_zero(gpu_device, planner):
    """No episodes to end: every environment keeps episode 0's world, and past the 12 initial turns the robots walk it."""
    from vlfm_amd.harness import BatchedEpisodes

    h = BatchedEpisodes(2, device=gpu_device, use_blip2=False, select_frontiers=True, closed_loop=True, worlds=S.ProceduralWorlds(3),
                        controller=S.MapPlannerController() if planner else None)
    made = [S.ProceduralWorlds(3).world(e, 0) for e in range(2)]
    assert all(np.array_equal(h.live.xy[e], made[e].start_xy) for e in range(2))
    for t in range(40):
        xy, k = h.live.xy.copy(), h.live.k.copy()
        h.step()
        if t % 13 == 0:
            want = np.stack([S.depth_from_profile(S.wall_profile(xy[e][0], xy[e][1], int(k[e]), h.W, boxes=made[e].boxes), h.H)
                             for e in range(2)])
            assert np.array_equal(_bits(h.live.frames), want.view(np.int32)), t
        for e in range(2):
            assert not S._blocked(h.live.xy[e][0], h.live.xy[e][1], S.STEP_MARGIN, boxes=made[e].boxes), (t, e)
    assert h.live.world_episode.tolist() == [0, 0] and all(np.array_equal(h.live.table.world(e), made[e].boxes) for e in range(2))
    assert h.live.stats["forward_steps"].sum() > 0 and h.live.stats["path_length"].sum() > 0
    if planner:
        ps = h.planner_stats
        assert ps["plans"].sum() > 0 and np.array_equal(ps["plans"], ps["ok"] + ps["unreachable"] + ps["too_long"] + ps["invalid"])
