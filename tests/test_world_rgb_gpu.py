"""-m gpu: the camera's RGB view of the synthetic worlds (vlfm_worlds_raycast with d_rgb through RoomsRenderer.cast_worlds_rgb /
cast_cameras_rgb) against the host statement synthetic.render_rgb_numpy, byte for byte, and BatchedEpisodes(render_rgb=True)."""
import numpy as np
import pytest

from vlfm_amd import synthetic as S
from world_object_cases import objects_array
from world_rgb_cases import ENV_OF, PALETTE, SIZES, SIZE_IDS, WORLD_OF, cameras, colours, kinds, objects, poison, reference, worlds

pytestmark = pytest.mark.gpu


def _bits(t):
    import torch

    return t.contiguous().view(torch.int32).cpu().numpy()


def _table(device, list_of_boxes, tails=None, max_boxes=S.WORLD_MAX_BOXES):
    import torch

    from vlfm_amd.harness import WorldTable

    table = WorldTable(len(list_of_boxes), device, max_boxes)
    table.assign(np.arange(len(list_of_boxes)), list_of_boxes)
    if tails is not None:                          # behind the wrapper's back: the rows beyond each count, on the device only
        d = table.d_boxes.cpu().numpy()
        for w, b in enumerate(list_of_boxes):
            d[w, len(b):] = tails[w]
        table.d_boxes.copy_(torch.from_numpy(d))
    return table


def _renderer(H, W, device):
    from vlfm_amd.harness import RoomsRenderer

    return RoomsRenderer([0], 500, H, W, device)


def _assert_frames(got, want):
    depth, ids, stats, rgb = got
    assert np.array_equal(stats.cpu().numpy(), want[2])
    assert np.array_equal(ids.cpu().numpy(), want[1])
    assert np.array_equal(_bits(depth), np.ascontiguousarray(want[0]).view(np.int32))
    g = rgb.cpu().numpy()
    assert g.shape == want[3].shape and g.dtype == np.uint8
    assert np.array_equal(g, want[3]), np.argwhere((g != want[3]).any(axis=-1))[:8].tolist()


@pytest.mark.parametrize("tails", ["nan", "box"])
@pytest.mark.parametrize("H,W", SIZES, ids=SIZE_IDS)
def test_kernel_equals_the_statement(gpu_device, H, W, tails):
    want = reference(H, W)
    kind, skirting, odd, yface = kinds(H, W)       # the reference is no blank frame: every kind of pixel is in it
    assert all((kind == k).any() for k in range(4)) and skirting.any()
    assert all((kind == 1)[m].any() for m in (odd, ~odd, yface, ~yface)) and all((kind == 3)[m].any() for m in (yface, ~yface))
    assert len({f.tobytes() for f in want[3]}) == 7
    tf, hfov, lo, hi = cameras()
    table = _table(gpu_device, worlds()[0], poison(tf) if tails == "box" else None)
    r = _renderer(H, W, gpu_device)
    objs = objects_array(objects())
    got = r.cast_worlds_rgb(tf, table, WORLD_OF, objs, ENV_OF, colours(), PALETTE, hfov, lo, hi)
    _assert_frames(got, want)
    old = r.cast_worlds(tf, table, WORLD_OF, objs, ENV_OF, hfov, lo, hi)            # one launch gives the step everything
    assert np.array_equal(_bits(got[0]), _bits(old[0])) and (got[1] == old[1]).all() and (got[2] == old[2]).all()


def test_unaligned_outputs_take_the_byte_path(gpu_device):
    """Views 8 bytes into a depth allocation and 1 byte into a colour allocation; nothing is written outside them."""
    import torch

    H, W = 12, 20
    tf, hfov, lo, hi = cameras()
    r = _renderer(H, W, gpu_device)
    depth = torch.full((2 + 7 * H * W,), -1.0, dtype=torch.float32, device=gpu_device)
    rgb = torch.full((1 + 7 * H * W * 3 + 3,), 77, dtype=torch.uint8, device=gpu_device)
    got = r.cast_worlds_rgb(tf, _table(gpu_device, worlds()[0]), WORLD_OF, objects_array(objects()), ENV_OF, colours(), PALETTE, hfov,
                            lo, hi, out=depth[2:].view(7, H, W), rgb_out=rgb[1:-3].view(7, H, W, 3))
    assert got[3].data_ptr() == rgb.data_ptr() + 1
    _assert_frames(got, reference(H, W))
    assert bool((depth[:2] == -1.0).all()) and int(rgb[0]) == 77 and bool((rgb[-3:] == 77).all())


def test_rooms_world_is_a_table_of_one_row(gpu_device):
    """cast_cameras_rgb: BOXES as the only world; default palette; no objects at all."""
    H, W = 48, 64
    tf, hfov, lo, hi = cameras()
    r = _renderer(H, W, gpu_device)
    objs, col = objects_array(objects()), colours()
    got = r.cast_cameras_rgb(tf, objs, ENV_OF, col, None, hfov, lo, hi)
    old = r.cast_cameras_objects(tf, objs, ENV_OF, hfov, lo, hi)
    assert np.array_equal(_bits(got[0]), _bits(old[0])) and (got[1] == old[1]).all() and (got[2] == old[2]).all()
    rgb = got[3].cpu().numpy()
    for i in (1, 3, 6):
        t = tf[i]
        want = S.render_rgb_numpy(t[0, 3], t[1, 3], t[0, 0], t[1, 0], t[2, 3], W / (2 * np.tan(hfov[i] / 2)), lo[i], hi[i], H, W,
                                  objects()[ENV_OF[i]], col[ENV_OF[i]][:len(objects()[ENV_OF[i]])])
        assert np.array_equal(rgb[i], want[2]), i
    bare = r.cast_cameras_rgb(tf[:2])
    assert not bool(bare[1].any()) and bool((bare[2].cpu().numpy() == [0, W, -1, H, -1]).all())
    t = tf[1]
    want = S.render_rgb_numpy(t[0, 3], t[1, 3], t[0, 0], t[1, 0], t[2, 3], S.camera_intrinsics(W)[0], S.MIN_DEPTH, S.MAX_DEPTH, H, W,
                              [], [])
    assert np.array_equal(bare[3][1].cpu().numpy(), want[2]) and np.array_equal(_bits(bare[0][1]), want[0].view(np.int32))


def test_frames_do_not_depend_on_the_band_height(gpu_device):
    """One camera 600 times in one call (bands of 24 rows) and once alone (bands of 4 rows): 601 equal frames."""
    H, W = 48, 64
    tf, hfov, lo, hi = cameras()
    i = 5
    r = _renderer(H, W, gpu_device)
    table = _table(gpu_device, worlds()[0])
    objs, col = objects_array(objects()), colours()
    rep = lambda a, n: np.repeat(np.asarray(a)[i:i + 1], n, axis=0)   # noqa: E731
    many = r.cast_worlds_rgb(rep(tf, 600), table, rep(WORLD_OF, 600), objs, rep(ENV_OF, 600), col, PALETTE, rep(hfov, 600),
                             rep(lo, 600), rep(hi, 600))
    one = r.cast_worlds_rgb(rep(tf, 1), table, rep(WORLD_OF, 1), objs, rep(ENV_OF, 1), col, PALETTE, rep(hfov, 1), rep(lo, 1),
                            rep(hi, 1))
    want = reference(H, W)
    _assert_frames(one, tuple(w[i:i + 1] for w in want))
    for a, b in zip(many, one):
        assert bool((a == b).all())                                   # [600, ...] against [1, ...]


def test_arguments_are_checked_before_any_launch(gpu_device):
    import torch

    H, W = 12, 20
    tf, hfov, lo, hi = cameras()
    r = _renderer(H, W, gpu_device)
    table = _table(gpu_device, worlds()[0])
    objs, col = objects_array(objects()), colours()
    out = torch.full((7, H, W), -1.0, dtype=torch.float32, device=gpu_device)
    rgb = torch.full((7, H, W, 3), 9, dtype=torch.uint8, device=gpu_device)
    good = dict(tf=tf, table=table, world_of=WORLD_OF, objects=objs, env_of=ENV_OF, colours=col, palette=PALETTE, out=out, rgb_out=rgb)
    cpu_table = _table("cpu", worlds()[0])                           # a table on another device
    bad = [dict(world_of=WORLD_OF[:6]), dict(world_of=[4] + WORLD_OF[1:]), dict(world_of=[-1] + WORLD_OF[1:]),
           dict(table=cpu_table), dict(objects=objs[:, :7]), dict(env_of=[3] + ENV_OF[1:]), dict(env_of=ENV_OF[:3]),
           dict(colours=col[:2]), dict(colours=col.astype(np.float64)), dict(palette=PALETTE[:11]),
           dict(objects=None), dict(max_depth=lo, min_depth=hi),
           dict(out=torch.empty((7, H, W), dtype=torch.float64, device=gpu_device)),
           dict(rgb_out=torch.empty((7, H, W, 4), dtype=torch.uint8, device=gpu_device)),
           dict(rgb_out=torch.empty((7, H, W, 3), dtype=torch.uint8)),
           dict(rgb_out=torch.empty((7, H, 2 * W, 3), dtype=torch.uint8, device=gpu_device)[:, :, ::2])]
    for kw in bad:
        with pytest.raises(ValueError):
            r.cast_worlds_rgb(**{**good, **kw})
    big = _table(gpu_device, worlds()[0], max_boxes=2100)            # 2100 * 32 bytes of boxes alone: beyond 64 KB of LDS
    with pytest.raises(RuntimeError, match="LDS"):
        r.cast_worlds_rgb(**{**good, "table": big})
    torch.cuda.synchronize()
    assert bool((out == -1.0).all()) and bool((rgb == 9).all())       # nothing was launched
    none = r.cast_worlds_rgb(np.zeros((0, 4, 4)), table, [])
    assert none[0].shape == (0, H, W) and none[3].shape == (0, H, W, 3)
    _assert_frames(r.cast_worlds_rgb(hfov=hfov, min_depth=lo, max_depth=hi, **good), reference(H, W))


# ------------------------------------------------------------------------------------------------------------------- harness
E, STEPS, HH, WW = 4, 6, 48, 64


def _ring_layout(env_id, episode, robot_xy):
    """Three objects 1.6 m around the robot, the environment's target class first: whichever way it turns, one is in view."""
    classes = list(S.OBJECT_SIZES)
    return [(classes[(env_id + j) % 6], S.object_box(classes[(env_id + j) % 6], robot_xy[0] + 1.6 * np.cos(a), robot_xy[1] + 1.6 * np.sin(a)))
            for j, a in enumerate((0.3 + episode, 2.4 + episode, 4.5 + episode))]


def _harness(device, **kw):
    from vlfm_amd.harness import BatchedEpisodes, WorldObjects

    return BatchedEpisodes(E, device=device, height=HH, width=WW, use_blip2=False, select_frontiers=True, closed_loop=True,
                           world_objects=WorldObjects(max_episode_steps=4, min_pixels=40, layout=_ring_layout),
                           worlds=S.ProceduralWorlds(0), **kw)


def _statement(h, e, x, y, k, boxes, objs, classes):
    c, s = S.HEADINGS[k]
    valid = objs[:, 6] != 0.0
    assert valid[:len(classes)].all() and not valid[len(classes):].any()
    return S.render_rgb_numpy(x, y, c, s, S.CAMERA_HEIGHT, S.camera_intrinsics(h.W)[0], S.MIN_DEPTH, S.MAX_DEPTH, h.H, h.W,
                              objs[valid, :6], [S.OBJECT_COLOURS[c] for c in classes], boxes=boxes)


def test_harness_renders_what_the_robot_sees(gpu_device):
    """Every step's live.rgb is the statement at that step's poses, layouts and worlds; and nothing else changes: with stub
    cosines and without a detector nothing downstream reads the colours."""
    import torch

    a, b = _harness(gpu_device, render_rgb=True), _harness(gpu_device)
    assert b.live.rgb is None and not b.render_rgb
    objects_seen = episodes = 0
    for t in range(STEPS):
        before = [(a.live.xy[e].copy(), int(a.live.k[e]), a.live.table.world(e), a.live.objects[e].copy(), list(a.live.object_classes[e]))
                  for e in range(E)]
        a.step()
        b.step()
        torch.cuda.synchronize()
        rgb = a.live.rgb.cpu().numpy()
        assert rgb.shape == (E, HH, WW, 3)
        for e in range(E):
            (x, y), k, boxes, objs, classes = before[e]
            want = _statement(a, e, x, y, k, boxes, objs, classes)
            assert np.array_equal(rgb[e], want[2]), (t, e)
            assert np.array_equal(_bits(a.live.frames[e]), want[0].view(np.int32)) and np.array_equal(a.live.ids[e].cpu().numpy(), want[1])
            objects_seen += int((want[1] > 0).sum())
        episodes += int(a.last_episode_end.sum())
        assert np.array_equal(a.last_poses, b.last_poses) and np.array_equal(a.last_world_actions, b.last_world_actions)
        assert np.array_equal(a.live.xy, b.live.xy) and np.array_equal(a.live.k, b.live.k)
        assert np.array_equal(_bits(a.live.frames), _bits(b.live.frames)) and bool((a.live.ids == b.live.ids).all())
        assert np.array_equal(a.live.seen_stats, b.live.seen_stats)
    assert objects_seen > 0 and episodes >= E                          # objects were in view; every world was left for the next
    for name in ("obstacle_bits", "navigable_bits", "explored_bits"):
        assert torch.equal(getattr(a.obstacles, name), getattr(b.obstacles, name)), name
    assert torch.equal(a.values.conf.view(torch.int32), b.values.conf.view(torch.int32))
    assert torch.equal(a.values.value.view(torch.int64), b.values.value.view(torch.int64))
    np.testing.assert_equal(a.live.stats, b.live.stats)
    np.testing.assert_equal(a.live.objectnav_stats, b.live.objectnav_stats)
    assert a.live.objectnav_stats["episodes"].sum() >= E


@pytest.mark.parametrize("mode", ["rooms", "rooms_objects", "worlds"])
def test_harness_other_worlds(gpu_device, mode):
    """The rooms world with and without objects, and procedural worlds without objects: two steps each."""
    import torch

    from vlfm_amd.harness import BatchedEpisodes, WorldObjects

    kw = dict(rooms={}, rooms_objects=dict(world_objects=WorldObjects()), worlds=dict(worlds=S.ProceduralWorlds(0)))[mode]
    h = BatchedEpisodes(2, device=gpu_device, height=HH, width=WW, use_blip2=False, select_frontiers=True, closed_loop=True,
                        render_rgb=True, **kw)
    for t in range(2):
        xy, k = h.live.xy.copy(), h.live.k.copy()
        h.step()
        torch.cuda.synchronize()
        for e in range(2):
            boxes = h.live.table.world(e) if mode == "worlds" else None
            objs = h.live.objects[e] if mode == "rooms_objects" else np.zeros((8, 8))
            classes = h.live.object_classes[e] if mode == "rooms_objects" else []
            want = _statement(h, e, xy[e][0], xy[e][1], int(k[e]), boxes, objs, classes)
            assert np.array_equal(h.live.rgb[e].cpu().numpy(), want[2]), (t, e)
            assert np.array_equal(_bits(h.live.frames[e]), want[0].view(np.int32)), (t, e)


def test_transport_hop_sees_the_rendered_frames(gpu_device):
    """emulate_jpeg=True: the transported frames are Pillow's q90 round trip of live.rgb.  jpeg_roundtrip_batch takes any frame
    size; 16 x 16 -- one MCU of the 4:2:0 coder, a width the depth ingest takes -- is the smallest the harness can step."""
    import torch

    from vlfm_amd.harness import BatchedEpisodes, WorldObjects
    from vlfm_amd.vlm.transport import jpeg_roundtrip

    h = BatchedEpisodes(E, device=gpu_device, height=16, width=16, use_blip2=False, select_frontiers=True, closed_loop=True,
                        world_objects=WorldObjects(), worlds=S.ProceduralWorlds(0), render_rgb=True, emulate_jpeg=True)
    frames = set()
    for _ in range(2):
        h.step()
        torch.cuda.synchronize()
        rgb, sent = h.live.rgb.cpu().numpy(), h.jpeg_frames.cpu().numpy()
        for e in range(E):
            assert np.array_equal(sent[e], jpeg_roundtrip(rgb[e], 90)), e
            frames.add(rgb[e].tobytes())
        assert len(np.unique(rgb.reshape(-1, 3), axis=0)) > 8          # a picture, not a flat colour
    assert len(frames) > E


def test_refusals():
    from vlfm_amd.harness import BatchedEpisodes, Camera, CameraRig

    with pytest.raises(ValueError, match="closed_loop"):
        BatchedEpisodes(2, use_blip2=False, select_frontiers=True, render_rgb=True)
    with pytest.raises(ValueError, match="rig"):
        BatchedEpisodes(2, use_blip2=False, select_frontiers=True, closed_loop=True, render_rgb=True, rig=CameraRig([Camera()]))
