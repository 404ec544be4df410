"""-m gpu: RoomsRenderer.cast_cameras_objects (csrc/world_render.hip: vlfm_worlds_raycast with objects, one launch) against the NumPy
statement of its contract (synthetic.render_objects_numpy / object_stats_numpy): depth as bits, ids and stats all equal."""
import functools

import numpy as np
import pytest

from vlfm_amd import synthetic as S
from world_object_cases import EDGES, ENV_OBJECTS, objects_array, poses, reference, render

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _renderer(H, W):
    import torch

    from vlfm_amd.harness import RoomsRenderer

    return RoomsRenderer([0], 500, H, W, torch.device("cuda:0"))


def _tfs(ps):
    return np.stack([S.tf_of(x, y, k) for (x, y, k) in ps])


def _assert_equal(got, want_depth, want_ids, want_stats):
    import torch

    depth, ids, stats = got
    assert depth.dtype == torch.float32 and ids.dtype == torch.uint8 and stats.dtype == torch.int32
    assert np.array_equal(stats.cpu().numpy(), want_stats)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert np.array_equal(depth.contiguous().view(torch.int32).cpu().numpy(), np.ascontiguousarray(want_depth).view(np.int32))


@pytest.mark.parametrize("n", [1, 3, 67])
@pytest.mark.parametrize("H,W", [(480, 640), (50, 70)], ids=["640x480", "70x50"])
def test_equals_the_numpy_renderer(gpu_device, H, W, n):
    """Camera i stands on pose 7 i mod 31 (every 25th pose of the tour and its 11 turns on the spot: all 12 headings, the exact
    zeros of dx / dy) and looks at environment i mod 5, each with other objects (a full set of 8, the contract's edge cases,
    none).  640 x 480 takes the 4-column stores, 70 x 50 the scalar ones and has tail rows; the number of row bands follows n."""
    idx = [(7 * i) % len(poses()) for i in range(n)]
    env = [i % len(ENV_OBJECTS) for i in range(n)]
    if n == 67:
        assert {poses()[i][2] for i in idx} == set(range(12)) and set(env) == set(range(5))
    ref = [reference(p, e, H, W) for p, e in zip(idx, env)]
    got = _renderer(H, W).cast_cameras_objects(_tfs([poses()[i] for i in idx]), objects_array(ENV_OBJECTS), env)
    _assert_equal(got, *(np.stack([r[j] for r in ref]) for j in range(3)))
    if n == 67:
        assert sum(int((r[2][:, 0] > 0).sum()) for r in ref) > 20           # the objects do show


@pytest.mark.parametrize("H,W", [(480, 640), (50, 70)], ids=["640x480", "70x50"])
def test_contract_edges(gpu_device, H, W):
    """Each edge scene of tests/test_world_objects_cpu.py from its own pose, one environment per scene, in one launch."""
    names = sorted(EDGES)
    ref = [render(EDGES[k][0], EDGES[k][1], H, W) for k in names]
    got = _renderer(H, W).cast_cameras_objects(_tfs([EDGES[k][0] for k in names]), objects_array([EDGES[k][1] for k in names]),
                                               np.arange(len(names)))
    _assert_equal(got, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]),
                  np.stack([S.object_stats_numpy(r[1]) for r in ref]))


@pytest.mark.parametrize("H,W", [(480, 640), (50, 70)], ids=["640x480", "70x50"])
def test_without_objects_it_is_cast_cameras(gpu_device, H, W):
    import torch

    tf = _tfs(poses())
    r = _renderer(H, W)
    depth, ids, stats = r.cast_cameras_objects(tf, np.zeros((2, 8, 8)), np.arange(len(tf)) % 2)
    assert torch.equal(depth.view(torch.int32), r.cast_cameras(tf).view(torch.int32))
    assert not bool(ids.any())
    assert np.array_equal(stats.cpu().numpy(), np.tile(np.array([0, W, -1, H, -1], np.int32), (len(tf), 8, 1)))
    # records whose valid flag is 0 are not objects, whatever else they hold
    junk = objects_array([ENV_OBJECTS[2], ENV_OBJECTS[0]])
    junk[:, :, 6] = 0.0
    d2, i2, _ = r.cast_cameras_objects(tf, junk, np.arange(len(tf)) % 2)
    assert torch.equal(d2.view(torch.int32), depth.view(torch.int32)) and not bool(i2.any())


def _rig_like_cameras():
    """The cameras of tests/test_world_render_gpu.py: arbitrary yaws, per-camera hfov, heights and depth ranges on five robot
    poses; here the robots stand in the hall around the objects of ENV_OBJECTS[2] (the ring of 8)."""
    from vlfm_amd.harness import Camera, CameraRig

    models = [(float(np.deg2rad(79.0)), 0.5, 5.0), (float(np.deg2rad(60.0)), 0.5, 2.5), (float(np.deg2rad(100.0)), 0.5, 4.0),
              (float(np.deg2rad(42.0)), 0.3, 3.5), (float(np.deg2rad(120.0)), 0.05, 9.0)]
    rig = CameraRig([Camera(yaw=0.5, hfov=models[0][0], min_depth=models[0][1], max_depth=models[0][2]),
                     Camera(yaw=-0.5, forward=0.1, hfov=models[1][0], min_depth=models[1][1], max_depth=models[1][2]),
                     Camera(yaw=np.pi, left=0.1, up=-0.4, hfov=models[2][0], min_depth=models[2][1], max_depth=models[2][2]),
                     Camera(yaw=1.234567, up=0.3, hfov=models[3][0], min_depth=models[3][1], max_depth=models[3][2]),
                     Camera(yaw=-2.9, forward=-0.05, left=-0.07, hfov=models[4][0], min_depth=models[4][1], max_depth=models[4][2])])
    robots = _tfs([(0.0, 0.0, 0), (0.5, -0.5, 4), (-0.6, 0.3, 7), (0.2, 0.8, 10), (3.4, 2.0, 6)])
    tf = rig.camera_tfs(robots).reshape(-1, 4, 4)
    cam = np.tile(np.arange(5), len(robots))
    return tf, np.array([m[0] for m in models])[cam], np.array([m[1] for m in models])[cam], np.array([m[2] for m in models])[cam]


@pytest.mark.parametrize("H,W", [(480, 640), (50, 70)], ids=["640x480", "70x50"])
def test_arbitrary_cameras(gpu_device, H, W):
    tf, hfov, lo, hi = _rig_like_cameras()
    env = np.arange(len(tf)) % 2
    objs = [ENV_OBJECTS[2], ENV_OBJECTS[1] + ENV_OBJECTS[0]]
    ref = [S.render_objects_numpy(t[0, 3], t[1, 3], t[0, 0], t[1, 0], t[2, 3], W / (2 * np.tan(f / 2)), a, b, H, W, objs[e])
           for t, f, a, b, e in zip(tf, hfov, lo, hi, env)]
    assert sum(int(r[1].any()) for r in ref) >= 10
    got = _renderer(H, W).cast_cameras_objects(tf, objects_array(objs), env, hfov, lo, hi)
    _assert_equal(got, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]),
                  np.stack([S.object_stats_numpy(r[1]) for r in ref]))


def test_out_is_used_and_a_misaligned_one_takes_the_scalar_stores(gpu_device):
    import torch

    idx, env = [0, 21, 20], [0, 2, 1]                      # pose 0 and two of the turns at (0, 0): the objects are in view
    tf, objs = _tfs([poses()[i] for i in idx]), objects_array(ENV_OBJECTS)
    want = [np.stack([reference(p, e, 50, 72)[j] for p, e in zip(idx, env)]) for j in range(3)]
    assert (want[2][:, :, 0] > 0).any()
    r = _renderer(50, 72)
    out = torch.full((3, 50, 72), -1.0, dtype=torch.float32, device=gpu_device)
    got = r.cast_cameras_objects(tf, objs, env, out=out)
    assert got[0].data_ptr() == out.data_ptr()
    _assert_equal(got, *want)
    # a view that starts 8 bytes into an allocation: rows are no longer 16-byte aligned
    odd = torch.full((2 + 3 * 50 * 72,), -1.0, dtype=torch.float32, device=gpu_device)
    view = odd[2:].view(3, 50, 72)
    _assert_equal(r.cast_cameras_objects(tf, objs, env, out=view), *want)
    assert bool((odd[:2] == -1.0).all())
    for bad in (torch.empty((2, 50, 72), dtype=torch.float32, device=gpu_device),
                torch.empty((3, 50, 72), dtype=torch.float64, device=gpu_device),
                torch.empty((3, 50, 144), dtype=torch.float32, device=gpu_device)[:, :, ::2]):
        with pytest.raises(ValueError):
            r.cast_cameras_objects(tf, objs, env, out=bad)
    for bad_env in ([0, 1, 5], [0, -1, 1], [0, 1]):
        with pytest.raises(ValueError):
            r.cast_cameras_objects(tf, objs, bad_env)
    with pytest.raises(ValueError):
        r.cast_cameras_objects(tf, np.zeros((5, 7, 8)), env)
    d0, i0, s0 = r.cast_cameras_objects(np.zeros((0, 4, 4)), objs, [])
    assert d0.shape == (0, 50, 72) and i0.shape == (0, 50, 72) and s0.shape == (0, 8, 5)


def test_launch_is_ordered_on_the_current_stream(gpu_device):
    """On a side stream, behind a chain of kernels that fills the output buffer on that stream first."""
    import torch

    n = 8
    idx, env = [(7 * i) % len(poses()) for i in range(n)], [i % 5 for i in range(n)]
    want = [np.stack([reference(p, e, 480, 640)[j] for p, e in zip(idx, env)]) for j in range(3)]
    r = _renderer(480, 640)
    side = torch.cuda.Stream(gpu_device)
    out = torch.empty((n, 480, 640), dtype=torch.float32, device=gpu_device)
    big = torch.ones((64, 480, 640), dtype=torch.float32, device=gpu_device)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):
            big.mul_(1.0001)
        out.copy_(big[:n])                     # queued BEFORE the launch: must not land after it
        _, ids, stats = r.cast_cameras_objects(_tfs([poses()[i] for i in idx]), objects_array(ENV_OBJECTS), env, out=out)
        after = out.clone()
    side.synchronize()
    _assert_equal((after, ids, stats), *want)
    _assert_equal((out, ids, stats), *want)


def test_a_geometry_beyond_the_lds_budget_is_refused(gpu_device):
    """1280 columns need 8 x 8 bytes each for the object entries alone: more than the 64 KB the kernel supports."""
    import torch

    r = _renderer(16, 1280)
    out = torch.full((1, 16, 1280), -1.0, dtype=torch.float32, device=gpu_device)
    with pytest.raises(RuntimeError, match="LDS"):
        r.cast_cameras_objects(_tfs(poses()[:1]), objects_array(ENV_OBJECTS), [0], out=out)
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    # the walls-only entry still renders that width
    assert r.cast_cameras(_tfs(poses()[:1])).shape == (1, 16, 1280)
