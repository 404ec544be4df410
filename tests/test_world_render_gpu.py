"""-m gpu: RoomsRenderer.cast_cameras (csrc/world_render.hip, one launch) against the NumPy renderers of vlfm_amd/synthetic.py
(wall_profile / depth_from_profile on the tour, render_objects_numpy for arbitrary cameras), bit for bit."""
import functools

import numpy as np
import pytest

from vlfm_amd import synthetic as S

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _tour():
    return S.integrate(S.plan_actions(S.ROOMS_STEPS))


@functools.lru_cache(maxsize=None)
def _numpy_frames(H, W):
    """(poses, frames [n,H,W] f32) of every 25th pose of the tour and of its initial turns on the spot (headings 1..11:
    with them every heading of the table occurs, whichever the sampled poses miss), rendered in NumPy once per size."""
    poses = _tour()[::25] + _tour()[1:12]
    return poses, np.stack([S.depth_from_profile(S.wall_profile(x, y, k, W), H) for (x, y, k) in poses])


@functools.lru_cache(maxsize=None)
def _renderer(H, W):
    import torch

    from vlfm_amd.harness import RoomsRenderer

    return RoomsRenderer([0], 500, H, W, torch.device("cuda:0"))


def _tfs(poses):
    return np.stack([S.tf_of(x, y, k) for (x, y, k) in poses])


def _same_bits(a, b) -> bool:
    import torch

    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


@pytest.mark.parametrize("H,W", [(480, 640), (50, 70)], ids=["640x480", "70x50"])
def test_equals_the_numpy_renderer_on_the_tour(gpu_device, H, W):
    """Every 25th pose of the tour plus its initial turns on the spot; all 12 headings occur, and headings 0 / 3 / 6 / 9 put an
    exact zero of dx or dy on the centre column (the 1e-12 substitution).  70 x 50 is no multiple of the 4-column lane tile or
    of a row band: the scalar store loop and the tail rows."""
    import torch

    poses, want = _numpy_frames(H, W)
    assert {k for (_, _, k) in poses} == set(range(12))
    got = _renderer(H, W).cast_cameras(_tfs(poses))
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert _same_bits(got, torch.from_numpy(want).to(gpu_device))


@pytest.mark.parametrize("n", [1, 3, 67])
def test_small_odd_size_at_several_batch_sizes(gpu_device, n):
    """70 x 50 at n = 1, 3, 67 cameras: the number of row bands a frame is split into follows n."""
    import torch

    poses, frames = _numpy_frames(50, 70)
    idx = [(7 * i) % len(poses) for i in range(n)]
    got = _renderer(50, 70).cast_cameras(_tfs([poses[i] for i in idx]))
    assert _same_bits(got, torch.from_numpy(frames[idx]).to(gpu_device))


def _rig_like_cameras():
    """Arbitrary (non-table) yaws, per-camera hfov, heights and depth ranges: the rig tests' camera models where they can be
    imported, hand-written ones otherwise, mounted on five robot poses of the tour."""
    try:
        from rig_cases import MODELS_1000

        models = [(f, 0.5, hi) for (f, hi) in MODELS_1000]
    except ImportError:
        models = [(float(np.deg2rad(79.0)), 0.5, 5.0), (float(np.deg2rad(60.0)), 0.5, 2.5), (float(np.deg2rad(100.0)), 0.5, 4.0)]
    models += [(float(np.deg2rad(42.0)), 0.3, 3.5), (float(np.deg2rad(120.0)), 0.05, 9.0)]
    from vlfm_amd.harness import Camera, CameraRig

    rig = CameraRig([Camera(yaw=0.5, hfov=models[0][0], min_depth=models[0][1], max_depth=models[0][2]),
                     Camera(yaw=-0.5, forward=0.1, hfov=models[1][0], min_depth=models[1][1], max_depth=models[1][2]),
                     Camera(yaw=np.pi, left=0.1, up=-0.4, hfov=models[2][0], min_depth=models[2][1], max_depth=models[2][2]),
                     Camera(yaw=1.234567, up=0.3, hfov=models[3][0], min_depth=models[3][1], max_depth=models[3][2]),
                     Camera(yaw=-2.9, forward=-0.05, left=-0.07, hfov=models[4][0], min_depth=models[4][1], max_depth=models[4][2])])
    robots = _tfs(_tour()[40:500:100])                                   # 5 robot poses
    tf = rig.camera_tfs(robots).reshape(-1, 4, 4)                        # 25 cameras
    cam = np.tile(np.arange(5), len(robots))
    return tf, np.array([m[0] for m in models])[cam], np.array([m[1] for m in models])[cam], np.array([m[2] for m in models])[cam]


def _numpy_cameras(H, W, tf, hfov=None, lo=None, hi=None):
    """[n,H,W] f32: render_objects_numpy without objects from each transform; None: the documented defaults (the renderer's
    own optics, 0.5 / 5 m)."""
    n = len(tf)
    fx = np.full(n, S.camera_intrinsics(W)[0]) if hfov is None else W / (2 * np.tan(np.asarray(hfov, np.float64) / 2))
    lo = np.full(n, S.MIN_DEPTH) if lo is None else lo
    hi = np.full(n, S.MAX_DEPTH) if hi is None else hi
    return np.stack([S.render_objects_numpy(t[0, 3], t[1, 3], t[0, 0], t[1, 0], t[2, 3], f, a, b, H, W, [])[0]
                     for t, f, a, b in zip(tf, fx, lo, hi)])


@pytest.mark.parametrize("H,W", [(480, 640), (50, 70)], ids=["640x480", "70x50"])
def test_equals_render_objects_numpy_for_arbitrary_cameras(gpu_device, H, W):
    import torch

    tf, hfov, lo, hi = _rig_like_cameras()
    r = _renderer(H, W)
    want = lambda *a: torch.from_numpy(_numpy_cameras(H, W, tf, *a)).to(gpu_device)   # noqa: E731
    assert _same_bits(r.cast_cameras(tf, hfov, lo, hi), want(hfov, lo, hi))
    # defaults: None means the renderer's own optics and the 0.5 / 5 m range, for each argument on its own
    assert _same_bits(r.cast_cameras(tf), want())
    assert _same_bits(r.cast_cameras(tf, hfov), want(hfov))
    assert _same_bits(r.cast_cameras(tf, None, lo, hi), want(None, lo, hi))


def test_camera_inside_a_box_sees_through_it(gpu_device):
    """A camera inside the hall's north wall segment (-1.4, 4.0)-(1.4, 4.3): that box is transparent (tmin <= 0), everything
    else is seen as usual -- equal to NumPy, and different from the frame an opaque wall at zero distance would give."""
    import torch

    H, W = 50, 70
    x, y = 0.0, 4.15
    assert np.any((S.BOXES[:, 0] < x) & (x < S.BOXES[:, 2]) & (S.BOXES[:, 1] < y) & (y < S.BOXES[:, 3]))
    want = np.stack([S.depth_from_profile(S.wall_profile(x, y, k, W), H) for k in range(12)])
    got = _renderer(H, W).cast_cameras(_tfs([(x, y, k) for k in range(12)]))
    assert _same_bits(got, torch.from_numpy(want).to(gpu_device))
    # heading 9 looks south across the hall: its centre column sees the south wall 8.15 m away (beyond range), not the box around it
    assert float(got[9, 0, W // 2]) == 1.0


def test_camera_outside_the_world_looking_away(gpu_device):
    """(30, 30) heading 1: no column hits anything.  Rows at and above the horizon are exactly 1.0; the floor rows are the floor."""
    import torch

    H, W = 48, 64
    assert np.isinf(S.wall_profile(30.0, 30.0, 1, W)).all()
    got = _renderer(H, W).cast_cameras(_tfs([(30.0, 30.0, 1)]))[0]
    assert bool((got[:H // 2 + 1] == 1.0).all())
    want = S.depth_from_profile(np.full(W, np.inf, np.float32), H)
    assert _same_bits(got, torch.from_numpy(want).to(gpu_device))
    assert float(got[-1].max()) < 1.0         # (the nearest floor row is in range)


def test_out_is_reused_and_checked(gpu_device):
    import torch

    poses, frames = _numpy_frames(50, 70)
    r = _renderer(50, 70)
    out = torch.full((3, 50, 70), -1.0, dtype=torch.float32, device=gpu_device)
    got = r.cast_cameras(_tfs(poses[:3]), out=out)
    assert got.data_ptr() == out.data_ptr() and _same_bits(out, torch.from_numpy(frames[:3]).to(gpu_device))
    # a view that starts 8 bytes into an allocation: rows are no longer 16-byte aligned
    odd = torch.full((2 + 3 * 50 * 72,), -1.0, dtype=torch.float32, device=gpu_device)
    r72 = _renderer(50, 72)
    view = odd[2:].view(3, 50, 72)
    r72.cast_cameras(_tfs(poses[:3]), out=view)
    want = np.stack([S.depth_from_profile(S.wall_profile(x, y, k, 72), 50) for (x, y, k) in poses[:3]])
    assert _same_bits(view, torch.from_numpy(want).to(gpu_device)) and bool((odd[:2] == -1.0).all())
    for bad in (torch.empty((2, 50, 70), dtype=torch.float32, device=gpu_device),
                torch.empty((3, 50, 70), dtype=torch.float64, device=gpu_device),
                torch.empty((3, 50, 140), dtype=torch.float32, device=gpu_device)[:, :, ::2]):
        with pytest.raises(ValueError):
            r.cast_cameras(_tfs(poses[:3]), out=bad)
    with pytest.raises(ValueError):
        r.cast_cameras(_tfs(poses[:3]), None, [0.5, 0.5, 2.0], [5.0, 5.0, 2.0])
    assert r.cast_cameras(np.zeros((0, 4, 4))).shape == (0, 50, 70)


def test_launch_is_ordered_on_the_current_stream(gpu_device):
    """On a side stream, behind work queued there: the frames are rendered into a buffer that a long chain of kernels on the
    same stream fills first, and a copy queued behind the launch on that stream sees the frames."""
    import torch

    poses, frames = _numpy_frames(480, 640)
    r = _renderer(480, 640)
    n = 8
    side = torch.cuda.Stream(gpu_device)
    out = torch.empty((n, 480, 640), dtype=torch.float32, device=gpu_device)
    big = torch.ones((64, 480, 640), dtype=torch.float32, device=gpu_device)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):
            big.mul_(1.0001)
        out.copy_(big[:n])                     # queued BEFORE the launch: must not land after it
        r.cast_cameras(_tfs(poses[:n]), out=out)
        after = out.clone()
    side.synchronize()
    want = torch.from_numpy(frames[:n]).to(gpu_device)
    assert _same_bits(after, want) and _same_bits(out, want)
