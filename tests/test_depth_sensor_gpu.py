"""-m gpu: the depth sensor on the device (vlfm_depth_sensor through RoomsRenderer.sense_depth, LiveWorld(depth_sensor=...) and
BatchedEpisodes(depth_sensor=...)) against the host statement synthetic.depth_sensor_numpy, bit for bit."""
import functools

import numpy as np
import pytest

import vlfm_amd.synthetic as S

pytestmark = pytest.mark.gpu

ENV_IDS = [3, 0, 11]
CLOCKS = [0, 7, 2 ** 32 + 5]                  # (taken modulo 2**32)
LO = np.array([0.5, 0.3, 0.05])
HI = np.array([5.0, 3.5, 9.0])
SENSORS = {
    "none": S.DepthSensor(seed=8),
    "noise": S.DepthSensor(seed=1, sigma0_m=0.004, sigma2_per_m=0.003),
    "quantise": S.DepthSensor(seed=2, disparity_k=35.0),
    "dropout": S.DepthSensor(seed=3, dropout=0.05),
    "patch": S.DepthSensor(seed=4, patch_dropout=0.15),
    "edge": S.DepthSensor(seed=5, edge_m=0.3),
    "range": S.DepthSensor(seed=6, min_range_m=0.6, max_range_m=4.5),
    "all": S.DepthSensor(seed=7, sigma0_m=0.004, sigma2_per_m=0.003, disparity_k=35.0, dropout=0.05, patch_dropout=0.15, edge_m=0.3,
                         min_range_m=0.6, max_range_m=4.5),
}


@functools.lru_cache(maxsize=None)
def _clean(H, W):
    """Three frames of the rooms world with a chair in view (one per camera range), with a NaN, 1e-3 and 1.0 poked into each --
    in a corner, at a row's end and next to each other, where the edge stage looks across them."""
    poses = [(0.6, 2.0, 1.0, 0.0), (3.4, 2.0, 0.0, 1.0), (0.0, 0.0, S.HEADINGS[1][0], S.HEADINGS[1][1])]
    chairs = [(2.0, 2.0), (3.4, 3.2), (1.2, 0.7)]
    out = np.stack([S.render_objects_numpy(x, y, c, s, S.CAMERA_HEIGHT, S.camera_intrinsics(W)[0], lo, hi, H, W,
                                           [S.object_box("chair", *chair)])[0]
                    for (x, y, c, s), chair, lo, hi in zip(poses, chairs, LO, HI)])
    out[:, 0, 0], out[:, 1, W - 1], out[:, H - 1, 0] = np.nan, 1.0, 1e-3
    out[:, H // 2, W // 2:W // 2 + 3] = (1e-3, np.nan, 1.0)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(H, W, name):
    made = [S.depth_sensor_numpy(f, lo, hi, SENSORS[name], e, c) for f, lo, hi, e, c in zip(_clean(H, W), LO, HI, ENV_IDS, CLOCKS)]
    frames, counts = np.stack([m[0] for m in made]), np.array([m[1] for m in made], np.int32)
    frames.setflags(write=False)
    return frames, counts


@functools.lru_cache(maxsize=None)
def _renderer(H, W):
    import torch

    from vlfm_amd.harness import RoomsRenderer

    return RoomsRenderer([0], 8, H, W, torch.device("cuda:0"))


def _bits(t):
    import torch

    return t.contiguous().view(torch.int32).cpu().numpy()


def _assert_frames(got, want, what=None):
    assert np.array_equal(_bits(got), np.ascontiguousarray(want).view(np.int32)), what


def _sense(r, clean, name, **kw):
    return r.sense_depth(clean, SENSORS[name], ENV_IDS, CLOCKS, LO, HI, **kw)


@pytest.mark.parametrize("H, W, band_rows", [(12, 20, 0), (9, 18, 0), (48, 64, 0), (48, 64, 1), (48, 64, 5), (48, 64, 48)])
def test_equals_the_statement(gpu_device, H, W, band_rows):
    """Each stage alone, all together and none, at three frames per call: 20 x 12, 18 x 9 (no multiple of 4: the scalar path),
    64 x 48 in planned bands, with a seam on every row, seams off the 8-row blocks, and as a single band."""
    import torch

    r = _renderer(H, W)
    clean = torch.from_numpy(_clean(H, W).copy()).to(gpu_device)
    for name in SENSORS:
        want, counts = _reference(H, W, name)
        out, invalid = _sense(r, clean, name, band_rows=band_rows)
        assert out.shape == clean.shape and invalid.dtype == torch.int32 and out.data_ptr() != clean.data_ptr()
        _assert_frames(out, want, name)
        assert np.array_equal(invalid.cpu().numpy(), counts), name
        assert (counts.sum() > 0) == (name not in ("none", "noise", "quantise")), name
    _assert_frames(clean, _clean(H, W))                                      # the input is read only
    _assert_frames(_sense(r, clean, "none")[0], _clean(H, W))                # every stage off: out == clean, NaN included


def test_everything_on_at_640x480(gpu_device):
    import torch

    H, W = 480, 640
    want, counts = _reference(H, W, "all")
    out, invalid = _sense(_renderer(H, W), torch.from_numpy(_clean(H, W).copy()).to(gpu_device), "all")
    _assert_frames(out, want)
    assert np.array_equal(invalid.cpu().numpy(), counts) and 0 < counts.min() and counts.max() < H * W


def test_out_invalid_out_unaligned_views_and_a_side_stream(gpu_device):
    import torch

    H, W = 48, 64
    r = _renderer(H, W)
    want, counts = _reference(H, W, "all")
    n = 3 * H * W
    # views 4 and 12 bytes into their allocations (the scalar loads and stores), guard floats on both sides of both
    src = torch.full((n + 2,), -3.0, dtype=torch.float32, device=gpu_device)
    dst = torch.full((n + 6,), -5.0, dtype=torch.float32, device=gpu_device)
    src[1:n + 1] = torch.from_numpy(_clean(H, W).copy()).to(gpu_device).reshape(-1)
    clean, out = src[1:n + 1].view(3, H, W), dst[3:n + 3].view(3, H, W)
    invalid = torch.full((5,), -9, dtype=torch.int32, device=gpu_device)
    got = _sense(r, clean, "all", out=out, invalid_out=invalid[1:4])
    assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == invalid[1:4].data_ptr()
    _assert_frames(out, want)
    assert invalid.cpu().numpy().tolist() == [-9] + counts.tolist() + [-9]
    assert bool((dst[:3] == -5.0).all()) and bool((dst[n + 3:] == -5.0).all())
    assert bool((src[0] == -3.0)) and bool((src[n + 1] == -3.0))
    _assert_frames(clean, _clean(H, W))
    # an aligned input into a misaligned output and the other way round
    aligned = clean.clone()
    _assert_frames(_sense(r, aligned, "all", out=out)[0], want)
    _assert_frames(_sense(r, clean, "all", out=torch.empty_like(aligned))[0], want)
    # a side stream: work queued before the launch lands before it
    side = torch.cuda.Stream(gpu_device)
    big = torch.ones((64, 480, 640), dtype=torch.float32, device=gpu_device)
    fresh = torch.empty_like(aligned)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):
            big.mul_(1.0001)
        fresh.copy_(big[:3, :H, :W])
        got = _sense(r, aligned, "all", out=fresh)
        after = (fresh.clone(), got[1].clone())
    side.synchronize()
    _assert_frames(after[0], want)
    assert np.array_equal(after[1].cpu().numpy(), counts)


def _raw(lib, clean, out, n, H, W, keys, rng, invalid, stream, band_rows=0, sigma0=0.0, edge=0.3, max_range=float("inf"), drop=1 << 28):
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    return lib.vlfm_depth_sensor(ptr(clean), ptr(out), n, H, W, ptr(keys), ptr(rng), sigma0, 0.0, 0.0, drop, 0, edge, 0.0, max_range,
                                 ptr(invalid), band_rows, stream)


def test_no_frames_and_the_optional_count(gpu_device):
    import torch

    from vlfm_amd import _lib as L

    H, W = 9, 18
    r = _renderer(H, W)
    out, invalid = r.sense_depth(torch.empty((0, H, W), dtype=torch.float32, device=gpu_device), SENSORS["all"], [], [])
    assert out.shape == (0, H, W) and invalid.shape == (0,)
    st = torch.cuda.current_stream().cuda_stream
    assert _raw(L.lib(), None, None, 0, H, W, None, None, None, st) == L.VLFM_OK
    # d_invalid == NULL: the frames all the same
    sensor = S.DepthSensor(seed=3, dropout=1 / 16, edge_m=0.3)
    assert sensor.thresholds() == (1 << 28, 0)
    clean = torch.from_numpy(_clean(H, W).copy()).to(gpu_device)
    keys = torch.from_numpy(sensor.frame_keys(ENV_IDS, CLOCKS).view(np.int32)).to(gpu_device)
    rng = torch.from_numpy(np.stack([LO, HI], axis=1).astype(np.float32)).to(gpu_device)
    got = torch.full_like(clean, -1.0)
    assert _raw(L.lib(), clean, got, 3, H, W, keys, rng, None, st) == L.VLFM_OK, L.last_error()
    want = [S.depth_sensor_numpy(f, lo, hi, sensor, e, c)[0] for f, lo, hi, e, c in zip(_clean(H, W), LO, HI, ENV_IDS, CLOCKS)]
    _assert_frames(got, np.stack(want))
    assert L.lib().vlfm_abi_version() >= 27


def test_refusals_leave_the_outputs_untouched(gpu_device):
    import torch

    from vlfm_amd import _lib as L

    H, W = 9, 18
    r = _renderer(H, W)
    clean = torch.from_numpy(_clean(H, W).copy()).to(gpu_device)
    out = torch.full_like(clean, -1.0)
    invalid = torch.full((3,), -7, dtype=torch.int32, device=gpu_device)
    keys = torch.zeros(3, dtype=torch.int32, device=gpu_device)
    rng = torch.from_numpy(np.stack([LO, HI], axis=1).astype(np.float32)).to(gpu_device)
    st = torch.cuda.current_stream().cuda_stream
    both = torch.cat([clean.reshape(-1), clean.reshape(-1)])
    first, shifted = both[:clean.numel()].view(3, H, W), both[H * W:H * W + clean.numel()].view(3, H, W)   # two frames in common
    nan = float("nan")
    for kw in (dict(clean=None), dict(out=None), dict(keys=None), dict(rng=None), dict(n=-1), dict(n=65536), dict(H=0), dict(W=0),
               dict(H=-4), dict(H=1 << 16, W=1 << 15), dict(band_rows=-1), dict(out=clean), dict(clean=first, out=shifted),
               dict(clean=shifted, out=first), dict(sigma0=-1.0), dict(sigma0=nan), dict(sigma0=float("inf")), dict(edge=-0.5),
               dict(edge=nan), dict(max_range=-1.0), dict(max_range=nan)):
        args = dict(clean=clean, out=out, n=3, H=H, W=W, keys=keys, rng=rng, invalid=invalid, stream=st)
        args.update(kw)
        assert _raw(L.lib(), **args) == L.VLFM_ERR_INVALID, kw
    torch.cuda.synchronize()
    assert bool((out == -1.0).all()) and bool((invalid == -7).all())
    _assert_frames(both[:clean.numel()].view(3, H, W), _clean(H, W))
    _assert_frames(both[clean.numel():].view(3, H, W), _clean(H, W))
    # sense_depth: everything before the launch
    sensor, ok = SENSORS["all"], dict(env_ids=ENV_IDS, clocks=CLOCKS)
    cpu = clean.cpu()
    for kw in (dict(clean=clean.double()), dict(clean=clean[:, :, :16]), dict(clean=clean[:, :8]), dict(clean=clean[0]),
               dict(clean=clean.transpose(1, 2).contiguous().transpose(1, 2)), dict(clean=cpu), dict(clean=clean.cpu().numpy()),
               dict(sensor=None), dict(sensor=dict(dropout=0.1)), dict(env_ids=[0, 1]), dict(clocks=[0, 1, 2, 3]),
               dict(env_ids=[0.5, 1.0, 2.0]), dict(min_depth=[0.5, 0.5, 5.0], max_depth=[5.0, 5.0, 5.0]), dict(band_rows=-2),
               dict(out=clean), dict(out=shifted, clean=first), dict(out=out.double()), dict(out=out[:2]), dict(out=out.cpu()),
               dict(out=out.transpose(1, 2).contiguous().transpose(1, 2)), dict(invalid_out=invalid[:2]),
               dict(invalid_out=invalid.long()), dict(invalid_out=invalid.cpu()),
               dict(invalid_out=torch.zeros(6, dtype=torch.int32, device=gpu_device)[::2])):
        args = dict(clean=clean, sensor=sensor, out=out, invalid_out=invalid, **ok)
        args.update(kw)
        with pytest.raises(ValueError):
            r.sense_depth(**args)
    torch.cuda.synchronize()
    assert bool((out == -1.0).all()) and bool((invalid == -7).all())
    got = r.sense_depth(clean, sensor, ENV_IDS, CLOCKS, LO, HI, out=out, invalid_out=invalid)      # the same call unrefused
    _assert_frames(got[0], _reference(H, W, "all")[0])
    assert np.array_equal(invalid.cpu().numpy(), _reference(H, W, "all")[1])


# ------------------------------------------------------------------------------------------------------------------ LiveWorld
E, STEPS, HH, WW = 4, 6, 48, 64
LIVE_SENSOR = S.DepthSensor(seed=1, sigma0_m=0.002, sigma2_per_m=0.002, dropout=0.01, edge_m=0.3)
_F, _L, _R = S.ACTION_FORWARD, S.ACTION_TURN_LEFT, S.ACTION_TURN_RIGHT
PATTERN = [_F, _L, _F, _F, _R, _F, _R, _F]


def _ring_layout(env_id, episode, robot_xy):
    """Three objects 1.6 m around the robot, the environment's target class first: whichever way it turns, one is in view."""
    classes = list(S.OBJECT_SIZES)
    return [(classes[(env_id + j) % 6], S.object_box(classes[(env_id + j) % 6], robot_xy[0] + 1.6 * np.cos(a), robot_xy[1] + 1.6 * np.sin(a)))
            for j, a in enumerate((0.3 + episode, 2.4 + episode, 4.5 + episode))]


def _grid_worlds():
    plans = []
    for wall in (12, 27):                     # two 40 x 40 plans of 0.25 m cells over [-5, 5]^2: the border and one inner wall
        occ = np.zeros((40, 40), bool)
        occ[[0, -1]], occ[:, [0, -1]] = True, True
        occ[wall, 5:30] = True
        plans.append(S.GridPlan.uniform(occ, 4, -20, -20))
    return S.GridWorlds(plans, starts=[(0.0, 0.0, 0), (0.5, -0.25, 3)], spots=[[(2.0, 2.0), (-2.0, 1.0), (1.0, -3.0)]] * 2)


def _statement_frames(clean, sensor, env_ids, clocks):
    made = [S.depth_sensor_numpy(f, S.MIN_DEPTH, S.MAX_DEPTH, sensor, e, c) for f, e, c in zip(clean.cpu().numpy(), env_ids, clocks)]
    return np.stack([m[0] for m in made]), np.array([m[1] for m in made], np.int32)


@pytest.mark.parametrize("mode", ["rooms_objects", "grid_objects", "grid"])
def test_live_world_senses_what_it_casts(gpu_device, mode):
    import torch

    from vlfm_amd.harness import TARGETS, LiveWorld, RoomsRenderer, WorldObjects

    env_ids = [2, 5, 7, 12]
    targets = [TARGETS[i % len(TARGETS)] for i in env_ids]

    def make(sensor):
        worlds = None if mode.startswith("rooms") else _grid_worlds()
        wo = WorldObjects(max_episode_steps=3, min_pixels=40, layout=_ring_layout) if "objects" in mode else None
        return LiveWorld(RoomsRenderer(env_ids, STEPS, HH, WW, gpu_device), env_ids, targets, wo, worlds, depth_sensor=sensor)

    a, b = make(LIVE_SENSOR), make(None)
    assert b.sensor_clock is None and b.clean_frames is None and b.sensor_invalid is None and b.depth_sensor is None
    holes = 0
    for t in range(STEPS):
        assert a.sensor_clock.tolist() == [t] * E
        fa, fb = a.observe(), b.observe()
        torch.cuda.synchronize()
        assert fa is a.frames and fb is b.frames and a.clean_frames is not a.frames
        _assert_frames(a.clean_frames, fb.cpu().numpy(), t)                                  # the ray caster's output is untouched
        want, counts = _statement_frames(a.clean_frames, LIVE_SENSOR, env_ids, [t] * E)
        _assert_frames(fa, want, t)
        assert np.array_equal(a.sensor_invalid.cpu().numpy(), counts)
        holes += int(counts.sum())
        if "objects" in mode:
            assert torch.equal(a.ids, b.ids) and np.array_equal(a.seen_stats, b.seen_stats) and a.sightings == b.sightings
            for w in (a, b):
                w.start_episodes(w.end_episodes(["explore"] * E, np.zeros(E, bool)))
        else:
            assert a.ids is None and a.seen_stats is None
        acts = np.array([PATTERN[(t + e) % len(PATTERN)] for e in range(E)], np.int64)
        for w in (a, b):
            w.advance(acts, np.zeros(E, bool))
        assert np.array_equal(a.xy, b.xy) and np.array_equal(a.k, b.k)
    assert a.sensor_clock.tolist() == [STEPS] * E and holes > 0
    peek = a.observe(fresh=True)                                    # the clock of the next noted observation, not advanced
    assert a.sensor_clock.tolist() == [STEPS] * E and peek.data_ptr() != a.frames.data_ptr()
    _assert_frames(peek, _statement_frames(b.observe(fresh=True), LIVE_SENSOR, env_ids, [STEPS] * E)[0])
    a.reset()
    assert a.sensor_clock.tolist() == [0] * E


# -------------------------------------------------------------------------------------------------------------------- harness
def _harness(device, **kw):
    from vlfm_amd.harness import BatchedEpisodes, WorldObjects

    return BatchedEpisodes(E, device=device, height=HH, width=WW, use_blip2=False, select_frontiers=True, closed_loop=True,
                           world_objects=WorldObjects(max_episode_steps=4, min_pixels=40, layout=_ring_layout),
                           worlds=S.ProceduralWorlds(0), **kw)


def test_harness_with_a_depth_sensor(gpu_device):
    """The run completes on frames with noise and holes, and every step's frames are the statement applied to what the ray
    caster wrote at that step's clocks."""
    import torch

    h = _harness(gpu_device, depth_sensor=LIVE_SENSOR)
    assert h.depth_sensor is LIVE_SENSOR and h.live.depth_sensor is LIVE_SENSOR
    holes = 0
    for t in range(STEPS):
        h.step()
        torch.cuda.synchronize()
        want, counts = _statement_frames(h.live.clean_frames, LIVE_SENSOR, h.env_ids, [t] * E)
        _assert_frames(h.live.frames, want, t)
        assert np.array_equal(h.live.sensor_invalid.cpu().numpy(), counts) and h.live.sensor_clock.tolist() == [t + 1] * E
        holes += int(counts.sum())
    assert holes > 0 and h.t == STEPS
    assert bool(h.obstacles.explored_bits.any())                   # the maps were fed
    h.reset()
    assert h.live.sensor_clock.tolist() == [0] * E


def test_harness_without_a_sensor_is_the_harness_it_was(gpu_device):
    import torch

    a, b = _harness(gpu_device, depth_sensor=None), _harness(gpu_device)
    assert a.depth_sensor is None and a.live.sensor_clock is None and a.live.clean_frames is None and a.live.sensor_invalid is None
    for t in range(STEPS):
        a.step()
        b.step()
        torch.cuda.synchronize()
        assert np.array_equal(a.last_poses, b.last_poses) and np.array_equal(a.last_world_actions, b.last_world_actions)
        assert np.array_equal(a.live.xy, b.live.xy) and np.array_equal(a.live.k, b.live.k)
        assert np.array_equal(_bits(a.live.frames), _bits(b.live.frames)) and bool((a.live.ids == b.live.ids).all())
    for name in ("obstacle_bits", "navigable_bits", "explored_bits"):
        assert torch.equal(getattr(a.obstacles, name), getattr(b.obstacles, name)), name
    assert torch.equal(a.values.conf.view(torch.int32), b.values.conf.view(torch.int32))
    assert torch.equal(a.values.value.view(torch.int64), b.values.value.view(torch.int64))
    np.testing.assert_equal(a.live.stats, b.live.stats)
    np.testing.assert_equal(a.live.objectnav_stats, b.live.objectnav_stats)


def test_harness_refusals():
    from vlfm_amd.harness import BatchedEpisodes, Camera, CameraRig
    from vlfm_amd.mapping.obstacle_map import ObstacleMapBatch

    kw = dict(use_blip2=False, select_frontiers=True)
    with pytest.raises(ValueError, match="closed_loop"):
        BatchedEpisodes(2, depth_sensor=LIVE_SENSOR, **kw)
    with pytest.raises(ValueError, match="rig"):
        BatchedEpisodes(2, closed_loop=True, depth_sensor=LIVE_SENSOR, rig=CameraRig([Camera()]), **kw)
    assert ObstacleMapBatch.HOLE_CAP_CONTOURS == 1 << 15
    with pytest.raises(ValueError, match=r"HOLE_CAP_CONTOURS.*0\.053"):
        BatchedEpisodes(2, closed_loop=True, depth_sensor=S.DepthSensor(dropout=0.054), **kw)          # 640 x 480
    with pytest.raises(ValueError, match="HOLE_CAP_CONTOURS"):
        BatchedEpisodes(2, height=240, width=320, closed_loop=True, depth_sensor=S.DepthSensor(dropout=0.22), **kw)
    with pytest.raises(ValueError, match="DepthSensor"):
        BatchedEpisodes(2, closed_loop=True, depth_sensor=dict(dropout=0.01), **kw)
