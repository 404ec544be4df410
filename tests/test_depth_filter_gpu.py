"""-m gpu: the depth filter on the device (vlfm_depth_filter through utils.depth_filter.filter_depth_batch / filter_depth,
RoomsRenderer.filter_depth, LiveWorld(depth_filter=...) and BatchedEpisodes(depth_filter=...)) against the host statement
synthetic.depth_filter_numpy: frames bit for bit, counts equal."""
import functools
import itertools

import numpy as np
import pytest

import vlfm_amd.synthetic as S
from vlfm_amd.synthetic import DepthFilter

pytestmark = pytest.mark.gpu

f32 = np.float32
# 1 x 1, a single row, a single column, the scalar path (18 x 9), the 16-byte path in one chunk, several bands; widths that cross
# the row pass's 256-column chunk (one wavefront holds 256 columns at once) and the column pass's 1024-column workgroup
SHAPES = [(1, 1), (1, 7), (7, 1), (9, 18), (12, 20), (48, 64), (5, 255), (5, 256), (5, 257), (5, 260), (3, 1023), (3, 1024),
          (3, 1028)]
REACHES = [1, 3, 65535, None]


@functools.lru_cache(maxsize=None)
def _frames(H, W):
    """Three frames: (0) random depths with isolated holes -- zeros, NaN, -0.0, negatives --, inf, the smallest denormal and holes
    in the four corners and along the four borders; (1) a whole row and a whole column of holes, and runs of 1, 2, 3 and 4 holes
    between sources along rows and columns -- with reach_px 1 and 3 those are runs of exactly reach_px and reach_px + 1, and the
    vertical ones cross the seams of 1- and 5-row bands --, everything else valid; (2) nothing but holes."""
    rng = np.random.Generator(np.random.PCG64(1000 * H + W))
    a = rng.uniform(0.05, 1.0, (H, W)).astype(f32)
    kind = rng.uniform(size=(H, W))
    a[kind < 0.12] = 0.0
    a[kind < 0.03] = np.nan
    a[(kind >= 0.03) & (kind < 0.05)] = -0.25
    a[(kind >= 0.05) & (kind < 0.07)] = -0.0
    a[rng.uniform(size=(H, W)) < 0.02] = np.inf
    a[rng.uniform(size=(H, W)) < 0.02] = np.finfo(f32).smallest_subnormal
    a[0, ::3], a[-1, 1::3], a[::3, 0], a[1::3, -1] = 0.0, 0.0, 0.0, 0.0
    a[0, 0] = a[0, -1] = a[-1, 0] = a[-1, -1] = 0.0
    b = rng.uniform(0.05, 1.0, (H, W)).astype(f32)
    b[H // 2, :] = 0.0
    b[:, W // 3] = 0.0
    col = 1
    for run in (1, 2, 3, 4, 3, 2):                   # along row 0 (and the last row, mirrored)
        if col + run < W:
            b[0, col:col + run] = 0.0
            b[-1, W - col - run:W - col] = np.nan
        col += run + 1
    row = 1
    for run in (1, 2, 3, 4, 3, 2):                   # along the last column (and column 0, from the bottom)
        if row + run < H:
            b[row:row + run, -1] = 0.0
            b[H - row - run:H - row, 0] = -1.0
        row += run + 1
    if W > 300:                                      # long runs across the chunk seams
        b[-1, 250:262] = 0.0
        b[0, 100:W - 100] = 0.0
    out = np.stack([a, b, np.zeros((H, W), f32)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(H, W, flt):
    made = [S.depth_filter_numpy(f, flt) for f in _frames(H, W)]
    frames, counts = np.stack([m[0] for m in made]), np.array([m[1:] for m in made], np.int32)
    frames.setflags(write=False)
    return frames, counts


def _bits(t):
    import torch

    return t.contiguous().view(torch.int32).cpu().numpy()


def _assert_frames(got, want, what=None):
    assert np.array_equal(_bits(got), np.ascontiguousarray(want).view(np.int32)), what


def _device_frames(H, W, device):
    import torch

    return torch.from_numpy(_frames(H, W).copy()).to(device)


@pytest.mark.parametrize("H, W", SHAPES)
def test_equals_the_statement(gpu_device, H, W):
    """Both fill modes, every reach, planned bands, a seam on every row, 5-row bands and a single band: every band_rows gives the
    statement's frames and counts."""
    import torch

    from vlfm_amd.utils.depth_filter import filter_depth_batch

    frames = _device_frames(H, W, gpu_device)
    some_filled = some_left = False
    for fill, reach in itertools.product(("far", "near"), REACHES):
        flt = DepthFilter(fill, reach)
        want, counts = _reference(H, W, flt)
        for band_rows in sorted({0, 1, 5, H}):
            out, got = filter_depth_batch(frames, flt, band_rows=band_rows)
            assert out.shape == frames.shape and got.dtype == torch.int32 and tuple(got.shape) == (3, 2)
            _assert_frames(out, want, (flt, band_rows))
            assert np.array_equal(got.cpu().numpy(), counts), (flt, band_rows)
        assert counts[2].tolist() == [0, H * W]                              # the frame of holes stays
        some_filled, some_left = some_filled or counts[:2, 0].sum() > 0, some_left or counts[:2, 1].sum() > 0
    assert some_filled == (H * W > 1)
    _assert_frames(frames, _frames(H, W))                                    # the input is read only


@pytest.mark.parametrize("H, W", [(9, 18), (12, 20), (5, 260)])
def test_clip_recover_and_black(gpu_device, H, W):
    from vlfm_amd.utils.depth_filter import filter_depth_batch

    frames = _device_frames(H, W, gpu_device)
    for fill, clip, recover, black in itertools.product(("far", "near"), (0.0, 0.6), (True, False), (None, -1.0, 0.5)):
        flt = DepthFilter(fill, 3, clip, recover, black)
        want, counts = _reference(H, W, flt)
        out, got = filter_depth_batch(frames, flt, band_rows=5)
        _assert_frames(out, want, flt)
        assert np.array_equal(got.cpu().numpy(), counts), flt
    # a threshold equal to a pixel keeps that pixel a source
    t = float(_frames(H, W)[1, 1, 1])
    flt = DepthFilter("near", None, t, False)
    _assert_frames(filter_depth_batch(frames, flt)[0], _reference(H, W, flt)[0])
    assert _reference(H, W, flt)[0][1, 1, 1] == f32(t)


def test_a_sensor_frame_at_640x480(gpu_device):
    """The frame a DepthSensor with every stage on makes of a host-made scene (a wall, a nearer box, a far strip out of range)."""
    import torch

    from vlfm_amd.utils.depth_filter import filter_depth_batch

    H, W = 480, 640
    clean = np.full((H, W), 0.55, f32)
    clean[:, :200] = np.linspace(0.2, 0.9, 200, dtype=f32)[None, :]
    clean[150:330, 260:420] = 0.12
    clean[:40] = 0.99
    sensor = S.DepthSensor(seed=7, sigma0_m=0.004, sigma2_per_m=0.003, disparity_k=35.0, dropout=0.05, patch_dropout=0.15, edge_m=0.3,
                           min_range_m=0.6, max_range_m=4.5)
    sensed = np.stack([S.depth_sensor_numpy(clean, S.MIN_DEPTH, S.MAX_DEPTH, sensor, e, 3)[0] for e in (0, 1)])
    for flt in (DepthFilter(), DepthFilter("near", 8, 0.9, False, 1.0)):
        made = [S.depth_filter_numpy(f, flt) for f in sensed]
        out, counts = filter_depth_batch(torch.from_numpy(sensed).to(gpu_device), flt)
        _assert_frames(out, np.stack([m[0] for m in made]), flt)
        assert counts.cpu().numpy().tolist() == [list(m[1:]) for m in made] and made[0][1] > 0.05 * H * W


def _raw(lib, src, out, n, H, W, counts, stream, fill=0, reach=3, clip=0.0, recover=1, set_black=0, black=0.0, band_rows=0):
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    return lib.vlfm_depth_filter(ptr(src), ptr(out), n, H, W, fill, reach, clip, recover, set_black, black, ptr(counts), band_rows,
                                 stream)


def test_no_frames_and_the_optional_counts(gpu_device):
    import torch

    from vlfm_amd import _lib as L
    from vlfm_amd.utils.depth_filter import filter_depth_batch

    H, W = 9, 18
    out, counts = filter_depth_batch(torch.empty((0, H, W), dtype=torch.float32, device=gpu_device))
    assert out.shape == (0, H, W) and counts.shape == (0, 2)
    st = torch.cuda.current_stream().cuda_stream
    assert _raw(L.lib(), None, None, 0, H, W, None, st) == L.VLFM_OK
    flt = DepthFilter(reach_px=3)
    frames = _device_frames(H, W, gpu_device)
    out, counts = filter_depth_batch(frames, flt, counts_out=None)           # counts_out=None: counts are made
    assert np.array_equal(counts.cpu().numpy(), _reference(H, W, flt)[1])
    got = torch.full_like(frames, -1.0)                                      # d_counts == NULL: the frames all the same
    assert _raw(L.lib(), frames, got, 3, H, W, None, st) == L.VLFM_OK, L.last_error()
    _assert_frames(got, _reference(H, W, flt)[0])
    assert L.lib().vlfm_abi_version() >= 28


def test_out_counts_out_unaligned_views_and_a_side_stream(gpu_device):
    import torch

    from vlfm_amd.utils.depth_filter import filter_depth_batch

    H, W = 12, 20
    flt = DepthFilter("near", 3, set_black_value=-2.0)
    want, counts = _reference(H, W, flt)
    n = 3 * H * W
    # views 4 and 12 bytes into their allocations (the scalar loads and stores), guard floats on both sides of both
    src = torch.full((n + 2,), -3.0, dtype=torch.float32, device=gpu_device)
    dst = torch.full((n + 6,), -5.0, dtype=torch.float32, device=gpu_device)
    src[1:n + 1] = _device_frames(H, W, gpu_device).reshape(-1)
    frames, out = src[1:n + 1].view(3, H, W), dst[3:n + 3].view(3, H, W)
    cnt = torch.full((10,), -9, dtype=torch.int32, device=gpu_device)
    got = filter_depth_batch(frames, flt, out=out, counts_out=cnt[2:8].view(3, 2))
    assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == cnt[2:8].data_ptr()
    _assert_frames(out, want)
    assert cnt.cpu().numpy().tolist() == [-9, -9] + counts.reshape(-1).tolist() + [-9, -9]
    assert bool((dst[:3] == -5.0).all()) and bool((dst[n + 3:] == -5.0).all())
    assert bool((src[0] == -3.0)) and bool((src[n + 1] == -3.0))
    _assert_frames(frames, _frames(H, W))
    # an aligned input into a misaligned output and the other way round
    aligned = frames.clone()
    _assert_frames(filter_depth_batch(aligned, flt, out=out)[0], want)
    _assert_frames(filter_depth_batch(frames, flt, out=torch.empty_like(aligned))[0], want)
    # a side stream: work queued before the launches lands before them
    side = torch.cuda.Stream(gpu_device)
    big = torch.ones((64, 480, 640), dtype=torch.float32, device=gpu_device)
    staged = torch.empty_like(aligned)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):
            big.mul_(1.0001)
        staged.copy_(big[:3, :H, :W])                                        # overwritten by what comes next on this stream
        staged.copy_(aligned)
        got = filter_depth_batch(staged, flt)
        after = (got[0].clone(), got[1].clone())
    side.synchronize()
    _assert_frames(after[0], want)
    assert np.array_equal(after[1].cpu().numpy(), counts)


def test_refusals_leave_the_outputs_untouched(gpu_device):
    import torch

    from vlfm_amd import _lib as L
    from vlfm_amd.harness import RoomsRenderer
    from vlfm_amd.utils.depth_filter import filter_depth_batch

    H, W = 9, 18
    frames = _device_frames(H, W, gpu_device)
    out = torch.full_like(frames, -1.0)
    counts = torch.full((3, 2), -7, dtype=torch.int32, device=gpu_device)
    st = torch.cuda.current_stream().cuda_stream
    both = torch.cat([frames.reshape(-1), frames.reshape(-1)])
    first, shifted = both[:frames.numel()].view(3, H, W), both[H * W:H * W + frames.numel()].view(3, H, W)   # two frames in common
    nan, inf = float("nan"), float("inf")
    for kw in (dict(src=None), dict(out=None), dict(n=-1), dict(n=65536), dict(H=0), dict(W=0), dict(H=-4), dict(H=1 << 16, W=1 << 15),
               dict(band_rows=-1), dict(out=frames), dict(src=first, out=shifted), dict(src=shifted, out=first), dict(fill=2),
               dict(fill=-1), dict(reach=-1), dict(reach=65536), dict(clip=-0.5), dict(clip=nan), dict(clip=inf), dict(black=nan),
               dict(black=inf), dict(black=-inf)):
        args = dict(src=frames, out=out, n=3, H=H, W=W, counts=counts, stream=st)
        args.update(kw)
        assert _raw(L.lib(), **args) == L.VLFM_ERR_INVALID, kw
    torch.cuda.synchronize()
    assert bool((out == -1.0).all()) and bool((counts == -7).all())
    _assert_frames(both[:frames.numel()].view(3, H, W), _frames(H, W))
    _assert_frames(both[frames.numel():].view(3, H, W), _frames(H, W))
    # filter_depth_batch: everything before the launch
    flt = DepthFilter(reach_px=3)
    for kw in (dict(frames=frames.double()), dict(frames=frames[0]), dict(frames=frames.transpose(1, 2)), dict(frames=frames.cpu()),
               dict(frames=frames.cpu().numpy()), dict(frames=frames[:, :0]), dict(flt=None), dict(flt=dict(reach_px=3)),
               dict(band_rows=-2), dict(band_rows=1.5), dict(out=frames), dict(out=shifted, frames=first), dict(out=out.double()),
               dict(out=out[:2]), dict(out=out.cpu()), dict(out=out[:, :, :16]), dict(out=out.transpose(1, 2).contiguous().transpose(1, 2)),
               dict(counts_out=counts[:2]), dict(counts_out=counts.long()), dict(counts_out=counts.cpu()),
               dict(counts_out=counts.reshape(-1)), dict(counts_out=torch.zeros((3, 4), dtype=torch.int32, device=gpu_device)[:, ::2])):
        args = dict(frames=frames, flt=flt, out=out, counts_out=counts)
        args.update(kw)
        with pytest.raises(ValueError):
            filter_depth_batch(**args)
    r = RoomsRenderer([0], 8, H, W, gpu_device)
    with pytest.raises(ValueError):
        r.filter_depth(_device_frames(12, 20, gpu_device), flt, out=out)     # not the renderer's shape
    torch.cuda.synchronize()
    assert bool((out == -1.0).all()) and bool((counts == -7).all())
    got = r.filter_depth(frames, flt, out=out, counts_out=counts)            # the same call unrefused
    _assert_frames(got[0], _reference(H, W, flt)[0])
    assert np.array_equal(counts.cpu().numpy(), _reference(H, W, flt)[1])


def test_the_single_frame_entry_equals_the_batch(gpu_device):
    from vlfm_amd.utils.depth_filter import filter_depth

    H, W = 12, 20
    for kw in (dict(), dict(clip_far_thresh=0.6, set_black_value=-1.0, recover_nonzero=False, fill="near", reach_px=3)):
        flt = DepthFilter(kw.get("fill", "far"), kw.get("reach_px"), kw.get("clip_far_thresh", 0.0), kw.get("recover_nonzero", True),
                          kw.get("set_black_value"))
        want = _reference(H, W, flt)[0]
        for i, frame in enumerate(_frames(H, W)):
            got = filter_depth(frame, blur_type=None, **kw)
            assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.tobytes() == want[i].tobytes()
        got = filter_depth(_frames(H, W)[0].astype(np.float64)[:, :, None], **kw)          # [H,W,1], any float type
        assert got.shape == (H, W, 1) and got.tobytes() == want[0].tobytes()
    with pytest.raises(NotImplementedError, match="blurring is not built"):
        filter_depth(_frames(H, W)[0], blur_type="gaussian")


# ------------------------------------------------------------------------------------------------------------------ LiveWorld
E, STEPS, HH, WW = 4, 6, 48, 64
LIVE_SENSOR = S.DepthSensor(seed=1, dropout=0.05, edge_m=0.3)
LIVE_FILTER = DepthFilter(reach_px=4)
_F, _L, _R = S.ACTION_FORWARD, S.ACTION_TURN_LEFT, S.ACTION_TURN_RIGHT
PATTERN = [_F, _L, _F, _F, _R, _F, _R, _F]
ACTIONS = np.array([[PATTERN[(t + e) % len(PATTERN)] for e in range(E)] for t in range(STEPS)], np.int64)


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


def _filter_statement(sensed, flt):
    made = [S.depth_filter_numpy(f, flt) for f in sensed.cpu().numpy()]
    return np.stack([m[0] for m in made]), np.array([m[1:] for m in made], np.int32)


def _sensor_statement(clean, sensor, env_ids, clocks):
    return np.stack([S.depth_sensor_numpy(f, S.MIN_DEPTH, S.MAX_DEPTH, sensor, e, c)[0]
                     for f, e, c in zip(clean.cpu().numpy(), env_ids, clocks)])


@pytest.mark.parametrize("mode", ["rooms_objects", "grid"])
def test_live_world_filters_what_it_senses(gpu_device, mode):
    import torch

    from vlfm_amd.harness import TARGETS, LiveWorld, RoomsRenderer, WorldObjects

    env_ids = [2, 5, 7, 12]
    targets = [TARGETS[i % len(TARGETS)] for i in env_ids]

    def make(flt):
        worlds = None if mode.startswith("rooms") else _grid_worlds()
        wo = WorldObjects(max_episode_steps=3, min_pixels=40, layout=_ring_layout) if "objects" in mode else None
        return LiveWorld(RoomsRenderer(env_ids, STEPS, HH, WW, gpu_device), env_ids, targets, wo, worlds, depth_sensor=LIVE_SENSOR,
                         depth_filter=flt)

    a, b = make(LIVE_FILTER), make(None)
    assert b.depth_filter is None and b.sensed_frames is None and b.filter_counts is None
    replay_a, replay_b = S.ReplayController(ACTIONS), S.ReplayController(ACTIONS)       # the same poses in both runs
    filled = 0
    for t in range(STEPS):
        fa, fb = a.observe(), b.observe()
        torch.cuda.synchronize()
        assert fa is a.frames and fb is b.frames and len({a.frames.data_ptr(), a.sensed_frames.data_ptr(), a.clean_frames.data_ptr()}) == 3
        _assert_frames(a.clean_frames, b.clean_frames.cpu().numpy(), t)                  # the ray caster's output is untouched
        _assert_frames(a.sensed_frames, _sensor_statement(a.clean_frames, LIVE_SENSOR, env_ids, [t] * E), t)
        _assert_frames(a.sensed_frames, fb.cpu().numpy(), t)                             # ... which is what b's readers get
        want, counts = _filter_statement(a.sensed_frames, LIVE_FILTER)
        _assert_frames(fa, want, t)
        assert np.array_equal(a.filter_counts.cpu().numpy(), counts)
        assert np.array_equal(a.sensor_invalid.cpu().numpy(), b.sensor_invalid.cpu().numpy())
        filled += int(counts[:, 0].sum())
        if "objects" in mode:
            assert torch.equal(a.ids, b.ids) and np.array_equal(a.seen_stats, b.seen_stats) and a.sightings == b.sightings
            for w in (a, b):
                w.start_episodes(w.end_episodes(["explore"] * E, np.zeros(E, bool)))
        else:
            assert a.ids is None and a.seen_stats is None
        a.advance(replay_a.act(None, None, None, None), np.zeros(E, bool))
        b.advance(replay_b.act(None, None, None, None), np.zeros(E, bool))
        assert np.array_equal(a.xy, b.xy) and np.array_equal(a.k, b.k)
    assert filled > 0 and a.sensor_clock.tolist() == [STEPS] * E
    np.testing.assert_equal(a.stats, b.stats)
    peek = a.observe(fresh=True)                                    # filtered too, into new buffers, nothing noted
    assert peek.data_ptr() not in (a.frames.data_ptr(), a.sensed_frames.data_ptr()) and a.sensor_clock.tolist() == [STEPS] * E
    _assert_frames(peek, _filter_statement(b.observe(fresh=True), LIVE_FILTER)[0])
    # without a sensor the filter stands right behind the ray caster
    c = LiveWorld(RoomsRenderer(env_ids, STEPS, HH, WW, gpu_device), env_ids, targets, None, None if mode.startswith("rooms") else _grid_worlds(),
                  depth_filter=LIVE_FILTER)
    fc = c.observe()
    assert c.clean_frames is None and c.sensor_clock is None and fc is c.frames
    _assert_frames(fc, _filter_statement(c.sensed_frames, LIVE_FILTER)[0])


# -------------------------------------------------------------------------------------------------------------------- harness
def _harness(device, **kw):
    from vlfm_amd.harness import BatchedEpisodes, WorldObjects

    return BatchedEpisodes(E, device=device, height=HH, width=WW, use_blip2=False, select_frontiers=True, closed_loop=True,
                           world_objects=WorldObjects(max_episode_steps=4, min_pixels=40, layout=_ring_layout),
                           worlds=S.ProceduralWorlds(0), **kw)


def test_harness_without_a_filter_is_the_harness_it_was(gpu_device):
    import torch

    a, b = _harness(gpu_device, depth_filter=None), _harness(gpu_device)
    assert a.depth_filter is None and a.live.depth_filter is None and a.live.sensed_frames is None and a.live.filter_counts is None
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


def test_harness_with_a_filter_runs_at_a_dropout_refused_without(gpu_device):
    """dropout = 0.2 is refused at the harness's own 640 x 480 without a filter (61 440 isolated holes against 16 384 contours);
    with one the harness builds there, and at 64 x 48 it steps: every step's frames are the statement applied to what the sensor
    wrote, and the maps are fed."""
    import torch

    from vlfm_amd.harness import BatchedEpisodes

    sensor = S.DepthSensor(seed=1, dropout=0.2, edge_m=0.3)
    kw = dict(use_blip2=False, select_frontiers=True, closed_loop=True, depth_sensor=sensor)
    with pytest.raises(ValueError, match="HOLE_CAP_CONTOURS"):
        BatchedEpisodes(2, device=gpu_device, **kw)
    big = BatchedEpisodes(2, device=gpu_device, depth_filter=DepthFilter(), **kw)
    assert big.live.depth_filter == DepthFilter() and (big.H, big.W) == (480, 640)
    h = _harness(gpu_device, depth_sensor=sensor, depth_filter=LIVE_FILTER)
    assert h.depth_filter is LIVE_FILTER and h.live.depth_filter is LIVE_FILTER
    filled = 0
    for t in range(STEPS):
        h.step()
        torch.cuda.synchronize()
        _assert_frames(h.live.sensed_frames, _sensor_statement(h.live.clean_frames, sensor, h.env_ids, [t] * E), t)
        want, counts = _filter_statement(h.live.sensed_frames, LIVE_FILTER)
        _assert_frames(h.live.frames, want, t)
        assert np.array_equal(h.live.filter_counts.cpu().numpy(), counts)
        filled += int(counts[:, 0].sum())
    assert filled > 0.1 * STEPS * E * HH * WW and h.t == STEPS
    assert bool(h.obstacles.explored_bits.any())                   # the maps were fed
    h.reset()
    assert h.live.sensor_clock.tolist() == [0] * E


def test_harness_refusals():
    from vlfm_amd.harness import BatchedEpisodes, Camera, CameraRig

    kw = dict(use_blip2=False, select_frontiers=True)
    with pytest.raises(ValueError, match="depth_filter needs closed_loop"):
        BatchedEpisodes(2, depth_filter=LIVE_FILTER, **kw)
    with pytest.raises(ValueError, match="depth_filter.*rig"):
        BatchedEpisodes(2, closed_loop=True, depth_filter=LIVE_FILTER, rig=CameraRig([Camera()]), **kw)
    with pytest.raises(ValueError, match="DepthFilter"):
        BatchedEpisodes(2, closed_loop=True, depth_filter=dict(reach_px=4), **kw)
    with pytest.raises(ValueError, match=r"dropout\*\*5 \* height \* width.*HOLE_CAP_CONTOURS"):
        BatchedEpisodes(2, closed_loop=True, depth_sensor=S.DepthSensor(dropout=0.5), depth_filter=LIVE_FILTER, height=2048,
                        width=2048, **kw)
