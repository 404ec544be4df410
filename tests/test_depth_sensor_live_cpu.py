"""LiveWorld(depth_sensor=...) on the host: the NumPy stand-in renderer of tests/live_world_cases.py, with a ``sense_depth``
that calls the statement.  The clocks, ``fresh=True``, ``reset()`` and what exists without a sensor.  No GPU."""
import numpy as np
import pytest
import torch

import vlfm_amd.synthetic as S
from live_world_cases import E, H, TARGETS3, W, NumpyRenderer, actions_at, planes_of, ring_layout
from vlfm_amd.worlds import LiveWorld, WorldObjects

SENSOR = S.DepthSensor(seed=4, sigma0_m=0.003, sigma2_per_m=0.002, dropout=0.1, edge_m=0.3)
ENV_IDS = [2, 0, 1]                         # not the slots' own indices: the keys are the environments' ids
TARGETS = [TARGETS3[e] for e in ENV_IDS]


class SensingRenderer(NumpyRenderer):
    def __init__(self) -> None:
        super().__init__()
        self.sensed = []                        # (env_ids, clocks) of every call

    def sense_depth(self, clean, sensor, env_ids, clocks, min_depth=None, max_depth=None, out=None, invalid_out=None, band_rows=0):
        assert out is None or out.data_ptr() != clean.data_ptr()
        self.sensed.append((list(env_ids), np.array(clocks).tolist()))
        made = [S.depth_sensor_numpy(f, S.MIN_DEPTH, S.MAX_DEPTH, sensor, e, c) for f, e, c in zip(clean.numpy(), env_ids, clocks)]
        frames = torch.from_numpy(np.stack([m[0] for m in made]))
        return (frames if out is None else out.copy_(frames)), torch.tensor([m[1] for m in made], dtype=torch.int32)


def _want(clean, clocks):
    return [S.depth_sensor_numpy(f, S.MIN_DEPTH, S.MAX_DEPTH, SENSOR, e, c) for f, e, c in zip(clean, ENV_IDS, clocks)]


@pytest.mark.parametrize("objects", [False, True])
def test_clocks_fresh_and_reset(objects):
    wo = WorldObjects(max_episode_steps=3, min_pixels=4, layout=ring_layout) if objects else None
    r = SensingRenderer()
    live = LiveWorld(r, ENV_IDS, TARGETS, wo, depth_sensor=SENSOR)
    assert live.depth_sensor is SENSOR and live.sensor_clock.tolist() == [0] * E and live.sensor_clock.dtype == np.int64
    assert live.clean_frames is None and live.sensor_invalid is None and live.frames is None
    for t in range(5):
        depth, ids, stats, _ = planes_of(live)
        want = _want(depth, [t] * E)
        # fresh: sensed with the clock the next noted observation will use; new buffers, nothing noted, nothing advanced
        peek = live.observe(fresh=True)
        assert peek is not live.frames and peek.numpy().tobytes() == np.stack([w[0] for w in want]).tobytes()
        assert live.sensor_clock.tolist() == [t] * E
        frames = live.observe()
        assert frames is live.frames and frames.numpy().tobytes() == peek.numpy().tobytes()
        assert live.clean_frames.numpy().tobytes() == depth.tobytes() and live.clean_frames is not live.frames
        assert live.sensor_invalid.tolist() == [w[1] for w in want] and sum(w[1] for w in want) > 0
        assert live.sensor_clock.tolist() == [t + 1] * E
        assert r.sensed[-2:] == [(ENV_IDS, [t] * E)] * 2
        if objects:                             # ids and statistics stay what the ray caster saw
            assert live.ids.numpy().tobytes() == ids.tobytes() and live.seen_stats.tobytes() == stats.tobytes()
            done = live.end_episodes(["explore"] * E, np.zeros(E, bool))
            live.start_episodes(done)           # an episode start leaves the clocks alone
            assert live.sensor_clock.tolist() == [t + 1] * E
        live.advance(actions_at(t), np.zeros(E, bool))
    live.reset()
    assert live.sensor_clock.tolist() == [0] * E
    depth = planes_of(live)[0]
    assert live.observe().numpy().tobytes() == np.stack([w[0] for w in _want(depth, [0] * E)]).tobytes()


def test_the_sensor_sees_what_the_painter_returns():
    r = SensingRenderer()
    live = LiveWorld(r, ENV_IDS, TARGETS, depth_sensor=SENSOR)

    def painter(t_ep, frames):
        assert frames is live.clean_frames
        frames[:, :4, :4] = 0.25 + 0.01 * t_ep
        return frames

    clean = planes_of(live)[0].copy()
    clean[:, :4, :4] = np.float32(0.25 + 0.01 * 3)
    got = live.observe(painter, 3)
    assert live.clean_frames.numpy().tobytes() == clean.tobytes()
    assert got.numpy().tobytes() == np.stack([w[0] for w in _want(clean, [0] * E)]).tobytes()


def test_without_a_sensor_nothing_exists():
    r = SensingRenderer()
    live = LiveWorld(r, ENV_IDS, TARGETS)
    depth = planes_of(live)[0]
    assert live.observe().numpy().tobytes() == depth.tobytes() and not r.sensed
    assert live.depth_sensor is None and live.sensor_clock is None and live.sensor_invalid is None and live.clean_frames is None
    live.reset()
    with pytest.raises(ValueError, match="DepthSensor"):
        LiveWorld(r, ENV_IDS, TARGETS, depth_sensor=dict(dropout=0.1))


def test_the_harness_refuses_before_the_device_is_touched():
    """No GPU here: anything that reached the device would raise RuntimeError, not ValueError."""
    from vlfm_amd.harness import BatchedEpisodes, Camera, CameraRig

    kw = dict(use_blip2=False, select_frontiers=True)
    with pytest.raises(ValueError, match="closed_loop"):
        BatchedEpisodes(2, depth_sensor=SENSOR, **kw)
    with pytest.raises(ValueError, match="rig"):
        BatchedEpisodes(2, closed_loop=True, depth_sensor=SENSOR, rig=CameraRig([Camera()]), **kw)
    with pytest.raises(ValueError, match=r"HOLE_CAP_CONTOURS.*0\.053"):
        BatchedEpisodes(2, closed_loop=True, depth_sensor=S.DepthSensor(dropout=0.054), **kw)
