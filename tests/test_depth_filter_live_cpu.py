"""LiveWorld(depth_filter=...) on the host: the NumPy stand-in renderer of tests/live_world_cases.py, with a ``sense_depth`` and a
``filter_depth`` that call the statements.  The order sensor -> filter, the new attributes, ``fresh=True``, ``reset()`` and what
exists without a filter.  No GPU."""
import numpy as np
import pytest
import torch

import vlfm_amd.synthetic as S
from live_world_cases import E, TARGETS3, NumpyRenderer, actions_at, planes_of, ring_layout
from vlfm_amd.worlds import LiveWorld, WorldObjects

SENSOR = S.DepthSensor(seed=4, sigma0_m=0.003, dropout=0.1, patch_dropout=0.05, edge_m=0.3)
FILTER = S.DepthFilter(reach_px=3)
ENV_IDS = [2, 0, 1]
TARGETS = [TARGETS3[e] for e in ENV_IDS]


class FilteringRenderer(NumpyRenderer):
    def __init__(self) -> None:
        super().__init__()
        self.calls = []                          # "sense" / "filter", in the order they came

    def sense_depth(self, clean, sensor, env_ids, clocks, min_depth=None, max_depth=None, out=None, invalid_out=None, band_rows=0):
        assert out is None or out.data_ptr() != clean.data_ptr()
        self.calls.append("sense")
        made = [S.depth_sensor_numpy(f, S.MIN_DEPTH, S.MAX_DEPTH, sensor, e, c) for f, e, c in zip(clean.numpy(), env_ids, clocks)]
        frames = torch.from_numpy(np.stack([m[0] for m in made]))
        return (frames if out is None else out.copy_(frames)), torch.tensor([m[1] for m in made], dtype=torch.int32)

    def filter_depth(self, frames, flt, out=None, counts_out=None):
        assert out is None or out.data_ptr() != frames.data_ptr()
        self.calls.append("filter")
        made = [S.depth_filter_numpy(f, flt) for f in frames.numpy()]
        filled = torch.from_numpy(np.stack([m[0] for m in made]))
        return (filled if out is None else out.copy_(filled)), torch.tensor([m[1:] for m in made], dtype=torch.int32)


def _sensed(clean, clocks):
    return np.stack([S.depth_sensor_numpy(f, S.MIN_DEPTH, S.MAX_DEPTH, SENSOR, e, c)[0] for f, e, c in zip(clean, ENV_IDS, clocks)])


def _filtered(sensed):
    made = [S.depth_filter_numpy(f, FILTER) for f in sensed]
    return np.stack([m[0] for m in made]), [list(m[1:]) for m in made]


@pytest.mark.parametrize("objects", [False, True])
@pytest.mark.parametrize("sensor", [None, SENSOR])
def test_order_attributes_fresh_and_reset(objects, sensor):
    wo = WorldObjects(max_episode_steps=3, min_pixels=4, layout=ring_layout) if objects else None
    r = FilteringRenderer()
    live = LiveWorld(r, ENV_IDS, TARGETS, wo, depth_sensor=sensor, depth_filter=FILTER)
    assert live.depth_filter is FILTER and live.sensed_frames is None and live.filter_counts is None and live.frames is None
    per_observe = ["sense", "filter"] if sensor is not None else ["filter"]
    for t in range(4):
        depth, ids, stats, _ = planes_of(live)
        sensed = depth if sensor is None else _sensed(depth, [t] * E)
        want, counts = _filtered(sensed)
        r.calls.clear()
        peek = live.observe(fresh=True)          # new buffers, nothing noted
        assert peek is not live.frames and peek.numpy().tobytes() == want.tobytes() and r.calls == per_observe
        assert live.filter_counts is None if t == 0 else live.filter_counts is not None
        frames = live.observe()
        assert r.calls == per_observe * 2
        assert frames is live.frames and frames.numpy().tobytes() == want.tobytes()
        assert live.sensed_frames is not live.frames and live.sensed_frames.numpy().tobytes() == sensed.tobytes()
        assert live.filter_counts.tolist() == counts and live.filter_counts.dtype == torch.int32
        if sensor is not None:
            assert live.clean_frames.numpy().tobytes() == depth.tobytes() and live.clean_frames is not live.sensed_frames
            assert live.sensor_clock.tolist() == [t + 1] * E and sum(c[0] for c in counts) > 0
        else:
            assert live.clean_frames is None and live.sensor_clock is None and live.sensor_invalid is None
        if objects:                              # ids and statistics stay what the ray caster saw
            assert live.ids.numpy().tobytes() == ids.tobytes() and live.seen_stats.tobytes() == stats.tobytes()
            live.start_episodes(live.end_episodes(["explore"] * E, np.zeros(E, bool)))
        live.advance(actions_at(t), np.zeros(E, bool))
    kept = live.frames
    live.reset()
    depth = planes_of(live)[0]
    sensed = depth if sensor is None else _sensed(depth, [0] * E)
    got = live.observe()
    assert got is kept and got.numpy().tobytes() == _filtered(sensed)[0].tobytes()


def test_the_filter_sees_what_the_painter_returns():
    r = FilteringRenderer()
    live = LiveWorld(r, ENV_IDS, TARGETS, depth_filter=FILTER)

    def painter(t_ep, frames):
        assert frames is live.sensed_frames
        frames[:, 2:6, 2:6] = 0.0                # a hole the filter has to close
        return frames

    holed = planes_of(live)[0].copy()
    holed[:, 2:6, 2:6] = 0.0
    got = live.observe(painter, 3)
    assert live.sensed_frames.numpy().tobytes() == holed.tobytes()
    want, counts = _filtered(holed)
    assert got.numpy().tobytes() == want.tobytes() and live.filter_counts.tolist() == counts
    assert all(c[0] >= 16 for c in counts)


def test_without_a_filter_nothing_exists():
    r = FilteringRenderer()
    for sensor in (None, SENSOR):
        live = LiveWorld(r, ENV_IDS, TARGETS, depth_sensor=sensor)
        r.calls.clear()
        live.observe()
        assert "filter" not in r.calls
        assert live.depth_filter is None and live.sensed_frames is None and live.filter_counts is None
        live.reset()
    with pytest.raises(ValueError, match="DepthFilter"):
        LiveWorld(r, ENV_IDS, TARGETS, depth_filter=dict(reach_px=3))


def test_the_harness_refuses_before_the_device_is_touched():
    """No GPU here: anything that reached the device would raise RuntimeError, not ValueError."""
    from vlfm_amd.harness import BatchedEpisodes, Camera, CameraRig

    kw = dict(use_blip2=False, select_frontiers=True)
    with pytest.raises(ValueError, match="depth_filter needs closed_loop"):
        BatchedEpisodes(2, depth_filter=FILTER, **kw)
    with pytest.raises(ValueError, match="depth_filter.*rig"):
        BatchedEpisodes(2, closed_loop=True, depth_filter=FILTER, rig=CameraRig([Camera()]), **kw)
    with pytest.raises(ValueError, match="DepthFilter"):
        BatchedEpisodes(2, closed_loop=True, depth_filter="far", **kw)
    # without a filter the dropout bound and its message are the sensor's own
    with pytest.raises(ValueError, match=r"dropout \* height \* width.*HOLE_CAP_CONTOURS.*0\.053"):
        BatchedEpisodes(2, closed_loop=True, depth_sensor=S.DepthSensor(dropout=0.054), **kw)
    # with one, it is the pixels dropped together with their four neighbours that count
    with pytest.raises(ValueError, match=r"dropout\*\*5 \* height \* width.*HOLE_CAP_CONTOURS"):
        BatchedEpisodes(2, closed_loop=True, depth_sensor=S.DepthSensor(dropout=0.5), depth_filter=FILTER, height=2048,
                        width=2048, **kw)
