"""-m gpu: the closed-loop world (vlfm_amd/worlds.py: LiveWorld) on the real RoomsRenderer, no harness around it: every
observe() against the NumPy statements' planes, byte for byte, every advance() against synthetic.step_poses."""
import numpy as np
import pytest

import vlfm_amd.synthetic as S
from live_world_cases import E, H, TARGETS3, W, actions_at, planes_of, ring_layout

pytestmark = pytest.mark.gpu
STEPS = 8


def _grid_worlds():
    plans = []
    for wall in (12, 27):                     # two 40 x 40 plans of 0.25 m cells over [-5, 5]^2: the border and one inner wall
        occ = np.zeros((40, 40), bool)
        occ[[0, -1]], occ[:, [0, -1]] = True, True
        occ[wall, 5:30] = True
        plans.append(S.GridPlan.uniform(occ, 4, -20, -20))
    return S.GridWorlds(plans, starts=[(0.0, 0.0, 0), (0.5, -0.25, 3)], spots=[[(2.0, 2.0), (-2.0, 1.0), (1.0, -3.0)]] * 2)


@pytest.mark.parametrize("mode", ["rooms_objects", "procedural_objects_rgb", "procedural_rgb", "grid_objects"])
def test_live_world_is_the_numpy_statements(gpu_device, mode):
    import torch

    from vlfm_amd.harness import LiveWorld, RoomsRenderer, WorldObjects

    worlds = None if mode.startswith("rooms") else S.ProceduralWorlds(seed=3) if mode.startswith("procedural") else _grid_worlds()
    objects = WorldObjects(max_episode_steps=3, min_pixels=4, layout=ring_layout) if "objects" in mode else None
    live = LiveWorld(RoomsRenderer(range(E), STEPS, H, W, gpu_device), range(E), TARGETS3, objects, worlds, render_rgb="rgb" in mode)
    seen = 0
    for t in range(STEPS):
        depth, ids, stats, rgb = planes_of(live)
        frames = live.observe()
        torch.cuda.synchronize()
        assert frames is live.frames and frames.cpu().numpy().tobytes() == depth.tobytes(), t
        if objects is not None:
            assert live.ids.cpu().numpy().tobytes() == ids.tobytes() and live.seen_stats.tobytes() == stats.tobytes(), t
            seen += int(ids.any())
        else:
            assert live.ids is None and live.seen_stats is None
        assert (live.rgb is None) if rgb is None else (live.rgb.cpu().numpy().tobytes() == rgb.tobytes()), t
        ended = np.zeros(E, bool)
        if objects is not None:                 # nobody stops: every episode times out after three steps
            done = live.end_episodes(["explore"] * E, ended.copy())
            assert done == ([0, 1, 2] if t % 3 == 2 else [])
            ended[done] = True
            live.start_episodes(done)
        acts = np.where(ended, S.ACTION_STOP, actions_at(t))
        extra = None if objects is None else np.where(live.objects[:, :, 6:7] != 0.0, live.objects[:, :, :4], np.nan)
        want = S.step_poses(live.xy, live.k, acts, extra, None if worlds is None else live.table.boxes,
                            live.table.grids if mode.startswith("grid") else None)
        assert np.array_equal(live.advance(actions_at(t), ended), acts)
        assert all(np.array_equal(a, b) for a, b in zip((live.xy, live.k, live.collided), want)), t
    assert live.stats["forward_steps"].sum() > live.stats["collisions"].sum() and (objects is None or seen > STEPS // 2)   # (objects were in view)
    assert worlds is None or live.world_episode.tolist() == [2 if objects is not None else 0] * E
