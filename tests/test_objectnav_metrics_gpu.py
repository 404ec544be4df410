"""-m gpu: BatchedEpisodes(..., world_objects=..., objectnav_metrics=True): SPL, SoftSPL and the geodesic distance_to_goal of the
scored ObjectNav episodes, from the geodesic kernels; with the flag off the harness is what it was."""
import numpy as np
import pytest

from vlfm_amd import synthetic as S
from vlfm_amd.policy_step import ACTION_FORWARD
from world_object_cases import A

pytestmark = pytest.mark.gpu

# behind the hall's north wall segment (and 5.1 m from (0, 0)): never seen from the start of environment 0
HIDDEN = (0.5, 4.8, 1.0, 5.3, 0.0, 0.9)
PARENT_KEYS = {"episodes", "successes", "wrong_stops", "no_frontier_stops", "timeouts", "episode_env", "episode_outcome",
               "episode_steps", "episode_path_length", "episode_first_sighting"}
METRIC_KEYS = {"episode_geodesic", "episode_distance_to_goal", "episode_spl", "episode_soft_spl"}


def _first_episode(per_env):
    return lambda env_id, episode, robot_xy: list(per_env.get(env_id, [])) if episode == 0 else []


def _sim(device, E, layout=None, wo=None, **kw):
    from vlfm_amd.harness import BatchedEpisodes, WorldObjects

    world = WorldObjects(**({} if layout is None else {"layout": layout}), **(wo or {}))
    return BatchedEpisodes(E, device=device, use_blip2=False, select_frontiers=True, episode_len=500, closed_loop=True,
                           world_objects=world, **kw)


def _host_distance(box6, points, others=()):
    """The host statement for a world with the objects ``box6`` (the target) and ``others``."""
    rects = S.inflated_rects(np.array([box6] + list(others), np.float64))
    src = S.goal_viewpoints(box6, rects, 1.0)
    nodes, dist = S.geodesic_field_numpy(rects, src)
    return S.geodesic_query_numpy(rects, src, nodes, dist, points)


def _bits(t):
    import torch

    return t.contiguous().view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def _equal(a, b) -> bool:
    import torch

    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def test_the_flag_needs_world_objects(gpu_device):
    from vlfm_amd.harness import BatchedEpisodes

    with pytest.raises(ValueError, match="world_objects"):
        BatchedEpisodes(2, device=gpu_device, use_blip2=False, select_frontiers=True, closed_loop=True, objectnav_metrics=True)


def test_target_in_line_of_sight_scores_spl(gpu_device):
    """The scenario of test_objectnav_closed_loop_gpu.py::test_target_in_line_of_sight_is_found_and_reached: environment 0
    starts at (0, 0) heading east, the chair A 2.25 m ahead; environment 1 has no target."""
    import torch

    E, cap = 2, 100
    sim = _sim(gpu_device, E, layout=_first_episode({0: [("chair", A)]}), wo=dict(max_episode_steps=cap), object_maps=True,
               objectnav_metrics=True)
    st = sim.live.objectnav_stats
    assert set(st) == PARENT_KEYS | METRIC_KEYS
    l_host = float(_host_distance(A, [(0.0, 0.0)])[0])
    assert sim.live.ep_geodesic[0] == l_host and np.isnan(sim.live.ep_geodesic[1])
    assert sim.live.distance_to_goal[0] == l_host and np.isnan(sim.live.distance_to_goal[1])
    dists, acts, poses = [], [], []
    while st["episodes"][0] == 0 and len(dists) < cap + 1:
        where = sim.live.xy[0].copy()
        sim.step()
        poses.append(where)
        acts.append(int(sim.last_world_actions[0]))
        if st["episodes"][0] == 0:
            dists.append(float(sim.live.distance_to_goal[0]))
            assert np.isnan(sim.live.distance_to_goal[1])
    torch.cuda.synchronize()
    assert st["episode_outcome"][0] == "success" and st["episode_env"][0] == 0
    l, p, d_end = st["episode_geodesic"][0], st["episode_path_length"][0], st["episode_distance_to_goal"][0]
    print("l", l, "path", p, "d_end", d_end, "spl", st["episode_spl"][0], "soft_spl", st["episode_soft_spl"][0],
          "distance per step", dists)
    assert l == l_host and 1.0 < l < 1.5                   # 2.25 m to the face, success within 1 m of it
    assert st["episode_spl"][0] == S.spl(True, l, p) and 0.0 < st["episode_spl"][0] <= 1.0
    final = poses[-1]                                      # the pose the last step judged: the STOP did not move the robot
    assert np.array_equal(final, sim.live.xy[0])
    assert d_end == float(_host_distance(A, [final])[0]) and d_end == 0.0 and S.rect_distance(final, A) <= 1.0
    assert st["episode_soft_spl"][0] == S.soft_spl(d_end, l, p) == st["episode_spl"][0]
    # every step's distance is the host's at the pose the step judged; it never grows on the way in
    want = _host_distance(A, poses[:len(dists)])
    assert np.array_equal(np.array(dists).view(np.int64), want.view(np.int64))
    assert dists[0] == l and all(b <= a for a, b in zip(dists, dists[1:]))
    moved = [i for i in range(1, len(dists)) if acts[i - 1] == ACTION_FORWARD]
    assert len(moved) >= 3 and all(dists[i] < dists[i - 1] for i in moved if dists[i - 1] > 0.0)
    # the next episode has no target: nan, and it is in no mean
    assert np.isnan(sim.live.distance_to_goal[0]) and np.isnan(sim.live.ep_geodesic[0])
    summary = sim.live.objectnav_summary()
    assert summary["episodes"] == 1 and summary["scored"] == 1 and summary["success_rate"] == 1.0
    assert summary["spl"] == st["episode_spl"][0] and summary["soft_spl"] == st["episode_soft_spl"][0]
    assert summary["distance_to_goal"] == 0.0 and summary["excluded_no_target"] == 0 and summary["excluded_unreachable"] == 0


def test_a_timeout_scores_zero_spl_and_soft_spl_as_defined(gpu_device):
    import torch

    E, cap = 2, 30
    sim = _sim(gpu_device, E, layout=_first_episode({0: [("chair", HIDDEN)]}), wo=dict(max_episode_steps=cap),
               objectnav_metrics=True)
    st = sim.live.objectnav_stats
    last = None
    while st["episodes"][0] == 0:
        last = sim.live.xy[0].copy()
        sim.step()
    torch.cuda.synchronize()
    i0, i1 = st["episode_env"].index(0), st["episode_env"].index(1)
    assert st["episode_outcome"][i0] == "timeout" and st["episode_steps"][i0] == cap
    l, p, d_end = st["episode_geodesic"][i0], st["episode_path_length"][i0], st["episode_distance_to_goal"][i0]
    assert l == float(_host_distance(HIDDEN, [(0.0, 0.0)])[0]) and np.isfinite(l) and l > S.rect_distance((0.0, 0.0), HIDDEN) - 1.0
    assert d_end == float(_host_distance(HIDDEN, [last])[0]) and np.isfinite(d_end)
    assert st["episode_spl"][i0] == 0.0
    assert st["episode_soft_spl"][i0] == max(0.0, 1.0 - d_end / l) * (l / max(p, l))
    print("timeout: l", l, "path", p, "d_end", d_end, "soft_spl", st["episode_soft_spl"][i0])
    # environment 1 had no target: recorded as nan, scored 0, excluded from the means
    assert st["episode_outcome"][i1] == "timeout" and np.isnan(st["episode_geodesic"][i1])
    assert np.isnan(st["episode_distance_to_goal"][i1]) and st["episode_spl"][i1] == 0.0 and st["episode_soft_spl"][i1] == 0.0
    summary = sim.live.objectnav_summary()
    assert summary["episodes"] == 2 and summary["scored"] == 1 and summary["excluded_no_target"] == 1
    assert summary["success_rate"] == 0.0 and summary["spl"] == 0.0 and summary["soft_spl"] == st["episode_soft_spl"][i0]
    assert summary["distance_to_goal"] == d_end


def test_the_metrics_change_nothing(gpu_device):
    """Two harnesses on the default layouts, flag on and off, side by side: identical frames, modes, goals, actions and poses;
    the one without the flag keeps exactly the keys it had."""
    import torch

    E = 3
    kw = dict(wo=dict(max_episode_steps=25), object_maps=True)
    on, off = _sim(gpu_device, E, objectnav_metrics=True, **kw), _sim(gpu_device, E, **kw)
    assert set(off.live.objectnav_stats) == PARENT_KEYS and off.live.distance_to_goal is None
    for t in range(30):
        on.step()
        off.step()
        torch.cuda.synchronize()
        assert _equal(on.live.frames, off.live.frames) and _equal(on.live.ids, off.live.ids), t
        assert on.last_modes == off.last_modes, t
        assert np.array_equal(on.last_goals, off.last_goals, equal_nan=True), t
        assert np.array_equal(on.last_world_actions, off.last_world_actions), t
        assert np.array_equal(on.last_poses, off.last_poses), t
        assert np.array_equal(on.last_episode_end, off.last_episode_end), t
        assert on.live.distance_to_goal.shape == (E,) and not np.isnan(on.live.distance_to_goal).any(), t
    assert np.array_equal(on.live.xy, off.live.xy) and np.array_equal(on.live.k, off.live.k)
    assert np.array_equal(on.live.objects, off.live.objects)
    for name in ("obstacle_bits", "navigable_bits", "explored_bits"):
        assert _equal(getattr(on.obstacles, name), getattr(off.obstacles, name)), name
    assert _equal(on.values.conf, off.values.conf) and _equal(on.values.value, off.values.value)
    assert set(off.live.objectnav_stats) == PARENT_KEYS
    for key in PARENT_KEYS:
        assert np.array_equal(np.asarray(on.live.objectnav_stats[key]), np.asarray(off.live.objectnav_stats[key])), key
    n = len(on.live.objectnav_stats["episode_outcome"])
    assert n >= E and all(len(on.live.objectnav_stats[k]) == n for k in METRIC_KEYS)               # 30 steps, 25 per episode
    # the default layouts from the environments' start poses: every episode has a reachable target
    assert np.isfinite(on.live.objectnav_stats["episode_geodesic"]).all()
    assert set(off.live.objectnav_summary()) == {"episodes", "success_rate"}
    print("summary after 30 steps:", on.live.objectnav_summary())
