"""-m gpu: BatchedEpisodes(closed_loop=True): the actions move the robots and every step observes from where they are.
Driven with the planned tour's own actions the closed-loop step IS the open-loop step, to the bit; driven by the bang-bang
controller it stays in free space, is reproducible, and its book-keeping adds up."""
import numpy as np
import pytest

from vlfm_amd import synthetic as S
from vlfm_amd.policy_step import ACTION_FORWARD, ACTION_TURN_LEFT, ACTION_TURN_RIGHT

pytestmark = pytest.mark.gpu

TO_ID = np.array([ACTION_TURN_LEFT, ACTION_TURN_RIGHT, ACTION_FORWARD])      # indexed by synthetic.LEFT / RIGHT / FORWARD


def _plan_table(env_ids, steps, episode_len=500):
    """[steps, E] action ids: environment e replays the tour from 37 * e steps in, where the open-loop harness starts it."""
    plan = S.plan_actions(2 * episode_len)
    return np.stack([TO_ID[plan[(37 * e) % episode_len:][:steps]] for e in env_ids], axis=1)


def _bits(t):
    import torch

    return t.contiguous().view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def _equal(a, b) -> bool:
    import torch

    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _maps_equal(a, b) -> None:
    for name in ("obstacle_bits", "navigable_bits", "explored_bits"):
        assert _equal(getattr(a.obstacles, name), getattr(b.obstacles, name)), name
    assert _equal(a.values.conf, b.values.conf) and _equal(a.values.value, b.values.value)


def test_replay_of_the_plan_equals_the_open_loop_step(gpu_device):
    import torch

    from vlfm_amd.harness import BatchedEpisodes, ReplayController

    E, steps = 3, 40
    kw = dict(device=gpu_device, use_blip2=False, select_frontiers=True, episode_len=500)
    closed = BatchedEpisodes(E, closed_loop=True, controller=ReplayController(_plan_table(range(E), steps)), **kw)
    opened = BatchedEpisodes(E, **kw)
    closed.prepare(steps)                                            # a documented no-op
    for t in range(steps):
        assert _equal(closed.current_depth(2), opened.current_depth(2)), t
        closed.step()
        opened.step()
        torch.cuda.synchronize()
        assert np.array_equal(closed.last_poses, opened.pose_table[t]), t           # x, y, yaw with ==
        assert _equal(closed.live.frames, opened.rooms.frame(t)), t
        fc, fo = closed.obstacles.frontiers_px(), opened.obstacles.frontiers_px()
        assert len(fc) == len(fo) and all(np.array_equal(x, y) for x, y in zip(fc, fo)), t
        assert np.array_equal(closed.last_goals, opened.last_goals, equal_nan=True) and closed.last_modes == opened.last_modes, t
        assert np.array_equal(closed.last_rho_theta, opened.last_rho_theta, equal_nan=True), t
    _maps_equal(closed, opened)
    closed.check()
    st = closed.live.stats
    assert not st["collisions"].any() and (st["forward_steps"] + st["turn_steps"] + st["stops"] == steps).all()


def test_replay_with_a_camera_rig(gpu_device):
    import torch

    from vlfm_amd.harness import BatchedEpisodes, Camera, CameraRig, ReplayController

    E, steps = 2, 20
    rig = CameraRig([Camera(yaw=0.5, max_depth=3.5), Camera(yaw=-0.5, forward=0.1, hfov=float(np.deg2rad(60.0)))])
    kw = dict(device=gpu_device, use_blip2=False, select_frontiers=True, episode_len=500, rig=rig)
    closed = BatchedEpisodes(E, closed_loop=True, controller=ReplayController(_plan_table(range(E), steps)), **kw)
    opened = BatchedEpisodes(E, **kw)
    for t in range(steps):
        closed.step()
        opened.step()
        torch.cuda.synchronize()
        assert _equal(closed.last_rig[0], opened.last_rig[0]), t
        assert np.array_equal(closed.last_rig[1], opened.last_rig[1]), t
        assert np.array_equal(closed.last_goals, opened.last_goals, equal_nan=True), t
    _maps_equal(closed, opened)


def _bang_bang_run(device, steps=60, E=4):
    import torch

    from vlfm_amd.harness import BatchedEpisodes

    sim = BatchedEpisodes(E, device=device, use_blip2=False, select_frontiers=True, episode_len=500, closed_loop=True)
    poses, actions, frames = [], [], {}
    for t in range(steps):
        sim.step()
        poses.append(sim.last_poses.copy())
        actions.append(sim.last_world_actions.copy())
        if t in (0, 25, steps - 1):
            torch.cuda.synchronize()
            frames[t] = sim.live.frames[0].cpu().numpy()
    torch.cuda.synchronize()
    sim.check()
    return sim, np.stack(poses), np.stack(actions), frames


@pytest.fixture(scope="module")
def bang_bang(gpu_device):
    return _bang_bang_run(gpu_device)


def test_bang_bang_run_is_consistent(bang_bang):
    sim, poses, actions, frames = bang_bang
    steps, E = actions.shape
    assert (actions[:12] == ACTION_TURN_LEFT).all()                  # initialisation: 12 turns for everybody
    # the recorded actions, re-integrated on the host from the start poses, give the recorded poses
    xy, k = sim.pose_table[0][:, :2].copy(), sim.rooms.k_table[0].copy()
    refused = np.zeros(E, np.int64)
    heading = {}
    for t in range(steps):
        assert np.array_equal(poses[t, :, :2], xy) and np.array_equal(poses[t, :, 2], np.array(S.YAWS)[k]), t
        assert not any(S._blocked(x, y, 0.2) for (x, y) in xy), t    # never inside a wall's margin
        heading[t] = int(k[0])
        xy, k, hit = S.step_poses(xy, k, actions[t])
        refused += hit
    assert np.array_equal(sim.live.xy, xy) and np.array_equal(sim.live.k, k)
    # what environment 0 saw at three steps is the NumPy renderer's frame at its recorded pose
    for t, got in frames.items():
        want = S.depth_from_profile(S.wall_profile(poses[t, 0, 0], poses[t, 0, 1], heading[t], sim.W), sim.H)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), t
    st = sim.live.stats
    forward = (actions == ACTION_FORWARD).sum(axis=0)
    turns = ((actions == ACTION_TURN_LEFT) | (actions == ACTION_TURN_RIGHT)).sum(axis=0)
    assert np.array_equal(st["forward_steps"], forward) and np.array_equal(st["turn_steps"], turns)
    assert np.array_equal(st["collisions"], refused)
    assert (st["forward_steps"] + st["turn_steps"] + st["stops"] == steps).all()
    assert np.array_equal(st["path_length"], 0.25 * (forward - refused))
    assert forward.sum() > 0                                         # (the robots do go somewhere)


def test_bang_bang_run_is_reproducible(gpu_device, bang_bang):
    _, poses, actions, _ = bang_bang
    _, poses2, actions2, _ = _bang_bang_run(gpu_device)
    assert np.array_equal(actions, actions2) and np.array_equal(poses, poses2)


def test_episode_wrap_returns_to_the_start_pose(gpu_device):
    import torch

    from vlfm_amd.harness import BatchedEpisodes

    E, L = 2, 20
    sim = BatchedEpisodes(E, device=gpu_device, use_blip2=False, select_frontiers=True, episode_len=L, closed_loop=True)
    fresh = BatchedEpisodes(E, device=gpu_device, use_blip2=False, select_frontiers=True, episode_len=L, closed_loop=True)
    start = sim.pose_table[0].copy()
    for _ in range(L):
        sim.step()
    assert (sim.live.stats["turn_steps"] >= 12).all()
    sim.step()                                                       # step 20: the wrap
    fresh.step()
    torch.cuda.synchronize()
    assert np.array_equal(sim.last_poses, start) and np.array_equal(fresh.last_poses, start) and sim.episodes_done == 1
    assert sim.last_modes == ["initialize"] * E and (sim.last_world_actions == ACTION_TURN_LEFT).all()
    # the maps hold this one step only: the planes and the confidence of a fresh harness's first step (the stub cosines, and
    # with them the values, are 20 draws further on)
    for name in ("obstacle_bits", "navigable_bits", "explored_bits"):
        assert _equal(getattr(sim.obstacles, name), getattr(fresh.obstacles, name)), name
    assert _equal(sim.values.conf, fresh.values.conf)
    assert (sim.live.stats["forward_steps"] + sim.live.stats["turn_steps"] + sim.live.stats["stops"]
            == L + 1).all()                                          # the statistics run on across episodes
