"""-m gpu: BatchedEpisodes(closed_loop=True, world_objects=WorldObjects(...)): objects stand in the rooms world, the detector
head reports what the ray caster saw of them, they block the robot, and the environments run scored ObjectNav episodes."""
import numpy as np
import pytest

from vlfm_amd import synthetic as S
from vlfm_amd.policy_step import ACTION_FORWARD
from world_object_cases import A, render

pytestmark = pytest.mark.gpu

# environment 1 starts at (1.75, 1.866) heading east: a bed in front of the hall's east doorway, 1.2 m ahead of it
BED = (2.95, 1.42, 3.95, 2.32, 0.0, 0.7)
# behind the hall's north wall segment (and 5.1 m from (0, 0)): never seen from the start of environment 0
HIDDEN = (0.5, 4.8, 1.0, 5.3, 0.0, 0.9)


def _first_episode(per_env):
    """A layout that places ``per_env[env_id]`` in the environment's first episode and nothing afterwards."""
    return lambda env_id, episode, robot_xy: list(per_env.get(env_id, [])) if episode == 0 else []


def _sim(device, E, layout=None, wo=None, **kw):
    from vlfm_amd.harness import BatchedEpisodes, WorldObjects

    world = WorldObjects(**({} if layout is None else {"layout": layout}), **(wo or {}))
    return BatchedEpisodes(E, device=device, use_blip2=False, select_frontiers=True, episode_len=500, closed_loop=True,
                           world_objects=world, **kw)


def _bits(t):
    import torch

    return t.contiguous().view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def _equal(a, b) -> bool:
    import torch

    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def test_without_objects_it_is_the_closed_loop_step(gpu_device):
    import torch

    from vlfm_amd.harness import BatchedEpisodes

    E = 3
    with_objects = _sim(gpu_device, E, layout=lambda env_id, episode, robot_xy: [])
    plain = BatchedEpisodes(E, device=gpu_device, use_blip2=False, select_frontiers=True, episode_len=500, closed_loop=True)
    for t in range(30):
        with_objects.step()
        plain.step()
        torch.cuda.synchronize()
        assert _equal(with_objects.live.frames, plain.live.frames), t
        assert not bool(with_objects.live.ids.any()), t
        fa, fb = with_objects.obstacles.frontiers_px(), plain.obstacles.frontiers_px()
        assert len(fa) == len(fb) and all(np.array_equal(x, y) for x, y in zip(fa, fb)), t
        assert np.array_equal(with_objects.last_goals, plain.last_goals, equal_nan=True), t
        assert with_objects.last_modes == plain.last_modes, t
        assert np.array_equal(with_objects.last_poses, plain.last_poses), t
        assert np.array_equal(with_objects.last_world_actions, plain.last_world_actions), t
    assert np.array_equal(with_objects.live.xy, plain.live.xy) and np.array_equal(with_objects.live.k, plain.live.k)
    for name in ("obstacle_bits", "navigable_bits", "explored_bits"):
        assert _equal(getattr(with_objects.obstacles, name), getattr(plain.obstacles, name)), name
    assert _equal(with_objects.values.conf, plain.values.conf) and _equal(with_objects.values.value, plain.values.value)
    assert not with_objects.live.objectnav_stats["episodes"].any() and (with_objects.live.ep_clock == 30).all()


def test_target_in_line_of_sight_is_found_and_reached(gpu_device):
    """Environment 0 starts at (0, 0) heading east with its target, the chair A, 2.25 m ahead.  Measured on an MI355X: the
    chair is sighted at step 0, the policy navigates from step 12 on, walks 6 steps and stops 0.75 m from the chair's footprint:
    success after 19 steps."""
    import torch

    E, cap = 2, 100
    sim = _sim(gpu_device, E, layout=_first_episode({0: [("chair", A)]}), wo=dict(max_episode_steps=cap), object_maps=True)
    assert sim.targets[0] == "chair" and sim.live.xy[0].tolist() == [0.0, 0.0] and sim.live.k[0] == 0
    modes, goals = [], []
    st = sim.live.objectnav_stats
    while st["episodes"][0] == 0 and len(modes) < cap + 1:
        sim.step()
        modes.append(sim.last_modes[0])
        goals.append(sim.last_goals[0].copy())
        if len(modes) == 1:
            assert sim.object_maps[0].has_object("chair")
    torch.cuda.synchronize()
    print("steps of the episode:", st["episode_steps"], "outcome:", st["episode_outcome"], "first sighting:",
          st["episode_first_sighting"], "robot:", sim.live.xy[0], "goal at step 12:", goals[12] if len(goals) > 12 else None)
    assert modes[:12] == ["initialize"] * 12 and modes[12] == "navigate"
    assert S.rect_distance(goals[12], A) <= 0.1
    assert st["episodes"][0] == 1 and st["successes"][0] == 1 and st["episode_outcome"][0] == "success"
    assert st["episode_env"][0] == 0 and st["episode_steps"][0] == len(modes) <= cap
    assert 0 <= st["episode_first_sighting"][0] < 12
    assert st["episode_path_length"][0] == sim.live.stats["path_length"][0] > 0
    assert sim.last_stops[0] and sim.last_episode_end[0] and not sim.last_episode_end[1]
    assert S.rect_distance(sim.live.xy[0], A) <= 1.0
    # the environment starts its next episode in place: maps, object map and clock are fresh, the neighbour's are not
    assert sim.live.ep_index[0] == 1 and sim.live.ep_clock[0] == 0
    assert not sim.object_maps[0].has_object("chair")
    assert not bool(sim.values.conf[0].any()) and bool(sim.values.conf[1].any())
    assert not bool(sim.obstacles.explored_bits[0].any()) and bool(sim.obstacles.explored_bits[1].any())
    assert not sim.live.objects[0].any()                                   # the second episode's layout: nothing
    where = sim.live.xy[0].copy()
    sim.step()                                                         # (the stop did not move the robot; a new episode initialises)
    assert np.array_equal(sim.last_poses[0, :2], where) and sim.last_modes[0] == "initialize" and sim.live.ep_clock[0] == 1


def test_a_distractor_in_view_is_not_a_detection(gpu_device):
    sim = _sim(gpu_device, 2, layout=_first_episode({0: [("chair", HIDDEN), ("tv", A)]}), object_maps=True)
    seen = set()
    for t in range(14):
        sim.step()
        seen |= {(s[1], s[2]) for s in sim.live.sightings if s[0] == 0}
        if t == 12:
            assert sim.last_modes[0] == "explore"
    assert seen == {("tv", 0.9)}                                       # the distractor was in view, the target never
    assert sim.object_stats["detections"] == 0 and sim.object_stats["masks"] == 0
    assert not sim.object_maps[0].has_object("chair") and sim.last_modes[0] == "explore"


def test_objects_block_the_robot(gpu_device):
    from vlfm_amd.harness import ReplayController

    E, steps = 2, 11
    drive = ReplayController(np.full((steps, E), ACTION_FORWARD))
    sim = _sim(gpu_device, E, layout=_first_episode({0: [("chair", A)]}), controller=drive)
    xs = []
    for _ in range(steps):
        sim.step()
        xs.append(sim.live.xy[0].copy())
    # 0.25 m steps towards the face at x = 2.25: x = 2.0 keeps the 0.2 m margin, x = 2.25 would not
    assert [float(p[0]) for p in xs] == [0.25 * i for i in range(1, 9)] + [2.0] * 3 and all(p[1] == 0.0 for p in xs)
    assert sim.live.stats["collisions"][0] == 3 and sim.live.stats["path_length"][0] == 2.0
    # without the object nothing stops the robot there
    assert not S.step_poses([[2.0, 0.0]], [0], [ACTION_FORWARD])[2][0]


def test_the_mask_is_the_instance(gpu_device):
    import torch

    sim = _sim(gpu_device, 2, layout=_first_episode({0: [("tv", (3.2, 0.6, 3.6, 1.0, 0.0, 1.3)), ("chair", A)]}), object_maps=True)
    sim.step()
    torch.cuda.synchronize()
    envs, masks = sim.last_masks
    want_depth, want_ids = render((0.0, 0.0, 0), [(3.2, 0.6, 3.6, 1.0, 0.0, 1.3), A], 480, 640)
    assert envs == [0] and masks.dtype == torch.bool and masks.shape == (1, 480, 640)
    assert np.array_equal(masks[0].cpu().numpy(), want_ids == 2) and int(masks.sum()) == 13485      # the chair is slot 1
    assert torch.equal(masks[0], sim.live.ids[0] == 2)
    assert np.array_equal(sim.live.frames[0].cpu().numpy().view(np.int32), want_depth.view(np.int32))
    assert sim.object_stats["detections"] == 1 and sim.object_stats["masks"] == 1


def _run(device, steps=60):
    import torch

    sim = _sim(device, 3, wo=dict(max_episode_steps=25), object_maps=True)
    poses = []
    for _ in range(steps):
        sim.step()
        poses.append(sim.last_poses.copy())
    torch.cuda.synchronize()
    sim.check()
    return sim, np.stack(poses)


def test_runs_are_reproducible_and_the_counts_add_up(gpu_device):
    a, pa = _run(gpu_device)
    b, pb = _run(gpu_device)
    assert np.array_equal(pa, pb)
    sa, sb = a.live.objectnav_stats, b.live.objectnav_stats
    assert sa.keys() == sb.keys()
    for key in sa:
        assert np.array_equal(np.asarray(sa[key]), np.asarray(sb[key])), key
    for name in ("obstacle_bits", "navigable_bits", "explored_bits"):
        assert _equal(getattr(a.obstacles, name), getattr(b.obstacles, name)), name
    assert _equal(a.values.conf, b.values.conf) and _equal(a.values.value, b.values.value)
    assert np.array_equal(a.live.objects, b.live.objects)
    total = sa["successes"] + sa["wrong_stops"] + sa["no_frontier_stops"] + sa["timeouts"]
    assert np.array_equal(sa["episodes"], total) and (sa["episodes"] >= 2).all()          # 60 steps, at most 25 per episode
    assert len(sa["episode_steps"]) == len(sa["episode_outcome"]) == len(sa["episode_path_length"]) == int(sa["episodes"].sum())
    assert all(1 <= n <= 25 for n in sa["episode_steps"])
    for e in range(3):
        mine = [n for n, env in zip(sa["episode_steps"], sa["episode_env"]) if env == e]
        assert sum(mine) + a.live.ep_clock[e] == 60
        assert np.array_equal(a.live.ep_index, sa["episodes"])
    # every episode drew the default layout: the environment's target and one distractor, away from the robot
    for e in range(3):
        assert a.live.object_classes[e][0] == a.targets[e] and len(a.live.object_classes[e]) == 2 and a.live.target_slot[e] == 0


def test_the_real_detector_head_reports_the_visible_boxes(gpu_device):
    """The YOLOv7 client (random weights) at E = 2: the sightings go through its own NMS / scale_coords / rounding
    (yolov7.py:91-110) and come back as the visible bounding boxes, within the 2 pixels tests/test_full_step_gpu.py allows that
    path."""
    import torch

    from vlfm_amd.vlm.yolov7 import YOLOv7

    det = YOLOv7(device=gpu_device, allow_random_init=True, width_multiple=0.25)
    sim = _sim(gpu_device, 2, layout=_first_episode({0: [("chair", A)], 1: [("bed", BED)]}), detector=det, object_maps=True,
               scripted_masks=True)
    assert sim.scripted_through_nms and sim.targets[:2] == ["chair", "bed"]
    seen = 0
    for t in range(12):
        sim.step()
        torch.cuda.synchronize()
        want = sim._scripted_detections(t)               # from the sightings of the frames this step rendered
        got = sim.last_detections
        for e in range(2):
            w = want[e]
            w.filter_by_class(sim.targets[e].split("|"))
            w.filter_by_conf(sim.det_threshold)
            assert got[e].num_detections == w.num_detections, (t, e, got[e].phrases, w.phrases)
            for i in range(w.num_detections):
                assert got[e].phrases[i] == w.phrases[i] and abs(float(got[e].logits[i]) - 0.9) <= 2e-3
                px = (got[e].boxes[i].cpu() - w.boxes[i]).abs() * torch.tensor([640.0, 480.0, 640.0, 480.0])
                assert float(px.max()) <= 2.0, (px, got[e].boxes[i], w.boxes[i])
                seen += 1
    assert sim.object_stats.get("head_mismatch", 0) == 0 and seen >= 4
    # step 0 of environment 0: the visible bounding box of A (columns 277-363, rows 237-391)
    assert sim.live.objectnav_stats["episodes"].sum() == 0
