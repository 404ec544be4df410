"""The closed-loop world's episode life cycle (vlfm_amd/worlds.py: LiveWorld) on the host: a renderer that answers with the
NumPy statements stands in for the device, a script for the policy.  No GPU."""
import itertools

import numpy as np
import pytest

import vlfm_amd.synthetic as S
from live_world_cases import E, H, TARGETS3, W, NumpyRenderer, actions_at, planes_of
from vlfm_amd.worlds import LiveWorld, WorldObjects

STATE = ["xy", "k", "collided", "start_xy", "start_k", "table", "world_of", "world_episode", "stats", "objects", "object_classes",
         "target_slot", "ep_index", "ep_clock", "ep_path", "ep_first", "ep_geodesic", "distance_to_goal", "geodesic", "frames",
         "ids", "seen_stats", "sightings", "rgb", "objectnav_stats"]
STEPS, MAX_STEPS = 20, 6
SUCCESS_AT, WRONG_STOP_AT = 3, 1          # environment 0 stops at the target in step 3, environment 1 at nothing in step 1


def _layout(worlds):
    def layout(env_id, episode, robot_xy):
        """The target 1 m in front of environment 0 at its world's start heading; a distractor there for the others."""
        c, s = S.HEADINGS[worlds.world(env_id, episode).start_k]
        cls = TARGETS3[env_id] if env_id == 0 else "tv"
        return [(cls, S.object_box(cls, robot_xy[0] + c, robot_xy[1] + s))]
    return layout


def _records(layout):
    rec = np.zeros((S.WORLD_MAX_OBJECTS, 8))
    for k, (_, box) in enumerate(layout):
        rec[k, :6], rec[k, 6] = box, 1.0
    return rec


def test_episode_life_cycle():
    worlds = S.ProceduralWorlds(seed=3)
    layout = _layout(worlds)
    live = LiveWorld(NumpyRenderer(), range(E), TARGETS3, WorldObjects(max_episode_steps=MAX_STEPS, min_pixels=4, layout=layout),
                     S.ProceduralWorlds(seed=3))
    assert TARGETS3[1] != "tv" != TARGETS3[2] and live.target_slot.tolist() == [0, -1, -1]
    clock, path, episode, want = np.zeros(E, int), np.zeros(E), np.zeros(E, int), []
    for t in range(STEPS):
        planes = planes_of(live)
        frames = live.observe()
        assert frames is live.frames and frames.numpy().tobytes() == planes[0].tobytes()
        assert live.ids.numpy().tobytes() == planes[1].tobytes() and live.seen_stats.tobytes() == planes[2].tobytes()
        stop = np.array([t == SUCCESS_AT, t == WRONG_STOP_AT, False])
        done = live.end_episodes(["navigate" if s else "explore" for s in stop], stop)
        clock += 1
        ends = {0: "success"} if t == SUCCESS_AT else {1: "wrong_stop"} if t == WRONG_STOP_AT else {}
        ends.update({e: "timeout" for e in range(E) if clock[e] >= MAX_STEPS and e not in ends})
        assert done == sorted(ends)
        want += [(e, ends[e], clock[e], path[e]) for e in done]
        clock[done], path[done] = 0, 0.0
        episode[done] += 1
        ended = np.zeros(E, bool)
        ended[done] = True
        live.start_episodes(done)
        for e in done:                          # episode k + 1's world, from its start, nothing refused, a fresh layout
            w = worlds.world(e, episode[e])
            assert live.world_episode[e] == live.ep_index[e] == episode[e] and np.array_equal(live.table.world(e), w.boxes)
            assert np.array_equal(live.xy[e], w.start_xy) and live.k[e] == w.start_k and not live.collided[e]
            assert np.array_equal(live.start_xy[e], w.start_xy) and live.start_k[e] == w.start_k
            assert np.array_equal(live.objects[e], _records(layout(e, episode[e], w.start_xy)))
            assert live.ep_clock[e] == 0 and live.ep_path[e] == 0.0 and live.ep_first[e] == -1
        acts = actions_at(t)
        extra = np.where(live.objects[:, :, 6:7] != 0.0, live.objects[:, :, :4], np.nan)
        moved = S.step_poses(live.xy, live.k, np.where(ended, S.ACTION_STOP, acts), extra, live.table.boxes)
        taken = live.advance(acts, ended)
        assert np.array_equal(taken, np.where(ended, S.ACTION_STOP, acts))
        assert all(np.array_equal(a, b) for a, b in zip((live.xy, live.k, live.collided), moved))
        path += 0.25 * ((taken == S.ACTION_FORWARD) & ~live.collided)
        assert np.array_equal(live.ep_path, path) and np.array_equal(live.ep_clock, clock)
    st = live.objectnav_stats
    outcomes = [o for _, o, _, _ in want]
    assert outcomes.count("success") == 1 and outcomes.count("wrong_stop") == 1 and outcomes.count("timeout") == len(want) - 2 >= 3
    assert (st["episode_env"], st["episode_outcome"]) == ([e for e, _, _, _ in want], outcomes)
    assert st["episode_steps"] == [c for _, _, c, _ in want] and st["episode_path_length"] == [p for _, _, _, p in want]
    assert want[0][1:3] == ("wrong_stop", WRONG_STOP_AT + 1) and want[1][1:3] == ("success", SUCCESS_AT + 1) and want[1][3] > 0
    assert st["episode_first_sighting"][1] == 0 and st["episode_first_sighting"][0] == -1      # seen at once; no target to see
    assert st["successes"].tolist() == [1, 0, 0] and st["wrong_stops"].tolist() == [0, 1, 0] and not st["no_frontier_stops"].any()
    assert np.array_equal(st["episodes"], episode) and st["episodes"].sum() == len(want)
    assert live.stats["path_length"].sum() == sum(p for _, _, _, p in want) + path.sum() > 0
    # reset(): the running episodes end as timeouts; everybody starts the next one
    running = np.flatnonzero(clock > 0)
    assert len(running) and len(running) + (clock == 0).sum() == E
    live.reset()
    assert st["episode_env"][len(want):] == running.tolist() and st["episode_outcome"][len(want):] == ["timeout"] * len(running)
    assert st["episode_steps"][len(want):] == clock[running].tolist() and st["episode_path_length"][len(want):] == path[running].tolist()
    episode[running] += 1
    assert np.array_equal(live.ep_index, episode) and np.array_equal(live.world_episode, episode) and not live.ep_clock.any()
    assert all(np.array_equal(live.xy[e], worlds.world(e, episode[e]).start_xy) for e in range(E)) and not live.collided.any()
    assert live.objectnav_summary() == {"episodes": len(want) + len(running), "success_rate": 1 / (len(want) + len(running))}


@pytest.mark.parametrize("objects, worlds, metrics, rgb", [c for c in itertools.product((False, True), ("rooms", "procedural", "grid"),
                                                                                        (False, True), (False, True))
                                                           if (c[0] or not c[2]) and not (c[1] == "grid" and (c[2] or c[3]))])
def test_every_attribute_exists_in_every_mode(objects, worlds, metrics, rgb):
    """The mode combinations BatchedEpisodes admits; after one step of each, what a mode does not use is None."""
    occ = np.zeros((40, 40), bool)
    occ[[0, -1]], occ[:, [0, -1]] = True, True
    made = {"rooms": None, "procedural": S.ProceduralWorlds(seed=3),
            "grid": S.GridWorlds([S.GridPlan.uniform(occ, 4, -20, -20)], starts=[(0.0, 0.0, 0)], spots=[[(2.0, 2.0), (-2.0, 1.0), (1.0, -3.0)]])}
    live = LiveWorld(NumpyRenderer(), range(E), TARGETS3, WorldObjects(max_episode_steps=1) if objects else None, made[worlds],
                     metrics, rgb)
    assert live.observe().shape == (E, H, W)
    if objects:
        assert live.end_episodes(["explore"] * E, np.zeros(E, bool)) == [0, 1, 2]
        live.start_episodes(range(E))
    live.advance(actions_at(0), np.ones(E, bool))
    unused = {"world_episode": worlds == "rooms", "rgb": not rgb, "frames": False, "xy": False, "k": False, "collided": False,
              "start_xy": False, "start_k": False, "table": False, "world_of": False, "stats": False}
    unused.update({name: not metrics for name in ("ep_geodesic", "distance_to_goal", "geodesic")})
    for name in STATE:
        assert (vars(live)[name] is None) == unused.get(name, not objects), name
    assert (live.ep_index.tolist() == [1] * E) if objects else (live.objectnav_stats is None)
