"""Multi-prompt scoring, the parts that need no device: prompt splitting / substitution / the text table of a batch, the
validation BatchedEpisodes runs before it asks for a GPU, the V3 reducer against the reference's own ``_reduce_values``
(live where the reference tree exists, and against the committed table tests/golden/v3_reduce_table.npz everywhere), and
the choices THE REFERENCE'S ``ITMPolicyV3`` made in the scripted episode tests/golden/policy_hm3d_v3.npz
(tests/golden/make_golden_v3.py) replayed through the shared reducer + FrontierSelector."""
import os
import sys
import types

import numpy as np
import pytest

from golden_util import GOLDEN_DIR, load, reference_present

if GOLDEN_DIR not in sys.path:
    sys.path.insert(0, GOLDEN_DIR)

V3_PROMPT = "Seems like there is a target_object ahead.|There is a lot of area to explore ahead."


# ------------------------------------------------------------------------------------------------ prompt plumbing
def test_split_and_substitute():
    from vlfm_amd.policy_step import split_text_prompt, substitute_target

    assert split_text_prompt("Seems like there is a target_object ahead.") == ["Seems like there is a target_object ahead."]
    base = split_text_prompt(V3_PROMPT, 0.3)
    assert base == ["Seems like there is a target_object ahead.", "There is a lot of area to explore ahead."]
    assert substitute_target(base, "chair") == ["Seems like there is a chair ahead.", "There is a lot of area to explore ahead."]
    # the "|" of a multi-name category is shown to BLIP-2 as "/" (itm_policy.py:197)
    assert substitute_target(["A target_object, a target_object."], "a|b") == ["A a/b, a a/b."]
    assert split_text_prompt("x|y|z", 0.1) == ["x", "y", "z"]


def test_validation_errors_need_no_device():
    from vlfm_amd.harness import PROMPT, BatchedEpisodes, episode_prompts
    from vlfm_amd.policy_step import split_text_prompt

    with pytest.raises(ValueError, match="Must provide a reduction function when using multiple value channels"):
        split_text_prompt("a|b")
    with pytest.raises(ValueError, match="two"):
        split_text_prompt("a", 0.3)
    with pytest.raises(ValueError):
        episode_prompts("a|b", None, ["chair"])
    # the constructor checks its prompts BEFORE it asks for a device: the same errors with or without a GPU
    with pytest.raises(ValueError, match="Must provide a reduction function"):
        BatchedEpisodes(2, text_prompt=V3_PROMPT)
    with pytest.raises(ValueError, match="two"):
        BatchedEpisodes(2, exploration_thresh=0.3)
    per = episode_prompts(V3_PROMPT, 0.3, ["chair", "potted plant", "a|b"])
    assert per == [["Seems like there is a chair ahead.", "There is a lot of area to explore ahead."],
                   ["Seems like there is a potted plant ahead.", "There is a lot of area to explore ahead."],
                   ["Seems like there is a a/b ahead.", "There is a lot of area to explore ahead."]]
    assert episode_prompts(PROMPT, None, ["tv"]) == [["Seems like there is a tv ahead."]]


def test_text_table_and_index_for_mixed_targets():
    from vlfm_amd.harness import TARGETS, episode_prompts
    from vlfm_amd.vlm.blip2itm import prompt_table

    targets = [TARGETS[i % len(TARGETS)] for i in range(16)]
    per = episode_prompts(V3_PROMPT, 0.3, targets)
    unique, rows = prompt_table(per, 16)
    # 6 targets -> 6 target prompts + ONE shared exploration prompt, in order of first appearance
    assert len(unique) == 7 and unique[1] == "There is a lot of area to explore ahead."
    assert unique[0] == "Seems like there is a chair ahead." and unique[2] == "Seems like there is a bed ahead."
    assert np.asarray(rows).shape == (16, 2)
    for e in range(16):
        assert [unique[i] for i in rows[e]] == per[e]
    assert rows[0] == rows[6] == rows[12] and all(r[1] == 1 for r in rows)
    # one shared list: every image the same row
    unique, rows = prompt_table(["p", "q", "p"], 3)
    assert unique == ["p", "q"] and rows == [[0, 1, 0]] * 3
    for bad, n in (([], 2), ([["a", "b"], ["a"]], 2), ([["a"], ["b"]], 3), ([[], []], 2)):
        with pytest.raises(ValueError):
            prompt_table(bad, n)


def test_text_index_is_validated_where_it_is_built():
    import torch

    from vlfm_amd.vlm import ops

    idx = ops.itc_text_index([[0, 2], [1, 1]], 3, torch.device("cpu"))
    assert idx.dtype == torch.int32 and idx.tolist() == [[0, 2], [1, 1]]
    for rows, n in (([[0, 3]], 3), ([[-1, 0]], 3), ([[0]], 0), ([0, 1], 2), ([[0] * (ops.ITC_MAX_PROMPTS + 1)], 1), ([[]], 1)):
        with pytest.raises(ValueError):
            ops.itc_text_index(rows, n, torch.device("cpu"))


# ------------------------------------------------------------------------------------------------ the reducer
def _table_cases():
    g = load("v3_reduce_table")
    offs = np.concatenate([[0], np.cumsum(g["counts"])])
    return [(g["values"][offs[i]:offs[i + 1]], float(g["thresh"][i]), g["reduced"][offs[i]:offs[i + 1]])
            for i in range(len(g["counts"]))]


def test_reducer_equals_the_references_reduce_values():
    import make_golden_v3 as mg3
    from vlfm_amd.policy_step import ITMPolicyV3Step, explore_reduce_values

    cases = _table_cases()
    assert len(cases) == 1000
    # the committed inputs are the generator's cases: ties at the threshold and single-frontier lists are among them
    for (vals, t, _), (want_vals, want_t) in zip(cases, mg3.reduce_cases()):
        assert np.array_equal(vals, want_vals) and t == want_t
    assert sum(len(v) == 1 for v, _, _ in cases) >= 100 and sum(v[:, 0].max() == t for v, t, _ in cases) >= 200
    ref = None
    if reference_present():
        from oracle import ref_shim

        ref = ref_shim.reference_policy()[0].ITMPolicyV3._reduce_values
    used = [0, 0]
    for i, (vals, t, want) in enumerate(cases):
        as_tuples = [tuple(v) for v in vals.tolist()]
        got = explore_reduce_values(as_tuples, t)
        assert got == want.tolist(), (i, "committed table")
        # the method of the single-environment policy is the same function
        assert ITMPolicyV3Step._reduce_values(types.SimpleNamespace(_exploration_thresh=t), as_tuples) == got
        if ref is not None:
            assert got == ref(types.SimpleNamespace(_exploration_thresh=t), as_tuples), (i, "live reference")
        used[mg3.reduce_branch(vals, t)] += 1
    assert min(used) >= 100, used


# ------------------------------------------------------------------------------------------------ the V3 fixture
def test_v3_fixture_choices_replayed_through_the_shared_reducer():
    """Per explore step of the reference's ITMPolicyV3 episode: the recorded [M, 2] values -> explore_reduce_values ->
    descending order (value_map.py:183) -> FrontierSelector == the reference's ``_last_frontier`` / ``_last_value``."""
    import make_golden_v3 as mg3
    from vlfm_amd.policy_step import FrontierSelector, explore_reduce_values

    g = load(mg3.NAME)
    thresh = float(g["exploration_thresh"])
    assert thresh == mg3.EXPLORATION_THRESH and str(g["text_prompt"]) == mg3.TEXT_PROMPT == V3_PROMPT
    f_offs = np.concatenate([[0], np.cumsum(g["frontier_counts"])])
    v_offs = np.concatenate([[0], np.cumsum(g["frontier_counts"][g["v3_steps"]])])
    branch = [0, 0]
    sel = FrontierSelector()
    for n, k in enumerate(g["v3_steps"]):
        frontiers = g["frontiers"][f_offs[k]:f_offs[k + 1]]
        values = g["v3_values"][v_offs[n]:v_offs[n + 1]]
        assert len(values) == len(frontiers) > 0 and str(g["mode"][k]) == "explore"
        reduced = explore_reduce_values([tuple(v) for v in values.tolist()], thresh)
        use = mg3.reduce_branch(values, thresh)
        assert use == int(g["v3_branch"][n]) and reduced == values[:, use].tolist()
        branch[use] += 1
        order = np.argsort([-v for v in reduced])
        goal, value = sel.choose(frontiers[order], [reduced[i] for i in order], frontiers, g["pose"][k][:2])
        assert np.array_equal(goal, g["last_frontier"][k]), f"step {k}: frontier"
        assert value == float(g["best_value"][k]), f"step {k}: value"
        assert np.array_equal(goal, g["nav_goal"][k]), f"step {k}: goal"
    assert min(branch) >= mg3.MIN_STEPS_PER_BRANCH, branch
    # the scripted cosines are keyed on (step, prompt): the prompts the reference asked for, step by step
    want = ["Seems like there is a toilet ahead.", "There is a lot of area to explore ahead."] * int(mg3.EPISODE[1])
    assert [str(p) for p in g["prompts"]] == want
    assert os.path.getsize(os.path.join(GOLDEN_DIR, mg3.NAME + ".npz")) < (1 << 20)


def test_v3_step_over_the_oracle_maps_reproduces_the_reference_episode(monkeypatch):
    """ITMPolicyV3Step's own logic over the oracle's maps (oracle/ref_*: present everywhere) through the whole episode the
    reference's ITMPolicyV3 ran: every step's mode, frontiers, goal and value; at the end the f32 confidence map and the
    exact f64 two-channel value map (SHA-256 of the reference's array)."""
    import make_golden_v3 as mg3
    import policy_script as ps
    from golden_util import dense, replay_policy_episode, sha, unpack_plane
    from oracle.ref_obstacle_map import RefObstacleMap
    from oracle.ref_value_map import RefValueMap
    from vlfm_amd.policy_step import ITMPolicyV3Step
    from vlfm_amd.vlm.detections import ObjectDetections

    class NoObjects:      # nothing is ever detected in this episode: the object map is only asked and told about explored area
        clouds = {}

        def reset(self):
            pass

        def has_object(self, name):
            return False

        def update_explored(self, *a):
            pass

    mg3.register()
    monkeypatch.setattr(ps, "ScriptedVLM", mg3.ScriptedVLMV3)

    def make(vlm, **kw):
        return ITMPolicyV3Step(mg3.EXPLORATION_THRESH, itm=vlm.itm, coco_detector=vlm.coco, detector=vlm.gdino, sam=vlm.sam,
                               text_prompt=mg3.TEXT_PROMPT, value_map=RefValueMap(2, use_max_confidence=False),
                               obstacle_map=RefObstacleMap(min_height=0.61, max_height=0.88, area_thresh=1.5, agent_radius=0.18),
                               object_map=NoObjects(), **kw)

    pol, g = replay_policy_episode(mg3.NAME, make, ObjectDetections, tol=0.0)
    obstacle, value, _ = pol.maps()
    assert np.array_equal(value._map, dense(g["conf_idx"], g["conf_val"], (1000, 1000), np.float32))
    vmap = np.asarray(value._value_map, np.float64)
    assert vmap.shape == (1000, 1000, 2) and sha(vmap) == str(g["v3_value_sha"])
    assert np.array_equal(obstacle.explored_area.astype(bool), unpack_plane(g["explored"]))
    assert np.array_equal(obstacle._map.astype(bool), unpack_plane(g["obstacles"]))


def test_policy_asks_for_all_prompts_of_a_camera_at_once_when_the_client_can():
    """ITMPolicyV2Step._update_value_map: ONE ``cosines`` call per camera for a client that has it, the reference's call per
    prompt for any other; all cosines first, then the maps camera by camera; the same values reach the map."""
    from vlfm_amd.policy_step import ITMPolicyV3Step

    class Map:
        def __init__(self):
            self.log = []

        def update_map(self, values, *a):
            self.log.append(("map", values.tolist()))

        def update_agent_traj(self, *a):
            self.log.append(("traj",))

    def run(client):
        pol = ITMPolicyV3Step.__new__(ITMPolicyV3Step)
        pol._target_object, pol._text_prompt, pol._itm, pol._value_map = "a|b", V3_PROMPT, client, Map()
        pol._value_map.log = client.log
        cams = [(np.full((2, 2, 3), c, np.uint8), None, None, 0.5, 5.0, 1.0) for c in (1, 2)]
        pol._update_value_map(cams, np.zeros(2), 0.0)
        return client.log

    val = lambda img, p: float(img[0, 0, 0]) + (0.5 if "explore" in p else 0.25)   # noqa: E731

    class Single:
        def __init__(self):
            self.log = []

        def cosine(self, image, txt):
            self.log.append(("cosine", int(image[0, 0, 0]), txt))
            return val(image, txt)

    class Multi(Single):
        def cosines(self, image, prompts):
            self.log.append(("cosines", int(image[0, 0, 0]), list(prompts)))
            return [val(image, p) for p in prompts]

    p = ["Seems like there is a a/b ahead.", "There is a lot of area to explore ahead."]
    assert run(Single()) == [("cosine", 1, p[0]), ("cosine", 1, p[1]), ("cosine", 2, p[0]), ("cosine", 2, p[1]),
                             ("map", [1.25, 1.5]), ("map", [2.25, 2.5]), ("traj",)]
    assert run(Multi()) == [("cosines", 1, p), ("cosines", 2, p), ("map", [1.25, 1.5]), ("map", [2.25, 2.5]), ("traj",)]


def test_reference_cosine_signatures_are_untouched_and_cosines_exists():
    import inspect

    from vlfm_amd.vlm.blip2itm import BLIP2ITM, BLIP2ITMClient

    for cls in (BLIP2ITM, BLIP2ITMClient):
        assert list(inspect.signature(cls.cosine).parameters) == ["self", "image", "txt"]
        assert list(inspect.signature(cls.cosines).parameters) == ["self", "image", "prompts"]


def test_episode_log_applies_the_rule_per_environment(tmp_path, monkeypatch):
    """BatchedEpisodes._log_finished_episodes with a threshold: each environment's best value is the best of ITS frontiers after
    ITS reduction (environment 0 stays below the threshold -> exploration channel, environment 1 reaches it -> target channel);
    an environment without frontiers logs none.  Host code only: run on a stand-in that carries the attributes it reads."""
    import json

    from vlfm_amd.harness import BatchedEpisodes

    class H:
        pass

    h = H()
    h.E, h.C, h.exploration_thresh, h.obstacles = 3, 2, 0.4, None
    h.live, h.closed_loop, h.device_object_clouds = None, False, True
    h.env_ids, h.targets, h.episodes_done, h.episode_len, h.t = [0, 1, 2], ["chair", "bed", "tv"], 0, 5, 5
    h.pose_table = np.zeros((5, 3, 3))
    h.last_frontier_values = np.array([[0.30, 0.20], [0.35, 0.10], [0.50, 0.90], [0.10, 0.95]])
    h.last_frontier_envs = np.array([0, 0, 1, 1])
    monkeypatch.setenv("ZSOS_LOG_DIR", str(tmp_path))
    BatchedEpisodes._log_finished_episodes(h)
    best = [json.load(open(tmp_path / f"{e}_synthetic{e:04d}.json"))["best_frontier_value_last_step"] for e in range(3)]
    assert best == [0.20, 0.50, None]
    # single prompt: the batch-wide maximum, as before
    h.C, h.exploration_thresh, h.episodes_done = 1, None, 1
    h.last_frontier_values = np.array([[0.3], [0.7], [0.5]])
    BatchedEpisodes._log_finished_episodes(h)
    assert json.load(open(tmp_path / "3_synthetic0000.json"))["best_frontier_value_last_step"] == 0.7
