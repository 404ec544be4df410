#!/usr/bin/env python
"""tests/golden/make_golden_v3.py -- the ITMPolicyV3 fixture, from THE REFERENCE'S OWN ``ITMPolicyV3``.

    python tests/golden/make_golden_v3.py            # (re)write tests/golden/policy_hm3d_v3.npz   (needs the reference tree)
    python tests/golden/make_golden_v3.py --check    # regenerate in memory and compare with the committed file

make_golden.gen_policy() drives the reference's ITMPolicyV2 through a scripted episode; here the class it derives from is
the reference's ITMPolicyV3 (itm_policy.py:270-317, real source through oracle/ref_shim.py) bound to a two-prompt
``text_prompt`` and an ``exploration_thresh``, on one scripted HM3D world without sightings (a long explore phase).  The
scripted ``cosine`` is keyed on (step, prompt), so a client that is asked for all prompts of a frame at once answers what
one asked prompt by prompt answers.  Besides what every policy fixture holds, the file records per explore step the
[M, 2] values the reference's ``sort_waypoints`` handed to ``_reduce_values``, ``_last_frontier`` and ``_last_value``.
Data only: arrays and strings, no program text."""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import policy_script as ps  # noqa: E402

NAME = "policy_hm3d_v3"
# (env seed, steps, dataset, objectgoal, non-coco caption): the world of policy_hm3d_explore_long, nothing ever detected
EPISODE = (21, 110, "hm3d", "toilet", "")
TEXT_PROMPT = "Seems like there is a target_object ahead.|There is a lot of area to explore ahead."   # semexp_env/eval.py:63-69
# the midpoint of the scripted cosines' range U(0.15, 0.45): the best target value of a step falls on either side of it
EXPLORATION_THRESH = 0.30
MIN_STEPS_PER_BRANCH = 10


def register() -> None:
    """Make the episode known to policy_script (its tables are keyed by fixture name)."""
    ps.EPISODES[NAME] = EPISODE
    ps.SIGHTINGS[NAME] = {}


def scripted_cosine(step: int, txt: str) -> float:
    """U(0.15, 0.45) keyed on (episode seed, step, which of the two prompts): independent of the order of the calls."""
    which = 1 if "explore" in txt else 0
    return float(np.random.Generator(np.random.PCG64([4242 + EPISODE[0], step, which])).uniform(0.15, 0.45))


class ScriptedVLMV3(ps.ScriptedVLM):
    """policy_script.ScriptedVLM with the (step, prompt)-keyed ``itm.cosine``; nothing but ``cosine`` on the ITM client."""

    def __init__(self, name: str, make_detections) -> None:
        super().__init__(name, make_detections)
        outer = self

        class _Itm:
            def cosine(self, image: np.ndarray, txt: str) -> float:
                outer.prompts.append(txt)
                outer.calls.append((int(image[0, 0, 0]), "itm"))
                return scripted_cosine(int(image[0, 0, 0]), txt)

        self.itm = _Itm()


def reduce_branch(values, thresh: float) -> int:
    """Which channel ITMPolicyV3 ranks by for these frontier values: 1 (exploration) iff every target value is below thresh."""
    return int(max(v[0] for v in values) < thresh)


def generate() -> dict:
    """Relies on exactly two things inside make_golden.gen_policy(): (1) it looks ``ITMPolicyV2`` up on the reference's
    ``itm_policy`` module and ``ScriptedVLM`` on ``policy_script`` BY NAME WHEN IT IS CALLED, so both can be rebound for the
    call; (2) it reads the policy's ``_value_map`` (one channel, flat indices) only AFTER the last ``act`` of the episode, so
    the two-channel map can be set aside at that moment.  ``--check`` fails if either stops holding."""
    from oracle import ref_shim

    import make_golden as mg

    register()
    itm_mod, _ = ref_shim.reference_policy()
    acts, final = [], []
    seen = []   # per call of _reduce_values: the [M, 2] values of the frontiers, in the order of obstacle_map.frontiers

    class BoundV3(itm_mod.ITMPolicyV3):
        def __init__(self, **kw):
            kw.update(text_prompt=TEXT_PROMPT, exploration_thresh=EXPLORATION_THRESH)
            super().__init__(**kw)

        def _reduce_values(self, values):
            seen.append(np.asarray(values, np.float64).reshape(-1, 2))
            return super()._reduce_values(values)

        def act(self, *a, **k):
            try:
                return super().act(*a, **k)
            finally:
                acts.append(1)
                if len(acts) == EPISODE[1]:
                    # gen_policy() stores a ONE-channel value map when the episode is over: hand it the target channel and
                    # keep the real two-channel map for this file's own record
                    final.append(self._value_map)
                    self._value_map = types.SimpleNamespace(_map=final[0]._map,
                                                            _value_map=np.ascontiguousarray(final[0]._value_map[:, :, :1]))

    v2, vlm = itm_mod.ITMPolicyV2, ps.ScriptedVLM
    itm_mod.ITMPolicyV2, ps.ScriptedVLM = BoundV3, ScriptedVLMV3
    try:
        g = mg.gen_policy(NAME)
    finally:
        itm_mod.ITMPolicyV2, ps.ScriptedVLM = v2, vlm
    explore = np.flatnonzero(g["mode"] == "explore")
    counts = g["frontier_counts"][explore]
    explore = explore[counts > 0]          # (an explore step without frontiers stops before it sorts)
    assert len(seen) == len(explore), (len(seen), len(explore))
    assert [len(s) for s in seen] == g["frontier_counts"][explore].tolist()
    branch = np.array([reduce_branch(s, EXPLORATION_THRESH) for s in seen], np.int8)
    n1, n0 = int(branch.sum()), int((branch == 0).sum())
    assert min(n0, n1) >= MIN_STEPS_PER_BRANCH, f"target branch {n0} steps, exploration branch {n1} steps"
    vmap = np.asarray(final[0]._value_map, np.float64)
    assert vmap.shape == (1000, 1000, 2) and not np.any(vmap.reshape(-1, 2)[np.setdiff1d(np.arange(10 ** 6), g["conf_idx"])])
    # both channels on the confidence support (f32 copies, as gen_policy keeps channel 0) and the exact f64 map's digest
    g.update(v3_value_val=vmap.reshape(-1, 2)[g["conf_idx"]].astype(np.float32), v3_value_sha=np.array(mg.sha(vmap)))
    g.update(v3_steps=explore.astype(np.int32), v3_values=np.concatenate(seen), v3_branch=branch,
             exploration_thresh=np.array(EXPLORATION_THRESH), text_prompt=np.array(TEXT_PROMPT))
    return g


REDUCE_TABLE = "v3_reduce_table"


def reduce_cases(seed: int = 2024, n: int = 1000):
    """(values [M][2], threshold) cases for ``_reduce_values``: random lists of 1-12 frontiers (every fifth a single frontier),
    every fourth with its best target value EXACTLY at the threshold (the comparison is a strict <), the rest on either side."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(n):
        m = 1 if i % 5 == 0 else int(rng.integers(2, 13))
        vals = np.round(rng.uniform(0.0, 1.0, size=(m, 2)), 3)
        if i % 8 == 4:      # ties among the target values themselves
            vals[:, 0] = vals[0, 0]
        thresh = float(vals[:, 0].max()) if i % 4 == 0 else float(np.round(rng.uniform(0.0, 1.0), 3))
        out.append((vals, thresh))
    return out


def generate_reduce_table() -> dict:
    """What the reference's ``ITMPolicyV3._reduce_values`` returns for ``reduce_cases()`` (an unbound call: the method reads
    nothing but ``_exploration_thresh``)."""
    from oracle import ref_shim

    itm_mod, _ = ref_shim.reference_policy()
    cases = reduce_cases()
    got = [itm_mod.ITMPolicyV3._reduce_values(types.SimpleNamespace(_exploration_thresh=t), [tuple(v) for v in vals.tolist()])
           for vals, t in cases]
    return dict(counts=np.array([len(v) for v, _ in cases], np.int32), values=np.concatenate([v for v, _ in cases]),
                thresh=np.array([t for _, t in cases]), reduced=np.concatenate([np.asarray(r, np.float64) for r in got]))


def main() -> int:
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    g, table = generate(), generate_reduce_table()
    path, table_path = os.path.join(HERE, NAME + ".npz"), os.path.join(HERE, REDUCE_TABLE + ".npz")
    if args.check:
        bad = []
        for have, file in ((g, path), (table, table_path)):
            with np.load(file, allow_pickle=False) as z:
                bad += [k for k in have if k not in z.files or not np.array_equal(np.asarray(have[k]), z[k],
                                                                                   equal_nan=np.asarray(have[k]).dtype.kind == "f")]
        print("identical" if not bad else f"DIFFERENT: {bad}")
        return int(bool(bad))
    np.savez_compressed(path, **g)
    np.savez_compressed(table_path, **table)
    b = g["v3_branch"]
    print(f"{path}: {os.path.getsize(path)} bytes, {len(b)} sorted steps, target branch {int((b == 0).sum())}, "
          f"exploration branch {int(b.sum())}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
