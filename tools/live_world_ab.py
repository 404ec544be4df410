"""Same behaviour of the closed-loop world, shown against the parent commit (profiles/live_world_ab.txt (1)).

    python tools/live_world_ab.py dump parent|change full|grid OUT.pkl    # from the root of the tree under test
    python tools/live_world_ab.py compare A.pkl B.pkl LABEL

``dump`` steps BatchedEpisodes(4, height=48, width=64, use_blip2=False, select_frontiers=True, closed_loop=True, object_maps=True,
world_objects=WorldObjects(max_episode_steps=12), ...) 60 times -- ``full``: objectnav_metrics, render_rgb and
ProceduralWorlds(seed=3) on; ``grid``: GridWorlds over the two plans of tests/test_grid_worlds_cpu.py -- and writes after every step
the live frames, ids, RGB, seen stats, poses, objects, episode counters, modes, goals, actions and both statistics as bytes;
``parent`` reads them under the attribute names BatchedEpisodes had before worlds.LiveWorld, ``change`` as sim.live.<name>.
``compare`` prints "identical" or the first differing step and arrays (exit status 1).  Procedure: export the parent commit next
to this tree (git archive), give it the same native library, dump both sides in one GPU session, compare."""
import hashlib
import os
import pickle
import sys

PARENT = {"frames": "_live_frames", "ids": "_live_ids", "rgb": "last_rgb", "xy": "world_xy", "k": "world_k",
          "stats": "closed_loop_stats", "objectnav_stats": "objectnav_stats", "collided": "_collided",
          "seen_stats": "_live_stats", "ep_clock": "_ep_clock", "ep_index": "_ep_index", "objects": "_objects"}


def dump(side: str, cfg: str, out: str) -> None:
    import numpy as np
    import torch

    sys.path.insert(0, os.getcwd())
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import vlfm_amd.harness as harness
    from vlfm_amd.synthetic import GridWorlds, ProceduralWorlds

    print("harness:", harness.__file__, flush=True)

    def get(sim, name):
        return getattr(sim, PARENT[name]) if side == "parent" else getattr(sim.live, name)

    def raw(v) -> bytes:
        if v is None:
            return b"None"
        if torch.is_tensor(v):
            v = v.cpu().numpy()
        if isinstance(v, dict):
            return b"".join(k.encode() + raw(v[k]) for k in sorted(v))
        if isinstance(v, list) and v and isinstance(v[0], str):
            return "|".join(v).encode()
        return np.ascontiguousarray(np.asarray(v)).tobytes()

    kw = dict(height=48, width=64, use_blip2=False, select_frontiers=True, closed_loop=True, object_maps=True,
              world_objects=harness.WorldObjects(max_episode_steps=12))
    if cfg == "full":
        kw.update(objectnav_metrics=True, render_rgb=True, worlds=ProceduralWorlds(seed=3))
    else:
        from test_grid_worlds_cpu import _two_plans

        kw.update(worlds=GridWorlds(_two_plans(), seed=3))
    sim = harness.BatchedEpisodes(4, **kw)
    steps = []
    for _ in range(60):
        sim.step()
        torch.cuda.synchronize()
        rec = {n: raw(get(sim, n)) for n in ("frames", "ids", "xy", "k", "collided", "seen_stats", "ep_clock", "ep_index", "objects",
                                             "stats", "objectnav_stats")}
        rec["rgb"] = raw(get(sim, "rgb")) if cfg == "full" else b"off"
        rec.update(last_poses=raw(sim.last_poses), last_modes=raw(sim.last_modes), last_goals=raw(sim.last_goals),
                   last_world_actions=raw(sim.last_world_actions), last_episode_end=raw(sim.last_episode_end))
        steps.append(rec)
    summary = sim.objectnav_summary() if side == "parent" else sim.live.objectnav_summary()
    print(side, cfg, "episodes:", summary, "bytes/step:", sum(len(v) for v in steps[-1].values()), flush=True)
    with open(out, "wb") as f:
        pickle.dump(steps, f)


def compare(path_a: str, path_b: str, label: str) -> int:
    a, b = (pickle.load(open(p, "rb")) for p in (path_a, path_b))
    verdict = "identical" if len(a) == len(b) else f"DIFFERENT step counts {len(a)} {len(b)}"
    for t, (ra, rb) in enumerate(zip(a, b)):
        bad = [n for n in ra if ra[n] != rb.get(n)] + [n for n in rb if n not in ra]
        if bad:
            verdict = f"DIFFERENT first at step {t}: {bad}"
            break
    n_bytes = sum(len(v) for r in a for v in r.values())
    digest = [hashlib.sha256(b"".join(r[n] for r in d for n in sorted(r))).hexdigest()[:16] for d in (a, b)]
    print(f"{label}: {len(a)} steps, {len(a[0])} arrays per step ({', '.join(sorted(a[0]))}), {n_bytes} bytes per dump: {verdict}"
          f" (sha256 {digest[0]} | {digest[1]})")
    return 0 if verdict == "identical" else 1


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(*sys.argv[2:5])
    else:
        sys.exit(compare(*sys.argv[2:5]))
