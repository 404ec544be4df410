"""What the map planner (csrc/map_planner.hip, ObstacleMapBatch.plan_paths, synthetic.MapPlannerController) costs and what it
buys, measured in one place.

  (a) kernel time of plan_paths_kernel from `rocprofv3 --kernel-trace --stats`, in a run of its own (a fresh child process:
      tracing slows the host, so nothing else is timed there), at 8 / 128 / 256 jobs on the mid-episode maps of a 256-environment
      closed-loop harness, both residences (the default windows: LDS; whole-map windows: the global scratch); and, from the same
      trace, the per-step kernel time of the depth pass and of the obstacle pipeline of that harness.
  (b) call time of ObstacleMapBatch.plan_paths by device events around the Python call (job upload, memset, launch, read-back
      and the wait included: what a step pays), same jobs, median (min-max) of --reps calls after warm-up; beside it the depth
      pass + obstacle pipeline of one harness step (ingest + update_after_ingest), timed the same way.
  (c) closed-loop env-steps/s and refused moves per environment at 256 environments, BangBangController and
      MapPlannerController alternating over the same windows in one process (no model: stub cosines, which makes the planner's
      share of the step as large as it gets).
  (d) objectnav_summary() for both controllers with world_objects + objectnav_metrics.

    python tools/map_planner_probe.py [--reps 50] [--steps 20] [--skip-steps] [--skip-trace] [--out profiles/map_planner_probe.txt]
    python tools/map_planner_probe.py --trace-child        # the process (a) points rocprofv3 at"""
import argparse
import glob
import os
import shutil
import sqlite3
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

JOBS = (8, 128, 256)
TRACE_LAUNCHES, TRACE_WARMUP, TRACE_STEPS = 20, 3, 10
DEPTH_KERNELS = ("depth_ingest_kernel", "fill_small_holes_kernel", "hole_scatter_kernel")       # the depth pass
OBSTACLE_KERNELS = ("navigable_kernel", "fog_of_war_kernel", "explored_select_kernel", "frontier_prepare_kernel", "frontier_kernel")


def timed(fn) -> float:
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3   # microseconds


def stats(xs):
    import numpy as np

    return float(np.median(xs)), float(np.min(xs)), float(np.max(xs))


def mid_episode(E: int = 256, controller=None, **kw):
    """A closed-loop harness without a model whose maps are mid-episode: 30 map-only steps, then the initialisation turns and the
    first decisions (with world objects: 45 steps of the full harness, whose episodes are being scored)."""
    import torch

    from vlfm_amd.harness import BatchedEpisodes

    sim = BatchedEpisodes(E, device=torch.device("cuda:0"), use_blip2=False, select_frontiers=True, episode_len=500,
                          closed_loop=True, controller=controller, **kw)
    if "world_objects" not in kw:
        sim.fast_forward(30)
    for _ in range(15 if "world_objects" not in kw else 45):
        sim.step()
    return sim


def jobs_of(sim, n: int):
    """(starts, goals, slots) of ``n`` planning jobs: the robots' poses and the goals of the last step (environments with a
    finite goal, repeated in order when there are fewer than ``n``)."""
    import numpy as np

    have = np.flatnonzero(np.isfinite(sim.last_goals).all(axis=1))
    env = have[np.arange(n) % len(have)]
    return sim.last_poses[env, :2], sim.last_goals[env], env


def whole_map(sim, n: int):
    import numpy as np

    S = sim.obstacles.size
    return np.tile(np.array([0, S - 1, 0, S - 1]), (n, 1))


def trace_child() -> None:
    """Per job count and residence TRACE_WARMUP + TRACE_LAUNCHES planning calls, in the order of JOBS x (lds, scratch); then
    TRACE_STEPS steps of the harness."""
    import torch

    sim = mid_episode()
    for n in JOBS:
        starts, goals, env = jobs_of(sim, n)
        for windows in (None, whole_map(sim, n)):
            for _ in range(TRACE_WARMUP + TRACE_LAUNCHES):
                sim.obstacles.plan_paths(starts, goals, env_ids=env, windows=windows)
    torch.cuda.synchronize()
    for _ in range(TRACE_STEPS):
        sim.step()
    torch.cuda.synchronize()


def probe_trace(lines, workdir: str) -> None:
    import numpy as np

    if shutil.which("rocprofv3") is None:
        raise RuntimeError("rocprofv3 not found: the kernel-time leg needs it (--skip-trace leaves the leg out)")
    shutil.rmtree(workdir, ignore_errors=True)
    os.makedirs(workdir)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", workdir, "-o", "map_planner", "--", sys.executable,
           os.path.abspath(__file__), "--trace-child"]
    with open(os.path.join(workdir, "child.log"), "w") as log:
        subprocess.run(cmd, check=True, stdout=log, stderr=subprocess.STDOUT, timeout=400)
    dbs = glob.glob(os.path.join(workdir, "**", "*_results.db"), recursive=True)
    if not dbs:
        raise RuntimeError(f"no rocprofv3 database under {workdir}")
    rows = sqlite3.connect(dbs[0]).execute("select name, start, end from kernels order by start").fetchall()
    ours = [((e - s) * 1e-3, s) for (name, s, e) in rows if "plan_paths_kernel" in name]
    per = TRACE_WARMUP + TRACE_LAUNCHES
    if len(ours) != per * 2 * len(JOBS):
        raise RuntimeError(f"expected {per * 2 * len(JOBS)} dispatches of plan_paths_kernel in the trace, found {len(ours)}")
    for i, n in enumerate(JOBS):
        for k, where in enumerate(("lds", "scratch")):
            at = (2 * i + k) * per
            us = np.array([t for t, _ in ours[at + TRACE_WARMUP:at + per]])
            lines.append("kernel jobs=%3d  planes in %-7s  plan_paths_kernel %9.1f us (%.1f-%.1f, %d launches)"
                         % (n, where, *stats(us), len(us)))
            print(lines[-1], flush=True)
    after = ours[-1][1]                                       # the harness steps follow the last planning launch
    for label, keys in (("depth pass", DEPTH_KERNELS), ("obstacle pipeline", OBSTACLE_KERNELS)):
        total = sum((e - s) * 1e-3 for (name, s, e) in rows if s > after and any(k in name for k in keys))
        names = sorted(set(name.split("(")[0] for (name, s, e) in rows if s > after and any(k in name for k in keys)))
        lines.append("kernel E=256 per step  %-17s %9.1f us of kernel time (%d steps; %s)"
                     % (label, total / TRACE_STEPS, TRACE_STEPS, ", ".join(names)))
        print(lines[-1], flush=True)


def probe_calls(reps: int, lines) -> None:
    import numpy as np
    import torch

    from vlfm_amd.synthetic import MAX_DEPTH, MIN_DEPTH

    sim = mid_episode()
    om = sim.obstacles
    for n in JOBS:
        starts, goals, env = jobs_of(sim, n)
        for windows in (None, whole_map(sim, n)):
            out = om.plan_paths(starts, goals, env_ids=env, windows=windows)
            full = om.plan_paths(starts, goals, env_ids=env, windows=windows, return_fields=True)
            same = all(np.array_equal(out[k], full[k]) for k in ("status", "cost", "waypoints_px", "steps"))
            ts = [timed(lambda: om.plan_paths(starts, goals, env_ids=env, windows=windows)) for _ in range(reps + 5)][5:]
            win = out["windows"]
            lines.append("calls  jobs=%3d  planes in %-7s  plan_paths %9.1f us (%.1f-%.1f)   windows up to %d x %d cells, cost %d-%d "
                         "(median %d), %d of %d PLAN_OK; early exit == full run: %s"
                         % (n, out["residence"], *stats(ts), int((win[:, 1] - win[:, 0] + 1).max()),
                            int((win[:, 3] - win[:, 2] + 1).max()), int(out["cost"][out["status"] == 0].min(initial=65535)),
                            int(out["cost"][out["status"] == 0].max(initial=0)),
                            int(np.median(out["cost"][out["status"] == 0])) if (out["status"] == 0).any() else -1,
                            int((out["status"] == 0).sum()), n, same))
            print(lines[-1], flush=True)
    # the depth pass and the obstacle pipeline of one step of the same harness, on the frames and poses of its next step
    t_ep = sim.t % sim.episode_len
    poses, tf = sim._poses_tf(t_ep)
    depth = sim.live.observe(sim.rooms.painter, t_ep, tf=tf)
    torch.cuda.synchronize()
    ti, tu = [], []
    for r in range(reps + 5):
        a = timed(lambda: om.ingest(depth, tf, MIN_DEPTH, MAX_DEPTH, sim.fx, sim.fy, want_colmax=True))
        b = timed(lambda: om.update_after_ingest(tf, MAX_DEPTH, sim.fov))
        if r >= 5:
            ti.append(a)
            tu.append(b)
    lines.append("calls  E=256  depth pass (ObstacleMapBatch.ingest) %9.1f us (%.1f-%.1f)   obstacle pipeline (update_after_ingest) "
                 "%9.1f us (%.1f-%.1f): the same frame and pose again and again, no read-back in either" % (*stats(ti), *stats(tu)))
    print(lines[-1], flush=True)
    del sim
    torch.cuda.empty_cache()


def probe_steps(steps: int, lines) -> None:
    import time

    import torch

    from vlfm_amd.harness import WorldObjects
    from vlfm_amd.synthetic import BangBangController, MapPlannerController

    E = 256
    for label, objectnav in (("frontier exploration", False), ("ObjectNav", True)):
        kw = (lambda: dict(object_maps=True, world_objects=WorldObjects(), objectnav_metrics=True)) if objectnav else dict
        sims = {"BangBangController": mid_episode(E, BangBangController(), **kw()),
                "MapPlannerController": mid_episode(E, MapPlannerController(), **kw())}
        rate = {k: [] for k in sims}
        for _ in range(3):                 # alternating windows
            for name, s in sims.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    s.step()
                torch.cuda.synchronize()
                rate[name].append(E * steps / (time.perf_counter() - t0))
        for name, s in sims.items():
            s.check()
            st, ps = s.live.stats, s.planner_stats
            lines.append("steps  E=%3d  %-20s %-21s %8.1f env-steps/s (%.1f-%.1f over 3 windows of %d steps)   per environment: "
                         "%.2f refused moves, %.1f forward steps, path %.2f m;  plans %d (ok %d, unreachable %d, too long %d, invalid %d)"
                         % (E, label, name, *stats(rate[name]), steps, float(st["collisions"].mean()),
                            float(st["forward_steps"].mean()), float(st["path_length"].mean()), int(ps["plans"].sum()),
                            int(ps["ok"].sum()), int(ps["unreachable"].sum()), int(ps["too_long"].sum()), int(ps["invalid"].sum())))
            print(lines[-1], flush=True)
            if objectnav:
                lines.append("summary E=%3d  %-21s %s" % (E, name, "  ".join(
                    "%s %s" % (k, ("%.4f" % v) if isinstance(v, float) else v) for k, v in s.live.objectnav_summary().items())))
                print(lines[-1], flush=True)
        del sims
        torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--workdir", default=os.path.join(ROOT, "scratch", "map_planner_trace"),
                    help="where the kernel trace of leg (a) is written (removed and rewritten by every run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "map_planner_probe measures on the GPU; there is no CPU path"
    if a.trace_child:
        return trace_child()
    lines = ["map_planner_probe: device %s; mid-episode maps of a 256-environment closed-loop harness without a model (30 map-only "
             "steps + 15 steps); (b) device events around the Python call, median (min-max) of %d calls after 5 warm-up calls; path "
             "lengths in metres are cost * 0.5 / pixels_per_meter, 6 %% long on pure diagonals" % (torch.cuda.get_device_name(0), a.reps)]
    if not a.skip_trace:
        probe_trace(lines, a.workdir)      # first, while this process has nothing queued on the device
    probe_calls(a.reps, lines)
    if not a.skip_steps:
        probe_steps(a.steps, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
