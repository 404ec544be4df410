"""What a floor plan per environment (synthetic.ProceduralWorlds, harness.WorldTable, vlfm_worlds_raycast,
vlfm_geodesic_fields) costs and what it shows, measured in one place.

  (a) kernel time of the ray caster from `rocprofv3 --kernel-trace --stats`, in a run of its own (a fresh child process), at 8 and
      256 cameras of 640x480 with objects: the rooms world (the renderer's own table of one row, max_boxes = 37), every camera on
      its own row of a 64-box table that holds BOXES (same cameras, same objects: the table is the only difference), and
      generated worlds (cameras at the worlds' start poses, box counts vary).  The three legs alternate over
      --windows windows of TRACE_LAUNCHES launches each; reported per leg: the median over all launches, their min-max, and the
      min-max of the per-window medians.  From the same trace: geodesic_fields_kernel for 256 fields, the rooms world and
      generated worlds.
  (b) closed-loop ObjectNav at 256 environments without a model (stub cosines): env-steps/s, success rate, SPL, SoftSPL for
      BangBangController and MapPlannerController, in the fixed rooms world and in procedural worlds, the four harnesses
      alternating over the same windows in one process (the windows of tools/map_planner_probe.py: 45 steps in, 3 x --steps).

    python tools/procedural_worlds_probe.py [--windows 5] [--steps 20] [--skip-steps] [--skip-trace] [--out profiles/procedural_worlds_probe.txt]
    python tools/procedural_worlds_probe.py --trace-child        # the process (a) points rocprofv3 at"""
import argparse
import glob
import os
import shutil
import sqlite3
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

CAMERAS = (8, 256)
LEGS = ("rooms world (table of one)", "table rows of BOXES", "generated worlds")
TRACE_LAUNCHES, TRACE_WARMUP = 20, 3
H, W = 480, 640


def stats(xs):
    import numpy as np

    return float(np.median(xs)), float(np.min(xs)), float(np.max(xs))


def scenes(n: int):
    """Per leg what one launch needs: (transforms, objects [n,8,8], table or None).  Fixed world: the tour poses of n
    environments and synthetic.object_layout around them; generated: world (e, 0)'s start pose and ProceduralWorlds.layout."""
    import numpy as np
    import torch

    from vlfm_amd import synthetic as S
    from vlfm_amd.harness import RoomsRenderer, WorldTable

    dev = torch.device("cuda:0")
    rooms = RoomsRenderer(list(range(n)), 500, H, W, dev)

    def records(layouts):
        out = np.zeros((n, S.WORLD_MAX_OBJECTS, 8))
        for e, lay in enumerate(layouts):
            for k, (_, box) in enumerate(lay):
                out[e, k, :6], out[e, k, 6] = box, 1.0
        return out

    fixed_tf = rooms.tf_table[0]
    fixed_obj = records([S.object_layout(e, 0, fixed_tf[e, :2, 3]) for e in range(n)])
    rows = WorldTable(n, dev)
    rows.assign(np.arange(n), [S.BOXES] * n)
    worlds = S.ProceduralWorlds(0)
    made = [worlds.world(e, 0) for e in range(n)]
    gen = WorldTable(n, dev)
    gen.assign(np.arange(n), [w.boxes for w in made])
    gen_tf = np.stack([S.tf_of(w.start_xy[0], w.start_xy[1], w.start_k) for w in made])
    gen_obj = records([worlds.layout(e, 0, made[e].start_xy) for e in range(n)])
    counts = [len(w.boxes) for w in made]
    return rooms, {LEGS[0]: (fixed_tf, fixed_obj, None), LEGS[1]: (fixed_tf, fixed_obj, rows), LEGS[2]: (gen_tf, gen_obj, gen)}, counts


def cast(rooms, scene, out):
    import numpy as np

    tf, obj, table = scene
    idx = np.arange(len(tf))
    if table is None:
        return rooms.cast_cameras_objects(tf, obj, idx, out=out)
    return rooms.cast_worlds(tf, table, idx, obj, idx, out=out)


def trace_child(windows: int) -> None:
    """Per camera count: `windows` windows; in each, per leg in the order of LEGS, TRACE_WARMUP + TRACE_LAUNCHES launches.  Then
    the geodesic fields of 256 environments, the rooms world and generated worlds alternating, the same counts."""
    import numpy as np
    import torch

    for n in CAMERAS:
        rooms, legs, _ = scenes(n)
        out = torch.empty((n, H, W), dtype=torch.float32, device="cuda:0")
        for _ in range(windows):
            for leg in LEGS:
                for _ in range(TRACE_WARMUP + TRACE_LAUNCHES):
                    cast(rooms, legs[leg], out)
                torch.cuda.synchronize()
    n = 256
    rooms, legs, _ = scenes(n)
    for _ in range(windows):
        for leg in (LEGS[0], LEGS[2]):
            tf, obj, table = legs[leg]
            for _ in range(TRACE_WARMUP + TRACE_LAUNCHES):
                if table is None:
                    rooms.geodesic_fields(obj, obj[:, 0, :4], 1.0)
                else:
                    rooms.geodesic_fields_worlds(table, np.arange(n), obj, obj[:, 0, :4], 1.0)
            torch.cuda.synchronize()


def probe_trace(lines, workdir: str, windows: int) -> None:
    import numpy as np

    if shutil.which("rocprofv3") is None:
        raise RuntimeError("rocprofv3 not found: the kernel-time leg needs it (--skip-trace leaves the leg out)")
    shutil.rmtree(workdir, ignore_errors=True)
    os.makedirs(workdir)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", workdir, "-o", "procedural_worlds", "--", sys.executable,
           os.path.abspath(__file__), "--trace-child", "--windows", str(windows)]
    with open(os.path.join(workdir, "child.log"), "w") as log:
        subprocess.run(cmd, check=True, stdout=log, stderr=subprocess.STDOUT, timeout=500)
    dbs = glob.glob(os.path.join(workdir, "**", "*_results.db"), recursive=True)
    if not dbs:
        raise RuntimeError(f"no rocprofv3 database under {workdir}")
    rows = sqlite3.connect(dbs[0]).execute("select name, start, end from kernels order by start").fetchall()
    per = TRACE_WARMUP + TRACE_LAUNCHES

    def table(kernel: str, legs, groups, label):
        ours = [((e - s) * 1e-3, name) for (name, s, e) in rows if kernel in name]
        if len(ours) != per * len(legs) * windows * len(groups):
            raise RuntimeError(f"expected {per * len(legs) * windows * len(groups)} dispatches of {kernel}, found {len(ours)}")
        for g, group in enumerate(groups):
            for k, leg in enumerate(legs):
                us = np.array([[t for t, _ in ours[((g * windows + w) * len(legs) + k) * per:][TRACE_WARMUP:per]] for w in range(windows)])
                med = np.median(us, axis=1)
                lines.append("kernel %s  %-27s %-30s %9.1f us (%.1f-%.1f over %d launches; per-window medians %.1f-%.1f, %d windows)"
                             % (label(group), leg, kernel, *stats(us.reshape(-1)), us.size, med.min(), med.max(), windows))
                print(lines[-1], flush=True)

    table("rooms_raycast_objects_kernel", LEGS, CAMERAS, lambda n: "cameras=%3d" % n)
    table("geodesic_fields_kernel", (LEGS[0], LEGS[2]), (256,), lambda n: "fields =%3d" % n)


def mid_episode(E: int, controller, worlds):
    import torch

    from vlfm_amd.harness import BatchedEpisodes, WorldObjects

    sim = BatchedEpisodes(E, device=torch.device("cuda:0"), use_blip2=False, select_frontiers=True, episode_len=500,
                          closed_loop=True, controller=controller, object_maps=True, world_objects=WorldObjects(),
                          objectnav_metrics=True, worlds=worlds)
    for _ in range(45):
        sim.step()
    return sim


def probe_steps(steps: int, lines) -> None:
    import time

    import numpy as np
    import torch

    from vlfm_amd.synthetic import BangBangController, MapPlannerController, ProceduralWorlds

    E = 256
    sims = {}
    for world in ("fixed rooms", "procedural"):
        for ctl in (BangBangController, MapPlannerController):
            sims[(world, ctl.__name__)] = mid_episode(E, ctl(), ProceduralWorlds(0) if world == "procedural" else None)
    rate = {k: [] for k in sims}
    for _ in range(3):                 # alternating windows
        for key, s in sims.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                s.step()
            torch.cuda.synchronize()
            rate[key].append(E * steps / (time.perf_counter() - t0))
    for (world, name), s in sims.items():
        s.check()
        st, ps = s.live.stats, s.planner_stats
        lines.append("steps  E=%3d  ObjectNav  %-12s %-21s %8.1f env-steps/s (%.1f-%.1f over 3 windows of %d steps)   per environment: "
                     "%.2f refused moves, %.1f forward steps, path %.2f m;  plans %d (ok %d, unreachable %d, too long %d, invalid %d)"
                     % (E, world, name, *stats(rate[(world, name)]), steps, float(st["collisions"].mean()),
                        float(st["forward_steps"].mean()), float(st["path_length"].mean()), int(ps["plans"].sum()),
                        int(ps["ok"].sum()), int(ps["unreachable"].sum()), int(ps["too_long"].sum()), int(ps["invalid"].sum())))
        print(lines[-1], flush=True)
        out = s.live.objectnav_stats["episode_outcome"]
        l = np.asarray(s.live.objectnav_stats["episode_geodesic"], np.float64)
        fin = l[np.isfinite(l)]
        lines.append("summary E=%3d  %-12s %-21s %s;  outcomes %s;  start-to-goal geodesic %.2f-%.2f m (median %.2f)"
                     % (E, world, name, "  ".join("%s %s" % (k, ("%.4f" % v) if isinstance(v, float) else v)
                                                  for k, v in s.live.objectnav_summary().items()),
                        ", ".join("%s %d" % (o, out.count(o)) for o in sorted(set(out))),
                        fin.min(initial=np.inf), fin.max(initial=-np.inf), float(np.median(fin)) if len(fin) else float("nan")))
        print(lines[-1], flush=True)
        if world == "procedural":
            counts = s.live.table.counts
            lines.append("worlds E=%3d  %-21s boxes per world %d-%d (median %d); episodes per environment up to %d"
                         % (E, name, counts.min(), counts.max(), int(np.median(counts)), int(s.live.world_episode.max()) + 1))
            print(lines[-1], flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--workdir", default=os.path.join(ROOT, "scratch", "procedural_worlds_trace"),
                    help="where the kernel trace of leg (a) is written (removed and rewritten by every run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "procedural_worlds_probe measures on the GPU; there is no CPU path"
    if a.trace_child:
        return trace_child(a.windows)
    import numpy as np

    from vlfm_amd.synthetic import ProceduralWorlds

    counts = [len(ProceduralWorlds(0).world(e, 0).boxes) for e in range(256)]
    lines = ["procedural_worlds_probe: device %s; (a) rocprofv3 kernel trace of %dx%d frames with objects, legs alternating over "
             "windows of %d launches after %d warm-up launches each; generated worlds: ProceduralWorlds(0).world(e, 0), %d-%d boxes "
             "(median %d) over 256; (b) no model, stub cosines, object maps on"
             % (torch.cuda.get_device_name(0), W, H, TRACE_LAUNCHES, TRACE_WARMUP, min(counts), max(counts), int(np.median(counts)))]
    if not a.skip_trace:
        probe_trace(lines, a.workdir, a.windows)      # first, while this process has nothing queued on the device
    if not a.skip_steps:
        probe_steps(a.steps, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
