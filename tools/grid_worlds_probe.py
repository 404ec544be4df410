"""What floor plans as occupancy grids (synthetic.GridPlan / GridWorlds, harness.WorldTable(max_grid=...),
vlfm_worlds_raycast_grids) cost, measured in one place.

  (a) kernel time of the ray caster from `rocprofv3 --kernel-trace --stats`, in a run of its own (a fresh child process), at 8 and
      256 cameras of 640x480 with objects, on up to three legs that alternate over --windows windows of TRACE_LAUNCHES launches
      each (their order rotates by one per window): the generated box worlds ProceduralWorlds(0).world(e, 0) through a library built from the PARENT commit
      (--parent-lib: the same device buffers, its vlfm_worlds_raycast; left out when not given), the same box worlds through this
      library (a table without grids: the box-only kernel), and the same worlds rasterised at 20 cells per metre
      (GridPlan.from_boxes: 400 x 400 cells, no boxes; same cameras, same objects, the same frames bit for bit).  Reported per
      leg: the median over all launches, their min-max, and the min-max of the per-window medians; and, from the host statement
      (grid_profile_numpy), the mean number of cells a column's walk enters.
  (b) closed-loop ObjectNav at 256 environments without a model (stub cosines): env-steps/s in procedural box worlds and in
      their rasterised twins, the two harnesses alternating over 3 windows of --steps steps in one process, 45 steps in.

  (c) --geodesic lattice: what scoring SPL on the metric lattice costs (RoomsRenderer.lattice_fields_worlds / lattice_distances):
      kernel times of lattice_free_kernel, lattice_fields_kernel and lattice_query_kernel from a rocprofv3 kernel trace in a child
      process of its own, for 8 and 256 fields of the rooms world and of the 400 x 400 plans of (a); the host statement's time for
      one field of each; and closed-loop env-steps/s at 256 environments in the rooms world with the metrics off, with
      geodesic="graph" and with geodesic="lattice", three harnesses alternating over 3 windows whose leg order rotates.  It
      runs INSTEAD of (a) and (b).

    python tools/grid_worlds_probe.py [--windows 5] [--steps 20] [--parent-lib PATH] [--skip-steps] [--skip-trace] [--out profiles/grid_worlds_probe.txt]
    python tools/grid_worlds_probe.py --geodesic lattice [--steps 20] [--skip-steps] [--skip-trace] [--out profiles/lattice_geodesic_probe.txt]
    python tools/grid_worlds_probe.py --trace-child        # the process (a) points rocprofv3 at
    python tools/grid_worlds_probe.py --lattice-child      # the process (c) points rocprofv3 at"""
import argparse
import ctypes
import glob
import os
import shutil
import sqlite3
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

CAMERAS = (8, 256)
LEG_PARENT, LEG_BOXES, LEG_GRIDS = "box worlds, parent library", "box worlds", "grid worlds 400x400"
TRACE_LAUNCHES, TRACE_WARMUP = 20, 3
H, W = 480, 640
CELLS_PER_METRE = 20


def stats(xs):
    import numpy as np

    return float(np.median(xs)), float(np.min(xs)), float(np.max(xs))


class RasterisedWorlds:
    """ProceduralWorlds(seed) with every world's boxes replaced by their occupancy grid: the box worlds' twins."""

    def __init__(self, seed: int = 0) -> None:
        from vlfm_amd.synthetic import ProceduralWorlds

        self.inner = ProceduralWorlds(seed)
        self.max_grid = (20 * CELLS_PER_METRE, 20 * CELLS_PER_METRE)
        self._made = {}

    def world(self, env_id: int, episode: int):
        import numpy as np

        from vlfm_amd.synthetic import GridPlan, World

        key = (int(env_id), int(episode))
        if key not in self._made:
            w = self.inner.world(*key)
            self._made[key] = World(np.zeros((0, 4)), w.start_xy, w.start_k, w.spots, w.doors, GridPlan.from_boxes(w.boxes, CELLS_PER_METRE))
        return self._made[key]

    def layout(self, env_id: int, episode: int, robot_xy):
        return self.inner.layout(env_id, episode, robot_xy)


class ParentEntry:
    """A library built from the parent commit behind the entry RoomsRenderer._raycast calls: the grid arguments (all NULL in a
    table without grids) are dropped and its vlfm_worlds_raycast is called with the rest."""

    def __init__(self, path: str) -> None:
        from vlfm_amd import _lib

        self.L = ctypes.CDLL(os.path.abspath(path))
        self.L.vlfm_worlds_raycast.argtypes = _lib.lib().vlfm_worlds_raycast.argtypes
        self.L.vlfm_worlds_raycast.restype = ctypes.c_int

    def vlfm_worlds_raycast_grids(self, *a):
        assert a[18] is None and a[19] is None and a[20] is None
        return self.L.vlfm_worlds_raycast(*a[:18], a[23])


def scenes(n: int):
    """(renderer, {leg: (transforms, objects [n,8,8], table)})."""
    import numpy as np
    import torch

    from vlfm_amd import synthetic as S
    from vlfm_amd.harness import RoomsRenderer, WorldTable

    dev = torch.device("cuda:0")
    rooms = RoomsRenderer(list(range(n)), 500, H, W, dev)
    worlds = S.ProceduralWorlds(0)
    made = [worlds.world(e, 0) for e in range(n)]
    plans = [S.GridPlan.from_boxes(w.boxes, CELLS_PER_METRE) for w in made]
    tf = np.stack([S.tf_of(w.start_xy[0], w.start_xy[1], w.start_k) for w in made])
    obj = np.zeros((n, S.WORLD_MAX_OBJECTS, 8))
    for e in range(n):
        for k, (_, box) in enumerate(worlds.layout(e, 0, made[e].start_xy)):
            obj[e, k, :6], obj[e, k, 6] = box, 1.0
    boxes = WorldTable(n, dev)
    boxes.assign(np.arange(n), [w.boxes for w in made])
    grids = WorldTable(n, dev, max_grid=(max(p.ny for p in plans), max(p.nx for p in plans)))
    grids.assign(np.arange(n), [np.zeros((0, 4))] * n, plans)
    return rooms, {LEG_PARENT: (tf, obj, boxes), LEG_BOXES: (tf, obj, boxes), LEG_GRIDS: (tf, obj, grids)}


def walk_steps(n: int):
    """(mean, max) over the columns of the first ``n`` cameras of (a) of the cells a column's walk enters (the host statement)."""
    import numpy as np

    from vlfm_amd import synthetic as S

    worlds = S.ProceduralWorlds(0)
    fx = S.camera_intrinsics(W)[0]
    steps = []
    for e in range(n):
        w = worlds.world(e, 0)
        plan = S.GridPlan.from_boxes(w.boxes, CELLS_PER_METRE)
        steps.append(S.grid_profile_numpy(w.start_xy[0], w.start_xy[1], *S.HEADINGS[w.start_k], fx, W, plan, return_steps=True)[1])
    return float(np.mean(steps)), int(np.max(steps))


def cast(rooms, scene, out, parent=None):
    import numpy as np

    from vlfm_amd import _lib

    tf, obj, table = scene
    idx = np.arange(len(tf))
    if parent is None:
        return rooms.cast_worlds(tf, table, idx, obj, idx, out=out)
    ours, _lib.lib = _lib.lib, lambda: parent
    try:
        return rooms.cast_worlds(tf, table, idx, obj, idx, out=out)
    finally:
        _lib.lib = ours


def legs_of(parent_lib, window: int = 0):
    """The legs in the order window ``window`` runs them: rotated by one per window, so that no leg always follows the same one."""
    legs = ((LEG_PARENT,) if parent_lib else ()) + (LEG_BOXES, LEG_GRIDS)
    return legs[window % len(legs):] + legs[:window % len(legs)]


def trace_child(windows: int, parent_lib) -> None:
    """Per camera count: `windows` windows; in each, per leg in the window's order (`legs_of`), TRACE_WARMUP + TRACE_LAUNCHES
    launches.  The legs' frames are compared once, before the windows: the same bits."""
    import torch

    parent = ParentEntry(parent_lib) if parent_lib else None
    for n in CAMERAS:
        rooms, legs = scenes(n)
        out = torch.empty((n, H, W), dtype=torch.float32, device="cuda:0")
        frames = [tuple(t.clone() for t in cast(rooms, legs[leg], out, parent if leg == LEG_PARENT else None)) for leg in legs_of(parent_lib)]
        for other in frames[1:]:
            assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(frames[0], other)), "legs disagree"
        for w in range(windows):
            for leg in legs_of(parent_lib, w):
                for _ in range(TRACE_WARMUP + TRACE_LAUNCHES):
                    cast(rooms, legs[leg], out, parent if leg == LEG_PARENT else None)
                torch.cuda.synchronize()


def probe_trace(lines, workdir: str, windows: int, parent_lib) -> None:
    import numpy as np

    if shutil.which("rocprofv3") is None:
        raise RuntimeError("rocprofv3 not found: the kernel-time leg needs it (--skip-trace leaves the leg out)")
    shutil.rmtree(workdir, ignore_errors=True)
    os.makedirs(workdir)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", workdir, "-o", "grid_worlds", "--", sys.executable,
           os.path.abspath(__file__), "--trace-child", "--windows", str(windows)] + (["--parent-lib", parent_lib] if parent_lib else [])
    with open(os.path.join(workdir, "child.log"), "w") as log:
        subprocess.run(cmd, check=True, stdout=log, stderr=subprocess.STDOUT, timeout=500)
    dbs = glob.glob(os.path.join(workdir, "**", "*_results.db"), recursive=True)
    if not dbs:
        raise RuntimeError(f"no rocprofv3 database under {workdir}")
    rows = sqlite3.connect(dbs[0]).execute("select name, start, end from kernels order by start").fetchall()
    per = TRACE_WARMUP + TRACE_LAUNCHES
    legs = legs_of(parent_lib)
    ours = [(e - s) * 1e-3 for (name, s, e) in rows if "rooms_raycast_objects_kernel" in name]
    want = (per * windows + 1) * len(legs) * len(CAMERAS)
    if len(ours) != want:
        raise RuntimeError(f"expected {want} dispatches of rooms_raycast_objects_kernel, found {len(ours)}")
    medians = {}
    for g, n in enumerate(CAMERAS):
        base = g * (per * windows + 1) * len(legs) + len(legs)          # past the one comparison launch per leg
        for leg in legs:
            us = np.array([ours[base + (w * len(legs) + legs_of(parent_lib, w).index(leg)) * per:][TRACE_WARMUP:per]
                           for w in range(windows)])
            med = np.median(us, axis=1)
            medians[(n, leg)] = (float(np.median(us)), float(med.min()), float(med.max()))
            lines.append("kernel cameras=%3d  %-27s rooms_raycast_objects_kernel %9.1f us (%.1f-%.1f over %d launches; per-window medians "
                         "%.1f-%.1f, %d windows)" % (n, leg, *stats(us.reshape(-1)), us.size, med.min(), med.max(), windows))
            print(lines[-1], flush=True)
    if parent_lib:
        for n in CAMERAS:
            m, (_, lo, hi) = medians[(n, LEG_BOXES)][0], medians[(n, LEG_PARENT)]
            lines.append("pass mark cameras=%3d  box worlds on this change, median %.1f us: %s the parent's spread of window medians %.1f-%.1f us"
                         % (n, m, "INSIDE" if lo <= m <= hi else ("BELOW (faster than)" if m < lo else "ABOVE (slower than)"), lo, hi))
            print(lines[-1], flush=True)


def mid_episode(E: int, worlds):
    import torch

    from vlfm_amd.harness import BatchedEpisodes, WorldObjects

    sim = BatchedEpisodes(E, device=torch.device("cuda:0"), use_blip2=False, select_frontiers=True, episode_len=500,
                          closed_loop=True, object_maps=True, world_objects=WorldObjects(), worlds=worlds)
    for _ in range(45):
        sim.step()
    return sim


def probe_steps(steps: int, lines) -> None:
    import time

    import numpy as np
    import torch

    from vlfm_amd.synthetic import ProceduralWorlds

    E = 256
    sims = {"procedural box worlds": mid_episode(E, ProceduralWorlds(0)), "their rasterised twins": mid_episode(E, RasterisedWorlds(0))}
    a, b = sims.values()
    same = np.array_equal(a.live.xy, b.live.xy) and np.array_equal(a.live.k, b.live.k)
    rate = {k: [] for k in sims}
    for _ in range(3):                 # alternating windows
        for key, s in sims.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                s.step()
            torch.cuda.synchronize()
            rate[key].append(E * steps / (time.perf_counter() - t0))
    for name, s in sims.items():
        s.check()
        st = s.live.stats
        lines.append("steps  E=%3d  ObjectNav  %-23s %8.1f env-steps/s (%.1f-%.1f over 3 windows of %d steps)   per environment: "
                     "%.2f refused moves, %.1f forward steps, path %.2f m; episodes per environment up to %d"
                     % (E, name, *stats(rate[name]), steps, float(st["collisions"].mean()), float(st["forward_steps"].mean()),
                        float(st["path_length"].mean()), int(s.live.world_episode.max()) + 1))
        print(lines[-1], flush=True)
    lines.append("steps  the two harnesses stood at the same poses after 45 steps: %s; after the windows: %s"
                 % (same, np.array_equal(a.live.xy, b.live.xy) and np.array_equal(a.live.k, b.live.k)))
    print(lines[-1], flush=True)


# ------------------------------------------------------------------------------------------------ (c) the lattice geodesic
LATTICE_FIELDS = (8, 256)
LATTICE_KINDS = ("rooms world", "400x400 plan")
LATTICE_LAUNCHES, LATTICE_WARMUP = 6, 2
LATTICE_KERNELS = ("lattice_free_kernel", "lattice_fields_kernel", "lattice_query_kernel")


def lattice_scene(n: int, kind: str):
    """(renderer, table, world_of [n], objects [n,8,8], target boxes [n,4], query points [n,2]) of ``n`` fields."""
    import numpy as np
    import torch

    from vlfm_amd import synthetic as S
    from vlfm_amd.harness import RoomsRenderer, WorldTable

    dev = torch.device("cuda:0")
    rooms = RoomsRenderer(list(range(n)), 500, 48, 64, dev)
    obj = np.zeros((n, S.WORLD_MAX_OBJECTS, 8))
    if kind == LATTICE_KINDS[0]:
        table, world_of, xy = rooms.table, np.zeros(n, np.int32), rooms.pose_table[0][:, :2].copy()
        lays = [S.object_layout(e, 0, xy[e]) for e in range(n)]
    else:
        worlds = RasterisedWorlds(0)
        made = [worlds.world(e, 0) for e in range(n)]
        table = WorldTable(n, dev, max_grid=worlds.max_grid)
        table.assign(np.arange(n), [w.boxes for w in made], [w.grid for w in made])
        world_of, xy = np.arange(n, dtype=np.int32), np.stack([w.start_xy for w in made])
        lays = [worlds.layout(e, 0, xy[e]) for e in range(n)]
    for e, lay in enumerate(lays):
        for k, (_, box) in enumerate(lay):
            obj[e, k, :6], obj[e, k, 6] = box, 1.0
    targets = np.array([obj[e, 0, :4] if len(lays[e]) else [np.nan] * 4 for e in range(n)])
    return rooms, table, world_of, obj, targets, xy


def lattice_child() -> None:
    """Per field count and kind of world: LATTICE_WARMUP + LATTICE_LAUNCHES times the two field launches, then as many queries."""
    import numpy as np
    import torch

    for n in LATTICE_FIELDS:
        for kind in LATTICE_KINDS:
            rooms, table, world_of, obj, targets, xy = lattice_scene(n, kind)
            for _ in range(LATTICE_WARMUP + LATTICE_LAUNCHES):
                h = rooms.lattice_fields_worlds(table, world_of, obj, targets, 1.0)
                torch.cuda.synchronize()
            for _ in range(LATTICE_WARMUP + LATTICE_LAUNCHES):
                rooms.lattice_distances(h, np.arange(n), xy)
            torch.cuda.synchronize()


def probe_lattice_trace(lines, workdir: str) -> None:
    import time

    import numpy as np

    from vlfm_amd import synthetic as S

    if shutil.which("rocprofv3") is None:
        raise RuntimeError("rocprofv3 not found: the kernel-time leg needs it (--skip-trace leaves the leg out)")
    shutil.rmtree(workdir, ignore_errors=True)
    os.makedirs(workdir)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", workdir, "-o", "lattice", "--", sys.executable, os.path.abspath(__file__),
           "--lattice-child"]
    with open(os.path.join(workdir, "child.log"), "w") as log:
        subprocess.run(cmd, check=True, stdout=log, stderr=subprocess.STDOUT, timeout=500)
    dbs = glob.glob(os.path.join(workdir, "**", "*_results.db"), recursive=True)
    if not dbs:
        raise RuntimeError(f"no rocprofv3 database under {workdir}")
    rows = sqlite3.connect(dbs[0]).execute("select name, start, end from kernels order by start").fetchall()
    per = LATTICE_WARMUP + LATTICE_LAUNCHES
    groups = [(n, kind) for n in LATTICE_FIELDS for kind in LATTICE_KINDS]
    for kernel in LATTICE_KERNELS:
        us = [(e - s) * 1e-3 for (name, s, e) in rows if kernel in name]
        if len(us) != per * len(groups):
            raise RuntimeError(f"expected {per * len(groups)} dispatches of {kernel}, found {len(us)}")
        for g, (n, kind) in enumerate(groups):
            lines.append("kernel fields=%3d  %-13s %-22s %10.1f us (%.1f-%.1f over %d launches after %d)"
                         % (n, kind, kernel, *stats(us[g * per + LATTICE_WARMUP:(g + 1) * per]), LATTICE_LAUNCHES, LATTICE_WARMUP))
            print(lines[-1], flush=True)
    for kind in LATTICE_KINDS:          # the host statement, one field
        if kind == LATTICE_KINDS[0]:
            boxes, grid, lay = None, None, S.object_layout(0, 0, np.zeros(2))
        else:
            w = RasterisedWorlds(0).world(0, 0)
            boxes, grid, lay = w.boxes, w.grid, RasterisedWorlds(0).layout(0, 0, w.start_xy)
        obj = np.zeros((S.WORLD_MAX_OBJECTS, 8))
        for k, (_, box) in enumerate(lay):
            obj[k, :6], obj[k, 6] = box, 1.0
        t0 = time.perf_counter()
        ext = S.lattice_extent(boxes, grid, obj)
        free = S.lattice_free_numpy(ext, boxes, grid, obj)
        t1 = time.perf_counter()
        pts = S.goal_viewpoints(obj[0, :4], S.inflated_rects(obj, S.STEP_MARGIN, boxes), 1.0, grid=grid)
        t2 = time.perf_counter()
        field = S.lattice_field_numpy(free, S.lattice_sources(pts), ext[:2])
        t3 = time.perf_counter()
        lines.append("host   one field     %-13s %d x %d nodes: free mask %.1f ms, view points %.1f ms, field %.1f ms (largest cost %d)"
                     % (kind, ext[2], ext[3], 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), int(field[field != S.LATTICE_NONE].max())))
        print(lines[-1], flush=True)


def probe_lattice_steps(steps: int, lines) -> None:
    import time

    import numpy as np
    import torch

    from vlfm_amd.harness import BatchedEpisodes, WorldObjects

    E = 256
    legs = {"metrics off": {}, 'geodesic="graph"': dict(objectnav_metrics=True, geodesic="graph"),
            'geodesic="lattice"': dict(objectnav_metrics=True, geodesic="lattice")}
    sims = {}
    for name, kw in legs.items():
        sims[name] = BatchedEpisodes(E, device=torch.device("cuda:0"), use_blip2=False, select_frontiers=True, episode_len=500,
                                     closed_loop=True, object_maps=True, world_objects=WorldObjects(), **kw)
        for _ in range(45):
            sims[name].step()
    names = list(sims)
    rate = {k: [] for k in sims}
    for w in range(3):                  # alternating windows, the order rotated by one per window
        for name in names[w % 3:] + names[:w % 3]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                sims[name].step()
            torch.cuda.synchronize()
            rate[name].append(E * steps / (time.perf_counter() - t0))
    ref = sims[names[0]]
    for name, s in sims.items():
        s.check()
        same = np.array_equal(s.live.xy, ref.live.xy) and np.array_equal(s.live.k, ref.live.k)
        lines.append("steps  E=%3d  ObjectNav, rooms world  %-19s %8.1f env-steps/s (%.1f-%.1f over 3 windows of %d steps); episodes "
                     "scored %d; poses equal to the first leg's: %s" % (E, name, *stats(rate[name]), steps,
                                                                       len(s.live.objectnav_stats["episode_outcome"]), same))
        print(lines[-1], flush=True)
    for name in names[1:]:
        lines.append("steps  summary %-19s %s" % (name, sims[name].live.objectnav_summary()))
        print(lines[-1], flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="a libvlfm_amd.so built from the parent commit: the third leg of (a)")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--workdir", default=os.path.join(ROOT, "scratch", "grid_worlds_trace"),
                    help="where the kernel trace of leg (a) is written (removed and rewritten by every run)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--geodesic", choices=("none", "lattice"), default="none", help="lattice: leg (c), the lattice geodesic")
    ap.add_argument("--lattice-child", action="store_true")
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "grid_worlds_probe measures on the GPU; there is no CPU path"
    if a.trace_child:
        return trace_child(a.windows, a.parent_lib)
    if a.lattice_child:
        return lattice_child()
    if a.geodesic == "lattice":
        lines = ["grid_worlds_probe --geodesic lattice: device %s; rocprofv3 kernel trace of lattice_fields_worlds / lattice_distances "
                 "at 20 nodes per metre, pad 1 m; closed loop without a model, stub cosines, object maps on"
                 % torch.cuda.get_device_name(0)]
        if not a.skip_trace:
            probe_lattice_trace(lines, a.workdir + "_lattice")
        if not a.skip_steps:
            probe_lattice_steps(a.steps, lines)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    lines = ["grid_worlds_probe: device %s; (a) rocprofv3 kernel trace of %dx%d frames with objects, legs alternating over windows of %d "
             "launches after %d warm-up launches each; worlds: ProceduralWorlds(0).world(e, 0) as boxes and rasterised at %d cells per "
             "metre; (b) no model, stub cosines, object maps on" % (torch.cuda.get_device_name(0), W, H, TRACE_LAUNCHES, TRACE_WARMUP,
                                                                   CELLS_PER_METRE)]
    if not a.skip_trace:
        probe_trace(lines, a.workdir, a.windows, a.parent_lib)      # first, while this process has nothing queued on the device
        for n in CAMERAS:
            lines.append("walk   cameras=%3d  cells entered per column (host statement): mean %.1f, at most %d" % (n, *walk_steps(n)))
            print(lines[-1], flush=True)
    if not a.skip_steps:
        probe_steps(a.steps, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
