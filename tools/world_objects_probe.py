"""What objects in the rooms world cost (csrc/world_render.hip: vlfm_rooms_raycast_objects), measured in one place.

  (a) kernel time of rooms_raycast_objects_kernel from `rocprofv3 --kernel-trace --stats`, in a run of its own (a fresh child
      process, started before this process touches the device): 256 and 8 frames of 640x480, each environment with the two
      objects of synthetic.object_layout and with a full set of 8 (the 8 spots nearest to the robot), and
      rooms_raycast_kernel (walls only) on the same cameras in the same session.
  (b) env-steps/s of a closed-loop harness with and without world_objects at 8 and 256 environments: stub cosines, no
      detector, object_maps=True, alternating windows.

    python tools/world_objects_probe.py [--steps 20] [--skip-steps] [--skip-trace] [--out profiles/world_objects_probe.txt]
    python tools/world_objects_probe.py --trace-child        # the process (a) points rocprofv3 at"""
import argparse
import glob
import os
import shutil
import sqlite3
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

CASES = [(256, 2), (256, 8), (8, 2), (8, 8)]                  # (frames, objects per environment), 640x480
H, W = 480, 640
TRACE_LAUNCHES, TRACE_WARMUP = 50, 5


def scene(n: int, k: int, dev):
    """(renderer, transforms [n,4,4], objects [n,8,8]): environment e on its mid-episode pose of the tour with k objects."""
    import numpy as np

    from vlfm_amd import synthetic as S
    from vlfm_amd.harness import RoomsRenderer

    rr = RoomsRenderer(list(range(n)), 500, H, W, dev)
    tf, xy = rr.tf_table[150], rr.pose_table[150][:, :2]
    objects = np.zeros((n, S.WORLD_MAX_OBJECTS, 8))
    classes = list(S.OBJECT_SIZES)
    for e in range(n):
        if k == 2:
            boxes = [b for _, b in S.object_layout(e, 0, xy[e])]
        else:
            near = sorted(S.OBJECT_SPOTS, key=lambda p: float(np.hypot(p[0] - xy[e, 0], p[1] - xy[e, 1])))[:k]
            boxes = [S.object_box(classes[(e + i) % len(classes)], *p) for i, p in enumerate(near)]
        for i, b in enumerate(boxes):
            objects[e, i, :6], objects[e, i, 6] = b, 1.0
    return rr, tf, objects


def stats(xs):
    import numpy as np

    return float(np.median(xs)), float(np.min(xs)), float(np.max(xs))


def trace_child() -> None:
    """Per case, TRACE_WARMUP + TRACE_LAUNCHES launches of the objects kernel, then as many of the walls-only kernel on the same
    cameras, and nothing else on the device; the share of object pixels of each case goes to stdout."""
    import numpy as np
    import torch

    dev = torch.device("cuda:0")
    for n, k in CASES:
        rr, tf, objects = scene(n, k, dev)
        out = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        env = np.arange(n)
        for _ in range(TRACE_WARMUP + TRACE_LAUNCHES):
            _, ids, st = rr.cast_cameras_objects(tf, objects, env, out=out)
        torch.cuda.synchronize()
        for _ in range(TRACE_WARMUP + TRACE_LAUNCHES):
            rr.cast_cameras(tf, out=out)
        torch.cuda.synchronize()
        count = st[:, :, 0].cpu().numpy()
        print("share n=%d k=%d %.6f %d" % (n, k, float(count.sum()) / (n * H * W), int((count > 0).sum())), flush=True)


def probe_trace(lines, workdir: str) -> None:
    import numpy as np

    if shutil.which("rocprofv3") is None:
        raise RuntimeError("rocprofv3 not found: the kernel-time leg needs it (--skip-trace leaves the leg out)")
    shutil.rmtree(workdir, ignore_errors=True)
    os.makedirs(workdir)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", workdir, "-o", "world_objects", "--", sys.executable,
           os.path.abspath(__file__), "--trace-child"]
    with open(os.path.join(workdir, "child.log"), "w") as log:
        subprocess.run(cmd, check=True, stdout=log, stderr=subprocess.STDOUT, timeout=300)
    share = {}
    for line in open(os.path.join(workdir, "child.log")):
        if line.startswith("share "):
            _, a, b, frac, seen = line.split()
            share[(int(a[2:]), int(b[2:]))] = (float(frac), int(seen))
    dbs = glob.glob(os.path.join(workdir, "**", "*_results.db"), recursive=True)
    if not dbs:
        raise RuntimeError(f"no rocprofv3 database under {workdir}")
    rows = sqlite3.connect(dbs[0]).execute("select name, start, end from kernels order by start").fetchall()
    per = TRACE_WARMUP + TRACE_LAUNCHES
    new = [(e - s) * 1e-3 for (name, s, e) in rows if "rooms_raycast_objects_kernel" in name]
    old = [(e - s) * 1e-3 for (name, s, e) in rows if "rooms_raycast_kernel" in name]
    fill = [(e - s) * 1e-3 for (name, s, e) in rows if "rooms_stats_init_kernel" in name]
    if len(new) != per * len(CASES) or len(old) != per * len(CASES):
        raise RuntimeError(f"expected {per * len(CASES)} dispatches of each kernel in the trace, found {len(new)} and {len(old)}")
    for i, (n, k) in enumerate(CASES):
        a, b = np.array(new[i * per + TRACE_WARMUP:(i + 1) * per]), np.array(old[i * per + TRACE_WARMUP:(i + 1) * per])
        frac, seen = share.get((n, k), (float("nan"), -1))
        lines.append("kernel n=%3d %dx%d  %d objects/env  rooms_raycast_objects_kernel %7.1f us (%.1f-%.1f)   rooms_raycast_kernel "
                     "%7.1f us (%.1f-%.1f)   ratio %4.2f   %d launches each; %.2f %% of the pixels are objects, %d (camera, object) "
                     "pairs in view; %.1f MB written against %.1f MB"
                     % (n, W, H, k, *stats(a), *stats(b), stats(a)[0] / stats(b)[0], len(a), 100 * frac, seen,
                        n * H * W * 5 / 1e6, n * H * W * 4 / 1e6))
        print(lines[-1], flush=True)
    lines.append("kernel rooms_stats_init_kernel (the fill of d_stats in front of every launch) %.1f us (%.1f-%.1f)" % stats(fill))
    print(lines[-1], flush=True)


def probe_steps(steps: int, lines) -> None:
    import time

    import torch

    from vlfm_amd.harness import BatchedEpisodes, WorldObjects

    dev = torch.device("cuda:0")
    for E in (8, 256):
        kw = dict(device=dev, use_blip2=False, select_frontiers=True, episode_len=500, closed_loop=True, object_maps=True)
        sims = {"with world_objects": BatchedEpisodes(E, world_objects=WorldObjects(), **kw), "without": BatchedEpisodes(E, **kw)}
        rate = {k: [] for k in sims}
        for s in sims.values():
            for _ in range(15):            # the initialisation turns and the first decisions
                s.step()
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
            extra = ""
            if s.world_objects is not None:
                st = s.objectnav_stats
                extra = "   %d detections, %d cloud updates; episodes ended: %d (%d successes, %d wrong stops, %d no frontier)" % (
                    s.object_stats["detections"], s.object_stats["cloud_updates"], int(st["episodes"].sum()),
                    int(st["successes"].sum()), int(st["wrong_stops"].sum()), int(st["no_frontier_stops"].sum()))
            lines.append("steps  E=%3d  %-19s %8.1f env-steps/s (%.1f-%.1f over 3 windows of %d steps)%s"
                         % (E, name, *stats(rate[name]), steps, extra))
            print(lines[-1], flush=True)
        del sims
        torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--workdir", default=os.path.join(ROOT, "scratch", "world_objects_trace"),
                    help="where the kernel trace of leg (a) is written (removed and rewritten by every run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace_child:
        return trace_child()
    lines = []
    if not a.skip_trace:
        probe_trace(lines, a.workdir)      # first: this process has not touched the device yet
    import torch

    assert torch.cuda.is_available(), "world_objects_probe measures on the GPU; there is no CPU path"
    lines.insert(0, "world_objects_probe: device %s; (a) rocprofv3 kernel trace, median (min-max); (b) stub cosines, no detector, "
                    "object_maps=True" % torch.cuda.get_device_name(0))
    if not a.skip_steps:
        probe_steps(a.steps, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
