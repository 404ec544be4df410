"""What objects in the rooms world cost (csrc/world_render.hip: vlfm_worlds_raycast with objects), measured in one place.

  (a) kernel time of rooms_raycast_objects_kernel from `rocprofv3 --kernel-trace --stats`, in a run of its own (a fresh child
      process, started before this process touches the device): 256 and 8 frames of 640x480, each environment with the two
      objects of synthetic.object_layout and with a full set of 8 (the 8 spots nearest to the robot), and
      rooms_raycast_kernel (walls only) on the same cameras in the same session.
  (b) env-steps/s of a closed-loop harness with and without world_objects at 8 and 256 environments: stub cosines, no
      detector, object_maps=True, alternating windows; --batch-object-maps on | off | both runs the world_objects harness with
      all detections of a step in one object-map update, with one update_map per detection, or both side by side, and reports the object-cloud
      kernel launches and host read-backs per step of each; --device-object-clouds on | off | both does the same for the device
      mirrors of the clouds (update_explored_batch / get_best_objects_batch against one NumPy pass per environment) and adds the
      cloud-query launches, the bytes uploaded to the mirrors and the points re-evaluated on the host per step.
  (c) --batch-trace: kernel time of the object-map update for 1 / 16 / 64 detections in one call (objects in view of the tour poses)
      at 640x480, from one `rocprofv3 --kernel-trace --stats` run of its own.

  (d) --cloud-trace: kernel time of the two cloud queries (csrc/cloud_query.hip) over 256 mirrored clouds of 20 000 and of
      100 000 points, from one `rocprofv3 --kernel-trace --stats` run of its own, against the bytes of the mirrors.

  (e) --objectnav-metrics: the geodesic kernels behind SPL / SoftSPL / distance_to_goal (csrc/geodesic.hip) at 256 environments
      of the rooms world with the two objects of synthetic.object_layout -- kernel time from the library's own dispatch events
      (vlfm_profile_enable), the host call around it, and the host statement (NumPy) for the same work; leg (b) then also runs a
      world_objects harness with objectnav_metrics=True beside the others and prints its objectnav_summary().

    python tools/world_objects_probe.py [--steps 20] [--skip-steps] [--skip-trace] [--out profiles/world_objects_probe.txt]
    python tools/world_objects_probe.py --skip-trace --batch-object-maps both --batch-trace --out profiles/object_maps_batch_probe.txt
    python tools/world_objects_probe.py --skip-trace --device-object-clouds both --out profiles/object_clouds_device_probe.txt
    python tools/world_objects_probe.py --skip-trace --objectnav-metrics --out profiles/objectnav_metrics_probe.txt
    python tools/world_objects_probe.py --trace-child        # the process (a) points rocprofv3 at
    python tools/world_objects_probe.py --batch-trace-child  # the process (c) points rocprofv3 at
    python tools/world_objects_probe.py --cloud-trace-child  # the process (d) points rocprofv3 at"""
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


BATCH_TRACE_JOBS, BATCH_TRACE_REPS, BATCH_TRACE_WARMUP = (1, 16, 64), 10, 2
BATCH_KERNELS = ("mask_pack_batch_kernel", "mask_erode_batch_kernel", "mask_stats_batch_kernel", "cloud_expand_batch_kernel",
                 "dbscan_adjacency_batch_kernel", "dbscan_cluster_batch_kernel")


def batch_trace_child() -> None:
    """64 objects as the cameras of `scene` see them; per D in BATCH_TRACE_JOBS: warm-up + BATCH_TRACE_REPS
    updates of the first D detections in one call."""
    import numpy as np
    import torch

    from vlfm_amd.mapping import object_point_cloud_map as opm
    from vlfm_amd.synthetic import MAX_DEPTH, MIN_DEPTH, camera_intrinsics

    dev = torch.device("cuda:0")
    # at the tour poses of `scene` the two objects of the default layout are in view of 16 cameras out of 256: the detections
    # come from the full set of 8 objects per environment instead -- (camera, object) pairs with at least 600 visible pixels that keep 100 points after the erosion, repeated if there are fewer than 64
    rr, tf, objects = scene(256, 8, dev)
    depth = torch.empty((256, H, W), dtype=torch.float32, device=dev)
    _, ids, seen = rr.cast_cameras_objects(tf, objects, np.arange(256), out=depth)
    visible = seen[:, :, 0].cpu().numpy()
    pairs = [(e, k) for e in range(256) for k in range(visible.shape[1]) if visible[e, k] >= 600][:4 * max(BATCH_TRACE_JOBS)]
    masks_all = torch.stack([ids[e] == k + 1 for e, k in pairs])
    _, st = opm.mask_stats_batch(masks_all.contiguous().view(torch.uint8), [5] * len(pairs), dev)
    good = [i for i in range(len(pairs)) if st[i, 0] >= 100]
    assert good, "no object in view"
    good = (good * max(BATCH_TRACE_JOBS))[:max(BATCH_TRACE_JOBS)]
    frames = [pairs[i][0] for i in good]
    masks_all = masks_all[torch.tensor(good, device=dev)]
    print("points " + " ".join(str(int(st[i, 0])) for i in good), flush=True)
    fx, fy, _ = camera_intrinsics(W)
    for D in BATCH_TRACE_JOBS:
        maps = [opm.ObjectPointCloudMap(5, device=dev, rng=np.random.RandomState(j)) for j in range(D)]
        masks = masks_all[:D]
        for _ in range(BATCH_TRACE_WARMUP + BATCH_TRACE_REPS):
            list(opm.extract_object_clouds_batch(maps, depth, frames[:D], masks, MIN_DEPTH, MAX_DEPTH, fx, fy))
        torch.cuda.synchronize()


def probe_batch_trace(lines, workdir: str) -> None:
    import numpy as np

    if shutil.which("rocprofv3") is None:
        raise RuntimeError("rocprofv3 not found: the kernel-time leg needs it")
    shutil.rmtree(workdir, ignore_errors=True)
    os.makedirs(workdir)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", workdir, "-o", "object_maps_batch", "--", sys.executable,
           os.path.abspath(__file__), "--batch-trace-child"]
    with open(os.path.join(workdir, "child.log"), "w") as log:
        subprocess.run(cmd, check=True, stdout=log, stderr=subprocess.STDOUT, timeout=420)
    dbs = glob.glob(os.path.join(workdir, "**", "*_results.db"), recursive=True)
    if not dbs:
        raise RuntimeError(f"no rocprofv3 database under {workdir}")
    rows = sqlite3.connect(dbs[0]).execute("select name, start, end from kernels order by start").fetchall()

    def short(name):
        base = name.split("(")[0].split("::")[-1]
        return base[:-3] if base.endswith(".kd") else base

    rows = [(short(n), (e - s) * 1e-3) for n, s, e in rows]
    # calls end with their clustering kernel (every traced detection keeps >= 100 points, one wave, one chunk)
    calls, cur = [], {}
    for n, us in rows:
        if n not in BATCH_KERNELS:
            continue
        cur[n] = cur.get(n, 0.0) + us
        if n == "dbscan_cluster_batch_kernel":
            calls.append(cur)
            cur = {}
    per = BATCH_TRACE_WARMUP + BATCH_TRACE_REPS
    # (the first call in the trace is the child's own mask_stats_batch, which never reaches the clustering kernel: its stage-1
    # kernels are counted with the first warm-up call)
    if len(calls) != per * len(BATCH_TRACE_JOBS):
        raise RuntimeError(f"expected {per * len(BATCH_TRACE_JOBS)} calls in the trace, found {len(calls)}")
    for i, D in enumerate(BATCH_TRACE_JOBS):
        batch = calls[i * per + BATCH_TRACE_WARMUP:(i + 1) * per]
        stage = lambda c: (c.get("mask_pack_batch_kernel", 0) + c.get("mask_erode_batch_kernel", 0) + c["mask_stats_batch_kernel"],
                           c["cloud_expand_batch_kernel"], c["dbscan_adjacency_batch_kernel"], c["dbscan_cluster_batch_kernel"])
        med = [float(np.median([stage(c)[i] for c in batch])) for i in range(4)]
        tot = [sum(stage(c)) for c in batch]
        lines.append("batch-kernels D=%2d 640x480  stage 1 %8.1f us  expansion %7.1f us  adjacency %8.1f us  clusters %8.1f us  "
                     "sum %9.1f us (%.1f-%.1f)   %d rounds" % (D, *med, *stats(tot), len(batch)))
        print(lines[-1], flush=True)


CLOUD_TRACE_POINTS, CLOUD_TRACE_CLOUDS, CLOUD_TRACE_REPS, CLOUD_TRACE_WARMUP = (20000, 100000), 256, 10, 2
CLOUD_KERNELS = ("cloud_cone_kernel", "cloud_closest_partial_kernel", "cloud_closest_final_kernel")
HBM_PEAK = 8.0e12        # bytes/s, MI355X specification


def cloud_trace_child() -> None:
    """256 maps with one cloud each: points uniform in a 2 m box, half of them trusted, the others under 8 far tags.  The cone looks
    AWAY from the box from 1.5 m with every point in range: every far point goes through the whole test and none is dropped, so
    all rounds see the same clouds."""
    import numpy as np
    import torch

    from vlfm_amd.mapping import object_point_cloud_map as opm

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    tf = np.eye(4)
    tf[0, 3] = 1.5
    for n in CLOUD_TRACE_POINTS:
        maps = []
        for _ in range(CLOUD_TRACE_CLOUDS):
            m = opm.ObjectPointCloudMap(5, device=dev)
            tags = np.where(rng.random(n) < 0.5, 1.0, (1 + rng.integers(0, 8, n)) / 16.0)
            m.clouds = {"chair": np.concatenate([rng.uniform(-1.0, 1.0, (n, 3)), tags[:, None]], axis=1)}
            maps.append(m)
        for _ in range(CLOUD_TRACE_WARMUP + CLOUD_TRACE_REPS):
            assert not any(opm.update_explored_batch(maps, [tf] * len(maps), 8.0, 1.38))
            goals = opm.get_best_objects_batch(maps, ["chair"] * len(maps), [np.array([1.5, 0.0])] * len(maps))
            assert all(g is not None for g in goals)
        torch.cuda.synchronize()
        del maps
        torch.cuda.empty_cache()


def probe_cloud_trace(lines, workdir: str) -> None:
    import numpy as np

    if shutil.which("rocprofv3") is None:
        raise RuntimeError("rocprofv3 not found: the kernel-time leg needs it")
    shutil.rmtree(workdir, ignore_errors=True)
    os.makedirs(workdir)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", workdir, "-o", "cloud_queries", "--", sys.executable,
           os.path.abspath(__file__), "--cloud-trace-child"]
    with open(os.path.join(workdir, "child.log"), "w") as log:
        subprocess.run(cmd, check=True, stdout=log, stderr=subprocess.STDOUT, timeout=420)
    dbs = glob.glob(os.path.join(workdir, "**", "*_results.db"), recursive=True)
    if not dbs:
        raise RuntimeError(f"no rocprofv3 database under {workdir}")
    rows = sqlite3.connect(dbs[0]).execute("select name, start, end from kernels order by start").fetchall()
    per = CLOUD_TRACE_WARMUP + CLOUD_TRACE_REPS
    us = {k: [(e - s) * 1e-3 for n, s, e in rows if k in n] for k in CLOUD_KERNELS}
    if any(len(v) != per * len(CLOUD_TRACE_POINTS) for v in us.values()):
        raise RuntimeError(f"expected {per * len(CLOUD_TRACE_POINTS)} dispatches of each cloud-query kernel, found "
                           f"{[len(v) for v in us.values()]}")
    for i, n in enumerate(CLOUD_TRACE_POINTS):
        cone, part, fin = (np.array(us[k][i * per + CLOUD_TRACE_WARMUP:(i + 1) * per]) for k in CLOUD_KERNELS)
        closest = part + fin
        rows_b, slots_b = 32.0 * n * CLOUD_TRACE_CLOUDS, 4.0 * n * CLOUD_TRACE_CLOUDS
        lines.append("cloud-kernels %d clouds x %6d points (%.1f MB of rows, %.1f MB of slots)  cone %7.1f us (%.1f-%.1f) = %4.1f %% of "
                     "the HBM peak for rows + slots   closest: partials %7.1f us + final %5.1f us = %7.1f us (%.1f-%.1f) = %4.1f %% of "
                     "the HBM peak for the rows   %d rounds"
                     % (CLOUD_TRACE_CLOUDS, n, rows_b / 1e6, slots_b / 1e6, *stats(cone),
                        100 * (rows_b + slots_b) / (stats(cone)[0] * 1e-6) / HBM_PEAK, float(np.median(part)), float(np.median(fin)),
                        *stats(closest), 100 * rows_b / (stats(closest)[0] * 1e-6) / HBM_PEAK, len(cone)))
        print(lines[-1], flush=True)


GEODESIC_ENVS, GEODESIC_GROUPS, GEODESIC_LAUNCHES, GEODESIC_HOST_ENVS = 256, 5, 10, 8


def probe_geodesic(lines) -> None:
    """Leg (e): 256 fields and 256 queries, warm, GEODESIC_GROUPS groups of GEODESIC_LAUNCHES launches each; per group the mean
    kernel time of the dispatch events and the mean host time of the whole call (uploads, launch, synchronise)."""
    import time

    import numpy as np
    import torch

    from vlfm_amd import _lib
    from vlfm_amd import synthetic as S

    dev = torch.device("cuda:0")
    n = GEODESIC_ENVS
    rr, _, objects = scene(n, 2, dev)
    xy = rr.pose_table[150][:, :2]
    targets = objects[:, 0, :4]
    field_of = np.arange(n)
    L = _lib.lib()

    def timed(kernel, call):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        k_us, h_us = [], []
        for _ in range(GEODESIC_GROUPS):
            L.vlfm_profile_enable(1)
            t0 = time.perf_counter()
            for _ in range(GEODESIC_LAUNCHES):
                call()
                torch.cuda.synchronize()
            h_us.append((time.perf_counter() - t0) / GEODESIC_LAUNCHES * 1e6)
            ms, got = _lib.profile_read(kernel)
            assert got == GEODESIC_LAUNCHES, (kernel, got)
            k_us.append(ms * 1e3)
        L.vlfm_profile_enable(0)
        return stats(k_us), stats(h_us)

    handle = rr.geodesic_fields(objects, targets, 1.0)
    counts, n_src = handle.counts.cpu().numpy(), handle.source_counts.cpu().numpy()
    fk, fh = timed("geodesic_fields_kernel", lambda: rr.geodesic_fields(objects, targets, 1.0))
    qk, qh = timed("geodesic_query_kernel", lambda: rr.geodesic_distances(handle, field_of, xy))
    d = rr.geodesic_distances(handle, field_of, xy).cpu().numpy()
    # the host statement for the first environments (every environment is the same amount of work: same walls, two objects)
    t_field = t_query = 0.0
    for e in range(GEODESIC_HOST_ENVS):
        t0 = time.perf_counter()
        rects = S.inflated_rects(objects[e])
        src = S.goal_viewpoints(targets[e], rects, 1.0)
        nodes, dist = S.geodesic_field_numpy(rects, src)
        t1 = time.perf_counter()
        want = S.geodesic_query_numpy(rects, src, nodes, dist, xy[e:e + 1])
        t2 = time.perf_counter()
        t_field, t_query = t_field + (t1 - t0), t_query + (t2 - t1)
        assert want.view(np.int64)[0] == d[e:e + 1].view(np.int64)[0], (e, want, d[e])
    lines.append("geodesic n=%d fields  rooms world + 2 objects: %d-%d rectangles, %d-%d nodes, %d-%d view points   "
                 "geodesic_fields_kernel %8.1f us (%.1f-%.1f)   host call with uploads and synchronise %8.1f us (%.1f-%.1f)   "
                 "%d groups of %d launches   host statement (NumPy) %.1f ms per environment = %.2f s for %d"
                 % (n, counts[:, 0].min(), counts[:, 0].max(), counts[:, 1].min(), counts[:, 1].max(), n_src.min(), n_src.max(),
                    *fk, *fh, GEODESIC_GROUPS, GEODESIC_LAUNCHES, 1e3 * t_field / GEODESIC_HOST_ENVS,
                    t_field / GEODESIC_HOST_ENVS * n, n))
    print(lines[-1], flush=True)
    lines.append("geodesic m=%d queries (one per field)   geodesic_query_kernel %8.1f us (%.1f-%.1f)   host call with upload, "
                 "synchronise and read-back %8.1f us (%.1f-%.1f)   host statement (NumPy) %.2f ms per point = %.1f ms for %d; "
                 "%d of %d distances finite, mean %.2f m; the first %d bit-equal to the host statement"
                 % (n, *qk, *qh, 1e3 * t_query / GEODESIC_HOST_ENVS, 1e3 * t_query / GEODESIC_HOST_ENVS * n, n,
                    int(np.isfinite(d).sum()), n, float(d[np.isfinite(d)].mean()), GEODESIC_HOST_ENVS))
    print(lines[-1], flush=True)


def probe_steps(steps: int, lines, batch: str = "on", clouds: str = "on", metrics: bool = False) -> None:
    import time

    import torch

    from vlfm_amd import _lib
    from vlfm_amd.harness import BatchedEpisodes, WorldObjects
    from vlfm_amd.mapping import object_point_cloud_map as opm

    dev = torch.device("cuda:0")
    L = _lib.lib()
    for E in (8, 256):
        kw = dict(device=dev, use_blip2=False, select_frontiers=True, episode_len=500, closed_loop=True, object_maps=True)
        sims = {}
        for device_clouds in ([True] if clouds == "on" else [False] if clouds == "off" else [True, False]):
            where = "" if clouds != "both" else (", device clouds" if device_clouds else ", host clouds")
            if batch in ("on", "both"):
                sims[("with world_objects" if batch == "on" else "world_objects batched") + where] = BatchedEpisodes(
                    E, world_objects=WorldObjects(), batch_object_maps=True, device_object_clouds=device_clouds, **kw)
            if batch in ("off", "both"):
                sims[("with world_objects" if batch == "off" else "world_objects one by one") + where] = BatchedEpisodes(
                    E, world_objects=WorldObjects(), batch_object_maps=False, device_object_clouds=device_clouds, **kw)
        if metrics:
            sims["world_objects, objectnav_metrics"] = BatchedEpisodes(E, world_objects=WorldObjects(), objectnav_metrics=True, **kw)
        sims["without"] = BatchedEpisodes(E, **kw)
        rate = {k: [] for k in sims}
        # object-cloud kernel launches, host read-backs, cloud-query launches, uploaded bytes, band points inside the windows
        work = {k: [0, 0, 0, 0, 0] for k in sims}
        for s in sims.values():
            for _ in range(15):            # the initialisation turns and the first decisions
                s.step()
        for _ in range(3):                 # alternating windows
            for name, s in sims.items():
                torch.cuda.synchronize()
                before = (L.vlfm_object_cloud_launch_count(), opm.SYNCS[0], L.vlfm_cloud_query_launch_count(),
                          opm.UPLOADED_BYTES[0], opm.BAND_POINTS[0])
                t0 = time.perf_counter()
                for _ in range(steps):
                    s.step()
                torch.cuda.synchronize()
                rate[name].append(E * steps / (time.perf_counter() - t0))
                work[name][0] += L.vlfm_object_cloud_launch_count() - before[0]
                work[name][1] += opm.SYNCS[0] - before[1]
                work[name][2] += L.vlfm_cloud_query_launch_count() - before[2]
                work[name][3] += opm.UPLOADED_BYTES[0] - before[3]
                work[name][4] += opm.BAND_POINTS[0] - before[4]
        for name, s in sims.items():
            s.check()
            extra = ""
            if s.world_objects is not None:
                st = s.live.objectnav_stats
                extra = ("   %d detections, %d cloud updates; episodes ended: %d (%d successes, %d wrong stops, %d no frontier); "
                         "object-map stage per step: %.1f kernel launches, %.1f host read-backs; cloud queries per step: %.1f "
                         "launches, %.0f bytes uploaded, %.2f band points") % (
                    s.object_stats["detections"], s.object_stats["cloud_updates"], int(st["episodes"].sum()),
                    int(st["successes"].sum()), int(st["wrong_stops"].sum()), int(st["no_frontier_stops"].sum()),
                    work[name][0] / (3 * steps), work[name][1] / (3 * steps), work[name][2] / (3 * steps),
                    work[name][3] / (3 * steps), work[name][4] / (3 * steps))
            lines.append("steps  E=%3d  %-40s %8.1f env-steps/s (%.1f-%.1f over 3 windows of %d steps)%s"
                         % (E, name, *stats(rate[name]), steps, extra))
            print(lines[-1], flush=True)
            if getattr(s, "objectnav_metrics", False):
                lines.append("summary E=%3d  %s" % (E, "  ".join("%s %s" % (k, ("%.4f" % v) if isinstance(v, float) else v)
                                                                  for k, v in s.live.objectnav_summary().items())))
                print(lines[-1], flush=True)
        del sims
        torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--batch-object-maps", choices=("on", "off", "both"), default="on",
                    help="leg (b): the world_objects harness with the batched object-map update, without it, or both")
    ap.add_argument("--device-object-clouds", choices=("on", "off", "both"), default="on",
                    help="leg (b): update_explored and the object goals asked of device mirrors of the clouds, of NumPy, or both")
    ap.add_argument("--batch-trace", action="store_true", help="leg (c): kernel time of the batched update, a trace of its own")
    ap.add_argument("--batch-trace-child", action="store_true")
    ap.add_argument("--cloud-trace", action="store_true", help="leg (d): kernel time of the cloud queries, a trace of its own")
    ap.add_argument("--cloud-trace-child", action="store_true")
    ap.add_argument("--objectnav-metrics", action="store_true",
                    help="leg (e): the geodesic kernels; leg (b) also runs a harness with objectnav_metrics=True and prints its summary")
    ap.add_argument("--workdir", default=os.path.join(ROOT, "scratch", "world_objects_trace"),
                    help="where the kernel trace of leg (a) is written (removed and rewritten by every run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace_child:
        return trace_child()
    if a.batch_trace_child:
        return batch_trace_child()
    if a.cloud_trace_child:
        return cloud_trace_child()
    lines = []
    if not a.skip_trace:
        probe_trace(lines, a.workdir)      # first: this process has not touched the device yet
    if a.batch_trace:
        probe_batch_trace(lines, a.workdir + "_batch")
    if a.cloud_trace:
        probe_cloud_trace(lines, a.workdir + "_clouds")
    import torch

    assert torch.cuda.is_available(), "world_objects_probe measures on the GPU; there is no CPU path"
    lines.insert(0, "world_objects_probe: device %s; (a) rocprofv3 kernel trace, median (min-max); (b) stub cosines, no detector, "
                    "object_maps=True" % torch.cuda.get_device_name(0))
    if a.objectnav_metrics:
        probe_geodesic(lines)
    if not a.skip_steps:
        probe_steps(a.steps, lines, a.batch_object_maps, a.device_object_clouds, a.objectnav_metrics)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
