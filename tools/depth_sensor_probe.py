"""What the depth sensor costs (csrc/depth_sensor.hip: vlfm_depth_sensor), measured in one place, with HIP events, in one session,
on the same buffers.

  (a) per launch at 256 frames of 640x480 (256 generated worlds with their objects, ray-cast once): the sensor with all stages
      on, with only dropout, with the edge stage alone and with every stage off, next to two yardsticks on the same buffers -- a
      plain device-to-device copy of the frames (the 8 bytes per pixel the kernel must move) and the ray caster's own launch for
      those frames.  Two clocks: the events the library attaches to the dispatch itself (vlfm_profile_enable: the kernel alone)
      and a pair of events around a window of calls (with the small host-to-device copy and, for the sensor, the memset of the
      counts).  The legs alternate over --windows windows of LAUNCHES launches after WARMUP warm-up launches each.
  (b) the step of a 256-environment closed-loop harness in procedural worlds with objects, no model (stub cosines), with and
      without the sensor, the two harnesses alternating over 3 windows of --steps steps after 15 steps in; then, in windows of
      their own with the library's per-dispatch events on, the depth pass and the obstacle map's hole path of both harnesses
      (depth_ingest_scatter_kernel, fill_small_holes_kernel, hole_scatter_kernel: mean per launch, one launch per step).

    python tools/depth_sensor_probe.py [--windows 5] [--steps 20] [--out profiles/depth_sensor_probe.txt]"""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N, H, W = 256, 480, 640
LAUNCHES, WARMUP = 20, 3
HOLE_KERNELS = ("depth_ingest_scatter_kernel", "fill_small_holes_kernel", "hole_scatter_kernel")


def stats(xs):
    import numpy as np

    return float(np.median(xs)), float(np.min(xs)), float(np.max(xs))


def harness_sensor():
    from vlfm_amd.synthetic import DepthSensor

    return DepthSensor(seed=1, sigma0_m=0.002, sigma2_per_m=0.002, dropout=0.01, edge_m=0.3)


def probe_launch(windows: int, lines) -> None:
    import numpy as np
    import torch

    from vlfm_amd import _lib
    from vlfm_amd import synthetic as S
    from vlfm_amd.harness import RoomsRenderer, WorldTable

    dev = torch.device("cuda:0")
    rooms = RoomsRenderer([0], 500, H, W, dev)
    worlds = S.ProceduralWorlds(0)
    made = [worlds.world(e, 0) for e in range(N)]
    table = WorldTable(N, dev)
    table.assign(np.arange(N), [w.boxes for w in made])
    tf = np.stack([S.tf_of(w.start_xy[0], w.start_xy[1], w.start_k) for w in made])
    objects = np.zeros((N, S.WORLD_MAX_OBJECTS, 8))
    for e in range(N):
        for k, (_, box) in enumerate(worlds.layout(e, 0, made[e].start_xy)):
            objects[e, k, :6], objects[e, k, 6] = box, 1.0
    idx = np.arange(N)
    clean = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    out = torch.empty_like(clean)
    invalid = torch.empty((N,), dtype=torch.int32, device=dev)
    sensors = {"all stages": S.DepthSensor(seed=1, sigma0_m=0.002, sigma2_per_m=0.002, disparity_k=35.0, dropout=0.01, patch_dropout=0.002,
                                           edge_m=0.3, min_range_m=0.55, max_range_m=4.9),
               "dropout only": S.DepthSensor(seed=1, dropout=0.01), "edge only": S.DepthSensor(seed=1, edge_m=0.3),
               "every stage off": S.DepthSensor(seed=1)}
    clocks = np.arange(N) % 7
    calls = {"sensor, " + k: (lambda s=s: rooms.sense_depth(clean, s, idx, clocks, out=out, invalid_out=invalid), "depth_sensor_kernel")
             for k, s in sensors.items()}
    calls["device-to-device copy"] = (lambda: out.copy_(clean), None)
    calls["vlfm_worlds_raycast"] = (lambda: rooms.cast_worlds(tf, table, idx, objects, idx, out=clean), "worlds_raycast_objects_kernel")
    calls["vlfm_worlds_raycast"][0]()
    holes = {}
    for name, (fn, _) in calls.items():
        fn()
        torch.cuda.synchronize()
        if name.startswith("sensor"):
            holes[name] = int(invalid.sum())
    # the launch is the statement's frames (three of the 256, all stages on)
    rooms.sense_depth(clean, sensors["all stages"], idx, clocks, out=out, invalid_out=invalid)
    torch.cuda.synchronize()
    for e in (0, 100, 255):
        want, count = S.depth_sensor_numpy(clean[e].cpu().numpy(), S.MIN_DEPTH, S.MAX_DEPTH, sensors["all stages"], e, int(clocks[e]))
        assert want.tobytes() == out[e].cpu().numpy().tobytes() and count == int(invalid[e]), e
    kernel = {k: [] for k in calls}
    call = {k: [] for k in calls}
    for _ in range(windows):
        for name, (fn, label) in calls.items():
            for _ in range(WARMUP):
                fn()
            torch.cuda.synchronize()
            if label:
                _lib.lib().vlfm_profile_enable(1)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(LAUNCHES):
                fn()
            stop.record()
            torch.cuda.synchronize()
            if label:
                ms, n = _lib.profile_read(label)
                _lib.lib().vlfm_profile_enable(0)
                assert n == LAUNCHES, (name, n)
                kernel[name].append(ms * 1e3)
            call[name].append(start.elapsed_time(stop) * 1e3 / LAUNCHES)
    moved = 8 * N * H * W
    for name in calls:
        c = stats(call[name])
        if kernel[name]:
            k = stats(kernel[name])
            text = "kernel %7.1f us (%.1f-%.1f)   whole call %7.1f us (%.1f-%.1f)" % (*k, *c)
            if name.startswith("sensor"):
                text += "   8 B/pixel: %.0f MB, %.2f TB/s over the kernel; %.2f %% of the pixels invalid" % (
                    moved / 1e6, moved / (k[0] * 1e-6) / 1e12, 100.0 * holes[name] / (N * H * W))
        else:
            text = "                                 whole call %7.1f us (%.1f-%.1f)   8 B/pixel: %.0f MB, %.2f TB/s" % (
                *c, moved / 1e6, moved / (c[0] * 1e-6) / 1e12)
        lines.append("launch n=%d %dx%d  %-26s %s   [medians of %d window means of %d launches]" % (N, W, H, name, text, windows, LAUNCHES))
        print(lines[-1], flush=True)
    copy_us, cast_us = stats(call["device-to-device copy"])[0], stats(kernel["vlfm_worlds_raycast"])[0]
    for name in calls:
        if name.startswith("sensor"):
            k = stats(kernel[name])[0]
            lines.append("ratio  %-26s kernel / copy %.2fx, kernel / ray caster's kernel %.2fx" % (name, k / copy_us, k / cast_us))
            print(lines[-1], flush=True)


def probe_steps(steps: int, lines) -> None:
    import time

    import torch

    from vlfm_amd import _lib
    from vlfm_amd.harness import BatchedEpisodes, WorldObjects
    from vlfm_amd.synthetic import ProceduralWorlds

    sims = {flag: BatchedEpisodes(N, device=torch.device("cuda:0"), use_blip2=False, select_frontiers=True, episode_len=500,
                                  closed_loop=True, world_objects=WorldObjects(), worlds=ProceduralWorlds(0),
                                  depth_sensor=harness_sensor() if flag else None)
            for flag in (False, True)}
    for s in sims.values():
        for _ in range(15):
            s.step()
    ms = {k: [] for k in sims}
    for _ in range(3):
        for flag, s in sims.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                s.step()
            torch.cuda.synchronize()
            ms[flag].append((time.perf_counter() - t0) * 1e3 / steps)
    for flag, s in sims.items():
        s.check()
        lines.append("step   E=%d %dx%d  closed loop, procedural worlds with objects, stub cosines, depth_sensor=%-5s %7.2f ms / step "
                     "(%.2f-%.2f over 3 windows of %d steps)" % (N, W, H, flag, *stats(ms[flag]), steps))
        print(lines[-1], flush=True)
    lines.append("step   the sensor costs %.2f ms / step (%.1f %%); invalid pixels of the last step: %.2f %%"
                 % (stats(ms[True])[0] - stats(ms[False])[0], 100.0 * (stats(ms[True])[0] / stats(ms[False])[0] - 1.0),
                    100.0 * float(sims[True].live.sensor_invalid.sum()) / (N * H * W)))
    print(lines[-1], flush=True)
    # the depth pass and the hole path, per-dispatch events, in windows of their own (the events slow the host: no step time here)
    for flag, s in sims.items():
        torch.cuda.synchronize()
        _lib.lib().vlfm_profile_enable(1)
        for _ in range(steps):
            s.step()
        torch.cuda.synchronize()
        read = {k: _lib.profile_read(k) for k in HOLE_KERNELS + ("depth_sensor_kernel",)}
        _lib.lib().vlfm_profile_enable(0)
        s.check()
        lines.append("kernels depth_sensor=%-5s  " % flag + "   ".join("%s %.1f us x %d" % (k, v[0] * 1e3, v[1]) for k, v in read.items())
                     + "   [mean per launch over %d steps]" % steps)
        print(lines[-1], flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "depth_sensor_probe measures on the GPU; there is no CPU path"
    lines = ["depth_sensor_probe: device %s; HIP events, one session, the legs / harnesses alternating" % torch.cuda.get_device_name(0)]
    try:
        probe_launch(a.windows, lines)
        probe_steps(a.steps, lines)
    finally:                                    # what was measured before a failure is kept
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
