"""What the depth filter costs (csrc/depth_filter.hip: vlfm_depth_filter), measured in one place, with HIP events, in one session,
on the same buffers.

  (a) per call at 256 frames of 640x480 (256 generated worlds with their objects, ray-cast once): the filter on the ray caster's
      frames (no holes), on what a sensor with dropout = 0.01 makes of them and on what a sensor with every stage on makes of
      them, next to a plain device-to-device copy of the frames.  Two clocks: the events the library attaches to each dispatch
      (vlfm_profile_enable: the row pass and the column pass alone) and a pair of events around a window of calls (with the
      memset of the counts).  The legs alternate over --windows windows of LAUNCHES calls after WARMUP warm-up calls each.
  (b) the step of a 256-environment closed-loop harness in procedural worlds with objects, no model (stub cosines): without a
      sensor, with the sensor, and with the sensor and the filter, the harnesses alternating over 3 windows of --steps steps
      after 15 steps in; then, in windows of their own with the library's per-dispatch events on, the hole path of the obstacle
      map and the new kernels (mean per launch, one launch per step).

    python tools/depth_filter_probe.py [--windows 5] [--steps 20] [--out profiles/depth_filter_probe.txt]"""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N, H, W = 256, 480, 640
LAUNCHES, WARMUP = 20, 3
FILTER_KERNELS = ("depth_filter_rows_kernel", "depth_filter_cols_kernel")
STEP_KERNELS = ("depth_ingest_scatter_kernel", "fill_small_holes_kernel", "hole_scatter_kernel", "depth_sensor_kernel") + FILTER_KERNELS


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
    idx, clocks = np.arange(N), np.arange(N) % 7
    clean = rooms.cast_worlds(tf, table, idx, objects, idx)[0]
    sensors = {"no holes": None, "dropout 0.01": S.DepthSensor(seed=1, dropout=0.01),
               "all sensor stages": S.DepthSensor(seed=1, sigma0_m=0.002, sigma2_per_m=0.002, disparity_k=35.0, dropout=0.01,
                                                  patch_dropout=0.002, edge_m=0.3, min_range_m=0.55, max_range_m=4.9)}
    inputs = {k: clean if s is None else rooms.sense_depth(clean, s, idx, clocks)[0] for k, s in sensors.items()}
    out = torch.empty_like(clean)
    counts = torch.empty((N, 2), dtype=torch.int32, device=dev)
    flt = S.DepthFilter()
    calls = {"filter, " + k: (lambda x=x: rooms.filter_depth(x, flt, out=out, counts_out=counts)) for k, x in inputs.items()}
    calls["filter, all sensor stages, reach_px=8"] = lambda: rooms.filter_depth(inputs["all sensor stages"], S.DepthFilter(reach_px=8),
                                                                                 out=out, counts_out=counts)
    calls["device-to-device copy"] = lambda: out.copy_(clean)
    holes = {}
    for name, fn in calls.items():
        fn()
        torch.cuda.synchronize()
        if name.startswith("filter"):
            c = counts.sum(dim=0).tolist()
            holes[name] = (c[0] + c[1], c[1])
    # the call is the statement's frames (three of the 256, all sensor stages on)
    rooms.filter_depth(inputs["all sensor stages"], flt, out=out, counts_out=counts)
    torch.cuda.synchronize()
    for e in (0, 100, 255):
        want, filled, left = S.depth_filter_numpy(inputs["all sensor stages"][e].cpu().numpy(), flt)
        assert want.tobytes() == out[e].cpu().numpy().tobytes() and [filled, left] == counts[e].tolist(), e
    kernel = {k: {f: [] for f in FILTER_KERNELS} for k in calls if k.startswith("filter")}
    call = {k: [] for k in calls}
    for _ in range(windows):
        for name, fn in calls.items():
            for _ in range(WARMUP):
                fn()
            torch.cuda.synchronize()
            if name in kernel:
                _lib.lib().vlfm_profile_enable(1)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(LAUNCHES):
                fn()
            stop.record()
            torch.cuda.synchronize()
            if name in kernel:
                for f in FILTER_KERNELS:
                    ms, n = _lib.profile_read(f)
                    assert n == LAUNCHES, (name, f, n)
                    kernel[name][f].append(ms * 1e3)
                _lib.lib().vlfm_profile_enable(0)
            call[name].append(start.elapsed_time(stop) * 1e3 / LAUNCHES)
    copy_us = stats(call["device-to-device copy"])
    lines.append("call   n=%d %dx%d  %-38s whole call %7.1f us (%.1f-%.1f)   8 B/pixel: %.0f MB   [medians of %d window means of %d calls]"
                 % (N, W, H, "device-to-device copy", *copy_us, 8 * N * H * W / 1e6, windows, LAUNCHES))
    print(lines[-1], flush=True)
    for name in kernel:
        rows, cols, c = stats(kernel[name][FILTER_KERNELS[0]]), stats(kernel[name][FILTER_KERNELS[1]]), stats(call[name])
        lines.append("call   n=%d %dx%d  %-38s row pass %7.1f us (%.1f-%.1f)   column pass %7.1f us (%.1f-%.1f)   whole call %7.1f us "
                     "(%.1f-%.1f)   %.2f %% of the pixels holes, %.4f %% left" % (N, W, H, name, *rows, *cols, *c,
                                                                                100.0 * holes[name][0] / (N * H * W),
                                                                                100.0 * holes[name][1] / (N * H * W)))
        print(lines[-1], flush=True)
        lines.append("ratio  %-38s (row pass + column pass) / copy %.2fx, row pass / copy %.2fx, column pass / copy %.2fx, whole call / "
                     "copy %.2fx" % (name, (rows[0] + cols[0]) / copy_us[0], rows[0] / copy_us[0], cols[0] / copy_us[0], c[0] / copy_us[0]))
        print(lines[-1], flush=True)


def probe_steps(steps: int, lines) -> None:
    import time

    import torch

    from vlfm_amd import _lib
    from vlfm_amd.harness import BatchedEpisodes, WorldObjects
    from vlfm_amd.synthetic import DepthFilter, ProceduralWorlds

    modes = {"no sensor": (None, None), "sensor": (harness_sensor(), None), "sensor + filter": (harness_sensor(), DepthFilter())}
    sims = {k: BatchedEpisodes(N, device=torch.device("cuda:0"), use_blip2=False, select_frontiers=True, episode_len=500,
                               closed_loop=True, world_objects=WorldObjects(), worlds=ProceduralWorlds(0), depth_sensor=s,
                               depth_filter=f)
            for k, (s, f) in modes.items()}
    for s in sims.values():
        for _ in range(15):
            s.step()
    ms = {k: [] for k in sims}
    for _ in range(3):
        for k, s in sims.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                s.step()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
    for k, s in sims.items():
        s.check()
        lines.append("step   E=%d %dx%d  closed loop, procedural worlds with objects, stub cosines, %-16s %7.2f ms / step "
                     "(%.2f-%.2f over 3 windows of %d steps)" % (N, W, H, k, *stats(ms[k]), steps))
        print(lines[-1], flush=True)
    live = sims["sensor + filter"].live
    c = live.filter_counts.sum(dim=0).tolist()
    lines.append("step   the filter takes the step with a sensor from %.2f to %.2f ms; last step: %.2f %% of the pixels invalid after the "
                 "sensor, %.2f %% filled, %.4f %% left" % (stats(ms["sensor"])[0], stats(ms["sensor + filter"])[0],
                                                          100.0 * float(live.sensor_invalid.sum()) / (N * H * W),
                                                          100.0 * c[0] / (N * H * W), 100.0 * c[1] / (N * H * W)))
    print(lines[-1], flush=True)
    # the hole path and the new kernels, per-dispatch events, in windows of their own (the events slow the host: no step time here)
    for k, s in sims.items():
        torch.cuda.synchronize()
        _lib.lib().vlfm_profile_enable(1)
        for _ in range(steps):
            s.step()
        torch.cuda.synchronize()
        read = {name: _lib.profile_read(name) for name in STEP_KERNELS}
        _lib.lib().vlfm_profile_enable(0)
        s.check()
        lines.append("kernels %-16s " % k + "   ".join("%s %.1f us x %d" % (name, v[0] * 1e3, v[1]) for name, v in read.items())
                     + "   [mean per launch over %d steps]" % steps)
        print(lines[-1], flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "depth_filter_probe measures on the GPU; there is no CPU path"
    lines = ["depth_filter_probe: device %s; HIP events, one session, the legs / harnesses alternating" % torch.cuda.get_device_name(0)]
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
