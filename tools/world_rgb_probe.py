"""What the camera's RGB view of the world costs (csrc/world_render.hip: vlfm_worlds_raycast + d_rgb), measured in one place, with HIP
events, in one session, on the same inputs.

  (a) per launch at 256 cameras of 640x480 in 256 generated worlds with their objects: vlfm_worlds_raycast (depth, ids, stats:
      5 bytes per pixel) next to vlfm_worlds_raycast + d_rgb (the same and the colour plane: 8 bytes per pixel).  Two clocks: the
      events the library attaches to the dispatch itself (vlfm_profile_enable: the kernel alone) and a pair of events around a
      window of calls (the small host-to-device copy, the fill of the stats and the kernel).  The two entries alternate over
      --windows windows of LAUNCHES launches after WARMUP warm-up launches each.
  (b) the step of a 256-environment closed-loop harness in procedural worlds with objects, no model (stub cosines), with and
      without render_rgb, the two harnesses alternating over 3 windows of --steps steps after 15 steps in.

    python tools/world_rgb_probe.py [--windows 5] [--steps 20] [--out profiles/world_rgb_probe.txt]"""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N, H, W = 256, 480, 640
LAUNCHES, WARMUP = 20, 3
KERNELS = {"vlfm_worlds_raycast": "worlds_raycast_objects_kernel", "vlfm_worlds_raycast + d_rgb": "worlds_raycast_rgb_kernel"}


def stats(xs):
    import numpy as np

    return float(np.median(xs)), float(np.min(xs)), float(np.max(xs))


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
    colours = np.zeros((N, S.WORLD_MAX_OBJECTS), np.int32)
    for e in range(N):
        for k, (cls, box) in enumerate(worlds.layout(e, 0, made[e].start_xy)):
            objects[e, k, :6], objects[e, k, 6], colours[e, k] = box, 1.0, S.OBJECT_COLOURS[cls]
    idx = np.arange(N)
    depth = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    rgb = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
    calls = {"vlfm_worlds_raycast": lambda: rooms.cast_worlds(tf, table, idx, objects, idx, out=depth),
             "vlfm_worlds_raycast + d_rgb": lambda: rooms.cast_worlds_rgb(tf, table, idx, objects, idx, colours, out=depth, rgb_out=rgb)}
    a = calls["vlfm_worlds_raycast"]()
    b = calls["vlfm_worlds_raycast + d_rgb"]()
    torch.cuda.synchronize()
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    pixels = int((b[1] > 0).sum())
    kernel = {k: [] for k in calls}
    call = {k: [] for k in calls}
    for _ in range(windows):
        for name, fn in calls.items():
            for _ in range(WARMUP):
                fn()
            torch.cuda.synchronize()
            _lib.lib().vlfm_profile_enable(1)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(LAUNCHES):
                fn()
            stop.record()
            torch.cuda.synchronize()
            ms, n = _lib.profile_read(KERNELS[name])
            _lib.lib().vlfm_profile_enable(0)
            assert n == LAUNCHES, (name, n)
            kernel[name].append(ms * 1e3)
            call[name].append(start.elapsed_time(stop) * 1e3 / LAUNCHES)
    written = {"vlfm_worlds_raycast": 5, "vlfm_worlds_raycast + d_rgb": 8}
    for name in calls:
        k = stats(kernel[name])
        lines.append("launch n=%d %dx%d  %-24s kernel %7.1f us (%.1f-%.1f)   whole call %7.1f us (%.1f-%.1f)   %d B/pixel: %.0f MB, "
                     "%.2f TB/s over the kernel   [medians of %d window means of %d launches]"
                     % (N, W, H, name, *k, *stats(call[name]), written[name], written[name] * N * H * W / 1e6,
                        written[name] * N * H * W / (k[0] * 1e-6) / 1e12, windows, LAUNCHES))
        print(lines[-1], flush=True)
    lines.append("ratio rgb / plain: kernel %.2fx, whole call %.2fx (the bytes written: 1.60x); object pixels %d of %d; boxes per "
                 "world %d-%d"
                 % (stats(kernel["vlfm_worlds_raycast + d_rgb"])[0] / stats(kernel["vlfm_worlds_raycast"])[0],
                    stats(call["vlfm_worlds_raycast + d_rgb"])[0] / stats(call["vlfm_worlds_raycast"])[0], pixels, N * H * W,
                    min(len(w.boxes) for w in made), max(len(w.boxes) for w in made)))
    print(lines[-1], flush=True)


def probe_steps(steps: int, lines) -> None:
    import time

    import torch

    from vlfm_amd.harness import BatchedEpisodes, WorldObjects
    from vlfm_amd.synthetic import ProceduralWorlds

    sims = {flag: BatchedEpisodes(N, device=torch.device("cuda:0"), use_blip2=False, select_frontiers=True, episode_len=500,
                                  closed_loop=True, world_objects=WorldObjects(), worlds=ProceduralWorlds(0), render_rgb=flag)
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
        lines.append("step   E=%d %dx%d  closed loop, procedural worlds with objects, stub cosines, render_rgb=%-5s %7.2f ms / step "
                     "(%.2f-%.2f over 3 windows of %d steps)" % (N, W, H, flag, *stats(ms[flag]), steps))
        print(lines[-1], flush=True)
    lines.append("step   render_rgb costs %.2f ms / step (%.1f %%)"
                 % (stats(ms[True])[0] - stats(ms[False])[0], 100.0 * (stats(ms[True])[0] / stats(ms[False])[0] - 1.0)))
    print(lines[-1], flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "world_rgb_probe measures on the GPU; there is no CPU path"
    lines = ["world_rgb_probe: device %s; HIP events, one session, the two entries / harnesses alternating" % torch.cuda.get_device_name(0)]
    probe_launch(a.windows, lines)
    probe_steps(a.steps, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
