"""What closing the loop costs and what the ray-cast kernel (csrc/world_render.hip) buys, measured in one place.

  (a) RoomsRenderer.cast_cameras (one launch): device events around the Python call -- host prologue, the record's H2D copy
      and the launch chain included, which is what a step pays -- median (min-max) of --reps calls after warm-up, at
      256 / 128 / 8 frames of 640x480 and 16 frames of 1280x720.  (profiles/world_render_probe.txt also holds the column of the
      chain of torch f64 operations the kernel replaced, and the bit comparison with it, from before that chain was removed.)
  (b) env-steps/s of a closed-loop harness next to an open-loop harness that renders on the fly (no prepare()), at 256 and 8
      environments, both with the BLIP-2 forward (random-init weights) and the frontier decision.
  (c) kernel time of rooms_raycast_kernel from `rocprofv3 --kernel-trace --stats`, in a run of its own (a fresh child
      process: tracing slows the host, so nothing else is timed there), and n*H*W*4 bytes over it as a share of the 8 TB/s HBM
      peak and of the 6.29 TB/s a float4 copy kernel reaches on this chip.

    python tools/world_render_probe.py [--reps 200] [--steps 20] [--skip-steps] [--skip-trace] [--out profiles/world_render_probe.txt]
    python tools/world_render_probe.py --trace-child        # the process (c) points rocprofv3 at"""
import argparse
import glob
import os
import shutil
import sqlite3
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SIZES = [(256, 480, 640), (128, 480, 640), (8, 480, 640), (16, 720, 1280)]      # (frames, H, W)
TRACE_LAUNCHES, TRACE_WARMUP = 50, 5
HBM_PEAK, COPY_RATE = 8.0e12, 6.29e12


def cameras(n: int, H: int, W: int, dev):
    """(renderer, transforms [n,4,4], hfov, lo, hi): a three-camera rig's cameras on mid-episode poses of the tour -- arbitrary
    yaws, two optics, two depth ranges."""
    import numpy as np

    from vlfm_amd.harness import Camera, CameraRig, RoomsRenderer
    from vlfm_amd.synthetic import camera_intrinsics

    rig = CameraRig([Camera(yaw=0.5, max_depth=3.5), Camera(yaw=-0.5, forward=0.1, hfov=float(np.deg2rad(60.0))), Camera()])
    E = -(-n // 3)
    rr = RoomsRenderer(list(range(E)), 500, H, W, dev)
    tf = rig.camera_tfs(rr.tf_table[150]).reshape(-1, 4, 4)[:n]
    cam = np.tile(np.arange(3), E)[:n]
    per = lambda f: np.array([f(c) for c in rig.cameras])[cam]   # noqa: E731
    fov = camera_intrinsics(W)[2]
    return rr, tf, per(lambda c: fov if c.hfov is None else c.hfov), per(lambda c: c.min_depth), per(lambda c: c.max_depth)


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


def probe_calls(reps: int, lines) -> None:
    import torch

    dev = torch.device("cuda:0")
    for n, H, W in SIZES:
        rr, tf, hfov, lo, hi = cameras(n, H, W, dev)
        out = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        t_k = [timed(lambda: rr.cast_cameras(tf, hfov, lo, hi, out=out)) for _ in range(reps + 10)][10:]
        torch.cuda.synchronize()
        lines.append("calls  n=%3d %4dx%-4d  cast_cameras %9.1f us (%.1f-%.1f)" % (n, W, H, *stats(t_k)))
        print(lines[-1], flush=True)
        del rr, out
        torch.cuda.empty_cache()


def probe_steps(steps: int, lines) -> None:
    import time

    import torch

    from vlfm_amd.harness import BatchedEpisodes
    from vlfm_amd.vlm.blip2itm import BLIP2ITM

    dev = torch.device("cuda:0")
    blip2 = BLIP2ITM(device=dev, allow_random_init=True)
    for E in (256, 8):
        kw = dict(device=dev, blip2=blip2, select_frontiers=True, episode_len=500)
        sims = {"closed loop": BatchedEpisodes(E, closed_loop=True, **kw), "open loop, rendered on the fly": BatchedEpisodes(E, **kw)}
        rate = {k: [] for k in sims}
        for s in sims.values():
            s.fast_forward(30)             # mid-episode maps; the closed-loop robots walk there under their controller
            for _ in range(3):
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
            if s.closed_loop:
                st = s.live.stats
                extra = "   path %.1f m mean, %d refused moves, %d stops" % (float(st["path_length"].mean()),
                                                                           int(st["collisions"].sum()), int(st["stops"].sum()))
            lines.append("steps  E=%3d  %-31s %8.1f env-steps/s (%.1f-%.1f over 3 windows of %d steps)%s"
                         % (E, name, *stats(rate[name]), steps, extra))
            print(lines[-1], flush=True)
        del sims
        torch.cuda.empty_cache()


def trace_child() -> None:
    """Per size, TRACE_WARMUP + TRACE_LAUNCHES launches of the kernel and nothing else on the device, in the order of SIZES."""
    import torch

    dev = torch.device("cuda:0")
    for n, H, W in SIZES:
        rr, tf, hfov, lo, hi = cameras(n, H, W, dev)
        out = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        for _ in range(TRACE_WARMUP + TRACE_LAUNCHES):
            rr.cast_cameras(tf, hfov, lo, hi, out=out)
        torch.cuda.synchronize()


def probe_trace(lines, workdir: str) -> None:
    import numpy as np

    if shutil.which("rocprofv3") is None:
        raise RuntimeError("rocprofv3 not found: the kernel-time leg needs it (--skip-trace leaves the leg out)")
    shutil.rmtree(workdir, ignore_errors=True)
    os.makedirs(workdir)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", workdir, "-o", "world_render", "--", sys.executable,
           os.path.abspath(__file__), "--trace-child"]
    with open(os.path.join(workdir, "child.log"), "w") as log:
        subprocess.run(cmd, check=True, stdout=log, stderr=subprocess.STDOUT, timeout=300)
    dbs = glob.glob(os.path.join(workdir, "**", "*_results.db"), recursive=True)
    if not dbs:
        raise RuntimeError(f"no rocprofv3 database under {workdir}")
    rows = sqlite3.connect(dbs[0]).execute("select name, start, end from kernels order by start").fetchall()
    ours = [(e - s) * 1e-3 for (name, s, e) in rows if "rooms_raycast_kernel" in name]
    per = TRACE_WARMUP + TRACE_LAUNCHES
    if len(ours) != per * len(SIZES):
        raise RuntimeError(f"expected {per * len(SIZES)} dispatches of rooms_raycast_kernel in the trace, found {len(ours)}")
    for i, (n, H, W) in enumerate(SIZES):
        us = np.array(ours[i * per + TRACE_WARMUP:(i + 1) * per])
        nbytes = n * H * W * 4
        rate = nbytes / (float(np.median(us)) * 1e-6)
        lines.append("kernel n=%3d %4dx%-4d  rooms_raycast_kernel %8.1f us (%.1f-%.1f, %d launches)   %6.1f MB written   %5.2f TB/s = "
                     "%4.1f %% of the 8 TB/s peak, %4.1f %% of the 6.29 TB/s float4 copy"
                     % (n, W, H, *stats(us), len(us), nbytes / 1e6, rate / 1e12, 100 * rate / HBM_PEAK, 100 * rate / COPY_RATE))
        print(lines[-1], flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--workdir", default=os.path.join(ROOT, "scratch", "world_render_trace"),
                    help="where the kernel trace of leg (c) is written (removed and rewritten by every run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "world_render_probe measures on the GPU; there is no CPU path"
    if a.trace_child:
        return trace_child()
    lines = ["world_render_probe: device %s; (a) device events around the Python call, median (min-max) of %d calls after 10 "
             "warm-up calls" % (torch.cuda.get_device_name(0), a.reps)]
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
