"""Times the camera-rig calls against the single-camera calls they replace, in one process, alternating the two:
  value side     one ValueMapBatch.update_cameras            vs  K x ValueMapBatch.update (one camera of every slot per call)
  obstacle side  one ingest_cameras + one update_after_ingest vs  K x (ingest + navigable recompute) + one reveal
for K = 3 and 6 cameras at 1, 16 and 256 slots of 640x480 frames of the rooms world (mid-episode poses).  A call is timed with
device events around the Python call(s) -- launch chain and host prologue included, which is what a step pays -- median / min /
max of --reps calls after warm-up.  The sequential calls are the unchanged single-camera entry points, so they are the baseline
in the same binary.
--harness E [E ...]: instead, env-steps/s of an open-loop BatchedEpisodes with a three-camera rig (stub cosines) at E environments:
the whole step, in which the 3 E frames are ray-cast on the fly -- --windows windows of --steps steps after warm-up.
    python tools/rig_probe.py [--reps 30] [--out profiles/rig_probe.txt]
    python tools/rig_probe.py --harness 8 256 [--steps 20] [--windows 3]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn, before=None):
    import torch

    if before is not None:
        before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3   # microseconds


def stats(xs):
    import numpy as np

    return float(np.median(xs)), float(np.min(xs)), float(np.max(xs))


def probe(E: int, K: int, reps: int, lines) -> None:
    import numpy as np
    import torch

    from vlfm_amd.harness import Camera, CameraRig, RoomsRenderer
    from vlfm_amd.mapping import ObstacleMapBatch, ValueMapBatch
    from vlfm_amd.synthetic import MAX_DEPTH, MIN_DEPTH, camera_intrinsics

    dev = torch.device("cuda:0")
    H, W = 480, 640
    fx, fy, fov = camera_intrinsics(W)
    rig = CameraRig([Camera(yaw=float(y)) for y in np.linspace(-0.5, 0.5, K)])     # overlapping cones, as on a robot
    rr = RoomsRenderer(list(range(E)), 500, H, W, dev)
    slot = np.repeat(np.arange(E), K)
    steps = [150, 151, 152, 153]
    tfs = [rig.camera_tfs(rr.tf_table[t]).reshape(E * K, 4, 4) for t in steps]
    robot = [rr.tf_table[t] for t in steps]
    frames = [rr.cast_cameras(tf) for tf in tfs]                                      # [E*K,H,W], environment-major
    by_cam = [[f.reshape(E, K, H, W)[:, k].contiguous() for k in range(K)] for f in frames]
    rng = np.random.default_rng(0)
    vals = rng.uniform(0.15, 0.45, (E * K, 1))
    d_vals = torch.from_numpy(vals).to(dev)
    d_vals_cam = [torch.from_numpy(vals.reshape(E, K, 1)[:, k].copy()).to(dev) for k in range(K)]

    # ---- value side
    va, vb = ValueMapBatch(E, 1, use_max_confidence=False, device=dev), ValueMapBatch(E, 1, use_max_confidence=False, device=dev)
    keys = [va.column_max(f).clone() for f in frames]
    va._colmax.zero_()
    keys_cam = [[k_.reshape(E, K, W)[:, c].contiguous() for c in range(K)] for k_ in keys]
    work = torch.zeros_like(keys[0])
    work_cam = [torch.zeros_like(keys_cam[0][0]) for _ in range(K)]
    env = np.arange(E)

    def rig_value(i):
        va.update_cameras(d_vals, None, tfs[i], MIN_DEPTH, MAX_DEPTH, fov, slot, colmax=work)

    def seq_value(i):
        for c in range(K):
            vb.update(d_vals_cam[c], None, tfs[i].reshape(E, K, 4, 4)[:, c], MIN_DEPTH, MAX_DEPTH, fov, env_ids=env, colmax=work_cam[c])

    def one_value(i):
        vb.update(d_vals_cam[0], None, tfs[i].reshape(E, K, 4, 4)[:, 0], MIN_DEPTH, MAX_DEPTH, fov, env_ids=env, colmax=work_cam[0])

    def load(i):
        work.copy_(keys[i])
        for c in range(K):
            work_cam[c].copy_(keys_cam[i][c])

    t_rig, t_seq, t_one = [], [], []
    for r in range(reps + 5):
        i = r % 4
        a = timed(lambda: rig_value(i), lambda: load(i))
        b = timed(lambda: seq_value(i), lambda: load(i))
        c = timed(lambda: one_value(i), lambda: load(i))
        if r >= 5:
            t_rig.append(a); t_seq.append(b); t_one.append(c)
    torch.cuda.synchronize()
    # kernel time alone (the library's own event timing of every launch), 10 calls each
    from vlfm_amd import _lib
    _lib.lib().vlfm_profile_enable(1)
    for r in range(10):
        load(r % 4); rig_value(r % 4)
        load(r % 4); seq_value(r % 4)
    torch.cuda.synchronize()
    k_rig, k_seq = _lib.profile_read("value_map_update_rig_kernel"), _lib.profile_read("value_map_update_fused_kernel")
    _lib.lib().vlfm_profile_enable(0)
    lines.append("value    E=%3d K=%d  kernel time: rig launch %.1f us (%d launches)   single-camera launch %.1f us x %d = %.1f us (%d launches)"
                 % (E, K, k_rig[0] * 1e3, k_rig[1], k_seq[0] * 1e3, K, k_seq[0] * 1e3 * K, k_seq[1]))
    lines.append("value    E=%3d K=%d  rig %8.1f us (%.1f-%.1f)   %d x update %8.1f us (%.1f-%.1f)   ratio %.2f   one update %7.1f us (%.1f-%.1f)"
                 % (E, K, *stats(t_rig), K, *stats(t_seq), stats(t_seq)[0] / stats(t_rig)[0], *stats(t_one)))
    del va, vb
    torch.cuda.empty_cache()

    # ---- obstacle side
    kw = dict(min_height=0.61, max_height=0.88, agent_radius=0.18, area_thresh=1.5, device=dev)
    oa, ob = ObstacleMapBatch(E, **kw), ObstacleMapBatch(E, **kw)

    def rig_obst(i):
        oa.ingest_cameras(frames[i], tfs[i], MIN_DEPTH, MAX_DEPTH, fx, fy, slot)
        oa.update_after_ingest(robot[i], MAX_DEPTH, fov)

    def seq_obst(i):
        for c in range(K):
            tf_c = tfs[i].reshape(E, K, 4, 4)[:, c]
            ob.ingest(by_cam[i][c], tf_c, MIN_DEPTH, MAX_DEPTH, fx, fy)
            ob.update_after_ingest(tf_c, MAX_DEPTH, fov, explore=False)
        ob.update_after_ingest(robot[i], MAX_DEPTH, fov, explore=True, update_obstacles=False)

    def one_ingest(i):
        ob.ingest(by_cam[i][0], tfs[i].reshape(E, K, 4, 4)[:, 0], MIN_DEPTH, MAX_DEPTH, fx, fy)

    t_rig, t_seq, t_one = [], [], []
    for r in range(reps + 5):
        i = r % 4
        a = timed(lambda: rig_obst(i))
        b = timed(lambda: seq_obst(i))
        if r >= 5:
            t_rig.append(a); t_seq.append(b)
    torch.cuda.synchronize()
    same = all(bool(torch.equal(x, y)) for x, y in ((oa.obstacle_bits, ob.obstacle_bits), (oa.explored_bits, ob.explored_bits),
                                                     (oa.navigable_bits, ob.navigable_bits)))
    for r in range(reps + 5):
        c = timed(lambda: one_ingest(r % 4))
        if r >= 5:
            t_one.append(c)
    oa.check_status()
    ob.check_status()
    lines.append("obstacle E=%3d K=%d  rig %8.1f us (%.1f-%.1f)   %d x ingest+nav, reveal %8.1f us (%.1f-%.1f)   ratio %.2f   one ingest %7.1f us (%.1f-%.1f)   planes equal: %s"
                 % (E, K, *stats(t_rig), K, *stats(t_seq), stats(t_seq)[0] / stats(t_rig)[0], *stats(t_one), same))
    del oa, ob
    torch.cuda.empty_cache()


def probe_harness(E: int, steps: int, windows: int, lines) -> None:
    import time

    import numpy as np
    import torch

    from vlfm_amd.harness import BatchedEpisodes, Camera, CameraRig

    rig = CameraRig([Camera(yaw=0.5, max_depth=3.5), Camera(yaw=-0.5, forward=0.1, hfov=float(np.deg2rad(60.0))),
                     Camera(yaw=np.pi, left=0.1, value=False, max_depth=2.5)])
    sim = BatchedEpisodes(E, device=torch.device("cuda:0"), use_blip2=False, rig=rig, episode_len=500)
    for _ in range(5):
        sim.step()
    rate = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            sim.step()
        torch.cuda.synchronize()
        rate.append(E * steps / (time.perf_counter() - t0))
    sim.check()
    lines.append("harness  E=%3d K=3  open loop, rig frames ray-cast on the fly: %s env-steps/s per window of %d steps, median %.1f"
                 % (E, " ".join("%.1f" % r for r in rate), steps, stats(rate)[0]))
    del sim
    torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--slots", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--cameras", type=int, nargs="*", default=[3, 6])
    ap.add_argument("--harness", type=int, nargs="+", default=None, help="environments: time whole open-loop rig steps instead")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "rig_probe measures on the GPU; there is no CPU path"
    if a.harness:
        lines = ["rig_probe --harness: device %s" % torch.cuda.get_device_name(0)]
        for E in a.harness:
            probe_harness(E, a.steps, a.windows, lines)
            print(lines[-1], flush=True)
    else:
        lines = ["rig_probe: median (min-max) of %d calls after 5 warm-up calls, device events around the Python call(s), 640x480, "
                 "device %s" % (a.reps, torch.cuda.get_device_name(0))]
        for E in a.slots:
            for K in a.cameras:
                probe(E, K, a.reps, lines)
                print("\n".join(lines[-3:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
