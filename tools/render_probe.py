"""Times the map renderer (csrc/map_render.hip) at 1 / 8 / 256 slots of 1000 x 1000 maps against the bytes it must move,
and the host path it replaces (download the slot's value map and explored plane, colour with NumPy).  Prints one JSON
line per configuration.  Usage: python tools/render_probe.py [--reps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0


def _kernels(names, fn, reps):
    """Mean device time per call of the named kernels (the library's own event timing), in ms."""
    from vlfm_amd import _lib

    _lib.lib().vlfm_profile_enable(1)
    for _ in range(reps):
        fn()
    import torch

    torch.cuda.synchronize()
    out = {}
    for k in names:
        ms, launches = _lib.profile_read(k)
        out[k] = round(ms, 4)
    _lib.lib().vlfm_profile_enable(0)   # (also clears the log)
    return out


def _time(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    import torch

    from vlfm_amd.mapping.obstacle_map import ObstacleMapBatch
    from vlfm_amd.mapping.value_map import ValueMapBatch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    S, dev = 1000, torch.device("cuda:0")
    rng = np.random.default_rng(0)
    for n in (1, 8, 256):
        vb = ValueMapBatch(n, 1, S, use_max_confidence=False, device=dev)
        vb.n_updates[:] = 1
        vb.value.uniform_(0, 1)
        vb.value[vb.value < 0.3] = 0
        W = (S + 31) // 32
        vb.explored_bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, S, W), dtype=torch.int32, device=dev)
        for e in range(n):
            pos = rng.uniform(-10, 10, (30, 2))
            vb.update_agent_traj([e] * len(pos), pos, [0.3] * len(pos))
        mk = np.array([[e, *rng.integers(0, S, 2), 5, 2, 0, 0, 255] for e in range(n) for _ in range(20)])
        out = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
        call = lambda: vb.render(range(n), markers=mk, out=out)  # noqa: E731
        ms = _time(call, args.reps)
        k = _kernels(("value_partials_kernel", "value_color_kernel", "primitive_kernel"), call, args.reps)
        # bytes the colour passes must move: the f64 value plane read twice (min/max, colour), explored + path words, frame
        nbytes = n * (2 * S * S * 8 + 2 * S * W * 4 + S * W * 4 + S * S * 3)
        dev_ms = k["value_partials_kernel"] + k["value_color_kernel"]
        row = {"map": "value", "slots": n, "call_ms": round(ms, 4), "kernels_ms": k, "colour_ms_per_slot": round(dev_ms / n, 5),
               "bytes": nbytes, "GBs": round(nbytes / dev_ms / 1e6, 1), "hbm_frac": round(nbytes / dev_ms / 1e6 / HBM_PEAK_GBS, 4)}
        if n == 1:
            t0 = time.perf_counter()
            for _ in range(3):
                v = vb.value[0].cpu().numpy()[..., 0]
                ex = vb.explored_bits[0].cpu().numpy()
                img = np.flipud(v.copy())
                zero = img == 0
                img[zero] = img.max()
                lo, hi = img.min(), img.max()
                _ = ((img - lo) / (hi - lo) * 255).astype(np.uint8), ex
            row["host_path_ms_per_slot"] = round((time.perf_counter() - t0) / 3 * 1e3, 2)
        print(json.dumps(row), flush=True)
        del vb, out
        torch.cuda.empty_cache()
    for n in (1, 8, 64):
        ob = ObstacleMapBatch(n, 0.61, 0.88, 0.18, size=S, device=dev)
        for t in (ob.obstacle_bits, ob.navigable_bits, ob.explored_bits):
            t.random_(-2 ** 31, 2 ** 31 - 1)
        fr = [rng.uniform(0, S, (20, 2)) for _ in range(n)]
        out = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
        call = lambda: ob.render(range(n), fr, out=out)  # noqa: E731
        ms = _time(call, args.reps)
        k = _kernels(("obstacle_color_kernel", "primitive_kernel"), call, args.reps)
        W = (S + 31) // 32
        nbytes = n * (3 * S * W * 4 + S * W * 4 + S * S * 3)
        dev_ms = k["obstacle_color_kernel"]
        print(json.dumps({"map": "obstacle", "slots": n, "call_ms": round(ms, 4), "kernels_ms": k,
                          "colour_ms_per_slot": round(dev_ms / n, 5), "bytes": nbytes, "GBs": round(nbytes / dev_ms / 1e6, 1),
                          "hbm_frac": round(nbytes / dev_ms / 1e6 / HBM_PEAK_GBS, 4)}), flush=True)
        del ob, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
