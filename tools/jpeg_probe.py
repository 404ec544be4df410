"""Times the device JPEG transport (csrc/jpeg_codec.hip via transport.jpeg_roundtrip_batch) with device events after warm-up,
as the median of repeats, at 1 / 8 / 64 / 256 frames of 640x480 and 16 / 128 frames of 1280x720.  With --step it then times the
256-environment BatchedEpisodes step with emulate_jpeg off and on, alternated within one process, set up as bench.py sets up
its headline run (blocking host waits before the first stream, one host thread, pre-rolled episodes, pre-rendered depth,
strict HIP attention); --step --no-blip2 does the same with stub cosines (no BLIP-2 forward) instead.  Prints one JSON line
per configuration.  Usage: python tools/jpeg_probe.py [--reps 30] [--step [--no-blip2] [--steps 10] [--rounds 3]]

--encode times the encoder instead (transport.jpeg_encode_batch, csrc/jpeg_entropy.hip): natural 640x480 and 1280x720 frames
and rendered 1000x1000 map frames of a stepped harness, each alternated call by call with the path it replaces -- download
the raw frames, encode them with Pillow on 16 threads.

--decode times the decoder (transport.jpeg_decode_batch, csrc/jpeg_decode.hip) in its device form on files Pillow wrote
without restart markers and with one restart interval per MCU row, and on this package's files of rendered 1000x1000 maps,
each alternated call by call with the path it replaces: Pillow decode on 16 threads plus the upload of the raw frames."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0


def roundtrip(device, n, h, w, reps):
    import numpy as np
    import torch

    from vlfm_amd.vlm.transport import jpeg_roundtrip_batch, jpeg_roundtrip_scratch

    g = torch.Generator(device=device).manual_seed(n * h)
    x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=device, generator=g)
    out, scratch = torch.empty_like(x), jpeg_roundtrip_scratch(n, h, w, device)
    for _ in range(3):
        jpeg_roundtrip_batch(x, 90, out=out, scratch=scratch)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        jpeg_roundtrip_batch(x, 90, out=out, scratch=scratch)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    med = float(np.median(ms))
    # frames in + out, plus the decoded planes written by the coding pass and read by the upsampling pass
    moved = 2 * x.numel() + 2 * scratch.numel()
    return {"what": "jpeg_roundtrip_batch q90", "n": n, "H": h, "W": w, "median_ms": round(med, 4),
            "min_ms": round(min(ms), 4), "us_per_frame": round(1000 * med / n, 2), "MB_moved": round(moved / 1e6, 1),
            "GB_s": round(moved / med / 1e6, 1), "pct_hbm_peak": round(100 * moved / med / 1e6 / HBM_PEAK_GBS, 1)}


def _natural_frames(n, h, w, seed):
    """Frames with smooth structure, edges and sensor noise, distinct per draw (what a camera or a renderer gives)."""
    import numpy as np

    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for _ in range(n):
        a, b, c = rng.uniform(3, 40, 3)
        img = np.stack([127 + 100 * np.sin(xx / a + rng.uniform(0, 6)), 127 + 100 * np.cos(yy / b + rng.uniform(0, 6)),
                        (xx + yy) * c % 256], axis=-1)
        for _ in range(4):
            y0, x0 = rng.integers(0, h), rng.integers(0, w)
            img[y0:y0 + rng.integers(1, h // 2 + 2), x0:x0 + rng.integers(1, w // 2 + 2)] = rng.integers(0, 256, 3)
        out.append(np.clip(img + rng.normal(0, rng.uniform(0, 6), img.shape), 0, 255).astype(np.uint8))
    return np.stack(out)


def encode(device, what, x, order, reps, pool):
    """Median device time of jpeg_encode_batch on the device frames x, alternated with the host path: D2H of the raw frames
    + Pillow on the thread pool (wall time)."""
    import io

    import numpy as np
    import torch
    from PIL import Image

    from vlfm_amd.vlm.transport import jpeg_encode_batch, jpeg_encode_bound, jpeg_encode_scratch

    n, h, w, _ = x.shape
    cap = jpeg_encode_bound(h, w)
    out = torch.empty((n, cap), dtype=torch.uint8, device=device)
    lengths = torch.empty(n, dtype=torch.int32, device=device)
    scratch = jpeg_encode_scratch(n, h, w, device)

    def host_one(f):
        buf = io.BytesIO()
        Image.fromarray(f if order == "rgb" else f[..., ::-1]).save(buf, format="JPEG", quality=90, subsampling="4:2:0")
        return buf.getvalue()

    def host_path():
        t0 = time.perf_counter()
        frames = x.cpu().numpy()
        files = list(pool.map(host_one, frames))
        return 1000 * (time.perf_counter() - t0), files

    for _ in range(3):
        jpeg_encode_batch(x, 90, order, out=out, lengths=lengths, scratch=scratch)
    host_path()
    torch.cuda.synchronize()
    ms, host_ms = [], []
    for r in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        jpeg_encode_batch(x, 90, order, out=out, lengths=lengths, scratch=scratch)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
        if r < max(3, reps // 5):   # (the host path is slow: a few alternations give its median)
            host_ms.append(host_path()[0])
    lens = lengths.cpu().numpy().astype(np.int64)
    files = host_path()[1]
    same = all(out[i, :lens[i]].cpu().numpy().tobytes() == files[i] for i in range(0, n, max(1, n // 4)))
    med, host_med = float(np.median(ms)), float(np.median(host_ms))
    mcus = n * ((h + 15) // 16) * ((w + 15) // 16)
    stream = int(lens.sum()) - 625 * n      # (about: the stuffing zeros are counted as stream bytes)
    # input read; coefficients written, read by the length and the pack pass; stream written, read by the count and the
    # copy pass; files written
    moved = x.numel() + 3 * 768 * mcus + 3 * stream + int(lens.sum())
    return {"what": what, "n": n, "H": h, "W": w, "order": order, "median_ms": round(med, 4), "min_ms": round(min(ms), 4),
            "us_per_frame": round(1000 * med / n, 2), "out_bytes": int(lens.sum()), "MB_moved": round(moved / 1e6, 1),
            "GB_s": round(moved / med / 1e6, 1), "pct_hbm_peak": round(100 * moved / med / 1e6 / HBM_PEAK_GBS, 2),
            "host_pillow16_ms": round(host_med, 2), "speedup": round(host_med / med, 1), "bytes_equal_pillow": bool(same)}


def encode_all(device, reps):
    from concurrent.futures import ThreadPoolExecutor

    import torch

    from vlfm_amd.harness import BatchedEpisodes

    with ThreadPoolExecutor(16) as pool:
        for n, h, w in [(1, 480, 640), (8, 480, 640), (64, 480, 640), (256, 480, 640), (16, 720, 1280)]:
            x = torch.from_numpy(_natural_frames(n, h, w, n * h)).to(device)
            print(json.dumps(encode(device, "jpeg_encode_batch q90 natural", x, "bgr", reps, pool)), flush=True)
            del x
        sim = BatchedEpisodes(64, device=device, use_blip2=False, world="rooms", render_trajectories=True)
        for _ in range(40):
            sim.step()
        torch.cuda.synchronize(device)
        for n in (8, 64):
            frames = sim.render(list(range(n)))
            for name in ("value_map", "obstacle_map"):
                print(json.dumps(encode(device, f"jpeg_encode_batch q90 rendered {name}", frames[name].contiguous(), "rgb",
                                        reps, pool)), flush=True)


def decode(device, what, files, reps, pool):
    """Median device time of jpeg_decode_batch (device form: the files lie in a [n, capacity] device tensor and share their
    header) alternated with the host path: Pillow decode on the thread pool + H2D of the raw frames (wall time).  Also the
    wall time of the host form (parse, one upload, decode)."""
    import io

    import numpy as np
    import torch
    from PIL import Image

    from vlfm_amd.vlm.transport import jpeg_decode_batch, jpeg_decode_scratch, jpeg_parse

    n = len(files)
    info = jpeg_parse(files[0])
    h, w, header = info["height"], info["width"], files[0][:info["scan_offset"]]
    assert all(f[:len(header)] == header for f in files)
    cap = (max(map(len, files)) + 15) & ~15
    host = np.zeros((n, cap), np.uint8)
    for i, f in enumerate(files):
        host[i, :len(f)] = np.frombuffer(f, np.uint8)
    d_files = torch.from_numpy(host).to(device)
    d_len = torch.tensor([len(f) for f in files], dtype=torch.int32, device=device)
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=device)
    status = torch.empty(n, dtype=torch.int32, device=device)
    scratch = jpeg_decode_scratch(n, h, w, cap, device)

    def host_one(f):
        return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))

    def host_path():
        t0 = time.perf_counter()
        frames = torch.from_numpy(np.stack(list(pool.map(host_one, files)))).to(device)
        torch.cuda.synchronize()
        return 1000 * (time.perf_counter() - t0), frames

    def host_form():
        t0 = time.perf_counter()
        jpeg_decode_batch(files, channel_order="rgb", out=out, status=status, scratch=scratch, device=device)
        torch.cuda.synchronize()
        return 1000 * (time.perf_counter() - t0)

    for _ in range(3):
        jpeg_decode_batch(d_files, d_len, header=header, channel_order="rgb", out=out, status=status, scratch=scratch)
    host_path()
    host_form()
    torch.cuda.synchronize()
    ms, host_ms, form_ms = [], [], []
    for r in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        jpeg_decode_batch(d_files, d_len, header=header, channel_order="rgb", out=out, status=status, scratch=scratch)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
        if r < max(3, reps // 5):   # (the host paths are slow: a few alternations give their medians)
            host_ms.append(host_path()[0])
            form_ms.append(host_form())
    jpeg_decode_batch(d_files, d_len, header=header, channel_order="rgb", out=out, status=status, scratch=scratch)
    same = bool(torch.equal(out, host_path()[1])) and not bool(status.any())
    med, host_med = float(np.median(ms)), float(np.median(host_ms))
    return {"what": what, "n": n, "H": h, "W": w, "restart_interval": info["restart_interval"], "median_ms": round(med, 4),
            "min_ms": round(min(ms), 4), "us_per_frame": round(1000 * med / n, 2), "file_bytes": int(sum(map(len, files))),
            "host_pillow16_upload_ms": round(host_med, 2), "speedup": round(host_med / med, 2),
            "host_form_wall_ms": round(float(np.median(form_ms)), 2), "pixels_equal_pillow": same}


def decode_all(device, reps):
    import io
    from concurrent.futures import ThreadPoolExecutor

    import torch
    from PIL import Image

    from vlfm_amd.harness import BatchedEpisodes

    def pillow_files(x, **kw):
        out = []
        for f in x:
            buf = io.BytesIO()
            Image.fromarray(f).save(buf, format="JPEG", quality=90, subsampling="4:2:0", **kw)
            out.append(buf.getvalue())
        return out

    with ThreadPoolExecutor(16) as pool:
        for n, h, w in [(1, 480, 640), (8, 480, 640), (64, 480, 640), (256, 480, 640), (16, 720, 1280)]:
            x = _natural_frames(n, h, w, n * h)
            print(json.dumps(decode(device, "jpeg_decode_batch q90 natural", pillow_files(x), reps, pool)), flush=True)
            if h == 480:
                print(json.dumps(decode(device, "jpeg_decode_batch q90 natural, Ri = one MCU row",
                                        pillow_files(x, restart_marker_rows=1), reps, pool)), flush=True)
        sim = BatchedEpisodes(64, device=device, use_blip2=False, world="rooms", render_trajectories=True)
        for _ in range(40):
            sim.step()
        torch.cuda.synchronize(device)
        for name, files in sim.render_jpeg().items():
            print(json.dumps(decode(device, f"jpeg_decode_batch q90 rendered {name}", files, reps, pool)), flush=True)


def step_rate(device, envs, steps, rounds, preroll, use_blip2):
    import torch

    from vlfm_amd.harness import BatchedEpisodes

    blip2 = None
    if use_blip2:
        from vlfm_amd.vlm.blip2itm import BLIP2ITM

        blip2 = BLIP2ITM(device=device, allow_random_init=True)
        blip2.strict_hip_attention = True   # as bench.py: a silent library fallback would change what is measured
    sims = {on: BatchedEpisodes(envs, device=device, blip2=blip2, use_blip2=use_blip2, emulate_jpeg=on)
            for on in (False, True)}
    for s in sims.values():
        s.fast_forward(preroll)
        s.prepare(2 + rounds * steps)
        for _ in range(2):
            s.step()
    torch.cuda.synchronize(device)
    res = {False: [], True: []}
    for _ in range(rounds):
        for on in (False, True):
            s = sims[on]
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(steps):
                s.step()
            torch.cuda.synchronize(device)
            res[on].append((time.perf_counter() - t0) / steps)
    out = []
    for on in (False, True):
        ms = sorted(1000 * v for v in res[on])
        out.append({"what": "BatchedEpisodes.step", "envs": envs, "blip2": use_blip2, "emulate_jpeg": on, "steps": steps,
                    "rounds": rounds,
                    "ms_per_step": [round(v, 2) for v in ms], "median_ms": round(ms[len(ms) // 2], 2),
                    "env_steps_per_s": round(envs / (ms[len(ms) // 2] / 1000), 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--preroll", type=int, default=150)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--step", action="store_true", help="also time the BatchedEpisodes step, switch off and on")
    ap.add_argument("--no-blip2", action="store_true", help="--step with stub cosines instead of the BLIP-2 forward")
    ap.add_argument("--encode", action="store_true", help="time the encoder (and the host path it replaces) instead")
    ap.add_argument("--decode", action="store_true", help="time the decoder (and the host path it replaces) instead")
    args = ap.parse_args()
    import torch

    from vlfm_amd import _lib

    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    _lib.host_wait_blocking(device)   # (bench.py: before the device's first stream exists)
    torch.set_num_threads(1)
    if args.encode:
        encode_all(device, args.reps)
        return
    if args.decode:
        decode_all(device, args.reps)
        return
    for n, h, w in [(1, 480, 640), (8, 480, 640), (64, 480, 640), (256, 480, 640), (16, 720, 1280), (128, 720, 1280)]:
        print(json.dumps(roundtrip(device, n, h, w, args.reps)), flush=True)
    if args.step:
        for line in step_rate(device, args.envs, args.steps, args.rounds, args.preroll, not args.no_blip2):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
