"""Steps a small BatchedEpisodes harness (no BLIP-2: stub cosines) and records its maps: one raw Motion-JPEG file per
environment and map, every frame encoded on the device (BatchedEpisodes.render_jpeg).  Play one with
`ffplay -f mjpeg out/env0_value_map.mjpeg`.  `--first-person` steps a closed-loop harness that renders the robots' RGB view of the
world (BatchedEpisodes(closed_loop=True, render_rgb=True)) and writes one more file per environment, env<e>_first_person.mjpeg:
what the robot saw (live.rgb), through the same encoder.
Usage: python tools/record_episodes.py [--envs 4] [--steps 50] [--every 1] [--quality 90] [--out recordings] [--first-person]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--every", type=int, default=1, help="record every n-th step")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--out", default="recordings")
    ap.add_argument("--first-person", action="store_true", help="closed loop; also record what each robot saw")
    args = ap.parse_args()
    import torch

    from vlfm_amd.harness import BatchedEpisodes
    from vlfm_amd.utils.mjpeg import MjpegWriter
    from vlfm_amd.vlm.transport import jpeg_encode_batch_bytes

    device = torch.device("cuda:0")
    os.makedirs(args.out, exist_ok=True)
    first_person = dict(closed_loop=True, select_frontiers=True, render_rgb=True) if args.first_person else {}
    sim = BatchedEpisodes(args.envs, device=device, use_blip2=False, world="rooms", render_trajectories=True, **first_person)
    writers = {}
    try:
        for t in range(args.steps):
            sim.step()
            if t % args.every:
                continue
            frames = sim.render_jpeg(quality=args.quality)
            if args.first_person:
                frames["first_person"] = jpeg_encode_batch_bytes(sim.live.rgb, args.quality, "rgb")
            for name, files in frames.items():
                for e, data in enumerate(files):
                    key = (e, name)
                    if key not in writers:
                        writers[key] = MjpegWriter(os.path.join(args.out, f"env{e}_{name}.mjpeg"))
                    writers[key].append(data)
    finally:
        for w in writers.values():
            w.close()
    total = sum(os.path.getsize(w.path) for w in writers.values())
    print(f"{len(writers)} files, {sum(w.frames for w in writers.values())} frames, {total} bytes in {args.out}")


if __name__ == "__main__":
    main()
