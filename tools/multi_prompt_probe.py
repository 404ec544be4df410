"""What a second prompt costs the batched step, three legs in ONE process that alternate window by window (so they share the
box and whatever else it is doing):
  (a) single prompt      BatchedEpisodes(E) as bench.py builds it: one BLIP-2 forward, one head, one value channel
  (b) two prompts (V3)   BatchedEpisodes(E, text_prompt="target|exploration", exploration_thresh=...): ONE forward, the
                         T-prompt head (vlfm_itc_head_multi), two value channels, [M, 2] frontier medians.  Like (a) it is
                         built without select_frontiers: the host-side frontier choice (_decide, V3's reduce rule) runs in
                         neither leg and is not part of what is timed
  (c) reference's shape  (a) plus a second cosine_batch forward on the same frames every step: what one ``cosine`` call per
                         prompt (itm_policy.py:193-202) costs here
at 256 and at 8 environments.  Every harness is pre-rolled by 150 map-only steps and warmed up at its own shapes; then
``--windows`` rounds of a, b, c, each window ``--steps`` steps timed wall-clock between two device synchronisations, the
window's depth frames rendered before its clock starts (as bench.py does).  Reported: every window, the medians, the spread
of (a) over its windows, (b)/(a) and (b)/(c).
    python tools/multi_prompt_probe.py [--windows 3] [--steps 100] [--envs 256 8] [--out profiles/multi_prompt_probe.txt]
    python tools/multi_prompt_probe.py --trace-steps 10 --envs 256     # a short (b)-only run for rocprofv3 --kernel-trace --stats"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

V3_PROMPT = "Seems like there is a target_object ahead.|There is a lot of area to explore ahead."
THRESH = 0.40
PREROLL = 150


def window(sim, n: int, after_step=None) -> float:
    """ms per step over n steps of ``sim`` (``after_step(sim)`` is part of the step when given)."""
    import torch

    sim.prepare(n)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        sim.step()
        if after_step is not None:
            after_step(sim)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sim.rooms.window = None          # (256 environments x 100 frames are 31 GB: one window resident at a time)
    return dt / n * 1e3


def probe(E: int, windows: int, steps: int, blip2, lines) -> None:
    import numpy as np
    import torch

    from vlfm_amd.harness import BatchedEpisodes

    dev = blip2.device
    a = BatchedEpisodes(E, device=dev, blip2=blip2)
    b = BatchedEpisodes(E, device=dev, blip2=blip2, text_prompt=V3_PROMPT, exploration_thresh=THRESH)
    c = BatchedEpisodes(E, device=dev, blip2=blip2)
    second = [p[1] for p in b.prompts]

    def second_forward(sim):
        rgb = sim.rgb_pool[(sim.t - 1) % sim.rgb_pool.shape[0]]
        sim.second = blip2.cosine_batch_graphed(rgb, second) if sim.graph_blip2 else blip2.cosine_batch(rgb, second)

    legs = (("a", a, None), ("b", b, None), ("c", c, second_forward))
    for _, sim, after in legs:
        sim.fast_forward(PREROLL)
        for _ in range(5):
            sim.step()
            if after is not None:
                after(sim)
    torch.cuda.synchronize()
    assert PREROLL + 5 + windows * steps <= a.episode_len, "the windows must fit into one episode"
    ms = {name: [] for name, _, _ in legs}
    for w in range(windows):
        for name, sim, after in legs:
            ms[name].append(window(sim, steps, after))
            lines.append("E=%3d window %d leg (%s) %9.3f ms/step  %8.1f env-steps/s" % (E, w, name, ms[name][-1], E / ms[name][-1] * 1e3))
            print(lines[-1], flush=True)
    for _, sim, _ in legs:
        sim.check()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = (max(ms["a"]) - min(ms["a"])) / med["a"]
    lines.append("E=%3d medians: (a) %.3f  (b) %.3f  (c) %.3f ms/step   spread of (a) over its %d windows: %.2f %% (%.3f .. %.3f)   "
                 "(b)/(a) = %.4f   (b)/(c) = %.4f" % (E, med["a"], med["b"], med["c"], windows, 100 * spread, min(ms["a"]),
                                                     max(ms["a"]), med["b"] / med["a"], med["b"] / med["c"]))
    print(lines[-1], flush=True)
    del a, b, c
    torch.cuda.empty_cache()


def trace_run(E: int, steps: int, blip2) -> None:
    """A short two-prompt run and nothing else: the process rocprofv3 --kernel-trace --stats is pointed at."""
    import torch

    from vlfm_amd.harness import BatchedEpisodes

    sim = BatchedEpisodes(E, device=blip2.device, blip2=blip2, text_prompt=V3_PROMPT, exploration_thresh=THRESH)
    sim.fast_forward(PREROLL)
    sim.prepare(steps)
    for _ in range(steps):
        sim.step()
    torch.cuda.synchronize()
    sim.check()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--envs", type=int, nargs="*", default=[256, 8])
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-steps", type=int, default=0)
    args = ap.parse_args()
    import torch

    from vlfm_amd import _lib
    from vlfm_amd.vlm.blip2itm import BLIP2ITM

    assert torch.cuda.is_available(), "multi_prompt_probe measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    _lib.host_wait_blocking(dev)
    torch.set_num_threads(1)
    blip2 = BLIP2ITM(device=dev, allow_random_init=True)
    blip2.strict_hip_attention = True
    if args.trace_steps:
        trace_run(args.envs[0], args.trace_steps, blip2)
        return
    lines = ["multi_prompt_probe: wall-clock ms/step of %d-step windows between device synchronisations, %d rounds of (a) single "
             "prompt, (b) two prompts through one forward, (c) single prompt + a second cosine_batch forward; %d map-only "
             "pre-roll steps, 5 warm-up steps per leg; device %s" % (args.steps, args.windows, PREROLL, torch.cuda.get_device_name(0))]
    for E in args.envs:
        probe(E, args.windows, args.steps, blip2, lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
