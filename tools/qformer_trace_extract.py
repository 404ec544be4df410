#!/usr/bin/env python
"""Per-launch durations of the Q-Former cross path's kernels from a rocprofv3 kernel trace written as CSV
(`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --steps 10 --warmup 5`):
the two library passes of the K/V projection (`...HSS_BH_Bias_S...`) or the pair GEMM that replaces them, and the attention launches
above `--long-us` (the six cross-attention calls of a step; the self-attention launches are ~12 us).  What
profiles/qformer_cross_path_ab.txt quotes.
    python tools/qformer_trace_extract.py DIR [--long-us 60] [--steps 15]"""
import argparse, csv, glob, os, statistics, sys

ap = argparse.ArgumentParser()
ap.add_argument("dir")
ap.add_argument("--long-us", type=float, default=60.0)
ap.add_argument("--steps", type=int, default=15, help="forwards in the run (warm-up + timed): per-step figures divide by it")
args = ap.parse_args()
files = glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True)
if not files:
    sys.exit(f"no *kernel_trace.csv under {args.dir}")
rows = []
for f in files:
    with open(f, newline="") as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3, r["Kernel_Name"]))
rows.sort()


def table(title, dur):
    if not dur:
        print(f"{title}: none"); return
    sd = statistics.pstdev(dur) if len(dur) > 1 else 0.0
    print(f"{title}: launches={len(dur)} ({len(dur) / args.steps:.1f} per step) mean={statistics.mean(dur):.1f} us "
          f"median={statistics.median(dur):.1f} min={min(dur):.1f} max={max(dur):.1f} sd={sd:.1f} total/step={sum(dur) / args.steps:.1f} us")


kv = [d for _, d, n in rows if "HSS_BH_Bias_S" in n]
table("K/V projection, library passes (HSS_BH_Bias_S)", kv)
if kv and len(kv) % 2 == 0:
    table("  pairs (second + first pass of one forward)", [kv[i] + kv[i + 1] for i in range(0, len(kv), 2)])
for tag in ("gemm_f16_8pp_kernel<3>", "gemm_f16_8pp_kernel<(int)3>"):
    table(f"K/V projection, pair GEMM ({tag})", [d for _, d, n in rows if tag in n])
att = [d for _, d, n in rows if "attn_fwd" in n]
table("attn_fwd, all launches", att)
long = [d for d in att if d >= args.long_us]
table(f"attn_fwd >= {args.long_us:.0f} us (cross-attention)", long)
if long and len(long) % 6 == 0:
    for l in range(6):
        table(f"  cross-attention layer {2 * l}", long[l::6])
table("qformer_cross_attention_kernel", [d for _, d, n in rows if "qformer_cross_attention" in n])
new = [d for _, d, n in rows if "qformer_cross_attention" in n]
if new and len(new) % 6 == 0:
    for l in range(6):
        table(f"  cross-attention layer {2 * l}", new[l::6])
