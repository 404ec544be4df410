#!/usr/bin/env python
"""The two halves of the Q-Former's fused cross path, standalone, against what they replace (random data, median of interleaved
rounds, HIP events around `--inner` back-to-back launches):
  * the K/V projection: ops.linear_pair_f32 (ONE pass of csrc/gemm_f16.hip, block-major f32) against blip2itm._split_gemm with two
    pieces (two f32-output library GEMMs, the second accumulating in place), [images * 257 x 1408] . [1408 x 9216];
  * one layer's cross-attention: ops.qformer_cross_attention on the block-major tensor against F.scaled_dot_product_attention on
    the strided K / V views of the row-major tensor (what the model ran), 32 queries, 12 heads of 64.
    python tools/qformer_cross_probe.py [--images 32,64,128,256] [--rounds 7] [--inner 5] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vlfm_amd.vlm import blip2itm, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--images", default="32,64,128,256")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
T, KD, HID, HEADS, LAYERS, Q = 257, 1408, 768, 12, 6, 32
N = LAYERS * 2 * HID
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / args.inner


g = torch.Generator().manual_seed(0)
w = (torch.randn(N, KD, generator=g) * 0.05).to(dev)
bias = torch.randn(N, generator=g).to(dev)
w1, w2, w3 = blip2itm._exact_split3(w)
pieces = (w1.t(), w2.t(), w3.t())
w_pair = ops.interleave_pair_weights(w1, w2)
say(f"{torch.cuda.get_device_name(0)}; us per call, median of {args.rounds} interleaved rounds of {args.inner} launches")
say("images | K/V projection: two library passes | pair GEMM | ratio || cross-attention (one layer): SDPA | kernel | ratio")
for images in [int(v) for v in args.images.split(",")]:
    M = images * T
    x16 = torch.randn(M, KD, generator=g).half().to(dev)
    q = torch.randn(images, Q, HID, generator=g).to(dev)
    rows = blip2itm._split_gemm(x16, pieces, bias, n_pieces=2)               # [M, N] row-major
    blocks = ops.linear_pair_f32(x16, w_pair, bias)                          # [N / 64, M, 64]
    k = rows.view(images, T, N)[..., :HID].unflatten(-1, (HEADS, 64)).transpose(1, 2)          # strided views, as in the model
    v = rows.view(images, T, N)[..., HID:2 * HID].unflatten(-1, (HEADS, 64)).transpose(1, 2)
    qh = q.view(images, Q, HEADS, 64).transpose(1, 2)
    forms = {
        "lib": lambda: blip2itm._split_gemm(x16, pieces, bias, n_pieces=2),
        "pair": lambda: ops.linear_pair_f32(x16, w_pair, bias, out=blocks),
        "sdpa": lambda: F.scaled_dot_product_attention(qh, k, v),
        "kern": lambda: ops.qformer_cross_attention(q, blocks, T, HEADS, 0, HEADS, 0.125),
    }
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    t = {n: [] for n in forms}
    for _ in range(args.rounds):
        for n, fn in forms.items():
            t[n].append(timed(fn))
    med = {n: statistics.median(v_) for n, v_ in t.items()}
    say(f"{images:6d} | {med['lib']:9.1f} | {med['pair']:9.1f} | {med['pair'] / med['lib']:.3f} || {med['sdpa']:8.1f} | {med['kern']:8.1f} | "
        f"{med['kern'] / med['sdpa']:.3f}    (spread lib {min(t['lib']):.0f}-{max(t['lib']):.0f}, pair {min(t['pair']):.0f}-{max(t['pair']):.0f}, "
        f"sdpa {min(t['sdpa']):.0f}-{max(t['sdpa']):.0f}, kernel {min(t['kern']):.0f}-{max(t['kern']):.0f})")
    del x16, rows, blocks, k, v
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
