#!/usr/bin/env python3
"""unet_tile_blend (csrc/tiles.hip) on a Gear-sized frame, beside the blend as torch operators compose it.

    python tools/bench_tile_blend.py [--runs 101] [--out profiles/tile_blend.json]

Workload: a 1080 x 1920 frame, 4 classes, 512 x 512 tiles overlapping by at least 64 (3 x 5 tiles), the default ramps.
The kernel: its mean time over --runs launches from the library's own event brackets (ops.prof_kernels) after warm-up
calls, the bytes it must move (the tile logits read once, labels and confidence written: the launcher's own accounting)
and bytes / time; and the median device time (torch.cuda.Event) of the whole tiling.blend_tiles call, which allocates
the outputs too.  The baseline, in the same process and alternating with it: the blend a user of the package would write
in torch -- per tile, slice-accumulate weight * logits and the weights, a division, then softmax(0).max(0) for labels and
confidence -- timed the same way (median device time of the whole composition).  The two label maps are compared and the
disagreeing pixels counted (the torch composition rounds differently; they are not expected to agree bit for bit).  No
threshold is asserted."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tiaozhanbei_unet_amd import ops, tiling  # noqa: E402


def device_us(fn, runs):
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def torch_blend(z, oy, ox, h, w, ramp_y, ramp_x):
    """the same blend from torch operators: weights as floats, accumulate by slices, divide, softmax"""
    t, c, th, tw = z.shape
    ky, kx = torch.arange(th, device=z.device), torch.arange(tw, device=z.device)
    qy = torch.minimum(torch.minimum(ky + 1, th - ky), torch.tensor(ramp_y, device=z.device)).float()
    qx = torch.minimum(torch.minimum(kx + 1, tw - kx), torch.tensor(ramp_x, device=z.device)).float()
    q = qy[:, None] * qx[None, :]
    acc = torch.zeros((c, h, w), device=z.device)
    wsum = torch.zeros((h, w), device=z.device)
    for i, y in enumerate(oy):
        for j, x in enumerate(ox):
            acc[:, y:y + th, x:x + tw] += q * z[i * len(ox) + j]
            wsum[y:y + th, x:x + tw] += q
    conf, labels = torch.softmax(acc / wsum, 0).max(0)
    return labels.to(torch.uint8), conf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=101)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tile_blend.py measures on an AMD GPU; none is visible")
    dev = torch.device("cuda:0")
    h, w, c = 1080, 1920, 4
    th, tw, oy, ox = tiling.plan_tiles((h, w), (512, 512), 64)
    ramp = (tiling.default_ramp(oy, th), tiling.default_ramp(ox, tw))
    g = torch.Generator(device=dev).manual_seed(0)
    z = torch.randn((len(oy) * len(ox), c, th, tw), generator=g, device=dev) * 4.0
    ours = lambda: tiling.blend_tiles(z, oy, ox, (h, w), ramp=ramp)              # noqa: E731
    theirs = lambda: torch_blend(z, oy, ox, h, w, *ramp)                         # noqa: E731
    for _ in range(5):
        a_out, b_out = ours(), theirs()
    torch.cuda.synchronize()
    differ = int((a_out[0] != b_out[0]).sum())
    conf_gap = float((a_out[1] - b_out[1]).abs().max())
    t_ours, t_theirs = [], []
    for _ in range(4):                                   # alternate the two in blocks
        t_ours += device_us(ours, a.runs // 4 + 1)
        t_theirs += device_us(theirs, a.runs // 4 + 1)
    ops.prof_enable(True)
    for _ in range(a.runs):
        ours()
    torch.cuda.synchronize()
    ops.prof_collect()
    k = ops.prof_kernels()["tile_blend"]
    ops.prof_enable(False)
    us = k["ms"] * 1e3 / k["launches"]
    per_launch = k["bytes"] / k["launches"]
    row = {"frame": [h, w], "classes": c, "tile": [th, tw], "origins_y": oy, "origins_x": ox, "ramp": list(ramp),
           "runs": a.runs, "kernel_us": us, "bytes_per_launch": per_launch, "bytes_per_s": per_launch / (us * 1e-6),
           "blend_tiles_call_us": {"median": statistics.median(t_ours), "min": min(t_ours), "max": max(t_ours)},
           "torch_composition_us": {"median": statistics.median(t_theirs), "min": min(t_theirs), "max": max(t_theirs)},
           "labels_that_differ": differ, "max_conf_gap": conf_gap}
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
