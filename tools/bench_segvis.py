#!/usr/bin/env python3
"""The kernels of the Gear / KolektorSDD visualisers (csrc/segvis.hip) on the device, beside unet_render_sheet
(csrc/render.hip) writing a sheet of the same byte count on the same box.

    python tools/bench_segvis.py [--runs 51] [--out profiles/segvis_bench.json]

Cases: unet_seg_confidence at 8 x 4 x 512 x 512 (Gear) and 4 x 2 x 1024 x 512 (labels and confidence both written);
unet_seg_render_sheet for the 2 x 5 Gear grid at 512 x 512 (10 samples, two overlay panels each, per_row 5, gutter 4);
unet_render_sheet for 2 rows of 5 image panels at 512 x 1028, gutter 4 (it takes at most 8 panels a row): the same
1028 x 5156 sheet.  Per case: the
kernel's mean time over --runs launches from the library's own event brackets (ops.prof_kernels) after two warm-up
calls, the algorithmic bytes of one launch (inputs and outputs, each once: the kernels' own accounting) and bytes / time;
and the median device time (torch.cuda.Event) of the whole ops call, which holds the host-side conversions too.  No
threshold is asserted.  With --profile-only it runs each case a few times and exits (for rocprofv3 --kernel-trace)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tiaozhanbei_unet_amd import ops  # noqa: E402


def device_us(fn, runs):
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


def kernel_stats(fn, runs, name):
    ops.prof_enable(True)
    for _ in range(runs):
        fn()
    torch.cuda.synchronize()
    ops.prof_collect()
    k = ops.prof_kernels()[name]
    ops.prof_enable(False)
    us = k["ms"] * 1e3 / k["launches"]
    per_launch = k["bytes"] / k["launches"]
    return {"kernel": name, "launches": k["launches"], "kernel_us": us, "bytes_per_launch": per_launch,
            "bytes_per_s": per_launch / (us * 1e-6)}


def cases(dev):
    g = torch.Generator(device=dev).manual_seed(0)
    out = []
    for n, c, h, w in ((8, 4, 512, 512), (4, 2, 1024, 512)):
        z = torch.randn((n, c, h, w), generator=g, device=dev) * 4.0
        out.append((f"seg_confidence {n}x{c}x{h}x{w}", "seg_confidence", lambda z=z: ops.seg_confidence(z)))
    n, c, size = 10, 4, 512
    x = torch.randn((n, 3, size, size), generator=g, device=dev) * 1.5
    truth = torch.randint(0, c, (n, size, size), generator=g, device=dev, dtype=torch.uint8)
    pred = torch.randint(0, c, (n, size, size), generator=g, device=dev, dtype=torch.uint8)
    palette = ops.class_palette(c, "index").to(dev)
    out.append(("seg_render_sheet 2x5 Gear grid 512x512", "seg_render_sheet",
                lambda: ops.render_seg_sheet(x, [("overlay", truth, 0.4), ("overlay", pred, 0.4)], gutter=4, per_row=5,
                                             palette=palette)))
    two = torch.randn((2, 3, size, 2 * size + 4), generator=g, device=dev) * 1.5      # 5 x 1028 + 4 x 4 = 5156 columns
    out.append(("render_sheet 2 rows x 5 image panels 512x1028", "render_sheet",
                lambda: ops.render_sheet([("image", two)] * 5, gutter=4)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=51)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_segvis.py measures on an AMD GPU; none is visible")
    dev = torch.device("cuda:0")
    rows = []
    for label, kernel, fn in cases(dev):
        for _ in range(2):
            res = fn()
        torch.cuda.synchronize()
        if a.profile_only:
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            continue
        row = {"case": label, "runs": a.runs, "call_us_median": device_us(fn, a.runs), **kernel_stats(fn, a.runs, kernel)}
        if torch.is_tensor(res):
            row["sheet_shape"] = list(res.shape)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out and rows:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
