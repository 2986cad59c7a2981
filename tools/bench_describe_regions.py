#!/usr/bin/env python3
"""What describing class regions (unet_describe_class_regions, csrc/defects.hip) costs next to labelling them
(unet_label_class_regions, csrc/segregions.hip) on the same maps.

    rocprofv3 --kernel-trace --stats -- python tools/bench_describe_regions.py --case blob
    rocprofv3 --kernel-trace --stats -- python tools/bench_describe_regions.py --case speckle

One case per process, so that the per-kernel sums of a kernel trace belong to one input.  ``blob``: every image one
region of class 1 that fills the frame (every wave and block shares one record: the contention case); ``speckle``: every
pixel drawn with p = 0.3 from three classes (tens of thousands of tiny regions: the per-lane fallback).  Each of --runs
rounds labels the maps and describes them with the confidence, through the C entry points with all buffers made
beforehand; the script itself prints the median device time (torch.cuda.Event) of both calls as one JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tiaozhanbei_unet_amd import _lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["blob", "speckle"], required=True)
    ap.add_argument("--shape", type=int, nargs=3, default=[8, 512, 512])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, h, w = a.shape
    c = 4
    g = torch.Generator(device=dev).manual_seed(0)
    if a.case == "blob":
        maps = torch.ones((n, h, w), dtype=torch.uint8, device=dev)
    else:
        draw = torch.rand((n, h, w), generator=g, device=dev)
        maps = torch.where(draw < 0.3, (draw * 10).to(torch.uint8) + 1, torch.zeros((), dtype=torch.uint8, device=dev))
    conf = torch.rand((n, h, w), generator=g, device=dev)
    lib, vp, px = L.lib(), ctypes.c_void_p, n * h * w
    region = torch.empty((n, h, w), dtype=torch.int32, device=dev)
    sizes = torch.empty_like(region)
    counts = torch.zeros((n, c), dtype=torch.int64, device=dev)
    records = torch.empty((px, 12), dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    ws_l = torch.empty(lib.unet_label_class_regions_workspace(n, h, w, c), dtype=torch.uint8, device=dev)
    ws_d = torch.empty(lib.unet_describe_class_regions_workspace(n, h, w, c), dtype=torch.uint8, device=dev)
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def label():
        counts.zero_()
        L.check(lib.unet_label_class_regions(vp(maps.data_ptr()), n, h, w, c, vp(region.data_ptr()), vp(sizes.data_ptr()),
                                             vp(counts.data_ptr()), vp(ws_l.data_ptr()), ws_l.numel(), stream), "label")

    def describe():
        count.zero_()
        L.check(lib.unet_describe_class_regions(vp(maps.data_ptr()), vp(region.data_ptr()), vp(sizes.data_ptr()),
                                                vp(conf.data_ptr()), n, h, w, c, 1, 0, vp(records.data_ptr()), px,
                                                vp(count.data_ptr()), vp(ws_d.data_ptr()), ws_d.numel(), stream), "describe")

    times = {"label": [], "describe": []}
    for r in range(a.warmup + a.runs):
        for name, fn in (("label", label), ("describe", describe)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    print(json.dumps({"case": a.case, "shape": [n, h, w], "classes": c, "records": int(count.item()), "runs": a.runs,
                      "label_us_median": round(statistics.median(times["label"]), 1),
                      "describe_us_median": round(statistics.median(times["describe"]), 1)}), flush=True)


if __name__ == "__main__":
    main()
