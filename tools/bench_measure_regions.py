#!/usr/bin/env python3
"""What measuring class regions (unet_measure_class_regions, csrc/shapes.hip) costs next to labelling them
(unet_label_class_regions, csrc/segregions.hip) and describing them (unet_describe_class_regions, csrc/defects.hip) on
the same maps, at the size of a Gear image.

    rocprofv3 --kernel-trace --stats -- python tools/bench_measure_regions.py --case large
    rocprofv3 --kernel-trace --stats -- python tools/bench_measure_regions.py --case speckle
    rocprofv3 --kernel-trace --stats -- python tools/bench_measure_regions.py --case frame

One case per process, so that the per-kernel sums of a kernel trace belong to one input.  ``large``: a few dozen discs
and bars of three classes (long boundaries, every block inside one or two regions); ``speckle``: every pixel drawn with
p = 0.3 from three classes (hundreds of thousands of tiny regions: the per-lane fallback); ``frame``: one region of class
1 that fills the frame (every wave and block shares one record: the contention case).  Each of --runs rounds labels the
maps, describes them with the confidence and measures them with 32 directions, through the C entry points with all
buffers made beforehand; the script itself prints the median device time (torch.cuda.Event) of the three calls as one
JSON line.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tiaozhanbei_unet_amd import _lib as L  # noqa: E402
from tiaozhanbei_unet_amd.defects import direction_table  # noqa: E402


def make_maps(case, n, h, w, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    if case == "frame":
        return torch.ones((n, h, w), dtype=torch.uint8, device=dev)
    if case == "speckle":
        draw = torch.rand((n, h, w), generator=g, device=dev)
        return torch.where(draw < 0.3, (draw * 10).to(torch.uint8) + 1, torch.zeros((), dtype=torch.uint8, device=dev))
    maps = torch.zeros((n, h, w), dtype=torch.uint8, device=dev)
    yy = torch.arange(h, device=dev)[:, None]
    xx = torch.arange(w, device=dev)[None, :]
    host = torch.Generator().manual_seed(0)
    for k in range(36):                                # discs and slanted bars, later ones drawn over earlier ones
        cy, cx = (torch.rand(2, generator=host) * torch.tensor([h, w])).tolist()
        r = 20 + 100 * torch.rand((), generator=host).item()
        if k % 3:
            on = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        else:
            t = torch.rand((), generator=host).item() * math.pi
            along = (xx - cx) * math.cos(t) + (yy - cy) * math.sin(t)
            across = -(xx - cx) * math.sin(t) + (yy - cy) * math.cos(t)
            on = (along.abs() <= 4 * r) & (across.abs() <= 6)
        maps[:, on] = 1 + k % 3
    return maps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["large", "speckle", "frame"], required=True)
    ap.add_argument("--shape", type=int, nargs=3, default=[1, 1080, 1920])
    ap.add_argument("--directions", type=int, default=32)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, h, w = a.shape
    c, d = 4, a.directions
    maps = make_maps(a.case, n, h, w, dev)
    conf = torch.rand((n, h, w), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    lib, vp = L.lib(), ctypes.c_void_p
    region = torch.empty((n, h, w), dtype=torch.int32, device=dev)
    sizes = torch.empty_like(region)
    counts = torch.zeros((n, c), dtype=torch.int64, device=dev)
    count = torch.zeros(2, dtype=torch.int64, device=dev)
    ws_l = torch.empty(lib.unet_label_class_regions_workspace(n, h, w, c), dtype=torch.uint8, device=dev)
    ws_d = torch.empty(lib.unet_describe_class_regions_workspace(n, h, w, c), dtype=torch.uint8, device=dev)
    ws_m = torch.empty(lib.unet_measure_class_regions_workspace(n, h, w, d), dtype=torch.uint8, device=dev)
    table = direction_table(d)
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def label():
        counts.zero_()
        L.check(lib.unet_label_class_regions(vp(maps.data_ptr()), n, h, w, c, vp(region.data_ptr()), vp(sizes.data_ptr()),
                                             vp(counts.data_ptr()), vp(ws_l.data_ptr()), ws_l.numel(), stream), "label")

    label()
    cap = int(counts.sum())                            # as the Python wrappers size their buffers
    records = torch.empty((cap, 12), dtype=torch.int64, device=dev)
    shapes = torch.empty((cap, 11 + 2 * d), dtype=torch.int64, device=dev)

    def describe():
        count[:1].zero_()
        L.check(lib.unet_describe_class_regions(vp(maps.data_ptr()), vp(region.data_ptr()), vp(sizes.data_ptr()),
                                                vp(conf.data_ptr()), n, h, w, c, 1, 0, vp(records.data_ptr()), cap,
                                                vp(count.data_ptr()), vp(ws_d.data_ptr()), ws_d.numel(), stream), "describe")

    def measure():
        count[1:].zero_()
        L.check(lib.unet_measure_class_regions(vp(region.data_ptr()), vp(sizes.data_ptr()), n, h, w, 1, 0,
                                               vp(table.ctypes.data), d, vp(shapes.data_ptr()), cap,
                                               vp(count[1:].data_ptr()), vp(ws_m.data_ptr()), ws_m.numel(), stream), "measure")

    times = {"label": [], "describe": [], "measure": []}
    for r in range(a.warmup + a.runs):
        for name, fn in (("label", label), ("describe", describe), ("measure", measure)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    assert count.tolist() == [cap, cap], (count.tolist(), cap)
    print(json.dumps({"case": a.case, "shape": [n, h, w], "classes": c, "directions": d, "records": cap, "runs": a.runs,
                      **{f"{k}_us_median": round(statistics.median(v), 1) for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
