#!/usr/bin/env python3
"""What grouping class regions (unet_group_class_regions, csrc/groups.hip) costs next to labelling them
(unet_label_class_regions, csrc/segregions.hip) on the same maps, at the size of a Gear image and at the gaps 2, 8 and 32.

    python tools/bench_group_regions.py --case large
    python tools/bench_group_regions.py --case speckle
    python tools/bench_group_regions.py --case frame
    rocprofv3 --kernel-trace --stats -- python tools/bench_group_regions.py --case speckle --gaps 32

One case per process.  The maps are tools/bench_measure_regions.py's: ``large``: a few dozen discs and bars of three
classes (long outlines, few fragments); ``speckle``: every pixel drawn with p = 0.3 from three classes (hundreds of
thousands of fragments, every one of them all edge, and nearly every scan finds a neighbour: the worst case of the link
pass); ``frame``: one region that fills the frame (no edge pixel but the frame's own border, which has no 4-neighbour
outside its region inside the frame: nothing is scanned).  Each of --runs rounds labels the maps and groups them at
every gap, through the C entry points with all buffers made beforehand; the script prints the median, minimum and
maximum device time (torch.cuda.Event) of every call as one JSON line, with the number of fragments and groups.
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
from tools.bench_measure_regions import make_maps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["large", "speckle", "frame"], required=True)
    ap.add_argument("--shape", type=int, nargs=3, default=[1, 1080, 1920])
    ap.add_argument("--gaps", type=int, nargs="+", default=[2, 8, 32])
    ap.add_argument("--min_pixels", type=int, default=1)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, h, w = a.shape
    c = 4
    maps = make_maps(a.case, n, h, w, dev)
    lib, vp = L.lib(), ctypes.c_void_p
    region = torch.empty((n, h, w), dtype=torch.int32, device=dev)
    sizes, group, group_sizes = (torch.empty_like(region) for _ in range(3))
    counts = torch.zeros((2, n, c), dtype=torch.int64, device=dev)         # regions, groups
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    ws_l = torch.empty(lib.unet_label_class_regions_workspace(n, h, w, c), dtype=torch.uint8, device=dev)
    ws_g = torch.empty(lib.unet_group_class_regions_workspace(n, h, w, c), dtype=torch.uint8, device=dev)
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def label():
        counts[0].zero_()
        L.check(lib.unet_label_class_regions(vp(maps.data_ptr()), n, h, w, c, vp(region.data_ptr()), vp(sizes.data_ptr()),
                                             vp(counts[0].data_ptr()), vp(ws_l.data_ptr()), ws_l.numel(), stream), "label")

    label()
    cap = int(counts[0].sum())                         # as the Python wrappers size their buffers
    fragments = torch.empty((cap, 5), dtype=torch.int64, device=dev)

    def grouper(gap):
        def run():
            counts[1].zero_()
            count.zero_()
            L.check(lib.unet_group_class_regions(vp(maps.data_ptr()), vp(region.data_ptr()), vp(sizes.data_ptr()), n, h, w,
                                                 c, gap, a.min_pixels, 0, vp(group.data_ptr()), vp(group_sizes.data_ptr()),
                                                 vp(counts[1].data_ptr()), vp(fragments.data_ptr()), cap,
                                                 vp(count.data_ptr()), vp(ws_g.data_ptr()), ws_g.numel(), stream), "group")
        return run

    calls = [("label", label)] + [(f"group_gap{g}", grouper(g)) for g in a.gaps]
    times = {name: [] for name, _ in calls}
    found = {}
    for r in range(a.warmup + a.runs):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
            if name != "label":
                found[name] = {"fragments": int(count), "groups": int(counts[1].sum())}
    out = {"case": a.case, "shape": [n, h, w], "classes": c, "min_pixels": a.min_pixels, "regions": cap, "runs": a.runs}
    for name, v in times.items():
        out[name] = {"us_median": round(statistics.median(v), 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                     **found.get(name, {})}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
