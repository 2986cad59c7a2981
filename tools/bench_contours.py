#!/usr/bin/env python3
"""What tracing the outlines of class regions (unet_count_class_region_edges + unet_trace_class_regions,
csrc/contours.hip) costs next to labelling them (unet_label_class_regions, csrc/segregions.hip), on the three 1080 x 1920
maps of tools/bench_measure_regions.py: ``frame`` (one region that fills the frame), ``large`` (a few dozen discs and
bars), ``speckle`` (about 400 000 tiny regions).

    python tools/bench_contours.py [--case frame large speckle]

Each of --runs rounds labels the maps, counts their edges and traces them, through the C entry points with all buffers
made beforehand (sized once from the counts, as the Python wrapper sizes them).  Prints one JSON line per case: the
counts, the doubling rounds, the launches of one trace and the median device time (torch.cuda.Event) of the three calls.
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


def bench(case, n, h, w, runs, warmup):
    dev = torch.device("cuda:0")
    c = 4
    maps = make_maps(case, n, h, w, dev)
    lib, vp = L.lib(), ctypes.c_void_p
    region = torch.empty((n, h, w), dtype=torch.int32, device=dev)
    sizes = torch.empty_like(region)
    class_counts = torch.zeros((n, c), dtype=torch.int64, device=dev)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    ws_l = torch.empty(lib.unet_label_class_regions_workspace(n, h, w, c), dtype=torch.uint8, device=dev)
    ws_c = torch.empty(lib.unet_count_class_region_edges_workspace(n, h, w), dtype=torch.uint8, device=dev)
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def label():
        class_counts.zero_()
        L.check(lib.unet_label_class_regions(vp(maps.data_ptr()), n, h, w, c, vp(region.data_ptr()), vp(sizes.data_ptr()),
                                             vp(class_counts.data_ptr()), vp(ws_l.data_ptr()), ws_l.numel(), stream), "label")

    def count():
        L.check(lib.unet_count_class_region_edges(vp(region.data_ptr()), vp(sizes.data_ptr()), n, h, w, 1,
                                                  vp(counts.data_ptr()), vp(ws_c.data_ptr()), ws_c.numel(), stream), "count")

    label()
    count()
    edges, n_loops, n_points = counts.tolist()
    loops = torch.empty((n_loops, 6), dtype=torch.int64, device=dev)
    points = torch.empty((n_points, 2), dtype=torch.int32, device=dev)
    ws_t = torch.empty(lib.unet_trace_class_regions_workspace(n, h, w, edges), dtype=torch.uint8, device=dev)

    def trace():
        L.check(lib.unet_trace_class_regions(vp(region.data_ptr()), vp(sizes.data_ptr()), n, h, w, 1, 0, edges,
                                             vp(loops.data_ptr()), n_loops, vp(points.data_ptr()), n_points,
                                             vp(counts.data_ptr()), vp(ws_t.data_ptr()), ws_t.numel(), stream), "trace")

    times = {"label": [], "count": [], "trace": []}
    for r in range(warmup + runs):
        for name, fn in (("label", label), ("count", count), ("trace", trace)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    assert counts.tolist() == [edges, n_loops, n_points]
    rounds = max(0, (edges - 1).bit_length())
    return {"case": case, "shape": [n, h, w], "regions": int(class_counts.sum()), "edges": edges, "loops": n_loops,
            "points": n_points, "longest_loop_points": int(loops[:, 3].max()), "rounds": rounds,
            "trace_launches": 6 + 1 + 2 * rounds + 2 + 6 + 2, "runs": runs,
            **{f"{k}_us_median": round(statistics.median(v), 1) for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs="+", choices=["frame", "large", "speckle"], default=["frame", "large", "speckle"])
    ap.add_argument("--shape", type=int, nargs=3, default=[1, 1080, 1920])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    for case in a.case:
        print(json.dumps(bench(case, *a.shape, a.runs, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
