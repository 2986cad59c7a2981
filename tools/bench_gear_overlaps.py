#!/usr/bin/env python3
"""The Gear class-overlap analysis: augment.polygon_class_histogram on the device against the host route of the
reference's analyze_class_overlaps.py (per polygon a full-resolution Pillow drawing with its numpy <-> PIL conversions,
OR per class, then ``&`` and ``np.sum`` over full frames for every class pair), on a synthetic set of 1920 x 1080 files
with LabelMe-like polygons of 10..200 vertices.

    python tools/bench_gear_overlaps.py [--files 32] [--polygons 10] [--runs 11] [--host-runs 3] [--out profiles/gear_overlaps_bench.txt]

Reported: the median over --runs of the device time (torch.cuda.Event) of one polygon_class_histogram call over all
files (host checks and the small host-to-device copies included, after two warm-up calls), the median wall time of the
call followed by the copy of the [N, 8] histogram to the host and ``overlap_stats``, and the median over --host-runs of
the host route's wall time.  Parsing is not timed on either side (both parse the same text the same way).  The run also
checks that the two routes report the same pixel counts."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image, ImageDraw

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tiaozhanbei_unet_amd import augment as A  # noqa: E402
from tiaozhanbei_unet_amd import gear_dataset as G  # noqa: E402
from tiaozhanbei_unet_amd import gear_overlaps as GO  # noqa: E402

W, H = 1920, 1080


def make_files(n_files, n_polys, seed=0):
    rng = np.random.default_rng(seed)
    files = []
    for _ in range(n_files):
        polys = []
        for k in range(n_polys):
            nv = int(rng.integers(10, 201))
            cx, cy, r = rng.uniform(100, W - 100), rng.uniform(80, H - 80), rng.uniform(60, 320)
            ang = np.sort(rng.uniform(0, 2 * np.pi, nv))
            rr = r * rng.uniform(0.55, 1.0, nv)
            polys.append((k % 3, [(int(cx + a * np.cos(t)), int(cy + a * np.sin(t))) for a, t in zip(rr, ang)]))
        files.append(polys)
    return files


def host_route(files):
    """Per file: class masks by Pillow as the reference builds them, totals and pairwise overlaps over full frames."""
    out = []
    for polys in files:
        masks = {}
        for cls, pts in polys:
            if cls not in masks:
                masks[cls] = np.zeros((H, W), dtype=bool)
            img = Image.fromarray(masks[cls].astype(np.uint8))
            ImageDraw.Draw(img).polygon(pts, fill=1)
            masks[cls] = np.array(img).astype(bool)
        ids = list(masks)
        totals = {c: int(np.sum(m)) for c, m in masks.items()}
        pairs = {(a, b): int(np.sum(masks[a] & masks[b])) for i, a in enumerate(ids) for b in ids[i + 1:]}
        out.append((totals, pairs))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--polygons", type=int, default=10)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gear_overlaps.py measures on an AMD GPU; none is visible")
    dev = torch.device("cuda:0")
    files = make_files(a.files, a.polygons)
    flat, sizes = G.flatten_polygons(files), [(H, W)] * len(files)
    for _ in range(2):
        hist = A.polygon_class_histogram(flat, sizes, device=dev)
    torch.cuda.synchronize()
    dev_ms, wall_ms = [], []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        A.polygon_class_histogram(flat, sizes, device=dev)
        e1.record()
        e1.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    for _ in range(a.runs):
        t0 = time.perf_counter()
        rows = A.polygon_class_histogram(flat, sizes, device=dev).cpu().tolist()
        stats = GO.overlap_stats([("bench", f"{i}.png", GO.first_appearance(p), r) for i, (p, r) in enumerate(zip(files, rows))])
        wall_ms.append((time.perf_counter() - t0) * 1e3)
    host_ms = []
    for _ in range(a.host_runs):
        t0 = time.perf_counter()
        host = host_route(files)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    same = all(tot == {c: GO.class_pixels(r, c) for c in tot} and pr == {k: GO.pair_pixels(r, *k) for k in pr}
               for (tot, pr), r in zip(host, hist.cpu().tolist()))
    d, w, h = statistics.median(dev_ms), statistics.median(wall_ms), statistics.median(host_ms)
    lines = [f"gear class-overlap analysis, {a.files} files of {W} x {H}, {a.polygons} polygons of 10..200 vertices each "
             f"({len(flat['verts'])} vertices), {torch.cuda.get_device_name(0)}",
             f"device: polygon_class_histogram call, one launch over all files  {d:10.3f} ms  (median of {a.runs}, "
             f"min {min(dev_ms):.3f}, max {max(dev_ms):.3f}; device events)",
             f"device: call + histogram to host + overlap_stats                 {w:10.3f} ms  (median of {a.runs}, wall)",
             f"host:   Pillow drawings + full-frame mask algebra                {h:10.3f} ms  (median of {a.host_runs}, "
             f"min {min(host_ms):.1f}, max {max(host_ms):.1f}; wall)",
             f"ratio host / device (wall): {h / w:.1f}",
             f"files with overlaps {stats['summary']['files_with_any_overlap']} / {stats['summary']['total_files_processed']}; "
             f"pixel counts equal on both routes: {same}"]
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
