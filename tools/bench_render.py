#!/usr/bin/env python3
"""The visualisation sheet of the evaluation CLI: ops.render_sheet on the device against the host route of the reference
(copy the tensors to the host, then numpy's denormalise / clamp and matplotlib's Normalize + colormap calls, tiled with
numpy; no figure is drawn, so the host route is what its arithmetic alone costs).

    python tools/bench_render.py [--sizes 256 1024] [--images 20] [--runs 21] [--out profiles/render_bench.json]

Per size: the median over --runs of the device time (torch.cuda.Event) of one render_sheet call (both launches) after
two warm-up calls, the per-kernel times of the library's own event brackets (ops.prof_kernels), the sheet pass as a
fraction of the rate of a device-to-device copy of the same number of bytes (read + written), the device-to-host copy the
host route needs and the host route's time.  K = 4: image | gray | hot | unit.  With --profile-only it renders a few
times and exits (for `rocprofv3 --kernel-trace --stats -- python tools/bench_render.py --profile-only`)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tiaozhanbei_unet_amd import ops  # noqa: E402


def inputs(n, size, dev):
    g = torch.Generator(device=dev).manual_seed(size)
    shape3, shape1 = (n, 3, size, size), (n, 1, size, size)
    return [("image", torch.randn(shape3, generator=g, device=dev) * 1.5),
            ("gray", (torch.rand(shape1, generator=g, device=dev) < 0.05).float()),
            ("hot", torch.sigmoid(torch.randn(shape1, generator=g, device=dev) * 2.0 - 3.0)),
            ("unit", torch.rand(shape3, generator=g, device=dev))]


def device_ms(fn, runs):
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def host_route(cols, gutter):
    """What the reference's visualize_results computes per panel, without drawing a figure."""
    from matplotlib import colormaps
    from matplotlib.colors import Normalize
    t0 = time.perf_counter()
    host = [(k, t.cpu().numpy()) for k, t in cols]
    t1 = time.perf_counter()
    mean, std = np.float32(ops.IMAGENET_MEAN).reshape(3, 1, 1), np.float32(ops.IMAGENET_STD).reshape(3, 1, 1)
    n, _, h, w = host[0][1].shape
    sheet = np.full((n * h + (n - 1) * gutter, len(host) * w + (len(host) - 1) * gutter, 3), 255, np.uint8)
    for i in range(n):
        for j, (kind, a) in enumerate(host):
            if kind in ("image", "unit"):
                v = a[i] * std + mean if kind == "image" else a[i]
                p = (np.clip(v, 0, 1).transpose(1, 2, 0) * 255).astype(np.uint8)
            else:
                p = colormaps[kind](Normalize()(a[i, 0].astype(np.float64)), bytes=True)[..., :3]
            sheet[i * (h + gutter):i * (h + gutter) + h, j * (w + gutter):j * (w + gutter) + w] = p
    return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, sheet


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--gutter", type=int, default=4)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py measures on an AMD GPU; none is visible")
    dev = torch.device("cuda:0")
    rows = []
    for size in a.sizes:
        cols = inputs(a.images, size, dev)
        for _ in range(2):
            sheet = ops.render_sheet(cols, gutter=a.gutter)
        torch.cuda.synchronize()
        if a.profile_only:
            for _ in range(5):
                ops.render_sheet(cols, gutter=a.gutter)
            torch.cuda.synchronize()
            continue
        total = device_ms(lambda: ops.render_sheet(cols, gutter=a.gutter), a.runs)
        ops.prof_enable(True)
        for _ in range(a.runs):
            ops.render_sheet(cols, gutter=a.gutter)
        torch.cuda.synchronize()
        ops.prof_collect()
        kern = {k: v["ms"] / max(v["launches"], 1) for k, v in ops.prof_kernels().items() if k.startswith("render_")}
        ops.prof_enable(False)
        in_bytes = sum(t.numel() * 4 for _, t in cols)
        moved = in_bytes + sheet.numel()                      # bytes the sheet pass reads and writes, each once
        src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        dst.copy_(src)
        copy_ms = device_ms(lambda: dst.copy_(src), a.runs)   # reads moved / 2, writes moved / 2
        d2h, host, want = host_route(cols, a.gutter)
        row = {"images": a.images, "size": size, "panels": len(cols), "gutter": a.gutter, "runs": a.runs,
               "sheet_shape": list(sheet.shape), "render_sheet_call_ms": total,
               "range_kernel_ms": kern.get("render_range"), "sheet_kernel_ms": kern.get("render_sheet"),
               "sheet_pass_bytes": moved, "copy_same_bytes_ms": copy_ms,
               "sheet_pass_fraction_of_copy_rate": copy_ms / kern["render_sheet"] if kern.get("render_sheet") else None,
               "host_d2h_copy_ms": d2h, "host_numpy_matplotlib_ms": host,
               "bytes_equal_host_route": bool(np.array_equal(sheet.cpu().numpy(), want))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out and rows:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
