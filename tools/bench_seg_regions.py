#!/usr/bin/env python3
"""Defect-level region pass of eval_regions: ops.ClassRegionMatcher.update (label + match, csrc/segregions.hip) per batch,
next to what the same batch costs anyway: metrics.per_image_stats and the seg-UNet eval forward.

    python tools/bench_seg_regions.py [--cases 8x1024x512x3 8x512x512x4] [--runs 21] [--warmup 3] [--out FILE]

Per case (images x height x width x classes) and input -- ``sparse``: about 1 % defect pixels in a few discs per image,
the prediction the same discs moved by a few pixels; ``dense``: every pixel drawn uniformly from the classes, truth and
prediction independently (hundreds of thousands of tiny regions: the worst case) -- the median over --runs device times
(torch.cuda.Event around the calls, after --warmup calls of the same shape) of
  update      one ClassRegionMatcher.update (label both maps, count hits, emit records, queue the count copy),
  label       ops.label_class_regions on the stacked truth + prediction alone,
  stats       metrics.per_image_stats(logits, truth, labels=True) on logits whose argmax is the prediction,
  forward     SegmentationUNet(3, classes) eval forward of the batch in fp32 and bf16,
and the library's own per-kernel event times of one profiled update (ops.prof_kernels brackets whole entry points).
Prints one JSON line per case and input; --out appends them to a file.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tiaozhanbei_unet_amd import SegmentationUNet, ops  # noqa: E402
from tiaozhanbei_unet_amd.metrics import per_image_stats  # noqa: E402


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def sparse_maps(n, h, w, c, dev, seed):
    """about 1 % defect pixels in four discs per image; the prediction is the same discs moved by 3 pixels"""
    g = torch.Generator(device=dev).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    truth = torch.zeros((n, h, w), dtype=torch.uint8, device=dev)
    pred = torch.zeros_like(truth)
    radius = (0.01 * h * w / 4 / 3.14159) ** 0.5
    for k in range(4):
        cy = torch.rand((n,), generator=g, device=dev) * h
        cx = torch.rand((n,), generator=g, device=dev) * w
        cls = 1 + k % (c - 1)
        for out, shift in ((truth, 0.0), (pred, 3.0)):
            d2 = (yy[None] - cy[:, None, None] - shift) ** 2 + (xx[None] - cx[:, None, None] - shift) ** 2
            out[d2 < radius ** 2] = cls
    return truth, pred


def dense_maps(n, h, w, c, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return tuple(torch.randint(0, c, (n, h, w), generator=g, device=dev, dtype=torch.uint8) for _ in range(2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["8x1024x512x3", "8x512x512x4"])
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for case in a.cases:
        n, h, w, c = (int(v) for v in case.split("x"))
        forward = {}
        if not a.no_forward:
            x = torch.randn((n, 3, h, w), device=dev)
            for precision in ("fp32", "bf16"):
                model = SegmentationUNet(3, c, precision=precision).to(dev).eval()
                with torch.no_grad():
                    forward[precision] = timed(lambda: model(x), a.runs, a.warmup)[0]
                del model
        for kind, maps in (("sparse", sparse_maps), ("dense", dense_maps)):
            truth, pred = maps(n, h, w, c, dev, seed=h + w)
            logits = torch.nn.functional.one_hot(pred.long(), c).permute(0, 3, 1, 2).float().contiguous()
            target = truth.long()
            both = torch.cat([truth, pred])

            def update():
                m = ops.ClassRegionMatcher(c)
                m.update(pred, truth)
                return m

            upd = timed(update, a.runs, a.warmup)
            lab = timed(lambda: ops.label_class_regions(both, c), a.runs, a.warmup)
            st = timed(lambda: per_image_stats(logits, target, labels=True), a.runs, a.warmup)
            res = update().compute()
            ops.prof_enable(True)
            update()
            torch.cuda.synchronize()
            ops.prof_collect()
            brackets = ops.prof_kernels()          # each bracket spans its entry point's launches, named by the first
            kernels = {k: round(brackets[k]["ms"], 4) for k in ("label_class_tile", "count_class_hits") if k in brackets}
            ops.prof_enable(False)
            row = {"case": case, "input": kind, "pixels": n * h * w, "runs": a.runs, "warmup": a.warmup,
                   "defect_fraction": float((truth > 0).float().mean()),
                   "truth_regions": int(len(res["truth"])), "pred_regions": int(len(res["pred"])),
                   "update_ms": upd[0], "update_min_ms": upd[1], "update_max_ms": upd[2],
                   "label_ms": lab[0], "per_image_stats_ms": st[0],
                   "entry_point_ms": kernels, "forward_ms": forward}
            if forward:
                row["update_over_forward_fp32"] = upd[0] / forward["fp32"]
                row["update_over_forward_bf16"] = upd[0] / forward["bf16"]
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
