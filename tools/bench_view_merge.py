#!/usr/bin/env python3
"""unet_view_merge (csrc/views.hip) on a Gear-sized frame, beside the merge as torch operators compose it.

    python tools/bench_view_merge.py [--runs 101] [--out profiles/view_merge.txt]

Workload: a 1080 x 1920 frame, 4 classes, the six views of scales {0.75, 1, 1.5} x flips {none, x}: logits of 810 x 1440,
1080 x 1920 and 1620 x 2880, N(0, 4^2).  The kernel: its mean time over --runs launches from the library's own event
brackets (ops.prof_kernels) after warm-up calls, the bytes it must move (every view logit read once; merged, labels,
confidence and agreement written: the launcher's own accounting) and bytes / time; and the median device time
(torch.cuda.Event) of the whole views.merge_views call, which allocates the outputs too.  The baseline, in the same
process and alternating with it: the merge a user of the package would write in torch -- per view torch.flip where it is
mirrored, F.interpolate(mode="bilinear", align_corners=False) where its size differs, an add; then a division -- timed
the same way, once for the merged logits alone and once with softmax(0).max(0) for labels and confidence and the
per-view argmax comparisons for the agreement, which the kernel writes in the same launch.  The label maps are compared
and the disagreeing pixels counted (the composition samples in floating point and rounds differently; the two are not
expected to agree bit for bit).  No threshold is asserted; the report says what one run showed."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tiaozhanbei_unet_amd import ops, predict_tiled, views  # noqa: E402


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


def torch_views(zs, flips, h, w):
    """every view on the frame, mirrored back: flip, then interpolate"""
    out = []
    for z, (fx, fy) in zip(zs, flips):
        dims = [d for d, on in ((2, fx), (1, fy)) if on]
        if dims:
            z = torch.flip(z, dims)
        if tuple(z.shape[1:]) != (h, w):
            z = F.interpolate(z[None], size=(h, w), mode="bilinear", align_corners=False)[0]
        out.append(z)
    return out


def torch_merge(zs, flips, h, w):
    vals = torch_views(zs, flips, h, w)
    acc = vals[0]
    for v in vals[1:]:
        acc = acc + v
    return acc / float(len(vals))


def torch_merge_all(zs, flips, h, w):
    vals = torch_views(zs, flips, h, w)
    acc = vals[0]
    for v in vals[1:]:
        acc = acc + v
    merged = acc / float(len(vals))
    conf, labels = torch.softmax(merged, 0).max(0)
    agreement = torch.zeros((h, w), dtype=torch.uint8, device=merged.device)
    for v in vals:
        agreement += (v.argmax(0) == labels).to(torch.uint8)
    return labels.to(torch.uint8), conf, agreement, merged


def spread(t):
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=101)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_view_merge.py measures on an AMD GPU; none is visible")
    dev = torch.device("cuda:0")
    h, w, c = 1080, 1920, 4
    plan = views.plan_views([0.75, 1.0, 1.5], "h")
    flips = [(fx, fy) for _s, fx, fy in plan]
    sizes = [predict_tiled.working_frame((h, w), s) for s, _fx, _fy in plan]
    g = torch.Generator(device=dev).manual_seed(0)
    zs = [torch.randn((c, hv, wv), generator=g, device=dev) * 4.0 for hv, wv in sizes]
    ours = lambda: views.merge_views(zs, flips, (h, w), merged=True)             # noqa: E731
    theirs = lambda: torch_merge(zs, flips, h, w)                                # noqa: E731
    theirs_all = lambda: torch_merge_all(zs, flips, h, w)                        # noqa: E731
    for _ in range(5):
        a_out, b_out, _m = ours(), theirs_all(), theirs()
    torch.cuda.synchronize()
    differ = int((a_out[0] != b_out[0]).sum())
    logit_gap = float((a_out[3] - b_out[3]).abs().max())
    t_ours, t_theirs, t_all = [], [], []
    for _ in range(4):                                   # alternate the three in blocks
        t_ours += device_us(ours, a.runs // 4 + 1)
        t_theirs += device_us(theirs, a.runs // 4 + 1)
        t_all += device_us(theirs_all, a.runs // 4 + 1)
    ops.prof_enable(True)
    for _ in range(a.runs):
        ours()
    torch.cuda.synchronize()
    ops.prof_collect()
    k = ops.prof_kernels()["view_merge"]
    ops.prof_enable(False)
    us = k["ms"] * 1e3 / k["launches"]
    per_launch = k["bytes"] / k["launches"]
    row = {"frame": [h, w], "classes": c, "views": [[s, fx, fy] for s, fx, fy in plan], "view_sizes": [list(s) for s in sizes],
           "runs": a.runs, "kernel_us": us, "bytes_per_launch": per_launch, "bytes_per_s": per_launch / (us * 1e-6),
           "merge_views_call_us": spread(t_ours), "torch_merged_only_us": spread(t_theirs),
           "torch_all_outputs_us": spread(t_all), "labels_that_differ": differ, "max_merged_logit_gap": logit_gap}
    print(json.dumps(row), flush=True)
    if a.out:
        call, only, full = (row[k]["median"] for k in ("merge_views_call_us", "torch_merged_only_us", "torch_all_outputs_us"))
        verdict = "faster than" if call < only else "NOT faster than"
        lines = [
            "unet_view_merge on one MI355X (tools/bench_view_merge.py): ONE run of this tool; nothing here was repeated on "
            "another day or another card.",
            f"frame {h} x {w}, {c} classes, views (scale, flip_x, flip_y): {row['views']}, sizes {row['view_sizes']}",
            f"kernel (library event brackets, mean of {a.runs} launches): {us:.1f} us",
            f"bytes it must move (views read once + merged, labels, conf, agreement written): {per_launch / 1e6:.1f} MB "
            f"-> {row['bytes_per_s'] / 1e12:.2f} TB/s",
            f"views.merge_views call, all four outputs, allocations included (device events, median / min / max of "
            f"{len(t_ours)}): {call:.1f} / {min(t_ours):.1f} / {max(t_ours):.1f} us",
            f"torch composition, merged logits only (flip + interpolate + add + divide): "
            f"{only:.1f} / {min(t_theirs):.1f} / {max(t_theirs):.1f} us",
            f"torch composition, all four outputs (+ softmax max, per-view argmax compare): "
            f"{full:.1f} / {min(t_all):.1f} / {max(t_all):.1f} us",
            f"the merge_views call is {verdict} the composition of the merged logits alone, which takes {only / call:.2f}x "
            f"the call's time; the composition of all four outputs takes {full / call:.2f}x the call's time",
            f"labels that differ between the two: {differ} of {h * w} (the composition samples in floating point); largest "
            f"gap of a merged logit {logit_gap:.3g}",
            json.dumps(row)]
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
