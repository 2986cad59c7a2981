#!/usr/bin/env python3
"""unet_affine_crop_u8 (csrc/crops.hip) on a train_gear_crops batch.

    python tools/bench_affine_crop.py [--runs 101] [--out profiles/affine_crop.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_affine_crop.py --profile-only

Workload: 8 images of 1080 x 1920 (random bytes, resident on the device), 4 crops of 512 x 512 each drawn by
crops.CropSampler with the trainer's defaults (scale 0.75..1.5, +-10 degrees, flip; no polygons, so uniform centres):
32 crops.  Two launches, as GearCropPreprocess makes them: the RGB images bilinearly, the one-channel masks with NEAREST.
Per launch: the kernel's mean time over --runs launches from the library's own event brackets (ops.prof_kernels) after
warm-up calls, the bytes written (crops x 512 x 512 x c) and written bytes / time -- the bytes READ are not counted: a
bilinear tap reads up to four source bytes per output byte, most of them from cache -- and the median device time
(torch.cuda.Event) of the whole crops.affine_crops_u8 call, which for device images also concatenates them into the
packed buffer (a copy of all 8 images) and uploads the tables.  No threshold is asserted."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tiaozhanbei_unet_amd import crops, ops  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=101)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--profile-only", action="store_true", help="a few launches of each case, then exit")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_affine_crop.py measures on an AMD GPU; none is visible")
    dev = torch.device("cuda:0")
    n, h, w, k, crop = 8, 1080, 1920, 4, (512, 512)
    g = torch.Generator(device=dev).manual_seed(0)
    sampler = crops.CropSampler(crop, seed=0)
    table = crops.crop_table(sampler.descs(sampler.draw([(h, w)] * n, [[]] * n, k)))
    rows = {}
    for name, c, mode, fill in (("images_bilinear", 3, 1, 0), ("masks_nearest", 1, 0, 255)):
        images = list(torch.randint(0, 256, (n, h, w, c), generator=g, device=dev, dtype=torch.uint8).unbind(0))
        call = lambda: crops.affine_crops_u8(images, table, crop, mode, fill)          # noqa: E731
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        if a.profile_only:
            continue
        whole = device_us(call, a.runs)
        ops.prof_enable(True)
        for _ in range(a.runs):
            call()
        torch.cuda.synchronize()
        ops.prof_collect()
        kern = ops.prof_kernels()["affine_crop"]
        ops.prof_enable(False)
        us = kern["ms"] * 1e3 / kern["launches"]
        written = n * k * crop[0] * crop[1] * c
        rows[name] = {"c": c, "mode": mode, "kernel_us": us, "launches": kern["launches"], "bytes_written": written,
                      "written_bytes_per_s": written / (us * 1e-6),
                      "affine_crops_u8_call_us": {"median": statistics.median(whole), "min": min(whole), "max": max(whole)}}
    if a.profile_only:
        return
    row = {"images": [n, h, w], "crops": n * k, "crop": list(crop), "runs": a.runs, **rows}
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
