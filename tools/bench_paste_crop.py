#!/usr/bin/env python3
"""unet_paste_crop_u8 (csrc/paste.hip) on a train_gear_paste batch, next to the two unet_affine_crop_u8 launches it
replaces.

    python tools/bench_paste_crop.py [--runs 101] [--rounds 3] [--out profiles/paste_crops.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_paste_crop.py --profile-only

Workload: 8 images of 1080 x 1920 (random bytes) and their class masks (six labelled rectangles of 40..160 pixels a side
each, classes 1..3), resident on the device; 4 crops of 512 x 512 each drawn by crops.CropSampler with the trainer's
defaults: 32 crops.  Three cases: `two_crops`, the bilinear image launch and the nearest mask launch of
crops.GearCropPreprocess without pasting (the yardstick: that code is untouched by the paste kernel's commit);
`paste_0`, crops.paste_crops_u8 with no paste; `paste_2`, the same with 2 pastes on every crop (a rectangle of any image,
the crop's scale times a log-uniform factor in 0.75..1.33, any rotation, flipped or not, anywhere in the crop).
Per case: the kernels' time per call from the library's own event brackets (ops.prof_kernels) over --runs calls, after
warm-up calls, in --rounds rounds that ALTERNATE the three cases, so a drift of the box shows as a spread between the
rounds and not as a difference between the cases; and the median device time (torch.cuda.Event) of the whole wrapper
call(s), which also pack the device images and upload the tables.  Both outputs of `paste_0` are checked against
`two_crops` first.  No threshold is asserted."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--profile-only", action="store_true", help="a few calls of each case, then exit")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_paste_crop.py measures on an AMD GPU; none is visible")
    dev = torch.device("cuda:0")
    n, h, w, k, crop = 8, 1080, 1920, 4, (512, 512)
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    images = list(torch.randint(0, 256, (n, h, w, 3), generator=g, device=dev, dtype=torch.uint8).unbind(0))
    masks, boxes = [], []
    for i in range(n):
        m = torch.zeros((h, w), dtype=torch.uint8, device=dev)
        for _ in range(6):
            bw, bh = (int(v) for v in rng.integers(40, 161, 2))
            x0, y0 = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
            m[y0:y0 + bh, x0:x0 + bw] = int(rng.integers(1, 4))
            boxes.append((i, (x0, y0, x0 + bw, y0 + bh)))
        masks.append(m)
    sampler = crops.CropSampler(crop, seed=0)
    params = sampler.draw([(h, w)] * n, [[]] * n, k)
    table = crops.crop_table(sampler.descs(params))
    pastes = []
    for c in range(n * k):
        for _ in range(2):
            donor, box = boxes[int(rng.integers(len(boxes)))]
            scale = min(params["scale"][c] * math.exp(rng.uniform(math.log(0.75), math.log(1.33))), crops.MAX_SCALE)
            b = crops.paste_matrix((box[0] + box[2]) / 2, (box[1] + box[3]) / 2, scale, rng.uniform(-180.0, 180.0),
                                   bool(rng.integers(2)), rng.uniform(0.0, crop[1]), rng.uniform(0.0, crop[0]))
            pastes.append((c, donor, b, box))
    masks_c1 = [m.unsqueeze(-1) for m in masks]

    def two_crops():
        return (crops.affine_crops_u8(images, table, crop, 1, 0),
                crops.affine_crops_u8(masks_c1, table, crop, 0, crops.IGNORE_INDEX)[..., 0])

    cases = {"two_crops": (two_crops, "affine_crop"),
             "paste_0": (lambda: crops.paste_crops_u8(images, masks, table, [], crop), "paste_crop"),
             "paste_2": (lambda: crops.paste_crops_u8(images, masks, table, pastes, crop), "paste_crop")}
    want, got, pasted = two_crops(), cases["paste_0"][0](), cases["paste_2"][0]()
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]), "paste_crops_u8 without pastes is not the two crops"
    changed = int((pasted[1] != want[1]).sum())
    for fn, _ in cases.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    if a.profile_only:
        return

    kernel_us = {name: [] for name in cases}
    call_us = {name: [] for name in cases}
    for _ in range(a.rounds):
        for name, (fn, kernel) in cases.items():
            call_us[name] += device_us(fn, a.runs)
            ops.prof_enable(True)
            for _ in range(a.runs):
                fn()
            torch.cuda.synchronize()
            ops.prof_collect()
            kern = ops.prof_kernels()[kernel]
            ops.prof_enable(False)
            kernel_us[name].append(kern["ms"] * 1e3 / a.runs)          # per call: two_crops is two launches
    written = n * k * crop[0] * crop[1] * 4
    row = {"images": [n, h, w], "crops": n * k, "crop": list(crop), "pastes_per_crop": 2, "runs": a.runs, "rounds": a.rounds,
           "bytes_written": written, "mask_pixels_changed_by_pastes": changed,
           "cases": {name: {"kernel_us_per_round": kernel_us[name], "kernel_us": statistics.mean(kernel_us[name]),
                            "call_us": {"median": statistics.median(call_us[name]), "min": min(call_us[name]),
                                        "max": max(call_us[name])}} for name in cases}}
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"tools/bench_paste_crop.py --runs {a.runs} --rounds {a.rounds}: {n} images of {h} x {w} on the device, "
                    f"{n * k} crops of {crop[0]} x {crop[1]},\n{written} bytes written per call (image and mask crops); "
                    f"the 2 pastes per crop change {changed} mask pixels of {n * k * crop[0] * crop[1]}.\n"
                    f"Kernel time per call: library event brackets, mean of {a.runs} calls in each of {a.rounds} rounds that "
                    f"alternate the cases.\nCall time: torch.cuda.Event around the wrapper call(s), median [min, max] of "
                    f"{a.runs * a.rounds} calls.\n\n")
            f.write(f"{'case':<12}{'kernel us (mean)':>18}  {'per round':<36}{'call us':>10}\n")
            for name, c in row["cases"].items():
                rounds = ", ".join(f"{v:.1f}" for v in c["kernel_us_per_round"])
                f.write(f"{name:<12}{c['kernel_us']:>18.1f}  {rounds:<36}{c['call_us']['median']:>10.1f} "
                        f"[{c['call_us']['min']:.1f}, {c['call_us']['max']:.1f}]\n")
            f.write("\ntwo_crops = the unet_affine_crop_u8 image launch + mask launch; paste_0 / paste_2 = one "
                    "unet_paste_crop_u8 launch with 0 / 2 pastes per crop.\n" + json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
