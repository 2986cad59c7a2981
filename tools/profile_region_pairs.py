#!/usr/bin/env python3
"""The workload of profiles/region_pairs.txt: ops.pair_class_regions and, on the same maps, ops.ClassRegionMatcher
(count_class_hits: the existing kernel with the same traffic) on a pair of synthetic 1080 x 1920 label maps.

    rocprofv3 --kernel-trace --stats -f csv -d out -- python tools/profile_region_pairs.py [--runs 20] [--discs 60]

Truth: --discs discs of classes 1..3 with radii of 8 to 120 pixels; prediction: the same discs moved by up to 6 pixels
and resized by up to 10 %, a tenth of them dropped, as many false ones added.  Both maps are labelled once
(label_class_regions); then --runs calls of each.  Prints the map's figures (regions, pairs, bound, table slots) as one
JSON line; the kernel times are the profiler's.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tiaozhanbei_unet_amd import _lib, ops  # noqa: E402


def disc_maps(h, w, discs, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    truth, pred = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    for _ in range(discs):
        cy, cx, r, c = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(8, 120), int(rng.integers(1, 4))
        truth[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = c
        if rng.random() < 0.1:                         # missed; a false alarm elsewhere instead
            cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        cy, cx, r = cy + rng.uniform(-6, 6), cx + rng.uniform(-6, 6), r * rng.uniform(0.9, 1.1)
        pred[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = c
    return truth, pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--discs", type=int, default=60)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    h, w = args.size
    truth, pred = (torch.from_numpy(m)[None].cuda() for m in disc_maps(h, w, args.discs, args.seed))
    region, _sizes, counts = ops.label_class_regions(torch.cat([truth, pred]), 4)
    treg, preg = region[:1].contiguous(), region[1:].contiguous()
    pairs = None
    for _ in range(args.runs):
        pairs = ops.pair_class_regions(treg, preg)
        matcher = ops.ClassRegionMatcher(4)
        matcher.update(pred, truth)
        matcher.compute()
    bound = torch.zeros(1, dtype=torch.int64, device="cuda")
    vp = ctypes.c_void_p
    _lib.check(_lib.lib().unet_region_pair_bound(vp(treg.data_ptr()), vp(preg.data_ptr()), 1, h, w, vp(bound.data_ptr()),
                                                 None), "unet_region_pair_bound")
    b = int(bound)
    print(json.dumps({"size": [h, w], "runs": args.runs, "truth_regions": int(counts[0].sum()),
                      "pred_regions": int(counts[1].sum()), "pairs": int(len(pairs)), "bound": b,
                      "table_slots": 1 << (2 * max(b, 1) - 1).bit_length(),
                      "paired_pixels": int(pairs[:, 3].sum())}))


if __name__ == "__main__":
    main()
