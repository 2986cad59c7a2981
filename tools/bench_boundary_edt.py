#!/usr/bin/env python3
"""Kernel times of unet_boundary_distance_sq and unet_boundary_stats (csrc/distance.hip) on 4-class 1080 x 1920 label maps,
next to the wall time of scipy.ndimage.distance_transform_edt on the same boundary masks on the host.

    python tools/bench_boundary_edt.py [--repeats 10] [--threads 16]

Three cases: sparse blobs (discs, the prediction a shifted copy), a dense random map, and one boundary pixel in a corner
(the row pass's worst case: every lane scans far).  The device times are event brackets around each launch
(ops.prof_enable / prof_kernels), mean over the repeats after one warm-up call; the scipy time is the wall time of the three
class planes of ONE map, the planes spread over a pool of --threads threads (distance_transform_edt releases no more
parallelism than that).  Prints one block per case."""
import argparse
import ctypes
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

H, W, C = 1080, 1920, 4


def cases():
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    blobs, moved = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    for _ in range(60):
        cy, cx, r, c = rng.integers(0, H), rng.integers(0, W), rng.integers(8, 120), rng.integers(1, C)
        dy, dx = rng.integers(-6, 7, 2)
        blobs[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = c
        moved[(yy - cy - dy) ** 2 + (xx - cx - dx) ** 2 <= r * r] = c
    dense = rng.integers(0, C, (H, W), dtype=np.uint8)
    dense_pred = np.where(rng.random((H, W)) < 0.1, rng.integers(0, C, (H, W), dtype=np.uint8), dense)
    corner = np.zeros((H, W), np.uint8)
    corner[H - 1, W - 1] = 1
    corner_pred = np.zeros((H, W), np.uint8)
    corner_pred[0, 0] = 1
    return [("sparse blobs", blobs, moved), ("dense random", dense, dense_pred), ("one pixel in a corner", corner, corner_pred)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    from scipy import ndimage

    import _boundary_ref as B
    from tiaozhanbei_unet_amd import _lib as L
    from tiaozhanbei_unet_amd import ops
    dev = torch.device("cuda:0")
    vp, tol_sq, band = ctypes.c_void_p, (ctypes.c_int32 * 3)(1, 4, 16), B.band_width(H, W)
    for name, truth, pred in cases():
        t, p = (torch.from_numpy(m[None]).to(dev) for m in (truth, pred))
        both = torch.cat([t, p])

        def once():
            d2 = ops.boundary_distance_sq(both, C)
            records = torch.zeros((1, C - 1, len(ops.BOUNDARY_FIELDS)), dtype=torch.int64, device=dev)
            hist = torch.zeros((C - 1, 2, 1025), dtype=torch.int64, device=dev)
            L.check(L.lib().unet_boundary_stats(vp(t.data_ptr()), vp(p.data_ptr()), vp(d2[:1].data_ptr()),
                                                vp(d2[1:].data_ptr()), 1, H, W, C, tol_sq, 3, band * band, 0,
                                                vp(records.data_ptr()), vp(hist.data_ptr()), None), "unet_boundary_stats")
            return d2, records

        d2, records = once()                           # warm-up, and the check against scipy
        torch.cuda.synchronize()
        masks = [B.boundary_mask(truth == c) for c in range(1, C)]
        for c, b in enumerate(masks):
            want = np.rint(ndimage.distance_transform_edt(~b) ** 2) if b.any() else np.full((H, W), B.NONE)
            assert np.array_equal(d2[0, c].cpu().numpy(), want.astype(np.int64)), (name, c)
        ops.prof_enable(True)
        ops.prof_collect()
        for _ in range(args.repeats):
            once()
        torch.cuda.synchronize()
        ops.prof_collect()
        kernels = ops.prof_kernels()
        ops.prof_enable(False)
        with ThreadPoolExecutor(args.threads) as pool:
            walls = []
            for _ in range(3):
                t0 = time.perf_counter()
                list(pool.map(lambda b: ndimage.distance_transform_edt(~b) if b.any() else None, masks))
                walls.append(time.perf_counter() - t0)
        boundary = [int(b.sum()) for b in masks]
        print(f"{name}: truth boundary pixels per class {boundary}, records t_boundary "
              f"{records[0, :, 4].tolist()} p_boundary {records[0, :, 5].tolist()}")
        for k in ("edt_column_pass", "edt_row_pass", "boundary_stats"):
            s = kernels[k]
            print(f"  {k:<18} {1000.0 * s['ms'] / s['launches']:>9.1f} us per launch ({s['launches']} launches)")
        print(f"  scipy distance_transform_edt, the 3 class planes of one map: {1000.0 * min(walls):.1f} ms "
              f"(best of 3, {args.threads} threads); the device call above transforms two maps")


if __name__ == "__main__":
    main()
