#!/usr/bin/env python3
"""Kernel times of csrc/calibration.hip (unet_seg_confidence_scaled, unet_reliability_histogram, unet_temperature_sweep at
K = 32) next to unet_seg_confidence on the same logits: 8 x 4 x 512 x 512 and 1 x 4 x 1080 x 1920.

    python tools/bench_calibration.py [--repeats 10]

Logits are N(0, 4^2) with every target drawn uniformly (so no pixel is skipped and `select` leaves none out: the sweep's
worst case).  The device times are the library's event brackets around each call (ops.prof_enable / prof_kernels), mean
over the repeats after one warm-up call; the sweep's bracket holds its finalize launch too.  Before timing, the sweep of
the first shape's first image is checked against tests/_calibration_ref.py.  Prints one block per shape."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(8, 4, 512, 512), (1, 4, 1080, 1920)]
K = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    import _calibration_ref as CR
    import _ref64 as R64
    from tiaozhanbei_unet_amd import ops, seg_calibration
    dev = torch.device("cuda:0")
    grid = seg_calibration.temperature_grid(0.25, 4.0, K)
    checked = False
    for n, c, h, w in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(n * 1000 + h)
        logits = (torch.randn((n, c, h, w), generator=g) * 4.0).to(dev)
        target = torch.randint(0, c, (n, h, w), generator=g).to(dev)

        def once():
            ops.seg_confidence(logits)
            meter = ops.CalibrationMeter(c, bins=15, temperatures=grid, temperature=3.0)
            meter.update(logits, target)
            return meter

        res = once().compute()                         # warm-up
        assert res["counted"] == n * h * w and res["skipped"] == 0 and int(res["hist"][:, :, 0].sum()) == n * h * w
        if not checked:                                # one image against the float64 restatement
            meter = ops.CalibrationMeter(c, temperatures=grid)
            meter.update(logits[:1], target[:1])
            got = meter.compute()["nll"]
            z, t = logits[:1].cpu().numpy(), target[:1].cpu().numpy()
            inv = [CR.inv_t32(v) for v in grid]
            nll, scale, _, _ = CR.sweep64(z, t, -1, 0, inv)
            host = CR.sweep32(z, t, -1, 0, inv)
            R64.assert_measured(torch.from_numpy(got), (torch.from_numpy(nll), torch.from_numpy(scale)),
                                torch.from_numpy(host), "bench_calibration sweep", extra=R64.SUM_EPS)
            host_rel, kernel_rel, allowed = R64.MEASURED["bench_calibration sweep"]
            print(f"sweep of one {h} x {w} image against float64: kernel err {kernel_rel / 2.0 ** -24:.2f} u of S, host err "
                  f"{host_rel / 2.0 ** -24:.2f} u, allowed {allowed / 2.0 ** -24:.2f} u")
            checked = True
        torch.cuda.synchronize()
        ops.prof_enable(True)
        ops.prof_collect()
        for _ in range(args.repeats):
            once()
        torch.cuda.synchronize()
        ops.prof_collect()
        kernels = ops.prof_kernels()
        ops.prof_enable(False)
        pixels = n * h * w
        print(f"{n} x {c} x {h} x {w} ({pixels} pixels, {pixels * c * 4 / 1e6:.1f} MB of logits), K = {K}:")
        for name in ("seg_confidence", "seg_confidence_scaled", "reliability_histogram", "temperature_sweep"):
            s = kernels[name]
            us = 1000.0 * s["ms"] / s["launches"]
            print(f"  {name:<24} {us:>9.1f} us per call ({s['launches']} calls), {s['bytes'] / s['launches'] / us / 1e6:.2f} "
                  f"TB/s of algorithmic bytes")
        s = kernels["temperature_sweep"]
        us = 1000.0 * s["ms"] / s["launches"]
        print(f"  temperature_sweep: {K * c * pixels / us / 1e6:.2f} T expf/s, {us * 1e3 / pixels:.3f} ns per pixel")


if __name__ == "__main__":
    main()
