#!/usr/bin/env python3
"""AUPRO of the evaluation CLI: ops.RegionOverlapAUC on the device against the host route a user would take without
it (copy every anomaly map and mask to the host, scipy.ndimage.label per image, argsort + cumulative sums).

    python tools/bench_region_auc.py [--cases 83x256 32x1024] [--batch 16] [--runs 7] [--host-runs 5] [--spiral]

Per case (images x size): the median over --runs of the device time (torch.cuda.Event) of the update calls of one pass
(labelling + append) and of compute(), after two warm-up passes; the median over --host-runs (after one warm-up) of
the host route on the same inputs, split into copy, labelling and curve.  Masks: up to four discs per image, half of
the images good (about 1.5 % defective pixels over the split); scores sigmoid(N(-3, 2)) lifted on the defects.
--spiral adds the labelling alone on a one-pixel-wide 256 x 256 spiral (one region, the longest chain) against scipy.
Prints one JSON line per case.
"""
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


def one_pass(pred, truth, batch):
    m = ops.RegionOverlapAUC()
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    e0.record()
    for i in range(0, pred.shape[0], batch):
        m.update(pred[i:i + batch], truth[i:i + batch])
    e1.record()
    res = m.compute()                    # reads the counts and the result: ends in a synchronise
    e2.record()
    e2.synchronize()
    return e0.elapsed_time(e1), e1.elapsed_time(e2), res


def host_route(pred, truth, limit=0.3):
    from scipy.ndimage import label
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    maps, masks = pred.cpu().numpy(), truth.cpu().numpy() > 0.5
    t1 = time.perf_counter()
    weight = np.zeros(maps.shape)
    regions = 0
    for i in range(len(masks)):
        lab, n = label(masks[i, 0], np.ones((3, 3), int))
        regions += n
        sizes = np.bincount(lab.ravel(), minlength=n + 1)
        sizes[0] = 1
        weight[i, 0] = np.where(lab > 0, 1.0 / sizes[lab], 0.0)
    t2 = time.perf_counter()
    s = maps.ravel().astype(np.float64)
    order = np.argsort(-s, kind="stable")
    ok = ~masks.ravel()[order]
    x = np.cumsum(ok) / ok.sum()
    y = np.cumsum(weight.ravel()[order]) / regions
    keep = np.append(np.diff(s[order]) != 0, True)
    x, y = np.r_[0.0, x[keep]], np.r_[0.0, y[keep]]
    k = int(np.searchsorted(x, limit, "right"))
    area = np.trapz(y[:k], x[:k])
    if k < len(x) and x[k - 1] < limit:
        yi = y[k - 1] + (y[k] - y[k - 1]) * (limit - x[k - 1]) / (x[k] - x[k - 1])
        area += (limit - x[k - 1]) * (y[k - 1] + yi) / 2
    t3 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, area / limit


def blobs(n, size, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(size, device=dev), torch.arange(size, device=dev), indexing="ij")
    truth = torch.zeros((n, 1, size, size), device=dev)
    for _ in range(4):
        c = torch.rand((n, 2), generator=g, device=dev) * size
        r = (0.02 + 0.06 * torch.rand((n,), generator=g, device=dev)) * size
        d2 = (yy[None] - c[:, 0, None, None]) ** 2 + (xx[None] - c[:, 1, None, None]) ** 2
        truth[:, 0] = torch.maximum(truth[:, 0], (d2 < r[:, None, None] ** 2).float())
    truth[n // 2:] = 0                                                  # the good images of the test split
    pred = torch.sigmoid(torch.randn(truth.shape, generator=g, device=dev) * 2.0 - 3.0 + 1.5 * truth)
    return pred.contiguous(), truth.contiguous()


def spiral(n):
    m = np.zeros((n, n), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    moved = True
    while moved:
        moved = False
        for _ in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and not m[ny, nx] and not (0 <= ay < n and 0 <= ax < n and m[ay, ax]):
                y, x, moved = ny, nx, True
                m[y, x] = True
                break
            dy, dx = dx, -dy
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["83x256", "32x1024"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--host-runs", type=int, default=5)
    ap.add_argument("--spiral", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for case in a.cases:
        n, size = (int(v) for v in case.split("x"))
        pred, truth = blobs(n, size, dev, seed=size)
        for _ in range(2):
            one_pass(pred, truth, a.batch)
        upd, cmp = [], []
        for _ in range(a.runs):
            u, c, res = one_pass(pred, truth, a.batch)
            upd.append(u)
            cmp.append(c)
        row = {"case": case, "pixels": pred.numel(), "batch": a.batch, "runs": a.runs,
               "update_ms_per_pass": statistics.median(upd), "compute_ms": statistics.median(cmp),
               "device_total_ms": statistics.median(upd) + statistics.median(cmp), "aupro": res["aupro"],
               "regions": res["regions"], "defective": res["defective"], "ok": res["ok"]}
        if a.host_runs:
            host = [host_route(pred, truth) for _ in range(a.host_runs + 1)][1:]
            med = [statistics.median(h[i] for h in host) for i in range(3)]
            row.update(host_runs=a.host_runs, host_copy_ms=med[0], host_label_ms=med[1], host_curve_ms=med[2],
                       host_total_ms=statistics.median(sum(h[:3]) for h in host),
                       host_aupro_diff=abs(host[0][3] - res["aupro"]))
            row["host_over_device"] = row["host_total_ms"] / row["device_total_ms"]
        print(json.dumps(row), flush=True)
    if a.spiral:
        from scipy.ndimage import label
        m = spiral(256)
        t = torch.as_tensor(m[None].astype(np.float32)).to(dev)
        times = []
        for i in range(a.runs + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _, _, counts = ops.label_regions(t)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        host = []
        for _ in range(a.host_runs + 1):
            t0 = time.perf_counter()
            label(m, np.ones((3, 3), int))
            host.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"case": "spiral 256x256", "regions": counts.tolist()[0],
                          "label_regions_ms": statistics.median(times[2:]),
                          "scipy_label_ms": statistics.median(host[1:])}), flush=True)


if __name__ == "__main__":
    main()
