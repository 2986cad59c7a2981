#!/usr/bin/env python3
"""Pixel AUROC / AUPRC of the evaluation CLI: ops.BinaryAUC on the device against the host path of the reference
(copy every anomaly map to the host, then sklearn's roc_auc_score + auc(precision_recall_curve)).

    python tools/bench_pixel_auc.py [--sizes 256 1024] [--images 100] [--batch 16] [--runs 7] [--sklearn-sizes 256]

Per size: the median over --runs of the device time (torch.cuda.Event) of the update calls of one pass over the
images (also per batch) and of compute(), after two warm-up passes; the device-to-host copy of the maps and masks
the host path needs; sklearn's time on the same pixels (only for --sklearn-sizes: it grows with the pixel count).
Prints one JSON line per size.  Scores: sigmoid(N(-3, 2)) (a continuous anomaly map), 5 % positive pixels.
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
    m = ops.BinaryAUC()
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    e0.record()
    for i in range(0, pred.shape[0], batch):
        m.update(pred[i:i + batch], truth[i:i + batch])
    e1.record()
    res = m.compute()                    # reads the counts and the result: ends in a synchronise
    e2.record()
    e2.synchronize()
    return e0.elapsed_time(e1), e1.elapsed_time(e2), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--sklearn-sizes", type=int, nargs="*", default=[256])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for size in a.sizes:
        g = torch.Generator(device=dev).manual_seed(size)
        shape = (a.images, 1, size, size)
        truth = (torch.rand(shape, generator=g, device=dev) < 0.05).float()
        pred = torch.sigmoid(torch.randn(shape, generator=g, device=dev) * 2.0 - 3.0 + 1.5 * truth)
        for _ in range(2):
            one_pass(pred, truth, a.batch)
        upd, cmp = [], []
        for _ in range(a.runs):
            u, c, res = one_pass(pred, truth, a.batch)
            upd.append(u)
            cmp.append(c)
        batches = -(-a.images // a.batch)
        copies = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hp, ht = pred.cpu().numpy(), truth.cpu().numpy()
            copies.append((time.perf_counter() - t0) * 1e3)
        row = {"pixels": pred.numel(), "images": a.images, "size": size, "batch": a.batch, "runs": a.runs,
               "update_ms_per_pass": statistics.median(upd), "update_ms_per_batch": statistics.median(upd) / batches,
               "compute_ms": statistics.median(cmp), "device_total_ms": statistics.median(upd) + statistics.median(cmp),
               "d2h_copy_ms": statistics.median(copies), "auroc": res["auroc"], "auprc": res["auprc"],
               "positives": res["positives"], "negatives": res["negatives"]}
        if size in a.sklearn_sizes:
            from sklearn.metrics import auc, precision_recall_curve, roc_auc_score
            y, s = (ht.ravel() > 0.5).astype(int), hp.ravel()
            t0 = time.perf_counter()
            roc = roc_auc_score(y, s)
            p, r, _ = precision_recall_curve(y, s)
            pr = auc(r, p)
            row["sklearn_s"] = time.perf_counter() - t0
            row["sklearn_diff"] = [abs(roc - res["auroc"]), abs(pr - res["auprc"])]
            row["distinct_scores"] = int(np.unique(s).size)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
