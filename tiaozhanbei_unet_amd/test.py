#!/usr/bin/env python3
"""Evaluation CLI with the reference's contract (/root/reference/src/test.py: flags :26-61, test_model :66-133,
`test_metrics.json` / `detailed_results.json` :187-232, `visualizations.png` :315-332) on the HIP path.  The forward
runs on the GPU; thresholding and metrics are host numpy, as in the reference; the visualisation sheet is rendered on
the GPU (sheets.render_sheet) and only encoded on the host."""
import argparse
import json
import math
import os

import numpy as np
import torch

FLAGS = [  # reference src/test.py:26-61
    ("--data_root", dict(type=str, default="../datasets/mvtec_anomaly_detection")),
    ("--category", dict(type=str, default="bottle")),
    ("--image_size", dict(type=int, default=256)),
    ("--model", dict(type=str, default="anomaly_unet", choices=["unet", "anomaly_unet"])),
    ("--bilinear", dict(action="store_true")),
    ("--checkpoint", dict(type=str, required=True)),
    ("--batch_size", dict(type=int, default=16)),
    ("--num_workers", dict(type=int, default=4)),
    ("--device", dict(type=str, default="auto")),
    ("--threshold", dict(type=float, default=None)),
    ("--pixel_thresholds", dict(type=float, nargs="+", default=[0.3, 0.5, 0.7])),
    ("--output_dir", dict(type=str, default="../test_results")),
    ("--save_visualizations", dict(action="store_true")),
    ("--max_vis_samples", dict(type=int, default=20)),
    ("--precision", dict(type=str, default="fp32", choices=["fp32", "bf16"])),   # build-only
    ("--pro_fpr_limit", dict(type=float, default=0.3)),     # build-only: the PRO curve is integrated up to this fpr
    ("--binary_masks", dict(action="store_true")),          # build-only: masks as (mask > 0) instead of k / 255
    ("--vis_overlay_alpha", dict(type=float, default=None)),    # build-only: adds an anomaly-map-over-image column
    ("--map_sigma", dict(type=float, default=0.0)),         # build-only: Gaussian smoothing of the anomaly map (0: none)
    ("--map_truncate", dict(type=float, default=4.0)),      # build-only: the Gaussian is cut at this many sigmas
    ("--image_score", dict(type=str, default="reconstruction", choices=["reconstruction", "map_max"])),   # build-only
]
VIS_GUTTER = 4              # white pixels between the panels of visualizations.png


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Test UNet for MVTec anomaly detection (MI355X HIP path)")
    for name, kw in FLAGS:
        ap.add_argument(name, **kw)
    args = ap.parse_args(argv)
    if not 0.0 < args.pro_fpr_limit <= 1.0:
        raise SystemExit(f"--pro_fpr_limit must be in (0, 1], got {args.pro_fpr_limit}")
    if args.vis_overlay_alpha is not None and not 0.0 <= args.vis_overlay_alpha <= 1.0:
        raise SystemExit(f"--vis_overlay_alpha must be in [0, 1], got {args.vis_overlay_alpha}")
    for flag in ("map_sigma", "map_truncate"):
        if not (math.isfinite(getattr(args, flag)) and getattr(args, flag) >= 0.0):
            raise SystemExit(f"--{flag} must be finite and >= 0, got {getattr(args, flag)}")
    try:
        map_radius(args.map_sigma, args.map_truncate)
    except ValueError as e:
        raise SystemExit(f"--map_sigma {args.map_sigma} with --map_truncate {args.map_truncate}: {e}")
    return args


def map_radius(map_sigma, map_truncate):
    """Radius of the smoothing window (scipy's rule); ValueError when the kernel does not cover it."""
    from .evaluation import GaussianSmoother
    return GaussianSmoother(map_sigma, map_truncate).radius


def test_model(model, test_loader, device, threshold=None, pixel_thresholds=None, pro_fpr_limit=0.3,
               binary_masks=False, *, map_sigma=0.0, map_truncate=4.0, image_score="reconstruction"):
    """With map_sigma > 0 the anomaly map is smoothed on the device (evaluation.GaussianSmoother) before anything reads
    it; with image_score == "map_max" an image's score is the peak of that map (the raw one at sigma 0), from the same
    launch, instead of its mean reconstruction error.  At the defaults nothing is launched."""
    from . import AnomalyUNet, evaluation
    from .utils import compute_anomaly_score, get_optimal_threshold
    if image_score not in ("reconstruction", "map_max"):
        raise ValueError(f"test_model: image_score {image_score!r}")
    smoother = evaluation.GaussianSmoother(map_sigma, map_truncate) if map_sigma > 0 or image_score == "map_max" else None
    model.eval()
    out = {k: [] for k in ("images", "reconstructions", "anomaly_maps", "masks_true", "labels", "anomaly_types",
                           "image_paths", "anomaly_scores")}
    pix = None
    pix_auc = evaluation.BinaryAUC()  # pixel AUROC / AUPRC of the anomalous images, ranked on the device (:172-178)
    pix_pro = evaluation.RegionOverlapAUC(pro_fpr_limit)     # AUPRO over every test image (good ones supply ok pixels)
    with torch.no_grad():
        from .train_utils import _batches
        for batch, images, _ in _batches(test_loader, device):     # (raw uint8 batches are transformed on the device)
            if isinstance(model, AnomalyUNet):
                recon, amap = model(images)
            else:
                amap, recon = model(images, sigmoid=True), images      # sigmoid inside the head kernel
            masks = (batch["mask"] > 0).float() if binary_masks else batch["mask"]
            if smoother is not None:
                amap, peak = smoother(amap)
            if pixel_thresholds:          # pixel-level confusion counts of the anomalous images, on the device (:86-101)
                bad = torch.as_tensor(np.asarray(batch["label"]) == 1)
                pix = evaluation.threshold_confusion(amap, masks, pixel_thresholds, select=bad, counts=pix)
                pix_auc.update(amap, masks, select=bad)
                pix_pro.update(amap, masks)
            if image_score == "map_max":
                out["anomaly_scores"].extend(peak.cpu().numpy())
            else:
                out["anomaly_scores"].extend(compute_anomaly_score(recon, images).cpu().numpy())
            out["images"].extend(images.cpu()); out["reconstructions"].extend(recon.cpu())
            out["anomaly_maps"].extend(amap.cpu().numpy()); out["masks_true"].extend(masks.cpu().numpy())
            out["labels"].extend(np.asarray(batch["label"])); out["anomaly_types"].extend(batch["anomaly_type"])
            out["image_paths"].extend(batch["image_path"])
    for k in ("labels", "anomaly_scores", "masks_true", "anomaly_maps"):
        out[k] = np.array(out[k])
    if threshold is None:
        # the reference feeds per-pixel score maps here; image-level score = their mean
        img_scores = out["anomaly_scores"].reshape(len(out["labels"]), -1).mean(1)
        threshold = float(get_optimal_threshold(out["labels"], img_scores)[0]) if len(np.unique(out["labels"])) > 1 else 0.5
        print(f"Optimal threshold: {threshold:.4f}")
    out["image_scores"] = out["anomaly_scores"].reshape(len(out["labels"]), -1).mean(1)
    out["predictions"] = (out["image_scores"] > threshold).astype(int)
    out["threshold"] = threshold
    if pix is not None:
        out["pixel_counts"] = {float(t): c for t, c in zip(pixel_thresholds, pix.cpu().tolist())}
        out["pixel_auc"] = pix_auc.compute()
        out["pixel_pro"] = pix_pro.compute()
    return out


def evaluate_results(results, pixel_thresholds):
    from .utils import calculate_metrics
    ev = {"image_metrics": calculate_metrics(results["labels"], results["predictions"], results["image_scores"]),
          "pixel_metrics": {}, "type_metrics": {}}
    bad = results["labels"] == 1
    if bad.sum() > 0 and "pixel_counts" in results:         # counted on the device by test_model
        from .utils import metrics_from_counts
        for t in pixel_thresholds:
            tp, fp, fn, tn = results["pixel_counts"][float(t)]
            if tp + fn > 0 and fp + tn > 0:
                ev["pixel_metrics"][f"threshold_{t}"] = {**metrics_from_counts(tp, fp, fn, tn),
                                                         "auroc": results["pixel_auc"]["auroc"],
                                                         "auprc": results["pixel_auc"]["auprc"]}
    elif bad.sum() > 0:
        truth = (results["masks_true"][bad] > 0.5).astype(np.uint8).ravel()
        if len(np.unique(truth)) > 1:
            for t in pixel_thresholds:
                pred = (results["anomaly_maps"][bad] > t).astype(np.uint8).ravel()
                ev["pixel_metrics"][f"threshold_{t}"] = calculate_metrics(truth, pred, results["anomaly_maps"][bad].ravel())
    for kind in sorted(set(results["anomaly_types"])):
        sel = np.array([k == kind for k in results["anomaly_types"]])
        ev["type_metrics"][kind] = {"count": int(sel.sum()),
                                    "detected": int(results["predictions"][sel].sum())}
    pro = results.get("pixel_pro")
    if pro and pro["regions"] > 0 and pro["ok"] > 0:         # build-only: AUPRO of the MVTec AD evaluation
        ev["region_metrics"] = {k: pro[k] for k in ("aupro", "pro_at_limit", "fpr_limit", "regions")}
    return ev


def save_visualizations(results, out_dir, max_samples, with_reconstruction, overlay_alpha=None):
    """`visualizations.png` of the reference (src/test.py:315-332 -> src/utils.py:111-157 visualize_results): a random
    choice of min(max_samples, all) test samples, one row each: original | true mask (gray) | predicted map (hot) |
    reconstruction (with_reconstruction) | map over original (overlay_alpha).  Rendered on the device at native resolution
    (sheets.render_sheet), encoded once with Pillow; no titles or axes: `visualizations.json` beside it names, row by row,
    what matplotlib's titles would.  Returns the path of the PNG (None when there is nothing to draw)."""
    from PIL import Image
    from . import sheets
    total = len(results["images"])
    n = min(max_samples, total)
    if n <= 0:
        return None
    indices = np.random.choice(total, n, replace=False)         # the reference's draw (:321)
    dev = torch.device("cuda")
    images = torch.stack([results["images"][i] for i in indices]).to(dev)
    masks = torch.as_tensor(np.stack([results["masks_true"][i] for i in indices])).to(dev)
    maps = torch.as_tensor(np.stack([results["anomaly_maps"][i] for i in indices])).to(dev)
    columns = [("image", images), ("gray", masks), ("hot", maps)]
    if with_reconstruction:
        columns.append(("unit", torch.stack([results["reconstructions"][i] for i in indices]).to(dev)))
    if overlay_alpha is not None:
        columns.append(("overlay", images, maps, float(overlay_alpha)))
    sheet = sheets.render_sheet(columns, gutter=VIS_GUTTER)
    path = os.path.join(out_dir, "visualizations.png")
    Image.fromarray(sheet.cpu().numpy()).save(path)
    names = {"image": "original", "gray": "mask_true", "hot": "anomaly_map", "unit": "reconstruction",
             "overlay": "overlay"}
    rows = [{"index": int(i), "image_path": str(results["image_paths"][i]), "label": int(results["labels"][i]),
             "anomaly_type": str(results["anomaly_types"][i]), "image_score": float(results["image_scores"][i]),
             "prediction": int(results["predictions"][i])} for i in indices]
    with open(os.path.join(out_dir, "visualizations.json"), "w") as f:
        json.dump({"columns": [names[c[0]] for c in columns], "gutter": VIS_GUTTER, "overlay_alpha": overlay_alpha,
                   "panel_size": [int(images.shape[2]), int(images.shape[3])], "rows": rows}, f, indent=2)
    print(f"Visualization saved to {path}")
    return path


def main(argv=None):
    from . import AnomalyUNet, UNet
    from .dataset import get_available_categories, get_dataloaders
    from .utils import load_checkpoint, print_metrics
    args = parse_args(argv)
    if args.device == "cpu" or not torch.cuda.is_available():
        raise SystemExit("this build computes only on an AMD GPU (libunet_hip.so); there is no CPU path")
    device = torch.device("cuda")
    if args.category not in get_available_categories(args.data_root):
        print(f"Category '{args.category}' not found!")
        return
    out_dir = os.path.join(args.output_dir, f"{args.category}_test_results")
    os.makedirs(out_dir, exist_ok=True)
    _, loader = get_dataloaders(args.data_root, args.category, args.batch_size, args.image_size, args.num_workers,
                                device_preprocess=True)                     # workers decode, the GPU transforms
    model = (AnomalyUNet(3, args.bilinear, precision=args.precision) if args.model == "anomaly_unet"
             else UNet(3, 1, args.bilinear, precision=args.precision)).to(device)
    load_checkpoint(model, None, args.checkpoint, device)
    results = test_model(model, loader, device, args.threshold, pixel_thresholds=args.pixel_thresholds,
                         pro_fpr_limit=args.pro_fpr_limit, binary_masks=args.binary_masks, map_sigma=args.map_sigma,
                         map_truncate=args.map_truncate, image_score=args.image_score)
    ev = evaluate_results(results, args.pixel_thresholds)
    print_metrics(ev["image_metrics"], "Image-level")

    def plain(o):
        if isinstance(o, dict):
            return {k: plain(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return [plain(v) for v in o]
        if isinstance(o, np.generic):
            return o.item()
        return o.tolist() if isinstance(o, np.ndarray) else o

    with open(os.path.join(out_dir, "test_metrics.json"), "w") as f:
        post = {}
        if args.map_sigma > 0 or args.image_score != "reconstruction":          # build-only; absent at the defaults
            post = {"postprocess": {"map_sigma": args.map_sigma, "map_truncate": args.map_truncate,
                                    "radius": map_radius(args.map_sigma, args.map_truncate),
                                    "image_score": args.image_score}}
        json.dump({**plain(ev), "threshold": float(results["threshold"]), **post, "args": vars(args)}, f, indent=2)
    with open(os.path.join(out_dir, "detailed_results.json"), "w") as f:
        json.dump({"labels": results["labels"].tolist(), "predictions": results["predictions"].tolist(),
                   "anomaly_scores": results["image_scores"].tolist(), "anomaly_types": list(results["anomaly_types"]),
                   "image_paths": list(results["image_paths"]), "threshold": float(results["threshold"])}, f, indent=2)
    if args.save_visualizations:
        print("Saving visualizations...")
        save_visualizations(results, out_dir, args.max_vis_samples, args.model == "anomaly_unet",
                            args.vis_overlay_alpha)
    print(f"\nTesting completed!\nResults saved to: {out_dir}")
    return out_dir


if __name__ == "__main__":
    main()
