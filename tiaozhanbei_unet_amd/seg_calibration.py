"""Calibration figures from the reliability histogram and the temperature sweep of ``evaluation.CalibrationMeter``:
reliability diagram, ECE, MCE, a fitted temperature, and the fold of 1 / T into a checkpoint's 1x1 head.  Host arithmetic
in float64, importable without a GPU or the library; an empty denominator gives 0.0, never NaN.

A histogram is ``[..., bins, 3]`` integers {pixels, correct pixels, sum of q} per confidence bin, q = rint(65536 conf); the
meter keeps one per PREDICTED class.  Per bin: accuracy = correct / pixels, confidence = sum q / (65536 pixels), gap =
confidence - accuracy (positive: overconfident).  ECE = sum_b pixels_b / N |gap_b|, MCE = max_b |gap_b| over the bins that
hold a pixel.
"""
from __future__ import annotations

import math

import numpy as np

Q_ONE = 65536                                            # the fixed-point 1.0 of the histogram's sum of q
HEAD_KEYS = ("outc.conv.weight", "outc.conv.bias")       # the 1x1 head of UNet / SegmentationUNet


def _ratio(a, b):
    return float(a) / float(b) if b else 0.0


def reliability(hist):
    """{"pixels", "accuracy", "mean_confidence", "confidence_minus_accuracy", "ece", "mce", "bins": [{"lo", "hi", "count",
    "accuracy", "confidence", "gap"}]} of one histogram [bins, 3]."""
    h = np.asarray(hist, dtype=np.int64).reshape(-1, 3)
    bins = h.shape[0]
    n = int(h[:, 0].sum())
    rows, ece, mce = [], 0.0, 0.0
    for b in range(bins):
        count, correct, sq = (int(v) for v in h[b])
        acc, conf = _ratio(correct, count), _ratio(sq, Q_ONE * count)
        gap = conf - acc if count else 0.0
        rows.append({"lo": b / bins, "hi": (b + 1) / bins, "count": count, "accuracy": acc, "confidence": conf, "gap": gap})
        if count:
            ece += _ratio(count, n) * abs(gap)
            mce = max(mce, abs(gap))
    acc, conf = _ratio(int(h[:, 1].sum()), n), _ratio(int(h[:, 2].sum()), Q_ONE * n)
    return {"pixels": n, "accuracy": acc, "mean_confidence": conf, "confidence_minus_accuracy": conf - acc if n else 0.0,
            "ece": ece, "mce": mce, "bins": rows}


def calibration_summary(hist, class_names):
    """{"overall", "defects", "per_class": {name: ...}} of a histogram [num_classes, bins, 3] by predicted class: every
    pixel, the pixels predicted as a class other than 0 pooled, and each predicted class on its own (``reliability``)."""
    h = np.asarray(hist, dtype=np.int64)
    if h.ndim != 3 or h.shape[2] != 3 or h.shape[0] != len(class_names):
        raise ValueError(f"calibration_summary: a histogram [{len(class_names)}, bins, 3], got {h.shape}")
    return {"overall": reliability(h.sum(0)), "defects": reliability(h[1:].sum(0)),
            "per_class": {name: reliability(h[i]) for i, name in enumerate(class_names)}}


def temperature_grid(lo, hi, k):
    """k temperatures from lo to hi, evenly spaced in log T: T_i = lo (hi / lo)^(i / (k - 1)); the ends are exact."""
    lo, hi, k = float(lo), float(hi), int(k)
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo < hi):
        raise ValueError(f"temperature_grid: 0 < lo < hi, got {lo} and {hi}")
    if k < 2:
        raise ValueError(f"temperature_grid: at least 2 points, got {k}")
    return [lo if i == 0 else hi if i == k - 1 else lo * (hi / lo) ** (i / (k - 1)) for i in range(k)]


def fit_temperature(grid, nll):
    """The temperature that minimises ``nll`` over ``grid`` (increasing temperatures; nll any positive multiple of the
    negative log-likelihood at each): {"value", "at_edge", "index", "resolution"}.  ``index`` = the first argmin on the
    grid.  An interior argmin is refined to the vertex of the parabola through its three points in (log T, nll), clamped
    between the two neighbours (three collinear points: the grid point itself); at an end of the grid the value is that T
    and ``at_edge`` is True -- the minimum may lie outside the range.  ``resolution`` = the largest ratio of neighbouring
    grid temperatures: what the grid alone resolves."""
    t = np.asarray(grid, dtype=np.float64).reshape(-1)
    y = np.asarray(nll, dtype=np.float64).reshape(-1)
    if t.size < 1 or t.size != y.size:
        raise ValueError(f"fit_temperature: {t.size} temperatures for {y.size} values")
    if not (np.isfinite(t).all() and (t > 0).all() and (np.diff(t) > 0).all()):
        raise ValueError("fit_temperature: the grid must be finite, positive and increasing")
    if not np.isfinite(y).all():
        raise ValueError("fit_temperature: a non-finite negative log-likelihood")
    i = int(np.argmin(y))
    resolution = float((t[1:] / t[:-1]).max()) if t.size > 1 else 1.0
    if i == 0 or i == t.size - 1:
        return {"value": float(t[i]), "at_edge": True, "index": i, "resolution": resolution}
    x0, x1, x2 = (math.log(v) for v in t[i - 1:i + 2])
    y0, y1, y2 = (float(v) for v in y[i - 1:i + 2])
    a, b = (x1 - x0) * (y1 - y2), (x1 - x2) * (y1 - y0)
    den = a - b
    x = x1 if den == 0.0 else x1 - 0.5 * ((x1 - x0) * a - (x1 - x2) * b) / den
    x = min(max(x, x0), x2)
    return {"value": float(math.exp(x)), "at_edge": False, "index": i, "resolution": resolution}


def fold_temperature(state_dict, temperature):
    """A copy of a model state dict whose 1x1 head (``outc.conv.weight`` / ``outc.conv.bias``) is divided by T in float64
    and cast back to its dtype, so that the model's logits are z / T; every other tensor is the same object.  Exact up to
    the rounding of the scaled head to its dtype, and to what the forward pass makes of it (a bf16 model quantises the
    scaled weights anew)."""
    import torch
    t = float(temperature)
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError(f"fold_temperature: temperature {temperature!r} is not a finite value > 0")
    missing = [k for k in HEAD_KEYS if k not in state_dict]
    if missing:
        raise KeyError(f"fold_temperature: the state dict has no {missing} (a UNet / SegmentationUNet head)")
    out = dict(state_dict)
    for k in HEAD_KEYS:
        w = state_dict[k]
        out[k] = (w.detach().to(torch.float64) / t).to(w.dtype)
    return out


def calibrated_checkpoint(checkpoint, temperature, calibration):
    """A copy of a ``utils.save_checkpoint`` dict with ``fold_temperature`` applied to its ``model_state_dict`` and the
    keys ``temperature`` (float) and ``calibration`` (the summary after calibration, JSON-like) added;
    ``utils.load_checkpoint`` reads it as it is."""
    out = dict(checkpoint)
    out["model_state_dict"] = fold_temperature(checkpoint["model_state_dict"], temperature)
    out["temperature"] = float(temperature)
    out["calibration"] = calibration
    return out


def format_table(before, after, temperature, class_names):
    """The printed table: one row per group (overall, defects, each predicted class) before and after calibration."""
    lines = [f"{'group':<16}{'pixels':>12}{'accuracy':>10}{'conf':>9}{'ECE':>9}{'MCE':>9}   |"
             f"{'conf':>9}{'ECE':>9}{'MCE':>9}   (T = {temperature:.4f})"]
    groups = [("overall", before["overall"], after["overall"]), ("defects", before["defects"], after["defects"])]
    groups += [(name, before["per_class"][name], after["per_class"][name]) for name in class_names]
    for name, b, a in groups:
        lines.append(f"{name[:15]:<16}{b['pixels']:>12d}{b['accuracy']:>10.4f}{b['mean_confidence']:>9.4f}{b['ece']:>9.4f}"
                     f"{b['mce']:>9.4f}   |{a['mean_confidence']:>9.4f}{a['ece']:>9.4f}{a['mce']:>9.4f}")
    return "\n".join(lines)
