"""CPU checks of the pixel AUROC / AUPRC feature (ops.BinaryAUC, csrc/rankauc.hip): the float64 restatement the GPU
tests compare against is pinned to sklearn here; the C-ABI is exported, sizes its workspace and refuses bad arguments
and oversize inputs before anything reaches a device; the evaluation CLI's pixel entries carry auroc / auprc."""
import ctypes

import numpy as np
import pytest

from _rank_auc_ref import rank_auc64
from tiaozhanbei_unet_amd import _lib

NAMES = ("unet_rank_auc_append", "unet_rank_auc_workspace", "unet_rank_auc")


def _sklearn(scores, positive):
    metrics = pytest.importorskip("sklearn.metrics")
    y = np.asarray(positive, dtype=int).ravel()
    s = np.asarray(scores, dtype=np.float32).ravel()
    p, r, _ = metrics.precision_recall_curve(y, s)
    return metrics.roc_auc_score(y, s), metrics.auc(r, p)


def _data(seed, n, frac, kind):
    rng = np.random.default_rng(seed)
    y = rng.random(n) < frac
    s = rng.standard_normal(n) * 2.0 + 0.8 * y
    if kind == "q256":
        s = np.round(s * 256) / 256
    elif kind == "q4096":
        s = np.round(s * 4096) / 4096
    elif kind == "coarse":
        s = np.round(s * 2) / 2
    return s.astype(np.float32), y


@pytest.mark.parametrize("kind", ["continuous", "q256", "q4096", "coarse"])
@pytest.mark.parametrize("n, frac", [(2, 0.5), (65, 0.05), (4097, 0.5), (200003, 0.005), (300000, 0.05)])
def test_restatement_matches_sklearn(n, frac, kind):
    s, y = _data(n, n, frac, kind)
    if y.all() or not y.any():
        y[0], y[-1] = True, False
    got = rank_auc64(s, y)
    roc, pr = _sklearn(s, y)
    assert abs(got["auroc"] - roc) <= 1e-12 and abs(got["auprc"] - pr) <= 1e-12, (got, roc, pr)
    assert got["positives"] == int(y.sum()) and got["negatives"] == n - int(y.sum())


def test_restatement_special_values_match_sklearn():
    rng = np.random.default_rng(7)
    pool = np.array([-np.finfo(np.float32).max, -1e3, -1.0, -1e-40, -1e-45, -0.0, 0.0, 1e-45, 1e-40,
                     np.finfo(np.float32).tiny, 0.5, 1.0, 7.0, np.finfo(np.float32).max], np.float32)
    s = pool[rng.integers(0, pool.size, 5000)]
    y = rng.random(5000) < 0.3
    got = rank_auc64(s, y)
    roc, pr = _sklearn(s, y)
    assert abs(got["auroc"] - roc) <= 1e-12 and abs(got["auprc"] - pr) <= 1e-12
    # -0.0 and +0.0 are one value
    flipped = np.where(s == 0, np.float32(0.0), s)
    assert rank_auc64(flipped, y) == got


def test_restatement_degenerate_cases():
    y = np.array([0, 1, 0, 1], bool)
    s = np.array([0.1, 0.9, 0.2, 0.8], np.float32)
    assert rank_auc64(s, y)["auroc"] == 1.0 and rank_auc64(s, y)["auprc"] == 1.0
    assert rank_auc64(-s, y)["auroc"] == 0.0
    eq = rank_auc64(np.full(10, 0.25, np.float32), np.arange(10) < 3)
    assert eq["auroc"] == 0.5 and abs(eq["auprc"] - (1 + 3 / 10) / 2) <= 1e-15
    for bad in (np.nan, np.inf, -np.inf):
        r = rank_auc64(np.r_[s, np.float32(bad)], np.r_[y, False])
        assert (r["auroc"], r["auprc"], r["nonfinite"]) == (0.0, 0.0, 1)
    one = rank_auc64(s, np.ones(4, bool))
    assert (one["auroc"], one["auprc"], one["negatives"]) == (0.0, 0.0, 0)


def test_rank_auc_symbols_declared_and_exported():
    _lib.build(force=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)                # loading needs no GPU
    for name in NAMES:
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES, name


def test_workspace_query():
    lib = _lib.lib()
    small = lib.unet_rank_auc_workspace(10, 20)
    assert small >= 4 * 30 and small % 16 == 0
    big = lib.unet_rank_auc_workspace(1 << 20, 5 << 20)
    assert big >= 4 * (6 << 20) and big > small
    assert lib.unet_rank_auc_workspace(1 << 30, (1 << 31) - (1 << 30) - 1) > 0      # P + N = 2^31 - 1: supported
    assert lib.unet_rank_auc_workspace(1 << 30, 1 << 30) == 0                        # P + N = 2^31: refused
    assert lib.unet_rank_auc_workspace(-1, 5) == 0


def test_abi_refuses_null_pointers_and_oversize_inputs_on_the_host():
    """decided before any launch: no device needed"""
    lib = _lib.lib()
    dummy = ctypes.c_void_p(256)                       # only checked for NULL / alignment: refused first
    assert lib.unet_rank_auc_append(None, dummy, None, 1, 64, dummy, 64, dummy, None) == -1
    assert lib.unet_rank_auc_append(dummy, dummy, None, 1, 64, dummy, 64, None, None) == -1
    assert lib.unet_rank_auc_append(dummy, dummy, None, 0, 64, dummy, 64, dummy, None) == -1
    assert lib.unet_rank_auc(dummy, 4, dummy, 4, None, dummy, 1 << 20, None) == -1
    assert lib.unet_rank_auc(None, 4, dummy, 4, dummy, dummy, 1 << 20, None) == -1
    assert lib.unet_rank_auc(dummy, 1 << 30, dummy, 1 << 30, dummy, dummy, 1 << 40, None) == -2
    assert b"2^31" in lib.unet_last_error()
    assert lib.unet_rank_auc(dummy, 4, dummy, 4, dummy, dummy, 16, None) == -3       # workspace too small


def _results(rng, with_counts):
    n, hw = 6, 16 * 16
    labels = np.array([0, 1, 1, 0, 1, 0])
    masks = (rng.random((n, 1, 16, 16)) < 0.2).astype(np.float32) * labels[:, None, None, None]
    amaps = np.clip(rng.random((n, 1, 16, 16)) * 0.7 + 0.3 * masks, 0, 1).astype(np.float32)
    res = {"labels": labels, "predictions": labels.copy(), "image_scores": rng.random(n),
           "anomaly_maps": amaps, "masks_true": masks, "anomaly_types": ["good", "x", "x", "good", "y", "good"]}
    bad = labels == 1
    ref = rank_auc64(amaps[bad], masks[bad] > 0.5)
    if with_counts:
        truth = masks[bad] > 0.5
        res["pixel_counts"] = {}
        for t in (0.3, 0.5, 0.7):
            pred = amaps[bad] > t
            res["pixel_counts"][t] = [int((pred & truth).sum()), int((pred & ~truth).sum()),
                                      int((~pred & truth).sum()), int((~pred & ~truth).sum())]
        res["pixel_auc"] = ref
    assert hw and ref["positives"] > 0
    return res, ref


@pytest.mark.parametrize("device_counts", [True, False])
def test_evaluate_results_pixel_entries_carry_auroc_auprc(device_counts):
    """both branches of evaluate_results give the reference's seven keys per threshold (src/utils.py:84-91)"""
    pytest.importorskip("sklearn.metrics")
    from tiaozhanbei_unet_amd.test import evaluate_results
    res, ref = _results(np.random.default_rng(3), device_counts)
    ev = evaluate_results(res, [0.3, 0.5, 0.7])
    assert len(ev["pixel_metrics"]) == 3
    for entry in ev["pixel_metrics"].values():
        assert list(entry) == ["accuracy", "precision", "recall", "specificity", "f1_score", "auroc", "auprc"]
        assert abs(entry["auroc"] - ref["auroc"]) <= 1e-12 and abs(entry["auprc"] - ref["auprc"]) <= 1e-12
