"""Pixel AUROC / AUPRC on the device (ops.BinaryAUC -> csrc/rankauc.hip) against the float64 restatement of
tests/_rank_auc_ref.py (pinned to sklearn by test_cpu_rank_auc.py): sizes across the sort's tile and table
boundaries, tie-heavy and special scores, the label threshold, image selection, bitwise invariance to how the pixels
are batched, no host synchronisation in update, and the evaluation CLI's test_metrics.json."""
import json
import os

import numpy as np
import pytest
import torch

from _rank_auc_ref import rank_auc64

pytestmark = pytest.mark.gpu

TOL = 1e-12
FMAX = float(np.finfo(np.float32).max)


def _ops():
    from tiaozhanbei_unet_amd import ops
    return ops


def _device(scores, truth):
    return (torch.as_tensor(np.ascontiguousarray(scores, np.float32)).cuda(),
            torch.as_tensor(np.ascontiguousarray(truth, np.float32)).cuda())


def _auc(pred, truth, select=None):
    m = _ops().BinaryAUC()
    m.update(pred, truth, select=select)
    return m.compute()


def _expect(got, pred, truth, select=None):
    p, t = pred.cpu().numpy(), truth.cpu().numpy()
    if select is not None:
        sel = np.asarray(torch.as_tensor(select).cpu().numpy(), bool)
        p, t = p[sel], t[sel]
    want = rank_auc64(p, t > 0.5)
    for k in ("positives", "negatives", "nonfinite"):
        assert got[k] == want[k], (k, got, want)
    assert abs(got["auroc"] - want["auroc"]) <= TOL, (got, want)
    assert abs(got["auprc"] - want["auprc"]) <= TOL, (got, want)
    return want


def _make(shape, frac, kind, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    truth = (torch.rand(shape, generator=g, device="cuda") < frac).float()
    if kind == "continuous":
        pred = torch.randn(shape, generator=g, device="cuda") * 2.0 + 0.7 * truth
    else:
        q = 256.0 if kind == "q256" else 4096.0
        pred = torch.round((torch.rand(shape, generator=g, device="cuda") * 0.8 + 0.2 * truth) * q) / q
    return pred.contiguous(), truth.contiguous()


# totals across wave, block, tile (2048 keys) and digit-table boundaries; the shape picks the vector (per_image % 4
# == 0) or the scalar append path
SMALL = [(1,), (2,), (63,), (64,), (65,), (255,), (4, 64), (257,), (4095,), (4097,), (65537,)]
FRACS = [0.005, 0.05, 0.5]
KINDS = ["continuous", "q256", "q4096"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("shape", SMALL)
def test_small_totals(shape, frac, kind):
    pred, truth = _make(shape if len(shape) > 1 else (1,) + shape, frac, kind, seed=sum(shape) + int(frac * 1000))
    _expect(_auc(pred, truth), pred, truth)


@pytest.mark.parametrize("shape, frac, kind", [
    ((1, 1000003), 0.005, "continuous"), ((1, 1000003), 0.05, "q256"), ((1, 1000003), 0.5, "q4096"),
    ((100, 1, 256, 256), 0.05, "continuous"), ((100, 1, 256, 256), 0.005, "q4096"), ((100, 1, 256, 256), 0.5, "q256"),
    ((1, (1 << 25) + 1), 0.05, "q4096"),
])
def test_large_totals(shape, frac, kind):
    pred, truth = _make(shape, frac, kind, seed=shape[-1] % 1000)
    _expect(_auc(pred, truth), pred, truth)


def test_signed_zero_ties_negative_and_large_scores():
    rng = np.random.default_rng(1)
    pool = np.array([-0.0, 0.0, -3.5, 2.5, 1e3, -1e3, 1.0, 0.0], np.float32)
    s = pool[rng.integers(0, pool.size, (8, 1000))]
    y = (rng.random((8, 1000)) < 0.3).astype(np.float32)
    pred, truth = _device(s, y)
    got = _auc(pred, truth)
    _expect(got, pred, truth)
    plus = _auc(torch.where(pred == 0, torch.zeros_like(pred), pred), truth)
    assert (got["auroc"], got["auprc"]) == (plus["auroc"], plus["auprc"])       # -0.0 and +0.0 are one value


def test_subnormal_and_extreme_scores():
    rng = np.random.default_rng(2)
    pool = np.array([-FMAX, -1e-40, -1e-45, 0.0, 1e-45, 2e-45, 1e-40, np.finfo(np.float32).tiny, 0.5, FMAX,
                     np.nextafter(np.float32(FMAX), np.float32(0))], np.float32)
    s = pool[rng.integers(0, pool.size, (3, 4099))]
    y = (rng.random((3, 4099)) < 0.4).astype(np.float32)
    pred, truth = _device(s, y)
    _expect(_auc(pred, truth), pred, truth)


@pytest.mark.parametrize("n, n_pos", [(1000, 10), (4096, 2048), (70001, 1)])
def test_all_scores_equal(n, n_pos):
    y = np.zeros((1, n), np.float32)
    y[0, :n_pos] = 1
    pred, truth = _device(np.full((1, n), 0.375, np.float32), y)
    got = _auc(pred, truth)
    assert got["auroc"] == 0.5
    assert abs(got["auprc"] - (1 + n_pos / n) / 2) <= TOL


def test_perfect_and_inverted_separation():
    rng = np.random.default_rng(4)
    y = rng.random((5, 3000)) < 0.1
    s = np.where(y, 2.0 + rng.random(y.shape), rng.random(y.shape)).astype(np.float32)
    pred, truth = _device(s, y)
    got = _auc(pred, truth)
    assert got["auroc"] == 1.0 and abs(got["auprc"] - 1.0) <= TOL
    inv = _auc(-pred, truth)
    assert inv["auroc"] == 0.0
    _expect(inv, -pred, truth)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_scores_give_zero(bad):
    pred, truth = _make((4, 1000), 0.2, "continuous", seed=5)
    pred[2, 777] = bad
    got = _auc(pred, truth)
    assert (got["auroc"], got["auprc"]) == (0.0, 0.0) and got["nonfinite"] == 1
    assert got["positives"] + got["negatives"] == 3999


@pytest.mark.parametrize("label", [0.0, 1.0])
def test_single_class_gives_zero(label):
    pred, _ = _make((2, 500), 0.5, "continuous", seed=6)
    got = _auc(pred, torch.full_like(pred, label))
    assert (got["auroc"], got["auprc"]) == (0.0, 0.0)
    assert got["positives" if label else "negatives"] == 1000


def test_label_threshold_is_strictly_above_half():
    rng = np.random.default_rng(8)
    levels = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(1)), 1 / 255, 0.0, 1.0], np.float32)
    y = levels[rng.integers(0, levels.size, (2, 5000))]
    s = (rng.random((2, 5000)) + 0.3 * (y > 0.5)).astype(np.float32)
    pred, truth = _device(s, y)
    got = _auc(pred, truth)
    want = _expect(got, pred, truth)
    assert want["positives"] == int(np.sum(y > 0.5)) and int(np.sum(y == 0.5)) > 0


@pytest.mark.parametrize("where", ["host", "device"])
def test_select_masks_images_out(where):
    pred, truth = _make((9, 1, 32, 33), 0.1, "q256", seed=9)
    sel = np.array([1, 0, 0, 1, 1, 0, 1, 0, 1], bool)
    select = torch.as_tensor(sel).cuda() if where == "device" else sel
    got = _auc(pred, truth, select)
    _expect(got, pred, truth, sel)
    assert got["positives"] + got["negatives"] == 5 * 32 * 33
    none = _auc(pred, truth, np.zeros(9, bool))
    assert (none["auroc"], none["positives"], none["negatives"]) == (0.0, 0, 0)


def test_batch_split_and_order_are_bitwise_invariant():
    pred, truth = _make((21, 1, 64, 64), 0.05, "continuous", seed=10)
    pred[:, :, :8] = torch.round(pred[:, :, :8] * 16) / 16          # some ties too
    sel = np.random.default_rng(10).random(21) < 0.8
    results = []
    for parts in (1, 3, 7):
        order = np.random.default_rng(parts).permutation(21)
        cuts = np.sort(np.random.default_rng(parts + 100).choice(np.arange(1, 21), parts - 1, replace=False))
        m = _ops().BinaryAUC()
        for chunk in np.split(order, cuts):
            idx = torch.as_tensor(chunk).cuda()
            m.update(pred[idx], truth[idx], select=sel[chunk] if parts != 3 else torch.as_tensor(sel[chunk]).cuda())
        first, second = m.compute(), m.compute()
        assert first == second
        results.append(first)
    assert results[0] == results[1] == results[2]
    _expect(results[0], pred, truth, sel)


def test_update_does_not_synchronise():
    pred, truth = _make((6, 1, 48, 48), 0.1, "continuous", seed=11)
    m = _ops().BinaryAUC()
    sel_dev = torch.ones(6, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.update(pred, truth)
        m.update(pred, truth, select=np.array([1, 0, 1, 1, 0, 1], bool))
        m.update(pred, truth, select=sel_dev)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    got = m.compute()
    assert got["positives"] + got["negatives"] == (6 + 4 + 6) * 48 * 48


@pytest.mark.parametrize("model_name", ["anomaly_unet", "unet"])
def test_cli_pixel_metrics_carry_auroc_auprc(tmp_path, monkeypatch, model_name):
    """test.main on an MVTec-layout tree: every pixel entry of test_metrics.json has auroc / auprc, the same for every
    threshold, equal to the restatement over test_model's host anomaly maps and masks of the anomalous images.
    The reference's loader scales the {0, 1} masks by 1/255 (no pixel is > 0.5, so there are no pixel entries);
    the masks are scaled back to {0, 1} here so that the pixel path has both classes to rank."""
    from tiaozhanbei_unet_amd import AnomalyUNet, UNet
    from tiaozhanbei_unet_amd.augment import DeviceTransform
    quirk = DeviceTransform.masks
    monkeypatch.setattr(DeviceTransform, "masks", lambda self, m, device="cuda": quirk(self, m, device) * 255.0)
    from tiaozhanbei_unet_amd import test as test_cli
    from tiaozhanbei_unet_amd.dataset import get_dataloaders, write_synthetic_mvtec
    from tiaozhanbei_unet_amd.utils import load_checkpoint, save_checkpoint
    root = write_synthetic_mvtec(str(tmp_path / "data"), "bottle", n_train=2, n_good=3, n_bad=4, size=64)
    torch.manual_seed(0)
    model = (AnomalyUNet(3, False) if model_name == "anomaly_unet" else UNet(3, 1, False)).cuda()
    ck = str(tmp_path / "model.pth")
    save_checkpoint(model, torch.optim.Adam(model.parameters()), 0, 0.0, ck)
    thresholds = ["0.3", "0.5", "0.7"]
    out = test_cli.main(["--data_root", root, "--category", "bottle", "--model", model_name, "--checkpoint", ck,
                         "--batch_size", "3", "--image_size", "64", "--num_workers", "0", "--pixel_thresholds",
                         *thresholds, "--output_dir", str(tmp_path / "test_out")])
    tm = json.load(open(os.path.join(out, "test_metrics.json")))
    entries = list(tm["pixel_metrics"].values())
    assert len(entries) == len(thresholds)
    for e in entries:
        assert {"auroc", "auprc"} <= set(e)
        assert (e["auroc"], e["auprc"]) == (entries[0]["auroc"], entries[0]["auprc"])

    _, loader = get_dataloaders(root, "bottle", 3, 64, 0, device_preprocess=True)
    load_checkpoint(model, None, ck, torch.device("cuda"))
    res = test_cli.test_model(model, loader, torch.device("cuda"), pixel_thresholds=[0.3, 0.5, 0.7])
    bad = res["labels"] == 1
    want = rank_auc64(res["anomaly_maps"][bad], res["masks_true"][bad] > 0.5)
    assert want["positives"] > 0 and want["negatives"] > 0
    for got in (res["pixel_auc"], entries[0]):
        assert abs(got["auroc"] - want["auroc"]) <= TOL and abs(got["auprc"] - want["auprc"]) <= TOL
