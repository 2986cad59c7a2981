"""GPU tests of the per-image evaluation statistics (csrc/segeval.hip through metrics.per_image_stats) against a NumPy
/ float64 restatement, and of the KolektorSDD trainer and the Gear / KolektorSDD evaluation CLIs end to end."""
import ctypes
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tiaozhanbei_unet_amd import _lib as L
from tiaozhanbei_unet_amd.metrics import SegmentationMetrics, per_image_stats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (c, n, h, w, quantised logits, ignore_index, with target)
CASES = [
    (2, 1, 37, 53, False, None, True),
    (3, 3, 37, 53, True, 255, True),
    (4, 8, 37, 53, False, None, False),
    (8, 3, 37, 53, True, None, True),
    (2, 8, 64, 64, True, 1, True),
    (3, 1, 64, 64, False, None, True),
    (4, 3, 64, 64, True, 255, True),
    (8, 8, 64, 64, False, 3, True),
    (3, 3, 64, 64, True, None, False),
    (3, 2, 1024, 512, False, None, True),
    (8, 2, 1024, 512, True, 255, True),
]
IDS = [f"c{c}-n{n}-{h}x{w}{'-ties' if q else ''}{'' if i is None else f'-ign{i}'}{'' if t else '-notarget'}"
       for c, n, h, w, q, i, t in CASES]


def _inputs(c, n, h, w, quantised, ignore, with_target, seed=0):
    rng = np.random.default_rng(seed + 97 * c + n + h)
    x = rng.standard_normal((n, c, h, w)).astype(np.float32) * 2.0
    if quantised:                                      # few levels: many pixels have tied maxima
        x = np.round(x).astype(np.float32)
    t = None
    if with_target:
        t = rng.integers(0, c, (n, h, w)).astype(np.int64)
        t[rng.random((n, h, w)) < 0.05] = -1           # out of range: skipped
        t[rng.random((n, h, w)) < 0.05] = c
        if ignore is not None:
            t[rng.random((n, h, w)) < 0.1] = ignore
    return x, t


def _restate(x, t, ignore):
    """labels (first maximum), per-image confusion counts, float64 mean / unbiased std of the max softmax probability"""
    n, c = x.shape[:2]
    labels = np.argmax(x, axis=1)                      # numpy: the first maximum
    z = x.astype(np.float64)
    pmax = 1.0 / np.exp(z - z.max(axis=1, keepdims=True)).sum(axis=1)
    flat = pmax.reshape(n, -1)
    mean, std = flat.mean(axis=1), flat.std(axis=1, ddof=1)
    cm = np.zeros((n, c, c), np.int64)
    if t is not None:
        for i in range(n):
            tt, pp = t[i].ravel(), labels[i].ravel()
            keep = (tt >= 0) & (tt < c)
            if ignore is not None:
                keep &= tt != ignore
            cm[i] = np.bincount(tt[keep] * c + pp[keep], minlength=c * c).reshape(c, c)
    return labels.astype(np.uint8), cm, mean, std


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_per_image_stats_match_restatement(case):
    c, n, h, w, quantised, ignore, with_target = case
    x, t = _inputs(*case)
    xd = torch.from_numpy(x).to(DEV)
    td = None if t is None else torch.from_numpy(t).to(DEV)
    got = per_image_stats(xd, td, ignore_index=ignore, labels=True)
    labels, cm, mean, std = _restate(x, t, ignore)

    assert got["labels"].dtype == torch.uint8 and tuple(got["labels"].shape) == (n, h, w)
    assert np.array_equal(got["labels"].cpu().numpy(), labels)
    metrics = SegmentationMetrics(c, ignore_index=ignore)
    assert torch.equal(got["labels"].long(), metrics.argmax(xd))
    if with_target:
        assert np.array_equal(got["confusion"].cpu().numpy(), cm)
        metrics.update(xd, td)
        assert np.array_equal(got["confusion"].sum(0).cpu().numpy(), metrics.confusion_matrix)
    else:
        assert got["confusion"] is None
    assert got["conf_mean"].dtype == torch.float64
    assert np.abs(got["conf_mean"].cpu().numpy() - mean).max() <= 4e-7
    assert np.abs(got["conf_std"].cpu().numpy() - std).max() <= 1e-6

    again = per_image_stats(xd, td, ignore_index=ignore, labels=True)
    for k in ("labels", "confusion", "conf_mean", "conf_std"):
        if got[k] is not None:                         # bitwise: the fp64 moments included
            assert got[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), k


MARGIN = 256    # bytes of sentinel on each side of every buffer (a multiple of 16: the vector path stays eligible)
SENTINEL = 0xA5


def _guarded(nbytes):
    buf = torch.full((nbytes + 2 * MARGIN,), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf, buf.data_ptr() + MARGIN


def _margins_intact(buf):
    return bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[-MARGIN:] == SENTINEL).all())


@pytest.mark.parametrize("case", [CASES[1], CASES[4], CASES[9]], ids=[IDS[1], IDS[4], IDS[9]])
def test_outputs_and_workspace_stay_in_bounds(case):
    c, n, h, w, quantised, ignore, with_target = case
    x, t = _inputs(*case)
    hw = h * w
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    lib = L.lib()
    need = lib.unet_seg_image_stats_workspace(n, c, hw)
    bufs = {k: _guarded(b) for k, b in (("labels", n * hw), ("confusion", n * c * c * 8), ("conf", n * 16), ("ws", need))}
    L.check(lib.unet_seg_image_stats(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(td.data_ptr()), n, c, hw,
                                     -1 if ignore is None else ignore, ctypes.c_void_p(bufs["labels"][1]),
                                     ctypes.c_void_p(bufs["confusion"][1]), ctypes.c_void_p(bufs["conf"][1]),
                                     ctypes.c_void_p(bufs["ws"][1]), need, None), "unet_seg_image_stats")
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert _margins_intact(buf), k
    labels, cm, mean, _std = _restate(x, t, ignore)
    assert np.array_equal(bufs["labels"][0][MARGIN:-MARGIN].cpu().numpy().reshape(n, h, w), labels)
    assert np.array_equal(bufs["confusion"][0][MARGIN:-MARGIN].view(torch.int64).cpu().numpy().reshape(n, c, c), cm)
    conf = bufs["conf"][0][MARGIN:-MARGIN].view(torch.float64).cpu().numpy().reshape(n, 2)
    assert np.abs(conf[:, 0] - mean).max() <= 4e-7


def test_unsupported_class_counts_are_errors():
    for c in (1, 9):
        x = torch.zeros((2, c, 8, 8), device=DEV)
        with pytest.raises(RuntimeError, match="2..8 classes"):
            per_image_stats(x, torch.zeros((2, 8, 8), dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------------------------------------ CLIs
def _run(module, *argv):
    res = subprocess.run([sys.executable, "-m", f"tiaozhanbei_unet_amd.{module}", *argv], cwd=ROOT, capture_output=True,
                         text=True, timeout=400)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    return res.stdout


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_train_kolektorsdd_cli_writes_reference_tree(tmp_path, precision):
    save = tmp_path / "out"
    out = _run("train_kolektorsdd", "--synthetic", "--epochs", "2", "--val_freq", "1", "--save_freq", "1",
               "--batch_size", "4", "--image_height", "64", "--image_width", "32", "--num_workers", "0",
               "--precision", precision, "--save_dir", str(save))
    assert "img/s" in out
    (exp,) = glob.glob(str(save / "kolektorsdd_seg_unet_*"))
    for sub in ("checkpoints", "results", "visualizations", "logs"):
        assert os.path.isdir(os.path.join(exp, sub))
    args = json.load(open(os.path.join(exp, "args.json")))
    assert args["precision"] == precision and args["class_weights"] == "1.0,50.0,50.0" and not args["sync_mask"]
    for e in (0, 1):
        assert os.path.exists(os.path.join(exp, "checkpoints", f"checkpoint_epoch_{e}.pth"))
    res = json.load(open(os.path.join(exp, "results", "training_results.json")))
    assert set(res) == {"train_losses", "val_losses", "best_val_miou", "total_epochs", "total_params", "num_classes",
                        "args"}
    assert len(res["train_losses"]) == 2 and len(res["val_losses"]) == 2 and res["num_classes"] == 3
    assert all(np.isfinite(res["train_losses"])) and all(np.isfinite(res["val_losses"]))


def _fresh_checkpoint(path, n_classes, seed=0):
    from tiaozhanbei_unet_amd import SegmentationUNet
    from tiaozhanbei_unet_amd.train_utils import get_optimizer
    from tiaozhanbei_unet_amd.utils import save_checkpoint
    torch.manual_seed(seed)
    model = SegmentationUNet(3, n_classes, precision="fp32").to(DEV)
    save_checkpoint(model, get_optimizer(model), 0, 0.0, str(path))
    return model


def _expected_confusion(model, batches, n_classes):
    model.eval()
    metrics = SegmentationMetrics(n_classes)
    with torch.no_grad():
        for x, m in batches:
            metrics.update(model(x), m)
    return metrics.confusion_matrix


EVAL_KEYS = {"evaluation_args", "overall_metrics", "per_class_metrics", "confusion_matrix"}
OVERALL_KEYS = {"pixel_accuracy", "mean_accuracy", "mean_iou", "mean_dice", "mean_precision", "mean_recall", "mean_f1"}


def _check_eval_outputs(save, n_samples, want_cm, class_names):
    res = json.load(open(save / "evaluation_results.json"))
    assert set(res) == EVAL_KEYS
    assert set(res["overall_metrics"]) == OVERALL_KEYS
    assert set(res["per_class_metrics"]) == {"iou", "dice", "precision", "recall", "f1"}
    assert np.array_equal(np.array(res["confusion_matrix"]), want_cm)
    per_image = json.load(open(save / "per_image_results.json"))
    assert len(per_image) == n_samples
    assert {"image_path", "accuracy", "confidence_mean", "confidence_std"} <= set(per_image[0])
    assert all(set(k[len("accuracy_"):] for k in e if k.startswith("accuracy_")) <= set(class_names) for e in per_image)
    return res, per_image


def test_eval_kolektorsdd_cli(tmp_path):
    from tiaozhanbei_unet_amd import kolektorsdd_dataset as K
    root = K.write_synthetic_kolektorsdd(str(tmp_path / "kol"), n_folders=6, per_folder=5)
    ckpt = tmp_path / "model.pth"
    model = _fresh_checkpoint(ckpt, 3)
    ds = K.KolektorSDDDataset(root, "test", (64, 32), raw=True)
    pre = K.GpuPreprocess((64, 32), train=False)
    samples = [ds[i] for i in range(len(ds))]
    batches = [pre(*K.collate_raw(samples[i:i + 2])[:2], device=DEV) for i in range(0, len(samples), 2)]
    want = _expected_confusion(model, batches, 3)
    assert want.sum() == len(ds) * 64 * 32

    save = tmp_path / "eval"
    argv = ["--checkpoint", str(ckpt), "--data_root", root, "--image_height", "64", "--image_width", "32",
            "--batch_size", "2", "--num_workers", "0", "--save_dir", str(save)]
    _run("eval_kolektorsdd", *argv)
    first = _check_eval_outputs(save, len(ds), want, K.CLASS_NAMES)
    assert first[1][0]["image_path"] == ds.image_paths[0]
    _run("eval_kolektorsdd", *argv)
    assert _check_eval_outputs(save, len(ds), want, K.CLASS_NAMES) == first


def test_eval_gear_cli_and_predictions(tmp_path):
    from tiaozhanbei_unet_amd import gear_dataset as G
    root = G.write_synthetic_gear(str(tmp_path / "gear"))
    ckpt = tmp_path / "model.pth"
    model = _fresh_checkpoint(ckpt, 4, seed=1)
    ds = G.GearDataset(root, "test", (64, 64), raw=True)
    pre = G.GearPreprocess((64, 64), train=False)
    samples = [ds[i] for i in range(len(ds))]
    batches = []
    for i in range(0, len(samples), 3):
        images, polys, sizes, _ = G.collate_raw(samples[i:i + 3])
        batches.append(pre(images, polys, sizes, device=DEV))
    want = _expected_confusion(model, batches, 4)

    save = tmp_path / "eval"
    argv = ["--checkpoint", str(ckpt), "--data_root", root, "--image_size", "64", "--batch_size", "3",
            "--num_workers", "0", "--save_dir", str(save)]
    _run("eval_gear", *argv)
    names = ["background"] + ds.class_names
    first = _check_eval_outputs(save, len(ds), want, names)
    _run("eval_gear", *argv)
    assert _check_eval_outputs(save, len(ds), want, names) == first

    pytest.importorskip("matplotlib")
    _run("eval_gear", *argv, "--save_predictions")
    expected = {"confusion_matrix.png"}
    for b in range(min(5, (len(ds) + 2) // 3)):
        for i, p in enumerate(ds.image_paths[3 * b:3 * b + 3][:4]):
            expected.add(f"prediction_batch{b}_img{i}_{os.path.basename(p).split('.')[0]}.png")
    assert {os.path.basename(p) for p in glob.glob(str(save / "*.png"))} == expected
    assert _check_eval_outputs(save, len(ds), want, names)[0]["confusion_matrix"] == first[0]["confusion_matrix"]
