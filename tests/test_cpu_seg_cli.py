"""CPU checks of the KolektorSDD trainer and the Gear / KolektorSDD evaluation CLIs: their flags against the
reference's (pinned as data), the refusal of a CPU device, the exports of the per-image statistics kernel, and the host
helper that turns one image's counts into the reference's ``compute_prediction_stats`` dict; and the refusals that the
tools over a checkpoint take from ``seg_cli``."""
import ctypes

import numpy as np
import pytest
import torch

from tiaozhanbei_unet_amd import (_lib, eval_boundaries, eval_calibration, eval_detection, eval_gear, eval_kolektorsdd,
                                 eval_views, predict, predict_tiled, predict_views, seg_cli, train_kolektorsdd)
from tiaozhanbei_unet_amd.metrics import image_prediction_stats

REFERENCE_KOLEKTOR_TRAIN_FLAGS = {  # reference train_kolektorsdd.py:26-101, pinned here as data
    "data_root": "datasets/KolektorSDD", "image_height": 1024, "image_width": 512, "model": "seg_unet",
    "bilinear": False, "dropout": 0.1, "train_split": 0.7, "val_split": 0.15, "epochs": 50, "batch_size": 8,
    "learning_rate": 1e-3, "weight_decay": 1e-4, "optimizer": "adam", "ce_weight": 1.0, "dice_weight": 1.0,
    "focal_weight": 0.0, "class_weights": "1.0,50.0,50.0", "num_workers": 4, "device": "auto", "seed": 42,
    "save_dir": "outputs", "save_freq": 10, "resume": None, "val_freq": 5, "debug": False, "debug_samples": 20,
}
_EVAL_COMMON = {  # reference test.py:20-64 and test_kolektorsdd.py:20-72 (--checkpoint is required in both)
    "split": "test", "model": "seg_unet", "bilinear": False, "dropout": 0.1, "batch_size": 8, "num_workers": 4,
    "device": "auto", "save_dir": "test_results", "save_predictions": False, "save_confusion_matrix": False,
    "debug": False, "debug_samples": 50,
}
REFERENCE_GEAR_EVAL_FLAGS = {"data_root": "datasets/Gear", "image_size": 512, **_EVAL_COMMON}
REFERENCE_KOLEKTOR_EVAL_FLAGS = {"data_root": "datasets/KolektorSDD", "image_height": 1024, "image_width": 512,
                                 "train_split": 0.7, "val_split": 0.15, **_EVAL_COMMON}


def test_train_kolektorsdd_flags_match_reference():
    args = vars(train_kolektorsdd.parse_args([]))
    for k, v in REFERENCE_KOLEKTOR_TRAIN_FLAGS.items():
        assert args[k] == v, k
    assert set(args) - set(REFERENCE_KOLEKTOR_TRAIN_FLAGS) == {"precision", "synthetic", "sync_mask"}
    assert args["precision"] == "fp32" and not args["synthetic"] and not args["sync_mask"]
    choices = {name: kw.get("choices") for name, kw in train_kolektorsdd.FLAGS}
    assert choices["--model"] == ["unet", "seg_unet"] and choices["--optimizer"] == ["adam", "adamw", "sgd"]


@pytest.mark.parametrize("cli, reference", [(eval_gear, REFERENCE_GEAR_EVAL_FLAGS),
                                            (eval_kolektorsdd, REFERENCE_KOLEKTOR_EVAL_FLAGS)])
def test_eval_flags_match_reference(cli, reference):
    args = vars(cli.parse_args(["--checkpoint", "ckpt.pth"]))
    for k, v in reference.items():
        assert args[k] == v, k
    assert set(args) - set(reference) == {"checkpoint", "precision"} and args["precision"] == "fp32"
    choices = {name: kw.get("choices") for name, kw in cli.FLAGS}
    assert choices["--split"] == ["test", "val"] and choices["--model"] == ["unet", "seg_unet"]
    with pytest.raises(SystemExit):                    # --checkpoint is required, as in the reference
        cli.parse_args([])


@pytest.mark.parametrize("main, argv", [(train_kolektorsdd.main, []),
                                        (eval_gear.main, ["--checkpoint", "ckpt.pth"]),
                                        (eval_kolektorsdd.main, ["--checkpoint", "ckpt.pth"])])
def test_seg_clis_refuse_cpu(main, argv):
    with pytest.raises(SystemExit) as e:
        main(["--device", "cpu"] + argv)
    assert "no CPU path" in str(e.value)


TILED_TOOLS = [eval_detection, eval_boundaries, eval_calibration, eval_views]


@pytest.mark.parametrize("tool", TILED_TOOLS, ids=[t.__name__.rsplit(".", 1)[1] for t in TILED_TOOLS])
def test_shared_tiling_refusals(tool, capsys):
    """the tiling flags are seg_cli's, object for object, and so are their rules; eval_views is always tiled"""
    gear = ["--dataset", "gear", "--checkpoint", "c.pth"]
    always_tiled = tool is eval_views
    tiled = [] if always_tiled else ["--tiled"]
    for dataset in (("gear",) if always_tiled else seg_cli.DATASETS):
        flags = dict(tool.flags_of(dataset))
        assert all(flags[name] is kw for name, kw in seg_cli.TILING_FLAGS)
    assert [name for name, _ in seg_cli.TILING_FLAGS] == ["--tiled", "--tile", "--min_overlap"]
    args = tool.parse_args(gear + tiled + ["--tile", "64", "64", "--min_overlap", "63"])
    assert (args.tiled, args.tile, args.min_overlap) == (True, [64, 64], 63)
    for bad, said in ((gear + ["--tile", "0", "64"], "--tile sides must be positive"),
                      (gear + tiled + ["--tile", "0", "64"], "--tile sides must be positive"),
                      (gear + tiled + ["--tile", "64", "64", "--min_overlap", "64"], "smaller than both tile sides"),
                      (gear + tiled + ["--tile", "64", "32", "--min_overlap", "32"], "smaller than both tile sides"),
                      (gear + tiled + ["--min_overlap", "-1"], "--min_overlap must be at least 0")):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)
        assert said in capsys.readouterr().err, bad
    if always_tiled:
        return
    args = tool.parse_args(gear + ["--min_overlap", "512"])        # the overlap binds only where tiles are cut
    assert (args.tiled, args.tile, args.min_overlap) == (False, [512, 512], 512)
    with pytest.raises(SystemExit):
        tool.parse_args(["--dataset", "kolektorsdd", "--checkpoint", "c.pth", "--tiled"])
    assert "--tiled needs --dataset gear" in capsys.readouterr().err
    assert tool.parse_args(["--dataset", "kolektorsdd", "--checkpoint", "c.pth"]).tile == [1024, 512]


PREDICT_TOOLS = [predict, predict_tiled, predict_views]


@pytest.mark.parametrize("tool", PREDICT_TOOLS, ids=[t.__name__.rsplit(".", 1)[1] for t in PREDICT_TOOLS])
@pytest.mark.parametrize("extra, said", [(["--batch_size", "0"], "--batch_size must be at least 1"),
                                         (["--min_region_pixels", "0"], "--min_region_pixels must be at least 1"),
                                         (["--min_confidence", "1.5"], "--min_confidence must lie in 0..1"),
                                         (["--min_confidence", "-0.1"], "--min_confidence must lie in 0..1")])
def test_shared_predict_refusals(tool, extra, said, capsys):
    base = ["--task", "gear", "--checkpoint", "c.pth", "--input", "photos"]
    args = tool.parse_args(base + ["--batch_size", "1", "--min_region_pixels", "1", "--min_confidence", "1"])
    assert (args.batch_size, args.min_region_pixels, args.min_confidence) == (1, 1, 1.0)
    with pytest.raises(SystemExit):
        tool.parse_args(base + extra)
    assert said in capsys.readouterr().err


def test_library_exports_per_image_stats():
    _lib.build(force=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)                # loading needs no GPU
    for name in ("unet_seg_image_stats", "unet_seg_image_stats_workspace"):
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES, name


def test_workspace_query_and_class_range_on_the_host():
    """both are decided before anything reaches the device: C outside 2..8 is an error, not a launch"""
    lib = _lib.lib()
    assert lib.unet_seg_image_stats_workspace(8, 3, 1024 * 512) > 0
    assert lib.unet_seg_image_stats_workspace(8, 9, 1024) == 0 and lib.unet_seg_image_stats_workspace(8, 1, 1024) == 0
    dummy = ctypes.c_void_p(16)                        # only checked for NULL: the shape is refused first
    for c in (1, 9):
        rc = lib.unet_seg_image_stats(dummy, None, 2, c, 64, -1, None, None, dummy, dummy, 1 << 20, None)
        assert rc == -2, c
        assert b"2..8 classes" in lib.unet_last_error()


def _reference_prediction_stats(pred_logits, gt_mask, class_names):
    """reference visualize.py:239-257 compute_prediction_stats, restated in torch on the CPU"""
    pred_probs = torch.softmax(pred_logits, dim=0)
    pred_mask = torch.argmax(pred_logits, dim=0)
    stats = {"accuracy": (pred_mask == gt_mask).float().mean().item(),
             "confidence_mean": pred_probs.max(dim=0)[0].mean().item(),
             "confidence_std": pred_probs.max(dim=0)[0].std().item()}
    for i, name in enumerate(class_names):
        m = gt_mask == i
        if m.sum() > 0:
            stats[f"accuracy_{name}"] = (pred_mask[m] == i).float().mean().item()
    return stats


@pytest.mark.parametrize("seed, c, h, w", [(0, 2, 7, 9), (1, 3, 16, 8), (2, 4, 5, 31), (3, 8, 12, 12), (4, 3, 1, 2)])
def test_host_stats_helper_matches_reference(seed, c, h, w):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((c, h, w), generator=g) * 3
    gt = torch.randint(0, c, (h, w), generator=g)
    gt[gt == c - 1] = 0 if seed % 2 else c - 1          # some cases leave a class out of the truth
    names = [f"class{i}" for i in range(c)]
    want = _reference_prediction_stats(logits, gt, names)

    # what per_image_stats computes on the device: counts, then the float64 max-probability moments
    pred = torch.argmax(logits, dim=0)
    cm = np.zeros((c, c), np.int64)
    np.add.at(cm, (gt.numpy().ravel(), pred.numpy().ravel()), 1)
    pmax = torch.softmax(logits.double(), dim=0).max(dim=0)[0]
    got = image_prediction_stats(cm, float(pmax.mean()), float(pmax.std()), names)
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-6, abs=1e-6), k
