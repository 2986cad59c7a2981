"""CPU checks of the defect-level region metrics: the scipy / numpy reference of the device kernels against maps whose
regions, sizes and hits are written out by hand, the host metric function (seg_regions.py) on hand-made records, the
flags of the eval_regions CLI, and the exports and host-side refusals of the new entry points."""
import ctypes
import json

import numpy as np
import pytest

import _seg_regions_ref as R
from tiaozhanbei_unet_amd import _lib, eval_regions, seg_regions


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_checkerboard_of_two_classes_is_two_regions():
    yy, xx = np.mgrid[0:4, 0:4]
    board = np.where((yy + xx) % 2 == 0, 1, 2).astype(np.uint8)[None]
    region, sizes, counts = R.class_regions64(board, 3)
    assert np.array_equal(region[0], np.where((yy + xx) % 2 == 0, 1, 2))     # roots: pixel 0 and pixel 1
    assert np.array_equal(sizes[0], np.full((4, 4), 8))
    assert counts.tolist() == [[0, 1, 1]]
    # the prediction swaps the classes: nothing agrees
    trec, prec = R.match_records(board, 3 - board, 3)
    assert trec.tolist() == [[0, 1, 0, 8, 0], [0, 2, 1, 8, 0]]
    assert prec.tolist() == [[0, 2, 0, 8, 0], [0, 1, 1, 8, 0]]
    trec, prec = R.match_records(board, board, 3, image_base=7)
    assert trec.tolist() == prec.tolist() == [[7, 1, 0, 8, 8], [7, 2, 1, 8, 8]]


TRUTH = np.array([[[1, 1, 2, 2, 0],
                   [1, 1, 2, 2, 0],
                   [0, 0, 0, 0, 3]]], np.uint8)
PRED = np.array([[[1, 1, 1, 2, 0],
                  [0, 1, 0, 2, 0],
                  [0, 0, 0, 0, 0]]], np.uint8)


def test_reference_touching_blobs_of_different_classes_stay_apart():
    region, sizes, counts = R.class_regions64(TRUTH, 4)
    assert region[0].tolist() == [[1, 1, 3, 3, 0], [1, 1, 3, 3, 0], [0, 0, 0, 0, 15]]
    assert sizes[0].tolist() == [[4, 4, 4, 4, 0], [4, 4, 4, 4, 0], [0, 0, 0, 0, 1]]
    assert counts.tolist() == [[0, 1, 1, 1]]
    region, sizes, counts = R.class_regions64(PRED, 4)
    assert region[0].tolist() == [[1, 1, 1, 4, 0], [0, 1, 0, 4, 0], [0, 0, 0, 0, 0]]
    assert sizes[0].tolist() == [[4, 4, 4, 2, 0], [0, 4, 0, 2, 0], [0, 0, 0, 0, 0]]
    assert counts.tolist() == [[0, 1, 1, 0]]


def test_reference_hits_and_the_min_pixels_convention():
    # agreeing pixels: (0,0) (0,1) (1,1) of class 1, (0,3) (1,3) of class 2
    trec, prec = R.match_records(TRUTH, PRED, 4)
    assert trec.tolist() == [[0, 1, 0, 4, 3], [0, 2, 2, 4, 2], [0, 3, 14, 1, 0]]
    assert prec.tolist() == [[0, 1, 0, 4, 3], [0, 2, 3, 2, 2]]
    # the predicted class-2 region has 2 pixels: kept at min_pixels = 2 (size >= min_pixels), dropped at 3, and then
    # it neither appears nor covers the truth region
    assert [a.tolist() for a in R.match_records(TRUTH, PRED, 4, 2)] == [trec.tolist(), prec.tolist()]
    trec, prec = R.match_records(TRUTH, PRED, 4, 3)
    assert trec.tolist() == [[0, 1, 0, 4, 3], [0, 2, 2, 4, 0], [0, 3, 14, 1, 0]]
    assert prec.tolist() == [[0, 1, 0, 4, 3]]
    assert R.match_records(TRUTH, PRED, 4, 4)[1].tolist() == [[0, 1, 0, 4, 3]]
    trec, prec = R.match_records(TRUTH, PRED, 4, 5)
    assert trec[:, 4].tolist() == [0, 0, 0] and prec.shape == (0, 5)


def test_reference_treats_255_and_classes_past_the_range_as_background():
    m = np.array([[[255, 1, 7], [1, 0, 3]]], np.uint8)
    region, sizes, counts = R.class_regions64(m, 3)
    assert region[0].tolist() == [[0, 2, 0], [2, 0, 0]] and sizes[0].tolist() == [[0, 2, 0], [2, 0, 0]]
    assert counts.tolist() == [[0, 1, 0]]
    trec, prec = R.match_records(m, m, 3)
    assert trec.tolist() == prec.tolist() == [[0, 1, 1, 2, 2]]
    region, _, counts = R.class_regions64(m, 4)                  # with 4 classes the 3 is a region of its own
    assert region[0].tolist() == [[0, 2, 0], [2, 0, 6]] and counts.tolist() == [[0, 1, 0, 1]]


# ------------------------------------------------------------------------------------------------ host metrics
T_REC = [(0, 1, 5, 10, 0), (0, 1, 50, 10, 2), (1, 2, 7, 4, 1), (1, 2, 30, 4, 2), (3, 1, 0, 8, 8)]
P_REC = [(0, 1, 48, 4, 2), (1, 2, 7, 6, 3), (2, 1, 9, 5, 0), (3, 1, 0, 20, 8)]
NAMES = ["background", "pit", "scrape"]


def _f1(p, r):
    return 2 * p * r / (p + r) if p + r else 0.0


def test_region_metrics_on_hand_made_records():
    res = seg_regions.region_metrics(T_REC, P_REC, 5, 3, (0, 0.25, 0.5), NAMES)
    assert res["images"] == 5 and list(res["thresholds"]) == ["0.0", "0.25", "0.5"]
    # images 0, 1, 3 are defective; 0, 1, 2, 3 are predicted defective; image 4 has nothing
    assert res["image_level"] == {"tp": 3, "fp": 1, "fn": 0, "tn": 1, "precision": 0.75, "recall": 1.0, "accuracy": 0.8}
    # t = 0: one common pixel is asked for, so the truth region with hit = 0 is not detected
    want = {"0.0": (4, 3), "0.25": (3, 3), "0.5": (2, 2)}
    for key, (det, mat) in want.items():
        o = res["thresholds"][key]["overall"]
        assert (o["truth_regions"], o["detected"], o["pred_regions"], o["matched"]) == (5, det, 4, mat), key
        assert o["region_recall"] == det / 5 and o["region_precision"] == mat / 4
        assert o["region_f1"] == _f1(mat / 4, det / 5)
        assert o["false_alarms_per_image"] == (4 - mat) / 5
    half = res["thresholds"]["0.5"]["per_class"]
    assert set(half) == {"pit", "scrape"}
    assert (half["pit"]["truth_regions"], half["pit"]["detected"], half["pit"]["pred_regions"],
            half["pit"]["matched"]) == (3, 1, 3, 1)
    assert (half["scrape"]["truth_regions"], half["scrape"]["detected"], half["scrape"]["pred_regions"],
            half["scrape"]["matched"]) == (2, 1, 1, 1)
    assert half["scrape"]["region_f1"] == _f1(1.0, 0.5) and half["scrape"]["false_alarms_per_image"] == 0.0
    assert half["pit"]["false_alarms_per_image"] == 2 / 5
    assert res["mean_coverage"]["overall"] == np.mean([0.0, 0.2, 0.25, 0.5, 1.0])
    assert res["mean_coverage"]["per_class"] == {"pit": np.mean([0.0, 0.2, 1.0]), "scrape": 0.375}


def test_coverage_rule_at_its_edges():
    rec = [(0, 1, 0, 4, 0), (0, 1, 9, 4, 1), (0, 1, 20, 3, 1), (0, 1, 30, 8, 2)]
    assert seg_regions.covered(rec, 0.0).tolist() == [False, True, True, True]
    assert seg_regions.covered(rec, 0.25).tolist() == [False, True, True, True]      # 1 >= 1.0, 1 >= 0.75, 2 >= 2.0
    assert seg_regions.covered(rec, 0.5).tolist() == [False, False, False, False]    # 1 < 2, 1 < 1.5, 2 < 4
    assert seg_regions.covered(rec, 1 / 3).tolist() == [False, False, True, False]   # float64: 1 >= (1 / 3) * 3


def test_empty_denominators_give_zero_not_nan():
    for images in (0, 2):
        res = seg_regions.region_metrics(np.zeros((0, 5), np.int32), [], images, 4, (0.0, 0.5))
        text = json.dumps(res)
        assert "NaN" not in text and "Infinity" not in text
        il = res["image_level"]
        assert (il["tp"], il["fp"], il["fn"], il["tn"]) == (0, 0, 0, images)
        assert il["precision"] == 0.0 and il["recall"] == 0.0 and il["accuracy"] == (1.0 if images else 0.0)
        for at in res["thresholds"].values():
            assert set(at["per_class"]) == {"class_1", "class_2", "class_3"}
            for f in [at["overall"], *at["per_class"].values()]:
                assert all(v == 0 for v in f.values())
        assert res["mean_coverage"]["overall"] == 0.0
    # truth regions but no prediction at all: recall 0, precision and F1 0.0 from empty denominators
    res = seg_regions.region_metrics(T_REC, [], 5, 3, (0.0,))
    o = res["thresholds"]["0.0"]["overall"]
    assert o["region_precision"] == 0.0 and o["region_f1"] == 0.0 and o["detected"] == 4
    assert res["image_level"]["fn"] == 3 and res["image_level"]["precision"] == 0.0


def test_region_entries_list_truth_regions_and_false_alarms():
    paths = [f"img{i}.png" for i in range(5)]
    entries = seg_regions.region_entries(T_REC, P_REC, paths, NAMES, 10, 0.5)
    assert len(entries) == 5 + 2
    assert entries[1] == {"kind": "truth", "image_path": "img0.png", "class": "pit", "y": 5, "x": 0, "size": 10,
                          "hit": 2, "coverage": 0.2}
    assert [(e["image_path"], e["size"]) for e in entries[5:]] == [("img2.png", 5), ("img3.png", 20)]
    assert all(e["kind"] == "false_alarm" for e in entries[5:])


# ------------------------------------------------------------------------------------------------ CLI flags
def test_eval_regions_flags():
    gear = vars(eval_regions.parse_args(["--dataset", "gear", "--checkpoint", "ckpt.pth"]))
    assert gear["min_region_pixels"] == 1 and gear["coverage_thresholds"] == [0.0, 0.25, 0.5]
    assert gear["data_root"] == "datasets/Gear" and gear["image_size"] == 512 and gear["precision"] == "fp32"
    assert set(gear) == {"dataset", "data_root", "image_size", "split", "model", "checkpoint", "bilinear", "dropout",
                         "batch_size", "num_workers", "device", "save_dir", "precision", "min_region_pixels",
                         "coverage_thresholds"}
    kol = vars(eval_regions.parse_args(["--dataset", "kolektorsdd", "--checkpoint", "ckpt.pth", "--min_region_pixels",
                                        "3", "--coverage_thresholds", "0.1", "0.9"]))
    assert kol["data_root"] == "datasets/KolektorSDD" and (kol["image_height"], kol["image_width"]) == (1024, 512)
    assert (kol["train_split"], kol["val_split"]) == (0.7, 0.15)
    assert kol["min_region_pixels"] == 3 and kol["coverage_thresholds"] == [0.1, 0.9]
    for argv in (["--checkpoint", "ckpt.pth"],                                   # --dataset is required
                 ["--dataset", "mvtec", "--checkpoint", "ckpt.pth"],
                 ["--dataset", "gear"],                                          # so is --checkpoint
                 ["--dataset", "gear", "--checkpoint", "c", "--min_region_pixels", "0"],
                 ["--dataset", "gear", "--checkpoint", "c", "--image_height", "64"]):      # a KolektorSDD flag
        with pytest.raises(SystemExit):
            eval_regions.parse_args(argv)


@pytest.mark.parametrize("dataset", ["gear", "kolektorsdd"])
def test_eval_regions_refuses_cpu(dataset):
    with pytest.raises(SystemExit) as e:
        eval_regions.main(["--dataset", dataset, "--device", "cpu", "--checkpoint", "ckpt.pth"])
    assert "no CPU path" in str(e.value)


# ------------------------------------------------------------------------------------------------ exports
NEW_SYMBOLS = ("unet_label_class_regions_workspace", "unet_label_class_regions", "unet_match_class_regions_workspace",
               "unet_match_class_regions")


def test_library_exports_class_regions():
    _lib.build(force=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)                # loading needs no GPU
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES, name


def test_unsupported_shapes_are_refused_on_the_host():
    """decided before anything reaches the device: the workspace queries return 0 and the entry points the
    unsupported status for C outside 2..255, 2^31 pixels or more, 65536 images or more"""
    lib = _lib.lib()
    assert lib.unet_label_class_regions_workspace(8, 1024, 512, 3) == 8 * 1024 * 512 * 4
    assert lib.unet_match_class_regions_workspace(8, 1024, 512, 3) == 8 * 1024 * 512 * 8
    assert lib.unet_label_class_regions_workspace(1, 1, 1, 2) == 16 and lib.unet_label_class_regions_workspace(1, 1, 1, 255)
    dummy = ctypes.c_void_p(16)                        # only checked for NULL: the shape is refused first
    bad = [(2, 64, 64, 1), (2, 64, 64, 256), (2, 64, 64, 0), (2, 32768, 32768, 3), (1, 1 << 16, 1 << 15, 3),
           (65536, 1, 1, 3)]
    for n, h, w, c in bad:
        assert lib.unet_label_class_regions_workspace(n, h, w, c) == 0, (n, h, w, c)
        assert lib.unet_match_class_regions_workspace(n, h, w, c) == 0, (n, h, w, c)
        rc = lib.unet_label_class_regions(dummy, n, h, w, c, dummy, dummy, dummy, dummy, 1 << 40, None)
        assert rc == -2, (n, h, w, c)
        assert b"2..255 classes" in lib.unet_last_error()
        rc = lib.unet_match_class_regions(dummy, dummy, dummy, dummy, dummy, dummy, n, h, w, c, 1, 0, dummy, dummy, 16,
                                          dummy, dummy, 1 << 40, None)
        assert rc == -2, (n, h, w, c)
    # the largest frame that is supported is one pixel short of 2^31
    assert lib.unet_label_class_regions_workspace(1, 1, (1 << 31) - 1, 3) > 0
    # bad arguments are told apart from unsupported shapes
    assert lib.unet_match_class_regions(dummy, dummy, dummy, dummy, dummy, dummy, 2, 8, 8, 3, 0, 0, dummy, dummy, 16,
                                        dummy, dummy, 1 << 40, None) == -1
    assert lib.unet_label_class_regions(None, 2, 8, 8, 3, dummy, dummy, dummy, dummy, 1 << 40, None) == -1
