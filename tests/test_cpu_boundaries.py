"""CPU checks of the boundary distance transform and the outline statistics: the numpy restatement of csrc/distance.hip
against scipy's exact distance transform and a brute-force minimum, hand-drawn maps with their records written out, the
exports and host-side refusals of the new entry points, seg_boundaries.py on hand-built records, and the eval_boundaries
CLI's flags."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import _boundary_ref as B
from tiaozhanbei_unet_amd import _lib, eval_boundaries, eval_detection, eval_regions, evaluation, ops, seg_boundaries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("unet_boundary_distance_sq_workspace", "unet_boundary_distance_sq", "unet_boundary_stats")
F = B.F


# ------------------------------------------------------------------------------------------------ the restatement
def _masks(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    sparse = np.zeros((h, w), bool)
    sparse[rng.integers(0, h), rng.integers(0, w)] = True
    return {"random": rng.random((h, w)) < 0.3, "sparse": sparse, "one in the corner": (yy == h - 1) & (xx == 0),
            "disc": (yy - 0.4 * h) ** 2 + (xx - 0.6 * w) ** 2 <= (0.3 * max(h, w)) ** 2}


@pytest.mark.parametrize("h, w", [(1, 1), (1, 70), (70, 1), (33, 31), (65, 33)], ids=lambda v: str(v))
def test_distance_equals_scipy_and_brute_force(h, w):
    for name, b in _masks(h, w, seed=h * 131 + w).items():
        got = B.distance_sq(b)
        assert got.dtype == np.int64 and np.array_equal(got, B.distance_sq_brute(b)), name
        if b.any():
            assert np.array_equal(got, np.rint(ndimage.distance_transform_edt(~b) ** 2).astype(np.int64)), name
    assert bool((B.distance_sq(np.zeros((h, w), bool)) == B.NONE).all())


def test_distance_at_the_widest_frame_with_one_pixel_in_a_corner():
    b = np.zeros((2, 4096), bool)
    b[1, 4095] = True
    got = B.distance_sq(b)
    xs = np.arange(4096, dtype=np.int64)
    assert np.array_equal(got, np.stack([(4095 - xs) ** 2 + 1, (4095 - xs) ** 2]))
    assert np.array_equal(got, np.rint(ndimage.distance_transform_edt(~b) ** 2).astype(np.int64))
    assert np.array_equal(got, B.distance_sq_brute(b))
    assert int(got.max()) == 4095 ** 2 + 1 < 2 ** 26 and B.NONE + 4095 ** 2 < 2 ** 31


def test_boundary_masks_by_hand():
    m = np.array([[1, 1, 1, 0],
                  [1, 1, 1, 0],
                  [1, 1, 1, 0]], bool)
    assert B.boundary_mask(m).astype(int).tolist() == [[0, 0, 1, 0]] * 3      # the frame edge makes no boundary
    assert not B.boundary_mask(np.ones((3, 4), bool)).any()                    # a full frame has none
    assert not B.boundary_mask(np.zeros((3, 4), bool)).any()
    assert B.boundary_mask(np.array([[0, 1, 0]], bool)).tolist() == [[False, True, False]]
    ring = np.ones((5, 5), bool)
    ring[2, 2] = False
    assert B.boundary_mask(ring).astype(int).tolist() == [[0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 1, 0, 1, 0],
                                                          [0, 0, 1, 0, 0], [0, 0, 0, 0, 0]]


def _row(image, cls, **kw):
    r = [0] * len(B.FIELDS)
    r[F["image"]], r[F["class"]] = image, cls
    for k, v in kw.items():
        r[F[k]] = v
    return r


def test_records_by_hand():
    truth = np.array([[[1, 1, 1, 0, 0, 0],
                       [1, 1, 1, 0, 0, 0],
                       [1, 1, 1, 0, 2, 2]]], np.uint8)
    pred = np.array([[[1, 1, 1, 1, 0, 0],
                      [1, 1, 1, 1, 0, 0],
                      [1, 1, 1, 1, 0, 0]]], np.uint8)
    # class 1 touches the frame on three sides: its only boundary is the column x = 2 (truth) / x = 3 (prediction), one
    # pixel apart everywhere.  Class 2: the truth's two pixels are both boundary pixels, the prediction has none.
    d2 = B.boundary_distance_sq(truth, 3)
    assert d2[0, 0].tolist() == [[4, 1, 0, 1, 4, 9]] * 3
    assert d2[0, 1].tolist() == [[20, 13, 8, 5, 4, 4], [17, 10, 5, 2, 1, 1], [16, 9, 4, 1, 0, 0]]
    assert bool((B.boundary_distance_sq(pred, 3)[0, 1] == B.NONE).all())
    rec, hist = B.stats(truth, pred, 3, (0, 1), band=1, image_base=4)
    # band 1: truth columns 1..2, prediction columns 2..3 of class 1: intersection column 2, union columns 1..3
    want1 = _row(4, 1, t_pixels=9, p_pixels=12, t_boundary=3, p_boundary=3, p_near0=0, p_near1=3, t_near0=0, t_near1=3,
                 band_inter=3, band_union=9, p_dist_sum_q8=3 * 256, t_dist_sum_q8=3 * 256, p_dist_max_sq=1, t_dist_max_sq=1)
    want2 = _row(4, 2, t_pixels=2, t_boundary=2, band_union=2)             # nothing to measure against: unmatched
    assert rec.tolist() == [want1, want2]
    assert hist.sum() == 6 and hist[0, 0, 1] == 3 and hist[0, 1, 1] == 3
    # a class that covers the whole frame has no boundary: BOUNDARY_NONE, and nothing but its pixel counts
    full = np.full((1, 3, 4), 2, np.uint8)
    assert bool((B.boundary_distance_sq(full, 3) == B.NONE).all())
    rec, hist = B.stats(full, full, 3, (0,), band=2)
    assert rec.tolist() == [_row(0, 1), _row(0, 2, t_pixels=12, p_pixels=12)] and hist.sum() == 0
    # identical maps: every distance 0
    rec, hist = B.stats(truth, truth, 3, (0, 3), band=2)
    assert rec[0].tolist() == _row(0, 1, t_pixels=9, p_pixels=9, t_boundary=3, p_boundary=3, p_near0=3, p_near1=3,
                                   t_near0=3, t_near1=3, band_inter=9, band_union=9)
    assert hist[:, :, 0].tolist() == [[3, 3], [2, 2]] and hist.sum() == 10
    # values >= num_classes and 255 are background; dist_q8 is floor(256 sqrt(d2))
    odd = np.array([[[1, 0, 0, 7, 255, 0]]], np.uint8)
    far = np.array([[[0, 0, 255, 1, 3, 0]]], np.uint8)
    rec, _ = B.stats(odd, far, 3, (2, 3), band=1)
    assert rec[0].tolist() == _row(0, 1, t_pixels=1, p_pixels=1, t_boundary=1, p_boundary=1, p_near1=1, t_near1=1,
                                   band_union=2, p_dist_sum_q8=768, t_dist_sum_q8=768, p_dist_max_sq=9, t_dist_max_sq=9)
    assert math.isqrt(2 << 16) == 362 == int(256 * math.sqrt(2))
    assert B.band_width(1080, 1920) == 44 and B.band_width(1, 1) == 1 and B.band_width(64, 64) == 2


# ------------------------------------------------------------------------------------------------ exports
def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    _lib.build(force=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)                # loading needs no GPU
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name), name
    assert handle.unet_abi_version() == 1
    makefile = open(os.path.join(ROOT, "tiaozhanbei_unet_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bdistance\.hip\b", makefile, re.M)
    assert ops.boundary_distance_sq is evaluation.boundary_distance_sq
    assert ops.BoundaryMatcher is evaluation.BoundaryMatcher
    assert ops.BOUNDARY_NONE is evaluation.BOUNDARY_NONE == 1 << 30 == B.NONE
    assert ops.BOUNDARY_FIELDS is evaluation.BOUNDARY_FIELDS == B.FIELDS == seg_boundaries.FIELDS
    assert len(evaluation.BOUNDARY_FIELDS) == 20 and "#define UNET_BOUNDARY_FIELDS 20" in header
    assert "#define UNET_BOUNDARY_NONE (1 << 30)" in header


def test_workspace_query_and_refusals_on_the_host():
    """decided before anything reaches the device"""
    lib = _lib.lib()
    query = lib.unet_boundary_distance_sq_workspace
    assert query(3, 8, 8, 4) == 48 and query(1, 1, 1, 2) == 16 and query(1, 4096, 4096, 32) == 128
    dummy = ctypes.c_void_p(16)                        # only checked for NULL and alignment: refused before any use
    tol = (ctypes.c_int32 * 2)(1, 4)
    distance = lambda n, h, w, c, ws=1 << 20: lib.unet_boundary_distance_sq(dummy, n, h, w, c, dummy, dummy, ws, None)  # noqa: E731
    stats = lambda n, h, w, c, k=2, band=4, base=0, t=tol: lib.unet_boundary_stats(  # noqa: E731
        dummy, dummy, dummy, dummy, n, h, w, c, t, k, band, base, dummy, dummy, None)
    unsupported = [(1, 4097, 8, 4), (1, 8, 4097, 4), (1, 8, 8, 1), (1, 8, 8, 33), (65536, 1, 1, 2),
                   (128, 4096, 4096, 2), (8, 4096, 4096, 17)]              # the last two: 2^31 distances
    for n, h, w, c in unsupported:
        assert query(n, h, w, c) == 0, (n, h, w, c)
        assert distance(n, h, w, c) == -2, (n, h, w, c)
        text = lib.unet_last_error()
        assert text.startswith(b"unet_boundary_distance_sq: n=%d h=%d w=%d num_classes=%d" % (n, h, w, c)) and b"2^31" in text
        assert stats(n, h, w, c) == -2, (n, h, w, c)
        assert lib.unet_last_error().startswith(b"unet_boundary_stats: n=%d h=%d w=%d num_classes=%d" % (n, h, w, c))
    assert query(127, 4096, 4096, 2) == 127 * 4 + 4 and query(65535, 1, 1, 2) > 0      # the largest that are taken
    assert stats(2, 8, 8, 4, base=(1 << 31) - 2) == -2 and b"image indices" in lib.unet_last_error()
    assert distance(0, 8, 8, 4) == -1 and distance(2, 0, 8, 4) == -1 and distance(2, 8, -1, 4) == -1
    assert distance(2, 8, 8, 4, ws=8) == -3 and b"workspace too small" in lib.unet_last_error()
    assert lib.unet_boundary_distance_sq(None, 2, 8, 8, 4, dummy, dummy, 1 << 20, None) == -1
    assert lib.unet_boundary_distance_sq(dummy, 2, 8, 8, 4, dummy, ctypes.c_void_p(18), 1 << 20, None) == -1
    assert stats(2, 8, 8, 4, k=5) == -1 and b"at most 4" in lib.unet_last_error()
    assert stats(2, 8, 8, 4, k=-1) == -1 and stats(2, 8, 8, 4, band=-1) == -1 and stats(2, 8, 8, 4, band=1 << 30) == -1
    assert stats(2, 8, 8, 4, t=(ctypes.c_int32 * 2)(1, -4)) == -1 and b"tol_sq[1]=-4" in lib.unet_last_error()
    assert stats(2, 8, 8, 4, base=-1) == -1 and stats(0, 8, 8, 4) == -1 and stats(2, 8, 8, 4, t=None) == -1
    assert lib.unet_boundary_stats(dummy, None, dummy, dummy, 2, 8, 8, 4, tol, 2, 4, 0, dummy, dummy, None) == -1


def test_matcher_refuses_bad_arguments_before_anything_is_launched():
    for bad in (dict(num_classes=1), dict(num_classes=33), dict(num_classes=4, tolerances=()),
                dict(num_classes=4, tolerances=(1, 2, 3, 4, 5)), dict(num_classes=4, tolerances=(-1,)),
                dict(num_classes=4, tolerances=(1.5,)), dict(num_classes=4, band_width=-2),
                dict(num_classes=4, tolerances=(5000,)), dict(num_classes=4, tolerances=(True,))):
        with pytest.raises(ValueError, match="BoundaryMatcher"):
            evaluation.BoundaryMatcher(**bad)
    m = evaluation.BoundaryMatcher(4, (0, 3), 5)
    assert (m.tolerances, m.band_width, list(m._tol_sq), m.images) == ((0, 3), 5, [0, 9], 0)
    got = m.compute()
    assert got["records"].shape == (0, 20) and got["hist"].shape == (3, 2, 1025) and got["images"] == 0
    assert evaluation.boundary_band_width(1080, 1920) == 44 == B.band_width(1080, 1920)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        import torch
        evaluation.boundary_distance_sq(torch.zeros((1, 4, 4), dtype=torch.uint8), 4)


# ------------------------------------------------------------------------------------------------ seg_boundaries
def test_seg_boundaries_by_hand():
    rec = np.array([
        _row(0, 1, t_pixels=50, p_pixels=40, t_boundary=10, p_boundary=8, p_near0=4, p_near1=8, t_near0=5, t_near1=9,
             band_inter=12, band_union=24, p_dist_sum_q8=8 * 128, t_dist_sum_q8=10 * 256, p_dist_max_sq=4, t_dist_max_sq=9),
        _row(0, 2, t_pixels=7, t_boundary=6, band_union=7),                          # the truth alone has an outline
        _row(1, 1, t_pixels=30, p_pixels=30, t_boundary=10, p_boundary=12, p_near0=12, p_near1=12, t_near0=10, t_near1=10,
             band_inter=20, band_union=20, p_dist_max_sq=0, t_dist_max_sq=0),
        _row(1, 2, p_pixels=5, p_boundary=5, band_union=5),                          # the prediction alone
        _row(2, 1), _row(2, 2)], np.int64)
    hist = np.zeros((2, 2, 1025), np.int64)
    hist[0, 0, 0], hist[0, 0, 1], hist[0, 1, 0], hist[0, 1, 2], hist[0, 1, 1024] = 16, 4, 15, 4, 1
    names = ["bg", "a", "b"]
    res = seg_boundaries.boundary_results(rec, hist, 3, 3, (1, 2), names)
    assert res["images"] == 3 and res["tolerances"] == [1, 2] and set(res["per_class"]) == {"a", "b"}
    o = res["overall"]
    assert (o["records"], o["truth_boundary"], o["pred_boundary"], o["truth_pixels"], o["pred_pixels"]) == (6, 26, 25, 87, 75)
    at1, at2 = o["tolerances"]["1"], o["tolerances"]["2"]
    assert at1["boundary_precision"] == 16 / 25 and at1["boundary_recall"] == 15 / 26      # the one-sided pixels count
    assert at1["boundary_f1"] == 2 * (16 / 25) * (15 / 26) / (16 / 25 + 15 / 26)
    assert (at2["pred_near"], at2["truth_near"]) == (20, 19)
    assert o["boundary_iou"] == 32 / 56 and (o["band_inter"], o["band_union"]) == (32, 56)
    assert (o["matched_pred_boundary"], o["matched_truth_boundary"]) == (20, 20)
    assert o["mean_dist_pred_to_truth"] == 4.0 / 20 and o["mean_dist_truth_to_pred"] == 10.0 / 20
    assert o["assd"] == 14.0 / 40
    assert (o["hausdorff_pairs"], o["hausdorff_mean"], o["hausdorff_max"]) == (2, 1.5, 3.0)
    assert (o["dist_p50_pred_to_truth"], o["dist_p95_pred_to_truth"]) == (0, 1)
    assert (o["dist_p50_truth_to_pred"], o["dist_p95_truth_to_pred"]) == (0, 2)
    b = res["per_class"]["b"]
    assert b["tolerances"]["1"] == {"pred_near": 0, "truth_near": 0, "boundary_precision": 0.0, "boundary_recall": 0.0,
                                    "boundary_f1": 0.0}
    assert b["hausdorff_pairs"] == 0 and b["assd"] == 0.0 and b["dist_p50_pred_to_truth"] is None
    assert b["boundary_iou"] == 0.0 and b["band_union"] == 12
    assert res["per_class"]["a"]["tolerances"]["1"]["boundary_precision"] == 16 / 20
    assert res["unmatched"]["overall"] == {"truth_only": {"records": 1, "boundary_pixels": 6},
                                           "pred_only": {"records": 1, "boundary_pixels": 5}}
    assert res["unmatched"]["per_class"]["a"] == {"truth_only": {"records": 0, "boundary_pixels": 0},
                                                  "pred_only": {"records": 0, "boundary_pixels": 0}}
    # the last bin is open and percentiles are whole pixels
    assert seg_boundaries.percentile_bin(hist[0, 1], 1.0) == 1024 and seg_boundaries.percentile_bin(hist[0, 1], 0.75) == 0
    assert seg_boundaries.percentile_bin(hist[0, 1], 0.76) == 2 and seg_boundaries.percentile_bin(hist[1, 0], 0.5) is None
    table = seg_boundaries.format_table(res, names)
    assert "Images: 3" in table and "F1@2" in table and len(table.splitlines()) == 2 + 3
    entries = seg_boundaries.image_entries(rec, ["x.png", "y.png", "z.png"], names, (1, 2), [3, 3, 7])
    assert [e["image_path"] for e in entries] == ["x.png", "y.png", "z.png"] and [e["band_width"] for e in entries] == [3, 3, 7]
    assert set(entries[0]["classes"]) == {"a", "b"} and entries[2]["classes"] == {}
    assert entries[0]["classes"]["a"]["hausdorff"] == 3.0 and entries[0]["classes"]["b"]["hausdorff"] is None
    assert entries[1]["classes"]["a"]["tolerances"]["1"]["boundary_f1"] == 1.0
    assert entries[1]["classes"]["b"]["pred_boundary"] == 5


def test_seg_boundaries_on_an_empty_record_set():
    res = seg_boundaries.boundary_results(np.zeros((0, 20), np.int64), np.zeros((2, 2, 1025), np.int64), 0, 3, (1,), None)
    o = res["overall"]
    assert o["records"] == 0 and o["boundary_iou"] == 0.0 and o["assd"] == 0.0 and o["hausdorff_mean"] == 0.0
    assert o["tolerances"]["1"]["boundary_f1"] == 0.0 and o["dist_p95_truth_to_pred"] is None
    assert set(res["per_class"]) == {"class_1", "class_2"}
    assert res["unmatched"]["overall"]["truth_only"] == {"records": 0, "boundary_pixels": 0}
    assert "Images: 0" in seg_boundaries.format_table(res, ["bg", "class_1", "class_2"])
    assert seg_boundaries.image_entries(np.zeros((0, 20), np.int64), [], ["bg"], (1,), []) == []
    doc = seg_boundaries.__doc__
    assert "erosion" in doc and "frame edge is no boundary" in doc and "WHOLE pixels" in doc and "open" in doc


# ------------------------------------------------------------------------------------------------ CLI
def test_parse_args_defaults_and_refusals(capsys):
    args = eval_boundaries.parse_args(["--dataset", "gear", "--checkpoint", "m.pth"])
    assert (args.boundary_tolerances, args.boundary_width, args.tiled, args.tile, args.min_overlap) == \
        ([1, 2, 4], 0, False, [512, 512], 64)
    args = eval_boundaries.parse_args(["--dataset", "kolektorsdd", "--checkpoint", "m.pth", "--boundary_tolerances", "0",
                                       "3", "--boundary_width", "5"])
    assert (args.tile, args.boundary_tolerances, args.boundary_width) == ([1024, 512], [0, 3], 5)
    args = eval_boundaries.parse_args(["--dataset", "gear", "--checkpoint", "m.pth", "--tiled", "--tile", "64", "96",
                                       "--min_overlap", "8"])
    assert (args.tiled, args.tile, args.min_overlap) == (True, [64, 96], 8)
    for dataset in eval_regions.DATASETS:
        names = [n for n, _ in eval_boundaries.flags_of(dataset)]
        shared = [n for n, _ in eval_regions.flags_of(dataset) if n not in ("--min_region_pixels", "--coverage_thresholds")]
        assert names == shared + ["--tiled", "--tile", "--min_overlap", "--boundary_tolerances", "--boundary_width"]
        tile_flags = {n: kw for n, kw in eval_detection.flags_of(dataset)}
        assert all(kw is tile_flags[n] for n, kw in eval_boundaries.flags_of(dataset) if n in ("--tiled", "--tile", "--min_overlap"))
    base = ["--dataset", "gear", "--checkpoint", "m.pth"]
    for bad in (["--dataset", "kolektorsdd", "--checkpoint", "m.pth", "--tiled"],
                base + ["--boundary_tolerances", "1", "2", "3", "4", "5"],
                base + ["--boundary_tolerances", "-1"],
                base + ["--boundary_tolerances", "1.5"],
                base + ["--boundary_width", "-1"],
                base + ["--tiled", "--tile", "64", "64", "--min_overlap", "64"],
                base + ["--min_overlap", "-1"],
                base + ["--tile", "0", "64"],
                base + ["--min_region_pixels", "2"]):
        with pytest.raises(SystemExit):
            eval_boundaries.parse_args(bad)
    err = capsys.readouterr().err
    assert "full-resolution" in err and "1 to 4 values" in err and "--boundary_width must lie" in err


def test_eval_boundaries_refuses_cpu():
    with pytest.raises(SystemExit) as e:
        eval_boundaries.main(["--dataset", "gear", "--checkpoint", "m.pth", "--device", "cpu"])
    assert "no CPU path" in str(e.value)
