"""CPU checks of the shape records and their host geometry: the exports and host-side refusals of the new entry points,
the numpy reference of the device kernel (tests/_shapes_ref.py) against identities that hold for any mask and against
scipy, ``defects.shape_measures`` on closed forms, ``defects.defect_entries`` with and without shapes, and the flags."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import _defects_ref as D
import _shapes_ref as S
from tiaozhanbei_unet_amd import _lib, defects, evaluation, ops, predict, predict_tiled, predict_views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("unet_measure_class_regions_workspace", "unet_measure_class_regions")


# ------------------------------------------------------------------------------------------------ exports
def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    _lib.build(force=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)                # loading needs no GPU
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name), name
    assert ops.measure_class_regions is evaluation.measure_class_regions
    assert ops.SHAPE_FIELDS is evaluation.SHAPE_FIELDS and len(ops.SHAPE_FIELDS) == S.HEAD + 64
    assert ops.SHAPE_FIELDS[:S.HEAD] == ("image", "root", "size", "sum_xx", "sum_yy", "sum_xy", "q1", "q2", "qd", "q3", "q4")
    assert ops.SHAPE_FIELDS[S.HEAD] == "pmin_0" and ops.SHAPE_FIELDS[-1] == "pmax_31"
    assert len(ops.shape_fields(2)) == S.HEAD + 4
    for d in (2, 16, 32):                              # Python owns the table; the reference restates it
        table = defects.direction_table(d)
        assert table.dtype == np.int32 and np.array_equal(table, S.directions(d))
    assert defects.direction_table(32)[0].tolist() == [16384, 0] and defects.direction_table(32)[16].tolist() == [0, 16384]
    for d in (1, 3, 34, 0):
        with pytest.raises(ValueError):
            defects.direction_table(d)


def test_workspace_query_and_refusals_on_the_host():
    """decided before anything reaches the device: the workspace query returns 0 and the entry point the unsupported
    status for a side of 16385 and 1, 3 or 34 directions; a null pointer is a bad argument, a short workspace its own"""
    lib = _lib.lib()
    assert lib.unet_measure_class_regions_workspace(8, 512, 512, 32) == 8 * 512 * 512 * 4
    assert lib.unet_measure_class_regions_workspace(1, 1, 1, 2) == 16
    assert lib.unet_measure_class_regions_workspace(1, 16384, 16384, 32) > 0
    dummy = ctypes.c_void_p(16)                        # only checked for NULL: the shape is refused first
    table = np.ascontiguousarray(S.directions(32), np.int32)
    tp = ctypes.c_void_p(table.ctypes.data)

    def call(n=2, h=8, w=8, d=32, region=dummy, tab=tp, ws=1 << 40, min_pixels=1, base=0, cap=16):
        return lib.unet_measure_class_regions(region, dummy, n, h, w, min_pixels, base, tab, d, dummy, cap, dummy, dummy, ws,
                                              None)

    for n, h, w, d in [(1, 16385, 8, 32), (1, 8, 16385, 32), (2, 8, 8, 1), (2, 8, 8, 3), (2, 8, 8, 34), (2, 8, 8, 0),
                       (65536, 1, 1, 32), (8, 16384, 16384, 32)]:
        assert lib.unet_measure_class_regions_workspace(n, h, w, d) == 0, (n, h, w, d)
        assert call(n, h, w, d) == -2, (n, h, w, d)
        assert b"2..32 directions" in lib.unet_last_error()
    assert call(region=None) == -1 and b"null pointer" in lib.unet_last_error()
    assert call(tab=None) == -1
    assert call(ws=2 * 8 * 8 * 4 - 1) == -3 and b"workspace too small" in lib.unet_last_error()
    assert call(min_pixels=0) == -1 and call(base=-1) == -1 and call(cap=-1) == -1
    assert call(base=(1 << 31) - 2) == -2 and call(cap=1 << 31) == -2
    wide = table.copy()
    wide[5, 1] = 16385                                 # |p| < 2^30 rests on the components
    assert call(tab=ctypes.c_void_p(wide.ctypes.data)) == -1 and b"direction 5" in lib.unet_last_error()


# ------------------------------------------------------------------------------------------------ the reference
def _holes(mask):
    """enclosed 4-connected components of the background"""
    lab, k = ndimage.label(~np.pad(mask, 1))           # the ring joins everything that reaches the frame
    return k - 1


def _crack_edges(mask):
    p = np.pad(mask, 1)
    return int((p[1:] != p[:-1]).sum() + (p[:, 1:] != p[:, :-1]).sum())


def test_reference_satisfies_the_quad_identities_on_random_masks():
    rng = np.random.default_rng(11)
    seen = 0
    for trial in range(120):
        h, w = rng.integers(1, 13, 2)
        maps = (rng.random((1, h, w)) < rng.choice([0.3, 0.5, 0.7, 0.95])).astype(np.uint8)
        region, _, _ = S.class_regions64(maps, 2)
        for r in S.shape_records(maps, 2, D=2).tolist():
            size, (q1, q2, qd, q3, q4) = r[2], r[6:11]
            mask = region[0] == r[1] + 1
            assert (q1 + 2 * q2 + 2 * qd + 3 * q3 + 4 * q4) == 4 * size
            assert (q1 - q3 - 2 * qd) % 4 == 0 and 1 - (q1 - q3 - 2 * qd) // 4 == _holes(mask)
            assert q1 + q2 + q3 + 2 * qd == _crack_edges(mask)
            seen += 1
    assert seen > 200


def test_reference_against_records_written_out_by_hand():
    #            a 3 x 2 block of class 1 and, apart from it, a diagonal pair of class 2
    maps = np.array([[[1, 1, 1, 0, 0],
                      [1, 1, 1, 0, 2],
                      [0, 0, 0, 2, 0]]], np.uint8)
    rec = S.shape_records(maps, 3, D=2, image_base=4)
    #                  image root size xx yy xy q1 q2 qd q3 q4  pmin(x) pmin(y)  pmax(x)    pmax(y)
    assert rec.tolist() == [[4, 0, 6, 10, 3, 3, 4, 6, 0, 0, 2, 0, 0, 2 * 16384, 16384],
                            [4, 9, 2, 25, 5, 10, 6, 0, 1, 0, 0, 3 * 16384, 16384, 4 * 16384, 2 * 16384]]
    assert S.shape_records(maps, 3, D=2, min_pixels=3)[:, 1].tolist() == [0]
    assert S.shape_records(maps, 2, D=2)[:, 1].tolist() == [0]            # with 2 classes the 2s are background
    assert S.shape_records(np.zeros((2, 3, 3), np.uint8), 3, D=4).shape == (0, S.HEAD + 8)


# ------------------------------------------------------------------------------------------------ host geometry
def _records_of(mask, directions=32):
    """(shape record, describe record) of a one-region boolean mask, from the two references"""
    maps = np.asarray(mask, np.uint8)[None]
    (shape,), (rec,) = S.shape_records(maps, 2, D=directions), D.describe_records(maps, 2)
    return shape, rec


def _measure(mask, original=None, pixel_size=None, directions=32):
    shape, rec = _records_of(mask, directions)
    return defects.shape_measures(shape, directions, mask.shape, original or mask.shape, pixel_size, defect_record=rec)


@pytest.mark.parametrize("a, b", [(20, 5), (7, 7), (31, 1)])
def test_rectangle_in_closed_form(a, b):
    mask = np.zeros((40, 50), bool)
    mask[9:9 + b, 13:13 + a] = True
    m = _measure(mask)
    assert m["area"] == a * b and m["area_original"] == a * b
    assert m["major_axis"] == pytest.approx(4 * math.sqrt(a * a / 12), rel=1e-12)
    assert m["minor_axis"] == pytest.approx(4 * math.sqrt(b * b / 12), rel=1e-12)
    if a != b:
        assert abs(m["orientation_deg"]) < 1e-9
        assert m["eccentricity"] == pytest.approx(math.sqrt(1 - b * b / (a * a)), rel=1e-12)
    assert m["feret_width"] == b                       # direction 16 is (0, 16384): exact
    diagonal = math.hypot(a, b)
    assert math.cos(math.pi / 64) * diagonal * (1 - 1e-12) <= m["feret_length"] <= diagonal * (1 + 1e-4)
    if a != b:                                         # the sampled direction next to the diagonal's
        assert abs(m["feret_angle_deg"] - math.degrees(math.atan2(b, a))) <= 180 / 32 + 1e-9
    assert m["perimeter_crack"] == 2 * (a + b) and m["euler_number"] == 1 and m["holes"] == 0
    assert m["perimeter"] == pytest.approx(2 * (a - 1) + 2 * (b - 1) + 4 / math.sqrt(2), rel=1e-12)
    assert m["perimeter_original"] == m["perimeter"]
    assert m["circularity"] == pytest.approx(4 * math.pi * a * b / m["perimeter"] ** 2, rel=1e-12)
    assert not [k for k in m if k.endswith("_mm") or k.endswith("_mm2")]


def test_vertical_and_diagonal_orientation():
    mask = np.zeros((40, 40), bool)
    mask[5:35, 20:23] = True                           # a vertical bar: 90 degrees
    assert abs(_measure(mask)["orientation_deg"]) == pytest.approx(90)
    mask = np.eye(30, dtype=bool)                      # x to the right, y down: the main diagonal is +45 degrees
    m = _measure(mask)
    assert m["orientation_deg"] == pytest.approx(45) and m["feret_angle_deg"] == pytest.approx(45)
    assert m["feret_length"] == pytest.approx(30 * math.sqrt(2), rel=1e-4)   # 29 sqrt 2 between centres + one pixel diagonal
    assert m["holes"] == 0 and m["euler_number"] == 1
    assert _measure(mask[:, ::-1])["orientation_deg"] == pytest.approx(-45)


def test_ring_has_one_hole():
    yy, xx = np.mgrid[0:41, 0:41]
    r2 = (yy - 20) ** 2 + (xx - 20) ** 2
    m = _measure((r2 <= 18 ** 2) & (r2 >= 10 ** 2))
    assert m["holes"] == 1 and m["euler_number"] == 0
    # centres at most 36 apart, plus a pixel's own extent along the direction (1 .. sqrt 2); along every direction a
    # lattice point lies within sqrt 2 of the circle's point, on the inside
    assert 37 <= m["feret_length"] <= 36 + math.sqrt(2)
    assert 2 * (18 - math.sqrt(2)) + 1 <= m["feret_width"] <= m["feret_length"]
    assert m["eccentricity"] < 1e-6
    two = np.ones((9, 9), bool)
    two[2, 2] = two[5:7, 5:7] = False
    assert _measure(two)["holes"] == 2


def test_anisotropic_frame_scales_lengths_by_axis():
    """a 64 x 64 frame of a 96 x 160 image: sx = 2.5, sy = 1.5"""
    horizontal, vertical = np.zeros((64, 64), bool), np.zeros((64, 64), bool)
    horizontal[30, 10:50] = True
    vertical[10:50, 30] = True
    mh, mv = _measure(horizontal, (96, 160)), _measure(vertical, (96, 160))
    assert mh["area_original"] == mv["area_original"] == 40 * 2.5 * 1.5
    # the exact diagonal of the scaled bar; sampling loses at most cos(pi / 64), the rounded table a little more
    for m, length, width in ((mh, 40 * 2.5, 1.5), (mv, 40 * 1.5, 2.5)):
        assert math.hypot(length, width) * math.cos(math.pi / 64) * (1 - 1e-4) <= m["feret_length"] <= math.hypot(length, width) * (1 + 1e-4)
        assert m["feret_width"] == width
        assert m["major_axis"] == pytest.approx(4 * math.sqrt(length * length / 12), rel=1e-12)
        assert m["minor_axis"] == pytest.approx(4 * math.sqrt(width * width / 12), rel=1e-12)
        assert m["perimeter_original"] is None and m["perimeter"] > 0
    assert abs(mh["orientation_deg"]) < 1e-9 and abs(mv["orientation_deg"]) == pytest.approx(90)
    # the same squeeze on both axes keeps the perimeter
    assert _measure(horizontal, (128, 128))["perimeter_original"] == 2 * _measure(horizontal)["perimeter"]


def test_millimetre_fields_follow_the_pixel_size():
    mask = np.zeros((64, 64), bool)
    mask[20:30, 10:40] = True
    px, mm = _measure(mask, (128, 128)), _measure(mask, (128, 128), pixel_size=0.05)
    for key in ("feret_length", "feret_width", "major_axis", "minor_axis", "perimeter_original"):
        assert mm[key] == px[key] and mm[key + "_mm"] == px[key] * 0.05
    assert mm["area_mm2"] == px["area_original"] * 0.05 * 0.05 and px["area_original"] == 1200
    assert set(mm) - set(px) == {"feret_length_mm", "feret_width_mm", "major_axis_mm", "minor_axis_mm",
                                 "perimeter_original_mm", "area_mm2"}
    assert _measure(mask, (96, 160), pixel_size=0.05)["perimeter_original_mm"] is None


def test_shape_measures_refuses_records_that_do_not_belong_together():
    mask = np.zeros((8, 8), bool)
    mask[2:4, 2:6] = True
    shape, rec = _records_of(mask)
    with pytest.raises(ValueError):
        defects.shape_measures(shape, 32, (8, 8), (8, 8))                 # no describe record: no centroid
    with pytest.raises(ValueError):
        defects.shape_measures(shape, 16, (8, 8), (8, 8), defect_record=rec)
    other = rec.copy()
    other[3] += 1
    with pytest.raises(ValueError):
        defects.shape_measures(shape, 32, (8, 8), (8, 8), defect_record=other)
    same = defects.shape_measures(shape, defects.direction_table(32), (8, 8), (8, 8), defect_record=rec)
    assert same == defects.shape_measures(shape, 32, (8, 8), (8, 8), defect_record=rec)


# ------------------------------------------------------------------------------------------------ defect_entries
NAMES = ["background", "pitting", "spalling", "scrape"]


def _scene():
    maps = np.zeros((1, 64, 64), np.uint8)
    maps[0, 10:12, 5:45] = 3                           # a scrape 40 long
    maps[0, 40:43, 40:43] = 1                          # a pit of 9 pixels
    conf = np.full(maps.shape, 0.75, np.float32)
    return D.describe_records(maps, 4, conf), S.shape_records(maps, 4)


def test_defect_entries_without_shapes_is_as_before_and_size_rules_uncount():
    rec, shapes = _scene()
    (plain,) = defects.defect_entries(rec, NAMES, (64, 64), [(64, 64)])
    assert [set(d) for d in plain["defects"]] == [{"class", "class_name", "pixels", "bbox", "bbox_original", "centroid",
                                                   "centroid_original", "mean_confidence", "peak_confidence",
                                                   "counted"}] * 2
    assert plain == defects.defect_entries(rec, NAMES, (64, 64), [(64, 64)], 0.0, None, None, None)[0]
    (shaped,) = defects.defect_entries(rec, NAMES, (64, 64), [(64, 64)], shapes=shapes[::-1])      # any order
    for d, p in zip(shaped["defects"], plain["defects"]):
        assert {k: v for k, v in d.items() if k != "shape"} == p and d["shape"]["area"] == d["pixels"]
    assert shaped["defects"][0]["shape"]["feret_width"] == 2 and shaped["defects"][1]["shape"]["feret_width"] == 3
    assert shaped["decision"] == "reject"
    rules = defects.size_rules(None, min_defect_length=10)
    assert rules == {"units": {"length": "pixel", "area": "pixel2"}, "pixel_size": None, "min_defect_length": 10.0,
                     "min_defect_area": 0.0}
    (ruled,) = defects.defect_entries(rec, NAMES, (64, 64), [(64, 64)], shapes=shapes, rules=rules)
    assert [d["counted"] for d in ruled["defects"]] == [True, False] and ruled["decision"] == "reject"
    (ruled,) = defects.defect_entries(rec, NAMES, (64, 64), [(64, 64)], shapes=shapes,
                                      rules=defects.size_rules(None, min_defect_area=81))
    assert [d["counted"] for d in ruled["defects"]] == [False, False] and ruled["decision"] == "accept"
    assert len(ruled["defects"]) == 2                  # listed all the same
    # in millimetres: 0.1 mm per pixel of a 128 x 128 image makes the scrape 8 mm long and the pit 0.36 mm2
    mm = defects.size_rules(0.1, min_defect_length=1.0, min_defect_area=0.3)
    assert mm["units"] == {"length": "mm", "area": "mm2"}
    (ruled,) = defects.defect_entries(rec, NAMES, (64, 64), [(128, 128)], shapes=shapes, rules=mm)
    assert [d["counted"] for d in ruled["defects"]] == [True, False]
    assert ruled["defects"][1]["shape"]["area_mm2"] == pytest.approx(0.36)
    with pytest.raises(ValueError):
        defects.defect_entries(rec, NAMES, (64, 64), [(64, 64)], rules=rules)          # rules without shapes
    with pytest.raises(ValueError):
        defects.defect_entries(rec, NAMES, (64, 64), [(64, 64)], shapes=shapes[:1])    # not one per record
    nothing = defects.defect_entries(np.zeros((0, 12), np.int64), NAMES, (64, 64), [(64, 64)],
                                     shapes=np.zeros((0, S.HEAD + 64), np.int64), rules=rules)
    assert nothing == [{"defects": [], "decision": "accept"}]


# ------------------------------------------------------------------------------------------------ CLI flags
BASE = ["--task", "gear", "--checkpoint", "c.pth", "--input", "photos"]


@pytest.mark.parametrize("cli", [predict, predict_tiled, predict_views])
def test_shape_flags(cli):
    plain = vars(cli.parse_args(BASE))
    assert not {"measure_shapes", "pixel_size", "min_defect_length", "min_defect_area"} & set(plain)
    on = vars(cli.parse_args(BASE + ["--measure_shapes"]))
    assert set(on) - set(plain) == {"measure_shapes", "pixel_size", "min_defect_length", "min_defect_area"}
    assert (on["measure_shapes"], on["pixel_size"], on["min_defect_length"], on["min_defect_area"]) == (True, None, 0.0, 0.0)
    assert {k: on[k] for k in plain} == plain
    for flag, key in (("--min_defect_length", "min_defect_length"), ("--min_defect_area", "min_defect_area")):
        implied = vars(cli.parse_args(BASE + [flag, "2.5", "--pixel_size", "0.05"]))
        assert implied["measure_shapes"] is True and implied[key] == 2.5 and implied["pixel_size"] == 0.05
    for bad in (["--min_defect_length", "-1"], ["--min_defect_area", "-0.5"], ["--measure_shapes", "--pixel_size", "0"],
                ["--measure_shapes", "--pixel_size", "-1"], ["--min_defect_length", "nan"], ["--pixel_size", "0.1"]):
        with pytest.raises(SystemExit):
            cli.parse_args(BASE + bad)
