"""CPU checks of the fragment grouping: the exports and host-side refusals of the new entry points, the numpy
restatement of the device kernel (tests/_groups_ref.py) against an all-pairs distance on small maps and against what
the shared cases (tests/_groups_cases.py) were drawn to show, and the host side -- ``defects.shape_measures`` with
several components, ``defects.defect_entries`` and ``polygons.outlines`` with a fragment table, the label lines against
Pillow's ``ImageDraw.polygon``, and the flag."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
from PIL import Image, ImageDraw
from scipy import ndimage

import _contours_ref as R
import _groups_cases as K
import _groups_ref as G
import _seg_regions_ref as SR
import _shapes_ref as S
from tiaozhanbei_unet_amd import _lib, defects, eval_detection, evaluation, ops, polygons, predict, predict_tiled, predict_views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("unet_group_class_regions_workspace", "unet_group_class_regions")
FOUR = ndimage.generate_binary_structure(2, 1)


# ------------------------------------------------------------------------------------------------ exports
def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    _lib.build(force=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)                # loading needs no GPU
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name), name
    assert ops.group_class_regions is evaluation.group_class_regions
    assert ops.FRAGMENT_FIELDS is evaluation.FRAGMENT_FIELDS == ("image", "class", "root", "group", "size")
    assert len(ops.FRAGMENT_FIELDS) == G.FIELDS


def test_workspace_query_and_refusals_on_the_host():
    """decided before anything reaches the device: the pointers below are not memory"""
    lib = _lib.lib()
    assert lib.unet_group_class_regions_workspace(8, 512, 512, 4) == 8 * 512 * 512 * 8
    assert lib.unet_group_class_regions_workspace(1, 1, 1, 2) == 16
    assert lib.unet_group_class_regions_workspace(1, 1, (1 << 31) - 1, 255) > 0
    dummy = ctypes.c_void_p(16)                        # only checked for NULL: the arguments are refused first

    def call(n=2, h=8, w=8, c=4, gap=5, min_pixels=1, base=0, cap=16, ws=1 << 40, classes=dummy, group=dummy, count=dummy):
        return lib.unet_group_class_regions(classes, dummy, dummy, n, h, w, c, gap, min_pixels, base, group, dummy, dummy,
                                            dummy, cap, count, dummy, ws, None)

    for n, h, w, c in [(2, 8, 8, 1), (2, 8, 8, 256), (65536, 1, 1, 4), (1, 1 << 16, 1 << 15, 4), (2, 1 << 15, 1 << 15, 4)]:
        assert lib.unet_group_class_regions_workspace(n, h, w, c) == 0, (n, h, w, c)
        assert call(n, h, w, c) == -2, (n, h, w, c)
        assert b"2..255" in lib.unet_last_error()
    assert call(gap=0) == -1 and b"gap=0" in lib.unet_last_error()
    assert call(gap=33) == -1 and call(gap=-1) == -1
    assert call(min_pixels=0) == -1 and call(base=-1) == -1 and call(cap=-1) == -1
    assert call(classes=None) == -1 and b"null pointer" in lib.unet_last_error()
    assert call(group=None) == -1 and call(count=None) == -1
    assert call(base=(1 << 31) - 2) == -2
    assert call(ws=2 * 8 * 8 * 8 - 1) == -3 and b"workspace too small" in lib.unet_last_error()


# ------------------------------------------------------------------------------------------------ the reference
def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _groups_of(frag, image=0):
    """{group root: [fragment roots]} of one image of a fragment table"""
    out = {}
    for i, _c, root, group, _s in frag.tolist():
        if i == image:
            out.setdefault(group, []).append(root)
    return out


def test_reference_equals_the_all_pairs_distance_on_random_small_maps():
    rng = np.random.default_rng(3)
    merged = 0
    for _ in range(60):
        h, w = rng.integers(1, 13, 2)
        maps = rng.choice(np.array([0] * 10 + [1, 1, 2, 3, 7], np.uint8), (2, h, w))
        for gap in (1, 2, 3, 5, 32):
            for mp in (1, 2):
                got, want = G.group_regions64(maps, 4, gap, mp, 3), G.brute_groups64(maps, 4, gap, mp, 3)
                assert _same(got, want), (maps.tolist(), gap, mp)
                merged += int((got[3][:, 2] != got[3][:, 3]).sum())
    assert merged > 500


def test_chain_is_transitive_and_classes_stay_apart():
    m = np.zeros((1, 6, 12), np.uint8)
    m[0, 1, 0:2] = 1; m[0, 1, 4:6] = 1; m[0, 1, 8:10] = 1      # A, B, C: 3 apart; A and C 7 apart
    m[0, 3, 0:2] = 2; m[0, 3, 4:6] = 2                         # another class 2 rows below
    for fn in (G.group_regions64, G.brute_groups64):
        group, sizes, counts, frag = fn(m, 3, 3)
        assert _groups_of(frag) == {12: [12, 16, 20], 36: [36, 40]}
        assert counts.tolist() == [[0, 1, 1]] and sizes[0, 1, 9] == 6 and group[0, 1, 9] == 13 and group[0, 3, 4] == 37
        assert fn(m, 3, 2)[2].tolist() == [[0, 3, 2]]          # 3 apart: not linked at gap 2
        assert frag[:, 1].tolist() == [1, 1, 1, 2, 2] and frag[:, 4].tolist() == [2] * 5


def test_a_bridge_below_min_pixels_links_nothing():
    m = np.zeros((1, 5, 12), np.uint8)
    m[0, 1:3, 0:2] = 1; m[0, 1, 5] = 1; m[0, 1:3, 9:11] = 1    # blocks 8 apart and a pixel 4 from each
    for fn in (G.group_regions64, G.brute_groups64):
        assert _groups_of(fn(m, 2, 4, 1)[3]) == {12: [12, 17, 21]}
        group, sizes, counts, frag = fn(m, 2, 4, 2)
        assert _groups_of(frag) == {12: [12], 21: [21]} and counts.tolist() == [[0, 2]]
        assert group[0, 1, 5] == 0 and sizes[0, 1, 5] == 0     # the dropped pixel is background in both maps


def test_gap_one_is_the_identity_and_rows_do_not_wrap():
    rng = np.random.default_rng(4)
    maps = rng.choice(np.array([0, 0, 1, 2, 3], np.uint8), (2, 9, 11))
    region, sizes, counts = SR.class_regions64(maps, 4)
    for fn in (G.group_regions64, G.brute_groups64):
        group, gsizes, gcounts, frag = fn(maps, 4, 1)
        assert np.array_equal(group, region) and np.array_equal(gsizes, sizes) and np.array_equal(gcounts, counts)
        assert np.array_equal(frag[:, 2], frag[:, 3])
    m = np.zeros((1, 4, 12), np.uint8)
    m[0, 1, 11] = 1; m[0, 2, 0] = 1                            # neighbours in memory, 11 apart in the frame
    for fn in (G.group_regions64, G.brute_groups64):
        assert _groups_of(fn(m, 2, 5)[3]) == {23: [23], 24: [24]}
        assert _groups_of(fn(m, 2, 12)[3]) == {23: [23, 24]}


def test_the_shared_cases_show_what_they_were_drawn_for():
    w = 100
    maps = K.maps_of((3, 40, 100), "layout")
    at = lambda y, x: y * w + x

    def together(gap, a, b, image=0, mp=1):
        frag = G.group_regions64(maps, K.C, gap, mp)[3]
        rows = {int(r[2]): int(r[3]) for r in frag if r[0] == image}
        return rows[a] == rows[b]

    assert together(5, at(5, 2), at(5, 18)) and together(5, at(8, 2), at(8, 18)) and not together(2, at(5, 2), at(5, 10))
    assert together(5, at(5, 2), at(5, 18), image=1)           # the same chain in the rotated classes
    assert together(5, at(14, 2), at(14, 11)) and not together(5, at(14, 2), at(14, 11), mp=2)
    assert together(5, at(24, 40), at(27, 44)) and not together(5, at(24, 52), at(25, 57))      # 25 and 26
    assert together(2, at(24, 20), at(24, 22)) and not together(2, at(28, 20), at(29, 22))      # 4 and 5
    assert together(32, at(30, 28), at(30, 62)) and not together(5, at(30, 28), at(30, 62))
    for gap in K.GAPS:
        assert not together(gap, at(20, 99), at(21, 0)) or gap == 32      # at 32 they meet through others, not by a wrap
    assert together(32, at(2, 3), at(2, 35), image=2) and not together(32, at(20, 3), at(21, 35), image=2)
    assert not together(32, at(10, 99), at(11, 0), image=2)
    small = K.maps_of((2, 33, 65), "layout")
    rows = {(int(r[0]), int(r[2])): int(r[3]) for r in G.group_regions64(small, K.C, 5)[3]}
    assert rows[(0, 20 * 65 + 64)] == 20 * 65 + 64 and rows[(0, 21 * 65)] == 21 * 65      # ends of consecutive rows
    rows = {(int(r[0]), int(r[2])): int(r[3]) for r in G.group_regions64(small, K.C, 32)[3]}
    assert rows[(1, 10 * 65 + 64)] == 10 * 65 + 64 and rows[(1, 11 * 65)] == 11 * 65
    assert rows[(1, 2 * 65 + 35)] == 2 * 65 + 3 and rows[(1, 21 * 65 + 35)] == 21 * 65 + 35      # 1024 and 1025
    for shape in K.SHAPES:
        for kind in K.KINDS[1:]:
            if shape != (1, 1, 1):
                assert K.maps_of(shape, kind).shape == shape
    dense = G.group_regions64(K.maps_of((3, 40, 100), "speckle30"), K.C, 2)[3]
    assert len(dense) > 500 and (dense[:, 2] != dense[:, 3]).sum() > 100


# ------------------------------------------------------------------------------------------------ the host side
NAMES = ["background", "pitting", "spalling", "scrape"]


def _two_rings():
    """two 5 x 5 rings of class 1, 3 apart, and a bar of class 2; (maps, gap)"""
    m = np.zeros((1, 12, 20), np.uint8)
    for x in (1, 9):
        m[0, 2:7, x:x + 5] = 1
        m[0, 3:6, x + 1:x + 4] = 0
    m[0, 9, 2:8] = 2
    return m, 4


def _shape_record(mask, image=0):
    """the shape record (tests/_shapes_ref.py's fields) of one boolean mask, connected or not"""
    ys, xs = np.nonzero(mask)
    table = S.directions(32)
    p = xs[:, None] * table[None, :, 0] + ys[:, None] * table[None, :, 1]
    return np.array([image, ys[0] * mask.shape[1] + xs[0], len(xs), (xs * xs).sum(), (ys * ys).sum(), (xs * ys).sum(),
                     *S.quads(mask), *p.min(axis=0), *p.max(axis=0)], np.int64)


def test_shape_measures_counts_holes_per_component():
    maps, gap = _two_rings()
    rec, frag = G.describe_groups(maps, 3, gap)
    assert rec[:, 3].tolist() == [32, 6] and len(frag) == 3
    group = G.group_regions64(maps, 3, gap)[0]
    shape = _shape_record(group[0] == rec[0, 2] + 1)
    both = defects.shape_measures(shape, 32, (12, 20), (12, 20), defect_record=rec[0], components=2)
    assert both["euler_number"] == 0 and both["holes"] == 2
    assert defects.shape_measures(shape, 32, (12, 20), (12, 20), defect_record=rec[0])["holes"] == 1      # the default
    one = _shape_record(maps[0] == 1) * 0 + _shape_record((group[0] == rec[0, 2] + 1) & (np.arange(20) < 8)[None, :])
    left = rec[0].copy()
    left[3], left[8], left[9] = 16, one[2] * 3, one[2] * 4                      # a ring of 16 centred at (3, 4)
    ring = defects.shape_measures(one, 32, (12, 20), (12, 20), defect_record=left)
    assert ring["holes"] == 1 and both["perimeter"] == pytest.approx(2 * ring["perimeter"])      # the sum over the fragments
    assert both["circularity"] == pytest.approx(ring["circularity"] / 2)        # not a roundness
    # the extents are those of the union: a 13 x 5 hull against a 5 x 5 one, low by at most cos(pi / 64) (0.12 %)
    assert both["feret_length"] == pytest.approx(math.hypot(13, 5), rel=1.3e-3)
    assert ring["feret_length"] == pytest.approx(math.hypot(5, 5), rel=1.3e-3)
    with pytest.raises(ValueError):
        defects.shape_measures(shape, 32, (12, 20), (12, 20), defect_record=rec[0], components=0)


def test_defect_entries_lists_the_fragments_of_every_group():
    maps, gap = _two_rings()
    rec, frag = G.describe_groups(maps, 3, gap)
    (entry,) = defects.defect_entries(rec, NAMES, (12, 20), [(24, 40)], fragments=frag[::-1])
    ring, bar = entry["defects"]
    assert ring["pixels"] == 32 and ring["bbox"] == [1, 2, 13, 6] and ring["class_name"] == "pitting"
    assert ring["fragments"] == [{"root": [1, 2], "pixels": 16}, {"root": [9, 2], "pixels": 16}]
    assert bar["fragments"] == [{"root": [2, 9], "pixels": 6}]
    (plain,) = defects.defect_entries(rec, NAMES, (12, 20), [(24, 40)])
    assert all("fragments" not in d for d in plain["defects"])
    with pytest.raises(ValueError):
        defects.defect_entries(rec, NAMES, (12, 20), [(24, 40)], fragments=frag[:-1])


def _draw(loops, h, w):
    im = Image.new("L", (w, h), 0)
    for pts in loops:
        pts = [tuple(p) for p in np.asarray(pts).tolist()]
        ImageDraw.Draw(im).polygon(pts if len(pts) >= 3 else (pts * 3)[:3], fill=1)
    return np.array(im).astype(bool)


def _filled(mask, ids):
    """the union over the region numbers ``ids`` of the region with its holes filled"""
    out = np.zeros(mask.shape, bool)
    for v in np.unique(ids[mask]):
        out |= ndimage.binary_fill_holes(ids == v, structure=FOUR)
    return out


def test_outlines_by_group_take_the_largest_fragment_and_keep_every_loop():
    maps, gap = _two_rings()
    maps = maps.copy()
    maps[0, 2, 14] = 1                                  # the second ring grows by a pixel: it leads
    region, sizes, _ = SR.class_regions64(maps, 3)
    loops, points = R.trace(region, sizes)
    rec, frag = G.describe_groups(maps, 3, gap)
    plain = polygons.outlines(loops, points)
    grouped = polygons.outlines(loops, points, frag)
    assert sorted(grouped) == [(0, 2 * 20 + 1), (0, 9 * 20 + 2)]
    outer, holes, pieces = grouped[(0, 41)]
    assert np.array_equal(outer, plain[(0, 49)][0]) and len(holes) == 2 and len(pieces) == 2
    assert np.array_equal(pieces[0], plain[(0, 41)][0]) and np.array_equal(pieces[1], plain[(0, 49)][0])
    maps[0, 2, 14] = 0                                  # a tie: the smaller root leads
    region, sizes, _ = SR.class_regions64(maps, 3)
    loops, points = R.trace(region, sizes)
    grouped = polygons.outlines(loops, points, G.describe_groups(maps, 3, gap)[1])
    assert np.array_equal(grouped[(0, 41)][0], polygons.outlines(loops, points)[(0, 41)][0])
    with pytest.raises(ValueError):
        polygons.outlines(loops, points, frag[:1])


@pytest.mark.parametrize("density,gap,min_pixels", [(0.1, 3, 1), (0.3, 2, 1), (0.3, 5, 3), (0.6, 2, 2)])
def test_pillow_redraws_the_label_lines_as_the_groups_with_holes_filled(density, gap, min_pixels):
    h, w = 31, 43
    rng = np.random.default_rng(int(density * 10) + gap)
    maps = ((rng.random((2, h, w)) < density) * rng.integers(1, 4, (2, h, w))).astype(np.uint8)
    region, sizes, _ = SR.class_regions64(maps, 4)
    loops, points = R.trace(region, sizes, min_pixels) if min_pixels > 1 else R.trace(region, sizes)
    rec, frag = G.describe_groups(maps, 4, gap, None, min_pixels)
    group = G.group_regions64(maps, 4, gap, min_pixels)[0]
    originals = [(h, w)] * 2
    entries = defects.defect_entries(rec, NAMES, (h, w), originals, fragments=frag)
    polygons.attach_outlines(entries, rec, polygons.outlines(loops, points, frag), (h, w), originals)
    multi = 0
    for i, e in enumerate(entries):
        lines = polygons.entry_label_lines(e, (h, w))
        assert len(lines) == sum(len(d["fragments"]) for d in e["defects"]) == int((frag[:, 0] == i).sum())
        at = 0
        for d, (_, _, root) in zip(e["defects"], rec[rec[:, 0] == i][:, :3].tolist()):
            k = len(d["fragments"])
            multi += k > 1
            mine = lines[at:at + k]
            at += k
            assert all(int(l.split()[0]) == d["class"] - 1 for l in mine)
            drawn = []
            for l in mine:
                v = [float(t) for t in l.split()[1:]]
                drawn.append([(int(x * w), int(y * h)) for x, y in zip(v[::2], v[1::2])])      # the loader's rounding
            want = _filled(group[i] == root + 1, region[i])
            assert want.sum() >= d["pixels"] and np.array_equal(_draw(drawn, h, w), want), (i, root)
    assert multi > 3


# ------------------------------------------------------------------------------------------------ CLI flags
BASE = ["--task", "gear", "--checkpoint", "c.pth", "--input", "photos"]


@pytest.mark.parametrize("cli", [predict, predict_tiled, predict_views])
def test_merge_gap_flag(cli):
    from tiaozhanbei_unet_amd import seg_cli
    plain = cli.parse_args(BASE)
    assert "merge_gap" not in vars(plain) and seg_cli.grouping_rules_of(plain) is None
    on = cli.parse_args(BASE + ["--merge_gap", "4"])
    assert set(vars(on)) - set(vars(plain)) == {"merge_gap"} and on.merge_gap == 4
    assert {k: vars(on)[k] for k in vars(plain)} == vars(plain)
    rules = seg_cli.grouping_rules_of(on)
    assert rules["merge_gap"] == 4 and "frame pixels" in rules["units"] and "anisotropically" in rules["units"]
    assert "--min_region_pixels" in rules["dropped"] and "before grouping" in rules["dropped"]
    assert cli.parse_args(BASE + ["--merge_gap", "2"]).merge_gap == 2 and cli.parse_args(BASE + ["--merge_gap", "32"])
    for bad in ("1", "33", "0", "-3", "2.5"):
        with pytest.raises(SystemExit):
            cli.parse_args(BASE + ["--merge_gap", bad])


def test_eval_detection_takes_the_flag_and_its_siblings_do_not():
    from tiaozhanbei_unet_amd import eval_regions, eval_views
    base = ["--dataset", "gear", "--checkpoint", "c.pth"]
    assert "merge_gap" not in vars(eval_detection.parse_args(base))
    assert eval_detection.parse_args(base + ["--merge_gap", "6"]).merge_gap == 6
    for bad in ("1", "33"):
        with pytest.raises(SystemExit):
            eval_detection.parse_args(base + ["--merge_gap", bad])
    for tool in (eval_regions, eval_views):
        with pytest.raises(SystemExit):
            tool.parse_args(base + ["--merge_gap", "6"])


def test_merge_gap_is_refused_outside_its_range_before_anything_runs():
    for fn in (evaluation.describe_class_regions, evaluation.measure_class_regions,
               evaluation.describe_and_measure_class_regions):
        for bad in (-1, 33):
            with pytest.raises(ValueError, match="merge_gap"):
                fn(None, 4, merge_gap=bad)
    with pytest.raises(ValueError, match="merge_gap"):
        evaluation.DetectionMatcher(4, merge_gap=33)
    assert evaluation.DetectionMatcher(4).merge_gap == 0 and evaluation.DetectionMatcher(4, 1, 32).merge_gap == 32
