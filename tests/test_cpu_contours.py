"""CPU tests of the outline rules and of polygons.py (no GPU, no library): the sequential follower of
tests/_contours_ref.py, which test_gpu_contours.py holds the kernels to byte for byte, is held here to Pillow's
``ImageDraw.polygon`` -- the rasteriser of the reference's loader -- on random masks with 1-pixel-thin parts, saddles and
holes; ``gear_label_lines`` is held to the loader's own parser and mask rules, ``simplify_closed`` to its tolerance."""
import functools

import numpy as np
import pytest
from PIL import Image, ImageDraw
from scipy import ndimage

import _contours_ref as R
import _seg_regions_ref as SR
from tiaozhanbei_unet_amd import polygons
from tiaozhanbei_unet_amd.gear_dataset import PRIORITY, RAW_TO_FINAL, mask_from_polygons_pil, parse_labelme_txt

EIGHT = np.ones((3, 3), int)
FOUR = ndimage.generate_binary_structure(2, 1)
FRAMES = [(37, 53), (5, 7)]
DENSITIES = [0.3, 0.5, 0.75]


@functools.lru_cache(maxsize=None)
def _traced(h, w, density):
    """(maps [n, h, w], loops, points) of random masks of 3 classes; the small frame has more images"""
    rng = np.random.default_rng([h, w, int(density * 100)])
    n = 2 if h > 10 else 40
    maps = ((rng.random((n, h, w)) < density) * rng.integers(1, 4, (n, h, w))).astype(np.uint8)
    region, sizes, _ = SR.class_regions64(maps, 4)
    loops, points = R.trace(region, sizes)
    for a in (maps, loops, points):
        a.setflags(write=False)
    return maps, loops, points


def _draw(points, h, w):
    """Pillow's polygon of an outline; one of fewer than 3 points repeats them, as the label file does"""
    pts = [tuple(p) for p in np.asarray(points).tolist()]
    im = Image.new("L", (w, h), 0)
    ImageDraw.Draw(im).polygon(pts if len(pts) >= 3 else (pts * 3)[:3], fill=1)
    return np.array(im).astype(bool)


def _filled_regions(mask_2d):
    """{root: the region with its holes filled} of one class mask, holes by 4-connectivity"""
    lab, k = ndimage.label(mask_2d, structure=EIGHT)
    out = {}
    for i in range(1, k + 1):
        out[int(np.flatnonzero(lab.ravel() == i)[0])] = ndimage.binary_fill_holes(lab == i, structure=FOUR)
    return out


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("density", DENSITIES)
def test_pillow_fills_every_outline_back_to_its_region_with_the_holes_closed(frame, density):
    h, w = frame
    maps, loops, points = _traced(h, w, density)
    traced = polygons.outlines(loops, points)
    seen = holes = 0
    for i in range(maps.shape[0]):
        for cls in (1, 2, 3):
            for root, want in _filled_regions(maps[i] == cls).items():
                outer, inner = traced[(i, root)]
                assert np.array_equal(_draw(outer, h, w), want), (i, cls, root)      # exact, no case excepted
                seen += 1
                holes += len(inner)
    assert seen == len(traced) and seen > 50
    if density == 0.75 and h > 10:
        assert holes > 0


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("density", DENSITIES)
def test_area2_one_outer_loop_per_region_and_twice_the_size_in_all(frame, density):
    maps, loops, points = _traced(*frame, density)
    region, sizes, counts = SR.class_regions64(maps, 4)
    assert (loops[:, 5] != 0).all() and (loops[:, 5] % 2 == 0).all()
    per = {}
    for image, root, _leader, n, first, area2 in loops.tolist():
        outer, total = per.get((image, root), (0, 0))
        per[(image, root)] = (outer + (area2 > 0), total + area2)
        assert n >= 1 and (n >= 2 or area2 == 2)                                 # one point only around one pixel
    assert len(per) == int(counts.sum())
    for (image, root), (outer, total) in per.items():
        assert outer == 1 and total == 2 * sizes[image].ravel()[root], (image, root)
    order = loops[:, 0] * (4 * frame[0] * frame[1]) + loops[:, 2]
    assert (np.diff(order) > 0).all()                                            # ascending (image, leader)
    assert np.array_equal(loops[:, 4], np.concatenate([[0], np.cumsum(loops[:-1, 3])])) and loops[:, 3].sum() == len(points)


def test_min_pixels_drops_whole_regions():
    maps, loops, _ = _traced(37, 53, 0.5)
    region, sizes, _ = SR.class_regions64(maps, 4)
    kept, _ = R.trace(region, sizes, 4, 7)
    roots = {(i + 7, r) for i, r in zip(*np.nonzero((region.reshape(2, -1) == np.arange(1, 37 * 53 + 1))
                                                    & (sizes.reshape(2, -1) >= 4)))}
    assert {(i, r) for i, r in kept[:, :2].tolist()} == roots and 0 < len(kept) < len(loops)


@pytest.mark.parametrize("width", [1, 7, 512, 1920, 16384])
def test_label_coordinates_land_on_their_pixel(width):
    xs = np.arange(width)
    pts = np.stack([xs, xs % 3], 1)
    (line,) = polygons.gear_label_lines([pts], [2], (3, width))
    tokens = line.split()
    assert tokens[0] == "1" and len(tokens) == 1 + 2 * max(width, 3)
    assert [int(float(t) * width) for t in tokens[1::2]][:width] == xs.tolist()
    assert [int(float(t) * 3) for t in tokens[2::2]][:width] == (xs % 3).tolist()
    (line,) = polygons.gear_label_lines([pts.T[::-1].T], [1], (width, 3))         # the same along y
    assert [int(float(t) * width) for t in line.split()[2::2]][:width] == xs.tolist()


def test_short_outlines_are_padded_to_three_points():
    one, two = polygons.gear_label_lines([[(4, 2)], [(0, 0), (5, 1)]], [1, 3], (4, 8))
    assert one == "0 0.562500 0.625000 0.562500 0.625000 0.562500 0.625000"
    assert two == "2 0.062500 0.125000 0.687500 0.375000 0.062500 0.125000"
    with pytest.raises(ValueError):
        polygons.gear_label_lines([[(0, 0)]], [0], (4, 8))


@pytest.mark.parametrize("density", DENSITIES)
def test_a_written_label_file_loads_as_the_priority_resolved_hole_filled_map(density, tmp_path):
    h, w = 37, 53
    maps, loops, points = _traced(h, w, density)
    for i in range(maps.shape[0]):
        mine = [(root, outer) for (image, root), (outer, _) in polygons.outlines(loops, points).items() if image == i]
        classes = [int(maps[i].ravel()[root]) for root, _ in mine]
        path = tmp_path / f"{i}.txt"
        path.write_text("".join(line + "\n" for line in polygons.gear_label_lines([o for _, o in mine], classes, (h, w))))
        parsed = parse_labelme_txt(str(path), w, h)
        assert len(parsed) == len(mine)                                          # no outline was dropped as too short
        for (cls, pts), (root, outer), c in zip(parsed, mine, classes):
            assert cls == c - 1 and pts[:len(outer)] == [tuple(p) for p in outer.tolist()]
        want = np.zeros((h, w), np.uint8)
        for raw in reversed(PRIORITY):
            for filled in _filled_regions(maps[i] == RAW_TO_FINAL[raw]).values():
                want[filled] = RAW_TO_FINAL[raw]
        assert np.array_equal(mask_from_polygons_pil(parsed, w, h), want)


def _disc_and_l():
    yy, xx = np.mgrid[0:41, 0:41]
    disc = ((yy - 20) ** 2 + (xx - 20) ** 2 <= 17 ** 2).astype(np.uint8)
    ell = np.zeros((41, 41), np.uint8)
    ell[3:38, 4:12] = 1
    ell[28:38, 4:35] = 1
    out = []
    for m in (disc, ell):
        region, sizes, _ = SR.class_regions64(m[None], 2)
        loops, points = R.trace(region, sizes)
        assert len(loops) == 1
        out.append(points)
    return out


def _distance_to_closed(p, poly):
    poly = np.asarray(poly, np.float64)
    best = np.inf
    for a, b in zip(poly, np.roll(poly, -1, 0)):
        ab = b - a
        t = 0.0 if not ab.any() else min(1.0, max(0.0, float((p - a) @ ab) / float(ab @ ab)))
        best = min(best, float(np.hypot(*(p - (a + t * ab)))))
    return best


@pytest.mark.parametrize("which", [0, 1])
def test_simplify_closed_keeps_a_subsequence_within_the_tolerance(which):
    pts = _disc_and_l()[which]
    assert polygons.simplify_closed(pts, 0) is pts or np.array_equal(polygons.simplify_closed(pts, 0), pts)
    assert np.array_equal(polygons.simplify_closed(pts, 0.0), pts)
    before = len(pts)
    for tol in (0.5, 1, 2):
        out = polygons.simplify_closed(pts, tol)
        assert out.dtype == pts.dtype and 3 <= len(out) <= before
        k = 0
        for p in pts.tolist():                                                   # a subsequence, in order
            if k < len(out) and p == out[k].tolist():
                k += 1
            else:
                assert _distance_to_closed(np.array(p, np.float64), out) <= tol + 1e-9, (tol, p)
        assert k == len(out) and out[0].tolist() == pts[0].tolist()
        before = len(out) if which == 1 else before
    if which == 0:
        assert len(polygons.simplify_closed(pts, 2)) < len(pts) // 2
    else:
        assert len(polygons.simplify_closed(pts, 0.5)) == 7                       # six corners, the inner one cut across
        assert len(polygons.simplify_closed(pts, 2)) == 6
    with pytest.raises(ValueError):
        polygons.simplify_closed(pts, -1)


def test_attach_outlines_follows_the_records_order():
    maps, loops, points = _traced(5, 7, 0.5)
    import _defects_ref as D
    from tiaozhanbei_unet_amd import defects
    rec = D.describe_records(maps, 4)
    names = ["background", "pitting", "spalling", "scrape"]
    originals = [(10, 21)] * maps.shape[0]
    entries = defects.defect_entries(rec, names, (5, 7), originals)
    polygons.attach_outlines(entries, rec[::-1], polygons.outlines(loops, points), (5, 7), originals)
    for i, e in enumerate(entries):
        drawn = np.zeros((5, 7), np.uint8)
        for d in e["defects"]:
            x0, y0, x1, y1 = d["bbox"]
            xs, ys = zip(*d["outline"])
            assert (min(xs), min(ys), max(xs), max(ys)) == (x0, y0, x1, y1)       # the outline touches its box
            assert d["outline_original"][0] == [(xs[0] + 0.5) * 3 - 0.5, (ys[0] + 0.5) * 2 - 0.5]
            assert isinstance(d["hole_outlines"], list)
        lines = polygons.entry_label_lines(e, (5, 7))
        assert len(lines) == len(e["defects"]) and [int(l.split()[0]) + 1 for l in lines] == [d["class"] for d in e["defects"]]


def test_polygon_flags_are_absent_unless_given():
    from tiaozhanbei_unet_amd import predict, predict_tiled, predict_views, seg_cli
    base = ["--task", "gear", "--checkpoint", "c.pth", "--input", "photos"]
    for tool in (predict, predict_tiled, predict_views):
        plain = tool.parse_args(base)
        assert not {"save_polygons", "polygon_tolerance"} & set(vars(plain)) and seg_cli.polygon_rules_of(plain) is None
        saved = tool.parse_args(base + ["--save_polygons"])
        assert saved.save_polygons is True and saved.polygon_tolerance == 0.0 and not hasattr(saved, "measure_shapes")
        thin = tool.parse_args(base + ["--polygon_tolerance", "1.5"])
        assert thin.save_polygons is True and seg_cli.polygon_rules_of(thin)["tolerance"] == 1.5
        with pytest.raises(SystemExit):
            tool.parse_args(base + ["--polygon_tolerance", "-1"])
