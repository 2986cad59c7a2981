"""GPU tests of the outline tracing (csrc/contours.hip through ops.trace_class_regions) against the sequential follower of
tests/_contours_ref.py, which test_cpu_contours.py holds to Pillow.  Everything is integers and prefix sums: ``loops`` and
``points`` are compared byte for byte.  The frames are the smallest at which the tracing can go wrong: every turn of the
successor rule, loops that cross the 1024-pixel blocks and the 32 x 32 labeller tiles, a loop longer than a workgroup
(many doubling rounds), frames of one row and one column, and maps whose kept regions differ from their regions."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

import _contours_ref as R
from tiaozhanbei_unet_amd import _lib as L
from tiaozhanbei_unet_amd import augment, ops, polygons

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FOUR = ndimage.generate_binary_structure(2, 1)


def _hand(rows):
    return np.array([[int(ch) for ch in row.replace(".", "0")] for row in rows], np.uint8)


def _nine(small):
    m = np.zeros((9, 9), np.uint8)
    m[2:2 + small.shape[0], 1:1 + small.shape[1]] = small
    return m


def _spiral(side):
    """a 1-pixel-wide square spiral with 1-pixel gaps: one region, one loop of several hundred edges"""
    m = np.zeros((side, side), np.uint8)
    x, y, dx, dy = 0, 0, 1, 0
    m[0, 0] = 1
    moved = True
    while moved:
        moved = False
        while 0 <= x + dx < side and 0 <= y + dy < side and not m[y + dy, x + dx] and not (
                0 <= x + 2 * dx < side and 0 <= y + 2 * dy < side and m[y + 2 * dy, x + 2 * dx]):
            x, y = x + dx, y + dy
            m[y, x] = 1
            moved = True
        dx, dy = -dy, dx
    return m


def _thick_shapes(h, w):
    """unions of rectangles and discs of radius >= 3: every part at least 3 pixels thick; one ring (a hole)"""
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), np.uint8)
    m[3:12, 4:20] = 1
    m[8:24, 10:16] = 1                                  # an L / T union
    m[(yy - 14) ** 2 + (xx - 40) ** 2 <= 9 ** 2] = 2    # a disc ...
    m[(yy - 14) ** 2 + (xx - 40) ** 2 <= 4 ** 2] = 0    # ... with a hole: a ring 5 thick
    m[(yy - 36) ** 2 + (xx - 12) ** 2 <= 3 ** 2] = 3    # the smallest disc
    m[30:44, 28:33] = 1
    m[(yy - 37) ** 2 + (xx - 36) ** 2 <= 5 ** 2] = 1    # a disc joined to a bar
    m[h - 6:h, w - 9:w] = 3                             # in the frame's corner
    return m


@functools.lru_cache(maxsize=None)
def _case(name):
    """(maps uint8 [n, h, w], C); built once, never modified"""
    rng = np.random.default_rng(9)
    C = 4
    if name == "single":
        m = _nine(_hand(["1"]))[None]
    elif name == "pair_side":
        m = _nine(_hand(["11"]))[None]
    elif name == "pair_diagonal":
        m = _nine(_hand(["1.", ".1"]))[None]
    elif name == "line":
        m = _nine(_hand(["11111"]))[None]
    elif name == "plus":
        m = _nine(_hand([".1.", "111", ".1."]))[None]
    elif name == "ring":
        m = _nine(_hand(["111", "1.1", "111"]))[None]
    elif name == "stairs":
        m = _nine(_hand(["1....", ".1...", "..1..", "...1.", "....1"]))[None]
    elif name == "nested":                              # another class inside a hole, and a third inside that
        m = _nine(_hand(["1111111", "1.....1", "1.222.1", "1.232.1", "1.222.1", "1.....1", "1111111"]))[None]
    elif name == "touch_all_edges":
        m = np.zeros((1, 9, 9), np.uint8)
        m[0, 4, :] = 2
        m[0, :, 4] = 2
    elif name == "filled":                              # two blocks of pixels, one loop around the frame
        m = np.ones((1, 40, 40), np.uint8)
    elif name == "1x1":
        m = np.ones((1, 1, 1), np.uint8)
    elif name == "1x53":
        m = (rng.random((1, 1, 53)) < 0.6).astype(np.uint8) * rng.integers(1, 4, (1, 1, 53)).astype(np.uint8)
    elif name == "37x1":
        m = (rng.random((1, 37, 1)) < 0.6).astype(np.uint8) * rng.integers(1, 4, (1, 37, 1)).astype(np.uint8)
    elif name == "batch":                               # the first image ends and the second begins with members
        m = np.zeros((2, 9, 9), np.uint8)
        m[0, 6:, 5:] = 1
        m[0, 1:4, 1:4] = 2
        m[1, :3, :4] = 1
        m[1, 5:8, 2:7] = 3
        m[1, 6, 4] = 0
    elif name == "spiral":
        m = _spiral(33)[None]
    elif name.startswith("speckle"):
        p = float(name[7:])
        m = (rng.random((2, 37, 53)) < p).astype(np.uint8) * rng.integers(1, 4, (2, 37, 53)).astype(np.uint8)
    elif name == "blobs":                               # smoothed noise: regions and loops over many tiles and blocks
        f = ndimage.gaussian_filter(rng.standard_normal((256, 320)), 5.0)
        m = np.zeros((1, 256, 320), np.uint8)
        m[0][f > 0.02] = 1
        m[0][f < -0.03] = 2
        m[0][np.abs(f) < 0.002] = 3
    elif name == "thick":
        m = _thick_shapes(48, 64)[None]
    else:
        raise KeyError(name)
    m = np.ascontiguousarray(m, np.uint8)
    m.setflags(write=False)
    return m, C


@functools.lru_cache(maxsize=None)
def _labelled(name):
    """(region, sizes) on the device, labelled once per case"""
    maps, C = _case(name)
    region, sizes, _ = ops.label_class_regions(torch.from_numpy(np.array(maps)).to(DEV), C)
    return region, sizes


@functools.lru_cache(maxsize=None)
def _want(name, min_pixels=1, image_base=0):
    region, sizes = _labelled(name)
    loops, points = R.trace(region.cpu().numpy(), sizes.cpu().numpy(), min_pixels, image_base)
    loops.setflags(write=False)
    points.setflags(write=False)
    return loops, points


def _got(name, min_pixels=1, image_base=0):
    return ops.trace_class_regions(*_labelled(name), min_pixels, image_base)


def _assert_equal(got, want, what):
    for g, w, part in zip(got, want, ("loops", "points")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {part} row {bad[0][0]}: {g[bad[0][0]].tolist()} != {w[bad[0][0]].tolist()}"
        assert g.tobytes() == w.tobytes()


HAND = ["single", "pair_side", "pair_diagonal", "line", "plus", "ring", "stairs", "nested"]
EDGES = ["touch_all_edges", "filled", "1x1", "1x53", "37x1", "batch"]


@pytest.mark.parametrize("name", HAND + EDGES + ["spiral", "blobs"])
def test_loops_and_points_equal_the_reference(name):
    want = _want(name)
    _assert_equal(_got(name), want, name)
    loops, points = want
    if name == "single":
        assert loops.tolist() == [[0, 2 * 9 + 1, 4 * (2 * 9 + 1), 1, 0, 2]] and points.tolist() == [[1, 2]]
    if name == "pair_side":
        assert loops[0, 3:].tolist() == [2, 0, 4] and points.tolist() == [[1, 2], [2, 2]]
    if name == "pair_diagonal":
        assert loops[0, 3:].tolist() == [2, 0, 4] and points.tolist() == [[1, 2], [2, 3]]
    if name == "line":
        assert points.tolist() == [[1, 2], [5, 2]]
    if name == "ring":
        assert loops[:, 5].tolist() == [18, -2] and loops[1, 3] == 4          # the hole loop: the ring's 4 edge pixels
    if name == "stairs":
        assert len(loops) == 1 and points.tolist() == [[1, 2], [5, 6]]
    if name == "nested":
        assert sorted(loops[:, 5].tolist()) == [-50, -2, 2, 18, 98]
    if name == "filled":
        assert loops.tolist() == [[0, 0, 1, 4, 0, 2 * 40 * 40]]          # (0, 0) has no bottom edge: its left side leads
        assert points.tolist() == [[0, 0], [0, 39], [39, 39], [39, 0]]
    if name == "1x1":
        assert loops.tolist() == [[0, 0, 0, 1, 0, 2]] and points.tolist() == [[0, 0]]
    if name == "batch":
        assert set(loops[:, 0].tolist()) == {0, 1} and (loops[:, 5] < 0).sum() == 1
    if name == "spiral":
        assert len(loops) == 1 and loops[0, 5] == 2 * int(_case(name)[0].sum())
        edges = 2 * int(_case(name)[0].sum()) + 2                               # a 1-wide path: 2 sides a pixel, 2 ends
        assert edges > 4 * 256                                                  # longer than a workgroup, 11 rounds
    if name == "blobs":
        assert len(loops) > 40 and (loops[:, 5] < 0).any() and loops[:, 3].max() > 256


@pytest.mark.parametrize("density", ["0.3", "0.5", "0.75"])
@pytest.mark.parametrize("min_pixels", [1, 4])
def test_speckle_keeps_the_regions_that_describe_keeps(density, min_pixels):
    name = "speckle" + density
    want = _want(name, min_pixels, 0)
    got = _got(name, min_pixels, 0)
    _assert_equal(got, want, f"{name} min_pixels {min_pixels}")
    maps, C = _case(name)
    rec = ops.describe_class_regions(torch.from_numpy(np.array(maps)).to(DEV), C, None, min_pixels)
    outer = got[0][got[0][:, 5] > 0]
    outer = outer[np.lexsort((outer[:, 1], outer[:, 0]))]
    assert np.array_equal(outer[:, :2], rec[:, [0, 2]])                        # one outer loop per kept region: aligned
    twice = {}
    for row in got[0].tolist():
        twice[(row[0], row[1])] = twice.get((row[0], row[1]), 0) + row[5]
    assert [twice[(r[0], r[2])] for r in rec.tolist()] == (2 * rec[:, 3]).tolist()      # area2 sums to twice the size
    if min_pixels == 4:
        assert 0 < len(want[0]) < len(_want(name, 1, 0)[0])


def test_image_base_moves_the_image_column_only():
    want = _want("batch", 1, 7)
    _assert_equal(_got("batch", 1, 7), want, "image_base 7")
    plain = _want("batch")
    assert np.array_equal(want[0][:, 0], plain[0][:, 0] + 7) and np.array_equal(want[0][:, 1:], plain[0][:, 1:])


def test_two_runs_are_bitwise_equal():
    first = _got("speckle0.5")
    for _ in range(2):
        again = _got("speckle0.5")
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    first = _got("blobs")
    again = _got("blobs")
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()


def test_describe_and_measure_traces_the_same_labelling():
    maps, C = _case("speckle0.5")
    dev = torch.from_numpy(np.array(maps)).to(DEV)
    rec, shapes, loops, points = ops.describe_and_measure_class_regions(dev, C, None, 2, 3, 16, contours=True)
    plain = ops.describe_and_measure_class_regions(dev, C, None, 2, 3, 16)
    assert rec.tobytes() == plain[0].tobytes() and shapes.tobytes() == plain[1].tobytes()
    _assert_equal((loops, points), _want("speckle0.5", 2, 3), "with the records")
    rec2, none, loops2, points2 = ops.describe_and_measure_class_regions(dev, C, None, 2, 3, None, contours=True)
    assert none is None and rec2.tobytes() == rec.tobytes() and loops2.tobytes() == loops.tobytes()
    empty = ops.describe_and_measure_class_regions(torch.zeros((1, 5, 5), dtype=torch.uint8, device=DEV), C, contours=True)
    assert empty[2].shape == (0, 6) and empty[3].shape == (0, 2) and empty[3].dtype == np.int32
    nothing = ops.trace_class_regions(torch.zeros((1, 5, 5), dtype=torch.int32, device=DEV),
                                      torch.zeros((1, 5, 5), dtype=torch.int32, device=DEV))
    assert nothing[0].shape == (0, 6) and nothing[1].shape == (0, 2)


MARGIN = 256
SENTINEL = 0xA5


def _guarded(nbytes):
    buf = torch.full((nbytes + 2 * MARGIN,), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf, buf.data_ptr() + MARGIN


def _direct(name, loop_short=0, point_short=0):
    """unet_trace_class_regions on exactly sized, guarded buffers; (loops bytes, points bytes, counts, guards intact)"""
    region, sizes = _labelled(name)
    n, h, w = region.shape
    lib, vp = L.lib(), ctypes.c_void_p
    counts = torch.zeros(3, dtype=torch.int64, device=DEV)
    need = lib.unet_count_class_region_edges_workspace(n, h, w)
    ws = _guarded(need)
    L.check(lib.unet_count_class_region_edges(vp(region.data_ptr()), vp(sizes.data_ptr()), n, h, w, 1, vp(counts.data_ptr()),
                                              vp(ws[1]), need, None), "unet_count_class_region_edges")
    edges, n_loops, n_points = counts.tolist()
    need = lib.unet_trace_class_regions_workspace(n, h, w, edges)
    loop_cap, point_cap = n_loops - loop_short, n_points - point_short
    bufs = {k: _guarded(b) for k, b in (("loops", n_loops * 48), ("points", n_points * 8), ("counts", 24), ("ws", need))}
    L.check(lib.unet_trace_class_regions(vp(region.data_ptr()), vp(sizes.data_ptr()), n, h, w, 1, 0, edges,
                                         vp(bufs["loops"][1]), loop_cap, vp(bufs["points"][1]), point_cap,
                                         vp(bufs["counts"][1]), vp(bufs["ws"][1]), need, None), "unet_trace_class_regions")
    torch.cuda.synchronize()
    for k, (buf, _) in list(bufs.items()) + [("count ws", ws)]:
        assert bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[-MARGIN:] == SENTINEL).all()), k
    inner = {k: buf[MARGIN:-MARGIN].cpu().numpy() for k, (buf, _) in bufs.items()}
    return inner["loops"], inner["points"], inner["counts"].view(np.int64).tolist(), [edges, n_loops, n_points]


def test_direct_call_with_exactly_sized_buffers_and_short_capacities():
    loops, points = _want("speckle0.5")
    got_loops, got_points, counts, counted = _direct("speckle0.5")
    assert counts == counted == [counted[0], len(loops), len(points)]
    assert got_loops.tobytes() == loops.tobytes() and got_points.tobytes() == points.tobytes()
    # one row short: the last row's bytes keep the sentinel, the rest and every point are there, the counts are true
    got_loops, got_points, counts, _ = _direct("speckle0.5", loop_short=1)
    assert counts == counted and got_points.tobytes() == points.tobytes()
    assert got_loops[:-48].tobytes() == loops[:-1].tobytes() and (got_loops[-48:] == SENTINEL).all()
    got_loops, got_points, counts, _ = _direct("speckle0.5", point_short=1)
    assert counts == counted and got_loops.tobytes() == loops.tobytes()
    assert got_points[:-8].tobytes() == points[:-1].tobytes() and (got_points[-8:] == SENTINEL).all()


def test_refused_calls_return_their_codes_before_any_launch():
    lib, vp = L.lib(), ctypes.c_void_p
    x = torch.zeros(16, dtype=torch.int64, device=DEV)
    p = vp(x.data_ptr())
    assert lib.unet_count_class_region_edges_workspace(65536, 1, 1) == 0
    assert lib.unet_count_class_region_edges_workspace(1, 1 << 15, (1 << 14) + 1) == 0          # 2^29 + 2^15 pixels
    assert lib.unet_count_class_region_edges_workspace(1, 1 << 15, 1 << 14) > 0
    assert lib.unet_trace_class_regions_workspace(1, 1 << 15, (1 << 14) + 1, 8) == 0
    assert lib.unet_trace_class_regions_workspace(1, 4, 4, 1 << 31) == 0
    big = (1, 1 << 15, (1 << 14) + 1)
    assert lib.unet_count_class_region_edges(p, p, *big, 1, p, p, 1 << 20, None) == -2
    assert lib.unet_trace_class_regions(p, p, *big, 1, 0, 8, p, 1, p, 1, p, p, 1 << 20, None) == -2
    assert lib.unet_trace_class_regions(p, p, 65536, 1, 1, 1, 0, 8, p, 1, p, 1, p, p, 1 << 20, None) == -2
    assert lib.unet_count_class_region_edges(None, p, 1, 2, 2, 1, p, p, 1 << 20, None) == -1
    assert lib.unet_count_class_region_edges(p, p, 1, 2, 2, 1, None, p, 1 << 20, None) == -1
    assert lib.unet_trace_class_regions(p, None, 1, 2, 2, 1, 0, 8, p, 1, p, 1, p, p, 1 << 20, None) == -1
    assert lib.unet_trace_class_regions(p, p, 1, 2, 2, 1, 0, 8, None, 1, p, 1, p, p, 1 << 20, None) == -1
    assert lib.unet_count_class_region_edges(p, p, 1, 2, 2, 0, p, p, 1 << 20, None) == -1
    assert lib.unet_trace_class_regions(p, p, 1, 2, 2, 0, 0, 8, p, 1, p, 1, p, p, 1 << 20, None) == -1
    assert lib.unet_trace_class_regions(p, p, 1, 2, 2, 1, 0, 8, p, 1, p, 1, p, p, 16, None) == -3       # workspace
    torch.cuda.synchronize()
    assert int(x.abs().sum()) == 0                                                              # nothing ran
    r = torch.zeros((1, 4, 4), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="min_pixels"):
        ops.trace_class_regions(r, r, 0)
    with pytest.raises(ValueError, match="image_base"):
        ops.trace_class_regions(r, r, 1, -1)
    with pytest.raises(ValueError, match="int32"):
        ops.trace_class_regions(r.long(), r)
    with pytest.raises(RuntimeError, match="2\\^29 pixels"):
        ops.trace_class_regions(r[:, :1, :1].expand(1, 1 << 15, (1 << 14) + 1), r[:, :1, :1].expand(1, 1 << 15, (1 << 14) + 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.trace_class_regions(r.cpu(), r.cpu())


def test_the_polygon_kernel_draws_thick_outlines_back_to_the_hole_filled_map():
    maps, C = _case("thick")
    loops, points = _got("thick")
    _assert_equal((loops, points), _want("thick"), "thick")
    h, w = maps.shape[1:]
    polys, want = [], np.zeros((h, w), np.uint8)
    for (image, root), (outer, holes) in polygons.outlines(loops, points).items():
        cls = int(maps[0].ravel()[root])
        assert len(outer) >= 3
        polys.append((cls - 1, [tuple(p) for p in outer.tolist()]))
        lab = ndimage.label(maps[0] == cls, structure=np.ones((3, 3), int))[0]
        want[ndimage.binary_fill_holes(lab == lab.ravel()[root], structure=FOUR)] = cls
    assert sum(len(hs) for _, hs in polygons.outlines(loops, points).values()) == 1           # the ring's hole
    from tiaozhanbei_unet_amd.gear_dataset import flatten_polygons
    got = augment.polygon_masks_u8(flatten_polygons([polys]), [(h, w)], h, w, device=DEV)[0].cpu().numpy()
    assert (want != maps[0]).sum() > 0 and np.array_equal(got, want)
