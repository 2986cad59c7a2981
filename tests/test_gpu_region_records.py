"""GPU tests of the named class-region result (ops.class_region_records -> ops.RegionRecords): every combination of its
options against the numpy restatements the family's own tests trust (tests/_defects_ref.py, _shapes_ref.py, _groups_ref.py,
_contours_ref.py; never against the three older functions, which share its code), the tuple shapes those three keep, and
the number of host reads of every function of the family.  Integers throughout: arrays are compared byte for byte."""
import functools
import itertools
import warnings

import numpy as np
import pytest
import torch

import _contours_ref as R
import _defects_ref as D
import _groups_cases as K
import _groups_ref as G
import _shapes_ref as S
from _seg_regions_ref import class_regions64
from tiaozhanbei_unet_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEMBERS = ops.RegionRecords._fields
MIN_PIXELS, BASE, DIRECTIONS, GAP = 2, 4, 16, 5
BIG, SMALL = (3, 40, 100), (2, 33, 65)
# (describe, directions, contours, merge_gap) without the one that asks for nothing
OPTIONS = [o for o in itertools.product((True, False), (None, DIRECTIONS), (False, True), (0, GAP)) if any(o)]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)       # a copy: the cases are read-only


@functools.lru_cache(maxsize=None)
def _conf(shape):
    conf = np.random.default_rng(5).random(shape, dtype=np.float32)
    conf.setflags(write=False)
    return conf


def _shapes_of_masks(ids, min_pixels, image_base, directions):
    """tests/_shapes_ref.py's record of every number of the int maps ``ids`` [n, h, w] (1 + root index, 0: nothing), the
    pixels of one number taken as one mask, connected or not: what a group's shape record is defined as"""
    table = S.directions(directions)
    out = []
    for i in range(ids.shape[0]):
        for number in np.unique(ids[i][ids[i] > 0]).tolist():
            mask = ids[i] == number
            ys, xs = np.nonzero(mask)
            if len(xs) < min_pixels:
                continue
            p = xs[:, None] * table[None, :, 0] + ys[:, None] * table[None, :, 1]
            out.append([image_base + i, number - 1, len(xs), int((xs * xs).sum()), int((ys * ys).sum()), int((xs * ys).sum()),
                        *S.quads(mask), *p.min(axis=0).tolist(), *p.max(axis=0).tolist()])
    a = np.array(out, np.int64).reshape(-1, S.HEAD + 2 * directions)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


@functools.lru_cache(maxsize=None)
def _want(shape, gap):
    """every member of the result for ``K.maps_of(shape, "layout")`` at MIN_PIXELS, BASE, DIRECTIONS, from numpy alone"""
    maps, conf = K.maps_of(shape, "layout"), _conf(shape)
    region, sizes, _ = class_regions64(maps, K.C)
    loops, points = R.trace(region, sizes, MIN_PIXELS, BASE)       # the outlines are the fragments' at every gap
    if gap:
        records, fragments = G.describe_groups(maps, K.C, gap, conf, MIN_PIXELS, BASE)
        group = G.group_regions64(maps, K.C, gap, MIN_PIXELS, BASE)[0]
        shapes = _shapes_of_masks(group, 1, BASE, DIRECTIONS)      # dropped regions are 0 in the group map already
    else:
        records, fragments = D.describe_records(maps, K.C, conf, MIN_PIXELS, BASE), None
        shapes = S.shape_records(maps, K.C, MIN_PIXELS, BASE, DIRECTIONS)
        assert np.array_equal(shapes, _shapes_of_masks(region, MIN_PIXELS, BASE, DIRECTIONS))      # the helper is the reference
    want = ops.RegionRecords(records, shapes, loops, points, fragments)
    for a in want:
        if a is not None:
            a.setflags(write=False)
    return want


def _asked(describe, directions, contours, gap):
    return dict(zip(MEMBERS, (describe, directions is not None, contours, contours, bool(gap))))


def _same(got, want, what):
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, \
        (what, getattr(got, "dtype", None), getattr(got, "shape", None), want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), f"{what}: first difference at {np.argwhere(got != want)[0].tolist()}"


@pytest.mark.parametrize("describe,directions,contours,gap", OPTIONS)
def test_every_member_asked_for_equals_the_reference_and_the_rest_is_none(describe, directions, contours, gap):
    got = ops.class_region_records(_dev(K.maps_of(BIG, "layout")), K.C, _dev(_conf(BIG)), MIN_PIXELS, BASE, describe=describe,
                                   directions=directions, contours=contours, merge_gap=gap)
    assert type(got) is ops.RegionRecords
    want = _want(BIG, gap)
    for name, asked in _asked(describe, directions, contours, gap).items():
        if asked:
            _same(getattr(got, name), getattr(want, name), f"{name} at {(describe, directions, contours, gap)}")
        else:
            assert getattr(got, name) is None, name
    if describe and directions is not None:
        assert np.array_equal(got.records[:, [0, 2, 3]], got.shapes[:, :3])      # the rows align, grouped or not
    if gap:
        assert len(want.records) < len(want.fragments) and len(want.shapes) == len(want.records)
    if contours and gap:
        _same(got.loops, _want(BIG, 0).loops, "loops are those of merge_gap=0")


@pytest.mark.parametrize("describe,directions,contours,gap", OPTIONS)
def test_maps_without_a_region_give_empty_arrays_for_what_was_asked(describe, directions, contours, gap):
    nothing = torch.zeros((1, 5, 5), dtype=torch.uint8, device=DEV)
    got = ops.class_region_records(nothing, K.C, describe=describe, directions=directions, contours=contours, merge_gap=gap)
    empty = {"records": ((0, 12), np.int64), "shapes": ((0, 11 + 2 * 16), np.int64), "loops": ((0, 6), np.int64),
             "points": ((0, 2), np.int32), "fragments": ((0, 5), np.int64)}
    for name, asked in _asked(describe, directions, contours, gap).items():
        member = getattr(got, name)
        if asked:
            assert (member.shape, member.dtype) == empty[name], name
        else:
            assert member is None, name


def _members(got, names):
    return [getattr(got, n) for n in names]


def _same_elements(out, members):
    assert type(out) is tuple and len(out) == len(members)
    for a, b in zip(out, members):
        assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes())


# (directions, contours, merge_gap) -> the members of the returned tuple, in its order
BOTH_FORMS = [((DIRECTIONS, False, 0), ("records", "shapes")),
              ((DIRECTIONS, False, GAP), ("records", "shapes", "fragments")),
              ((DIRECTIONS, True, 0), ("records", "shapes", "loops", "points")),
              ((DIRECTIONS, True, GAP), ("records", "shapes", "loops", "points", "fragments")),
              ((None, True, 0), ("records", "shapes", "loops", "points")),
              ((None, True, GAP), ("records", "shapes", "loops", "points", "fragments"))]


@pytest.mark.parametrize("form,names", BOTH_FORMS)
def test_describe_and_measure_keeps_its_tuple_shapes(form, names):
    directions, contours, gap = form
    maps, conf = _dev(K.maps_of(SMALL, "layout")), _dev(_conf(SMALL))
    out = ops.describe_and_measure_class_regions(maps, K.C, conf, MIN_PIXELS, BASE, directions, contours=contours,
                                                 merge_gap=gap)
    named = ops.class_region_records(maps, K.C, conf, MIN_PIXELS, BASE, directions=directions, contours=contours,
                                     merge_gap=gap)
    _same_elements(out, _members(named, names))
    assert len(out[0]) > 0 and (out[1] is None) == (directions is None)
    empty = ops.describe_and_measure_class_regions(torch.zeros((1, 5, 5), dtype=torch.uint8, device=DEV), K.C, None, 1, 0,
                                                   directions, contours=contours, merge_gap=gap)
    assert len(empty) == len(names)


@pytest.mark.parametrize("gap", (0, GAP))
def test_no_directions_without_contours_stay_refused_by_describe_and_measure(gap):
    """the two forms of (directions, contours, merge_gap) that it has never taken: the named entry gives ``shapes=None``
    there, the older function keeps saying that ``directions`` is no number"""
    maps = _dev(K.maps_of(SMALL, "layout"))
    with pytest.raises(TypeError):
        ops.describe_and_measure_class_regions(maps, K.C, None, MIN_PIXELS, BASE, None, merge_gap=gap)
    got = ops.class_region_records(maps, K.C, None, MIN_PIXELS, BASE, merge_gap=gap)
    assert got.shapes is None and len(got.records) > 0 and (got.fragments is None) == (gap == 0)


@pytest.mark.parametrize("gap", (0, GAP))
def test_describe_and_measure_alone_keep_an_array_or_a_pair(gap):
    maps, conf = _dev(K.maps_of(SMALL, "layout")), _dev(_conf(SMALL))
    described = ops.describe_class_regions(maps, K.C, conf, MIN_PIXELS, BASE, merge_gap=gap)
    measured = ops.measure_class_regions(maps, K.C, MIN_PIXELS, BASE, DIRECTIONS, merge_gap=gap)
    named = ops.class_region_records(maps, K.C, conf, MIN_PIXELS, BASE, directions=DIRECTIONS, merge_gap=gap)
    shapes_only = ops.class_region_records(maps, K.C, None, MIN_PIXELS, BASE, describe=False, directions=DIRECTIONS,
                                           merge_gap=gap)
    assert shapes_only.records is None
    if gap:
        _same_elements(described, [named.records, named.fragments])
        _same_elements(measured, [shapes_only.shapes, shapes_only.fragments])
    else:
        assert type(described) is np.ndarray and type(measured) is np.ndarray
        _same_elements((described, measured), [named.records, shapes_only.shapes])
    _same_elements((named.shapes,), [shapes_only.shapes])


def _host_reads(call):
    """how many synchronising operations ``call`` makes, after one untimed call that loads the library and the allocator"""
    call()
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            call()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    # (the first switch to "warn" in a process also says, once, that the mode is a prototype: that is no read)
    reads = [w for w in caught if "called a synchronizing" in str(w.message)]
    print(f"{len(reads)} host reads, {len(caught)} warnings in all")
    return len(reads)


@pytest.mark.parametrize("gap", (0, GAP))
def test_host_reads_of_the_describing_functions(gap):
    """two: the region counts, then every record set in one buffer; the outlines are a third"""
    maps, conf = _dev(K.maps_of(SMALL, "layout")), _dev(_conf(SMALL))
    args = (maps, K.C, conf, MIN_PIXELS, BASE)
    assert _host_reads(lambda: ops.describe_class_regions(*args, merge_gap=gap)) == 2
    assert _host_reads(lambda: ops.measure_class_regions(maps, K.C, MIN_PIXELS, BASE, DIRECTIONS, merge_gap=gap)) == 2
    assert _host_reads(lambda: ops.describe_and_measure_class_regions(*args, DIRECTIONS, merge_gap=gap)) == 2
    assert _host_reads(lambda: ops.describe_and_measure_class_regions(*args, DIRECTIONS, contours=True, merge_gap=gap)) == 3
    assert _host_reads(lambda: ops.class_region_records(*args, merge_gap=gap)) == 2
    assert _host_reads(lambda: ops.class_region_records(*args, describe=False, directions=DIRECTIONS, merge_gap=gap)) == 2
    assert _host_reads(lambda: ops.class_region_records(*args, directions=DIRECTIONS, merge_gap=gap)) == 2
    assert _host_reads(lambda: ops.class_region_records(*args, directions=DIRECTIONS, contours=True, merge_gap=gap)) == 3


def test_host_reads_of_grouping_tracing_and_pairing():
    maps = _dev(K.maps_of(SMALL, "layout"))
    region, sizes, _ = ops.label_class_regions(maps, K.C)
    other = ops.label_class_regions(maps.flip(-1).contiguous(), K.C)[0]
    assert _host_reads(lambda: ops.group_class_regions(maps, region, sizes, K.C, GAP, MIN_PIXELS, BASE)) == 2
    assert _host_reads(lambda: ops.trace_class_regions(region, sizes, MIN_PIXELS, BASE)) == 2
    assert len(ops.pair_class_regions(region, other, BASE)) > 0
    assert _host_reads(lambda: ops.pair_class_regions(region, other, BASE)) == 2
