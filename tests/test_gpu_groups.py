"""GPU tests of the fragment grouping (csrc/groups.hip through ops.group_class_regions, the merge_gap keyword of the
describe / measure calls and of ops.DetectionMatcher) against the numpy restatement of tests/_groups_ref.py, which
test_cpu_groups.py pins to an all-pairs distance.  Integers throughout: every output is compared for equality.  The maps
are tests/_groups_cases.py's: frames of one pixel, one row and one column, 33 x 65 (tile borders at 32 and 64) and
3 x 40 x 100, at the gaps 1, 2, 5 and 32."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _defects_ref as D
import _groups_cases as K
import _groups_ref as G
from _seg_regions_ref import class_regions64
from tiaozhanbei_unet_amd import _lib as L
from tiaozhanbei_unet_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(s, k) for s in K.SHAPES for k in K.KINDS if not (s == (1, 1, 1) and k != "layout")]


@functools.lru_cache(maxsize=None)
def _want(shape, kind, gap, min_pixels=1, image_base=0):
    out = G.group_regions64(K.maps_of(shape, kind), K.C, gap, min_pixels, image_base)
    for a in out:
        a.setflags(write=False)
    return out


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)       # a copy: the cases are read-only


def _got(maps, gap, min_pixels=1, image_base=0):
    t = _dev(maps)
    region, sizes, _ = ops.label_class_regions(t, K.C)
    group, gsizes, counts, frag = ops.group_class_regions(t, region, sizes, K.C, gap, min_pixels, image_base)
    assert group.dtype == torch.int32 and gsizes.dtype == torch.int32 and counts.dtype == torch.int64
    assert frag.dtype == np.int64
    return group.cpu().numpy(), gsizes.cpu().numpy(), counts.cpu().numpy(), frag


def _assert_outputs(got, want, what):
    for name, g, w in zip(("group", "group_sizes", "counts", "fragments"), got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g.astype(np.int64) != w)
        assert bad.size == 0, f"{what}: {name} differs first at {bad[0].tolist()}: " \
                              f"{g[tuple(bad[0])]} != {w[tuple(bad[0])]} ({len(bad)} in all)"


@pytest.mark.parametrize("gap", K.GAPS)
@pytest.mark.parametrize("shape,kind", CASES)
def test_outputs_equal_the_reference(shape, kind, gap):
    _assert_outputs(_got(K.maps_of(shape, kind), gap), _want(shape, kind, gap), f"{shape} {kind} gap {gap}")


@pytest.mark.parametrize("gap", K.GAPS)
@pytest.mark.parametrize("shape,kind", [((2, 33, 65), "layout"), ((3, 40, 100), "layout"), ((3, 40, 100), "speckle30")])
def test_min_pixels_drops_regions_before_grouping(shape, kind, gap):
    for mp, base in ((2, 0), (3, 7)):
        want = _want(shape, kind, gap, mp, base)
        _assert_outputs(_got(K.maps_of(shape, kind), gap, mp, base), want, f"{shape} {kind} gap {gap} min_pixels {mp}")
    if kind == "layout" and gap == 5:                  # the bridge pixel is gone: the two blocks stay apart
        frag = _want(shape, kind, 5, 2)[3]
        w = shape[2]
        blocks = frag[(frag[:, 0] == 0) & np.isin(frag[:, 2], (14 * w + 2, 14 * w + 11))]
        assert len(blocks) == 2 and (blocks[:, 2] == blocks[:, 3]).all()


@pytest.mark.parametrize("shape,kind", CASES)
def test_gap_one_is_the_labelling_with_dropped_regions_zeroed(shape, kind):
    maps = K.maps_of(shape, kind)
    region, sizes, counts = class_regions64(maps, K.C)
    for mp in (1, 2):
        group, gsizes, gcounts, frag = _got(maps, 1, mp)
        keep = sizes >= mp
        assert np.array_equal(group, np.where(keep, region, 0)) and np.array_equal(gsizes, np.where(keep, sizes, 0))
        assert np.array_equal(frag[:, 2], frag[:, 3]) and gcounts.sum() == len(frag)
        if mp == 1:
            assert np.array_equal(gcounts, counts)


def test_two_calls_give_the_same_bytes():
    maps = K.maps_of((3, 40, 100), "speckle30")
    a, b = _got(maps, 5), _got(maps, 5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _raw_call(maps, gap, capacity, counts_start, count_start, min_pixels=1):
    """unet_group_class_regions through ctypes with buffers of the test's own: (counts, fragment_count, records)"""
    t = _dev(maps)
    n, h, w = t.shape
    region, sizes, _ = ops.label_class_regions(t, K.C)
    lib = L.lib()
    group, gsizes = torch.empty_like(region), torch.empty_like(sizes)
    counts = torch.full((n, K.C), counts_start, dtype=torch.int64, device=DEV)
    count = torch.full((1,), count_start, dtype=torch.int64, device=DEV)
    records = torch.full((max(capacity, 1) + 2, 5), -7, dtype=torch.int64, device=DEV)     # two rows of guard
    nbytes = lib.unet_group_class_regions_workspace(n, h, w, K.C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    rc = lib.unet_group_class_regions(t.data_ptr(), region.data_ptr(), sizes.data_ptr(), n, h, w, K.C, gap, min_pixels, 0,
                                      group.data_ptr(), gsizes.data_ptr(), counts.data_ptr(), records.data_ptr(), capacity,
                                      count.data_ptr(), ws.data_ptr(), nbytes, ctypes.c_void_p(0))
    assert rc == 0, lib.unet_last_error()
    torch.cuda.synchronize()
    return counts.cpu().numpy(), int(count), records.cpu().numpy(), group.cpu().numpy()


def test_counts_and_fragment_count_are_added_to():
    shape, kind = (3, 40, 100), "layout"
    want = _want(shape, kind, 5)
    counts, count, records, _ = _raw_call(K.maps_of(shape, kind), 5, len(want[3]), 100, 0)
    assert np.array_equal(counts[:, 1:], want[2][:, 1:] + 100) and (counts[:, 0] == 100).all()      # column 0 untouched
    assert count == len(want[3])
    rec = records[:count]
    assert np.array_equal(rec[np.lexsort((rec[:, 2], rec[:, 3], rec[:, 0]))], want[3])
    assert (records[count:] == -7).all()


def test_a_capacity_overflow_is_counted_and_not_written():
    shape, kind = (3, 40, 100), "speckle30"
    want = _want(shape, kind, 2)
    total, cap = len(want[3]), 10
    assert total > 100
    # the count starts at 3: the slots 3 .. 9 are written, every fragment is counted, nothing lands past the capacity
    counts, count, records, group = _raw_call(K.maps_of(shape, kind), 2, cap, 0, 3)
    assert count == total + 3
    assert (records[:3] == -7).all() and (records[cap:] == -7).all() and (records[3:cap] != -7).all()
    have = {tuple(r) for r in want[3].tolist()}
    assert all(tuple(r) in have for r in records[3:cap].tolist())
    assert np.array_equal(group, want[0]) and np.array_equal(counts, want[2])      # the maps do not depend on the buffer


@pytest.mark.parametrize("gap", (2, 5, 32))
def test_described_and_measured_groups_are_the_sums_of_their_fragments(gap):
    shape, kind, mp, base = (3, 40, 100), "layout", 2, 4
    maps = K.maps_of(shape, kind)
    rng = np.random.default_rng(5)
    conf = rng.random(maps.shape, dtype=np.float32)
    rec, shapes, frag = ops.describe_and_measure_class_regions(_dev(maps), K.C, _dev(conf), min_pixels=mp, image_base=base,
                                                               merge_gap=gap)
    want_frag = _want(shape, kind, gap, mp, base)[3]
    assert np.array_equal(frag, want_frag)
    parts = D.describe_records(maps, K.C, conf, mp, base)                      # one row per fragment, by (image, root)
    key = {(int(f[0]), int(f[2])): int(f[3]) for f in want_frag}
    groups = sorted({(int(f[0]), int(f[3])) for f in want_frag})
    assert len(rec) == len(groups) == len(shapes) and (len(groups) < len(parts) if gap >= 5 else len(groups) <= len(parts))
    assert np.array_equal(rec[:, [0, 2, 3]], shapes[:, :3])                    # the rows align
    for row, (image, root) in zip(rec, groups):
        mine = parts[[key[(int(p[0]), int(p[2]))] == root and int(p[0]) == image for p in parts]]
        assert (row[0], row[2]) == (image, root) and row[1] == mine[0, 1]
        assert row[3] == mine[:, 3].sum()
        assert row[4:8].tolist() == [mine[:, 4].min(), mine[:, 5].min(), mine[:, 6].max(), mine[:, 7].max()]
        assert row[8:11].tolist() == mine[:, 8:11].sum(0).tolist() and row[11] == mine[:, 11].max()
    # the single calls give the same rows, and merge_gap = 0 keeps its arity
    rec1, frag1 = ops.describe_class_regions(_dev(maps), K.C, _dev(conf), min_pixels=mp, image_base=base, merge_gap=gap)
    shapes1, frag2 = ops.measure_class_regions(_dev(maps), K.C, min_pixels=mp, image_base=base, merge_gap=gap)
    assert np.array_equal(rec1, rec) and np.array_equal(shapes1, shapes)
    assert np.array_equal(frag1, frag) and np.array_equal(frag2, frag)
    plain = ops.describe_and_measure_class_regions(_dev(maps), K.C, _dev(conf), min_pixels=mp, image_base=base)
    assert len(plain) == 2 and np.array_equal(plain[0], parts)


def test_contours_stay_those_of_the_fragments():
    shape, kind = (2, 33, 65), "layout"
    maps = K.maps_of(shape, kind)
    rec, shapes, loops, points, frag = ops.describe_and_measure_class_regions(_dev(maps), K.C, min_pixels=2, contours=True,
                                                                              merge_gap=5)
    plain = ops.describe_and_measure_class_regions(_dev(maps), K.C, min_pixels=2, contours=True)
    assert np.array_equal(loops, plain[2]) and np.array_equal(points, plain[3])
    outer = loops[loops[:, 5] > 0]
    assert sorted(zip(outer[:, 0].tolist(), outer[:, 1].tolist())) == sorted(zip(frag[:, 0].tolist(), frag[:, 2].tolist()))
    assert np.array_equal(frag, _want(shape, kind, 5, 2)[3]) and len(rec) < len(frag)


def test_detection_matcher_pairs_a_broken_bar_as_one_defect():
    truth = np.zeros((1, 20, 60), np.uint8)
    truth[0, 8:11, 5:50] = 2
    pred = truth.copy()
    pred[0, :, 18:21] = 0                              # two breaks of 3 pixels: pieces of 13, 14 and 12 columns
    pred[0, :, 35:38] = 0
    conf = np.full(truth.shape, 0.75, np.float32)
    pieces = [3 * 13, 3 * 14, 3 * 12]
    res = {}
    for gap in (0, 4):
        m = ops.DetectionMatcher(3, min_pixels=1, merge_gap=gap)
        m.update(_dev(pred), _dev(conf), _dev(truth))
        res[gap] = m.compute()
    assert res[0]["pred"][:, 3].tolist() == pieces and res[0]["pairs"][:, 3].tolist() == pieces
    assert len(res[4]["pred"]) == 1 and len(res[4]["truth"]) == 1
    one = res[4]["pred"][0]
    assert one[2] == 8 * 60 + 5 and one[3] == sum(pieces) and one[4:8].tolist() == [5, 8, 49, 10]
    assert res[4]["pairs"].tolist() == [[0, 8 * 60 + 5, 8 * 60 + 5, sum(pieces)]]
    assert np.array_equal(res[4]["truth"], res[0]["truth"])
    with pytest.raises(ValueError):
        ops.DetectionMatcher(3, merge_gap=33)
