"""CPU checks of the named class-region result: the fields of ``evaluation.RegionRecords``, the export of
``class_region_records`` through ``ops``, and its refusal of a bad ``merge_gap`` before anything touches a device."""
import pytest

from tiaozhanbei_unet_amd import evaluation, ops


def test_the_result_names_its_five_members_in_order():
    assert evaluation.RegionRecords._fields == ("records", "shapes", "loops", "points", "fragments")
    assert evaluation.RegionRecords() == (None,) * 5


def test_the_entry_point_and_its_result_are_exported_through_ops():
    assert ops.class_region_records is evaluation.class_region_records
    assert ops.RegionRecords is evaluation.RegionRecords


def test_merge_gap_is_refused_outside_its_range_before_anything_runs():
    for bad in (-1, 33):
        for flags in ({}, {"describe": False, "directions": 16}, {"contours": True}):
            with pytest.raises(ValueError, match="merge_gap"):
                evaluation.class_region_records(None, 4, merge_gap=bad, **flags)
