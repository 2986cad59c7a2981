"""GPU tests of the Gear class-overlap analysis: the histogram kernel (csrc/polygon.hip through
augment.polygon_class_histogram) exact against Pillow on tests/golden/gear_overlaps.json and on the non-divergent cases
of tests/golden/gear_masks.npz, against the documented rule on the divergent ones, consistent with the mask kernel, and
the analyze_gear_overlaps CLI end to end against the reference's recorded statistics.  Everything is integer counting:
zero tolerance throughout."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import _overlap_ref as R
from test_cpu_gear import DIVERGENT
from tiaozhanbei_unet_amd import _lib as L
from tiaozhanbei_unet_amd import augment as A
from tiaozhanbei_unet_amd import gear_dataset as G
from tiaozhanbei_unet_amd import gear_overlaps as GO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


@pytest.fixture(scope="module")
def files(fx):
    """[(file record, polygons, Pillow histogram)] of the fixture's labelled files, computed once"""
    return [(f, polys, R.histogram(polys, f["size"][1], f["size"][0])) for f, polys in R.fixture_polys(fx)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "gear_masks.npz"))


def _hist(polys_per_image, sizes):
    return A.polygon_class_histogram(G.flatten_polygons(polys_per_image), sizes, device=DEV).cpu().tolist()


def _gold_polys(gold, i):
    return [(int(c), [tuple(v) for v in gold[f"{i}_verts"][gold[f"{i}_offsets"][p]:gold[f"{i}_offsets"][p + 1]].tolist()])
            for p, c in enumerate(gold[f"{i}_classes"])]


def test_every_fixture_file_alone_equals_pillow(files):
    assert sum(bool(polys) for _, polys, _ in files) >= 18
    for f, polys, want in files:
        assert _hist([polys], [tuple(f["size"])]) == [want], f["name"]


def test_fixture_as_one_mixed_size_batch_equals_pillow(files):
    """The grid scans as many rows as the tallest image has; images without polygons sit between images with some."""
    has = [bool(polys) for _, polys, _ in files]
    assert any(not has[k] and any(has[:k]) and any(has[k + 1:]) for k in range(len(has)))
    sizes = [tuple(f["size"]) for f, _, _ in files]
    assert len({h for h, _ in sizes}) > 4 and len({w for _, w in sizes}) > 4
    got = _hist([polys for _, polys, _ in files], sizes)
    for (f, _, want), row in zip(files, got):
        assert row == want, f["name"]


def test_exact_cases_of_the_mask_fixture_equal_pillow_and_the_stored_masks(gold):
    idx = [i for i, n in enumerate(gold["names"]) if not str(n).startswith(DIVERGENT)]
    polys = [_gold_polys(gold, i) for i in idx]
    sizes = [tuple(int(v) for v in gold[f"{i}_size"]) for i in idx]
    got = _hist(polys, sizes)
    for i, ps, (h, w), row in zip(idx, polys, sizes, got):
        assert row == R.histogram(ps, w, h), gold["names"][i]
        assert R.collapse(row) == np.bincount(gold[f"{i}_full"].reshape(-1), minlength=4).tolist(), gold["names"][i]


def test_divergent_cases_of_the_mask_fixture_follow_the_documented_rule(gold):
    idx = [i for i, n in enumerate(gold["names"]) if str(n).startswith(DIVERGENT)]
    assert len(idx) >= 8
    polys = [_gold_polys(gold, i) for i in idx]
    sizes = [tuple(int(v) for v in gold[f"{i}_size"]) for i in idx]
    for i, ps, (h, w), row in zip(idx, polys, sizes, _hist(polys, sizes)):
        assert row == R.histogram(ps, w, h, R.draw_rule), gold["names"][i]


def test_collapsed_bins_equal_the_mask_kernels_class_counts(files):
    for f, polys, _ in files:
        h, w = f["size"]
        flat = G.flatten_polygons([polys])
        mask = A.polygon_masks_u8(flat, [(h, w)], h, w, device=DEV)
        hist = A.polygon_class_histogram(flat, [(h, w)], device=DEV)
        assert R.collapse(hist[0].tolist()) == torch.bincount(mask.reshape(-1).long(), minlength=4).tolist(), f["name"]


def test_bins_sum_to_the_frame_and_runs_are_identical(files):
    polys, sizes = G.flatten_polygons([p for _, p, _ in files]), [tuple(f["size"]) for f, _, _ in files]
    a = A.polygon_class_histogram(polys, sizes, device=DEV)
    b = A.polygon_class_histogram(polys, sizes, device=DEV)
    torch.cuda.synchronize()
    assert a.dtype == torch.int64 and tuple(a.shape) == (len(sizes), 8)
    assert torch.equal(a, b)
    assert a.sum(1).tolist() == [h * w for h, w in sizes]


def test_nine_polygons_of_one_class_count_as_their_union():
    """More than two polygons per wave, all of one class, overlapping: OR-ed, not summed."""
    h, w = 70, 100
    nine = [(1, [(5 + 9 * k, 4 + 3 * k), (40 + 6 * k, 2 + 5 * k), (35 + 7 * k, 30 + 4 * k), (8 + 8 * k, 28 + 2 * k)])
            for k in range(9)]
    union = np.zeros((h, w), bool)
    for _, pts in nine:
        union |= R.draw_pillow(pts, w, h)
    covered = int(union.sum())
    assert sum(int(R.draw_pillow(pts, w, h).sum()) for _, pts in nine) > covered > 0
    assert _hist([nine], [(h, w)]) == [[h * w - covered, 0, covered, 0, 0, 0, 0, 0]]
    assert _hist([nine + [(2, [(0, 0), (99, 0), (99, 69), (0, 69)])]], [(h, w)]) == [
        [0, 0, 0, 0, h * w - covered, 0, covered, 0]]


def test_widest_frame_with_a_polygon_over_the_full_row():
    h, w = 3, 4096
    polys = [(0, [(0, 0), (4095, 0), (4095, 2), (0, 2)]), (2, [(100, -5), (4000, 1), (2000, 9)]),
             (1, [(4090, 0), (4200, 1), (4090, 2)])]
    want = R.histogram(polys, w, h)
    assert want[0] == 0 and want[1] > 0 and want[5] > 0 and want[3] > 0
    assert _hist([polys], [(h, w)]) == [want]
    assert _hist([[], polys, []], [(5, 7), (h, w), (1, 1)]) == [[35, 0, 0, 0, 0, 0, 0, 0], want, [1, 0, 0, 0, 0, 0, 0, 0]]


def test_narrowest_frames():
    for (h, w), polys in [((9, 1), [(0, [(-2, 1), (3, 2), (-1, 7)]), (1, [(-3, 3), (2, 3), (2, 8), (-3, 8)])]),
                          ((1, 70), [(2, [(5, -3), (40, -2), (30, 4)]), (0, [(20, -2), (60, -1), (50, 3)])]),
                          ((1, 1), [(1, [(-1, -1), (2, -1), (0, 3)])])]:
        assert _hist([polys], [(h, w)]) == [R.histogram(polys, w, h)], (h, w)


def test_batch_without_polygons_needs_no_launch(monkeypatch):
    def no_library():
        raise AssertionError("the library must not be reached")
    monkeypatch.setattr(L, "lib", no_library)
    got = A.polygon_class_histogram(G.flatten_polygons([[], []]), [(30, 40), (2, 4096)], device=DEV)
    assert got.dtype == torch.int64 and got.device.type == "cuda"
    assert got.tolist() == [[1200, 0, 0, 0, 0, 0, 0, 0], [8192, 0, 0, 0, 0, 0, 0, 0]]


def test_library_refuses_what_the_kernel_cannot_take():
    buf = torch.zeros(64, dtype=torch.int64, device=DEV)
    p, lib = buf.data_ptr(), L.lib()

    def call(n_polys=1, max_v=3, n=1, max_h=4, max_w=4, hist=p, verts=p):
        return lib.unet_polygon_class_histogram(verts, p, p, p, n_polys, max_v, p, n, max_h, max_w, hist, None)
    assert call(max_w=4097) == -2 and b"4096" in lib.unet_last_error()
    assert call(n=65536) == -2
    assert call(max_v=513) == -2 and b"512" in lib.unet_last_error()
    assert call(hist=None) == -1 and call(n=0) == -1 and call(max_h=0) == -1 and call(verts=None) == -1
    torch.cuda.synchronize()
    assert not buf.any()                                                          # nothing was launched


def _write_tree(fx, root):
    for f in fx["files"]:
        h, w = f["size"]
        for sub in ("images", "labels"):
            os.makedirs(os.path.join(root, sub, f["split"]), exist_ok=True)
        Image.new("RGB", (w, h)).save(os.path.join(root, "images", f["split"], f["name"]))
        if f["label"] is not None:
            with open(os.path.join(root, "labels", f["split"], os.path.splitext(f["name"])[0] + ".txt"), "w") as out:
                out.write(f["label"])
    return root


def test_cli_reproduces_the_reference_statistics(fx, files, tmp_path):
    root, save = _write_tree(fx, str(tmp_path / "gear")), tmp_path / "out"
    cmd = [sys.executable, "-m", "tiaozhanbei_unet_amd.analyze_gear_overlaps", "--data_root", root, "--save_dir",
           str(save), "--batch_size", "5"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.count("Warning: Could not parse label file") == 4          # three generated files, one written
    assert "HIGH OVERLAP DETECTED" in res.stdout and "Top 10 largest overlaps" in res.stdout
    got = R.normalised(json.load(open(save / "overlap_analysis_detailed.json")))
    want = fx["reference_stats"]
    assert set(got) == set(want) | {"device_extras"}
    for block in want:
        assert got[block] == want[block], block
    drawn = [(hist, polys) for _, polys, hist in files if polys]
    assert got["device_extras"] == R.extras_from_histograms([h for h, _ in drawn], [p for _, p in drawn])
    assert got["device_extras"]["triple_overlap_pixels"] > 0


def test_cli_synthetic_runs_to_completion(tmp_path):
    cmd = [sys.executable, "-m", "tiaozhanbei_unet_amd.analyze_gear_overlaps", "--synthetic", "--save_dir",
           str(tmp_path / "out")]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-3000:]
    stats = json.load(open(tmp_path / "out" / "overlap_analysis_detailed.json"))
    assert stats["summary"]["total_files_processed"] == 8                         # 4 + 2 + 2 files with polygons
    assert GO.to_jsonable(stats) == stats
