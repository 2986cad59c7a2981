"""Gear class-overlap analysis on the host (no GPU): the fixture's condition (Pillow and the polygon kernel's documented
rule agree on every file), the Pillow restatement against the reference's recorded statistics, ``overlap_stats`` on
hand-made records, the partial parse, the CLI's flags and the binding's argument checks."""
import numpy as np
import pytest

import _overlap_ref as R
from tiaozhanbei_unet_amd import analyze_gear_overlaps as CLI
from tiaozhanbei_unet_amd import augment as A
from tiaozhanbei_unet_amd import gear_dataset as G
from tiaozhanbei_unet_amd import gear_overlaps as GO


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


@pytest.fixture(scope="module")
def parsed(fx):
    return R.fixture_polys(fx)


def test_fixture_covers_the_listed_cases(fx, parsed):
    assert fx["pillow_version"] == "12.2.0"
    sizes = {f["name"]: tuple(f["size"]) for f in fx["files"]}
    assert {1, 63, 64, 65, 257, 300} <= {w for _, w in sizes.values()} and {1, 2} <= {h for h, _ in sizes.values()}
    polys = {f["name"]: p for f, p in parsed}
    assert [c for c, _ in polys["hand_reverse_order.png"]] == [2, 0]
    assert [c for c, _ in polys["hand_partial_parse.png"]] == [1, 0]            # the line after the bad one is not reached
    assert [c for c, _ in polys["hand_one_class.png"]] == [1]
    assert sorted(c for c, _ in polys["hand_same_class_twice.png"]) == [0, 0, 1, 2]
    oof = [v for _, pts in polys["hand_out_of_frame.png"] for v in pts]
    assert min(x for x, _ in oof) < 0 and max(x for x, _ in oof) >= 300 and min(y for _, y in oof) < 0
    rows = [pts for _, pts in polys["hand_edge_rows.png"]]
    assert sum(y == 0 for _, y in rows[0]) == 2 and sum(y == 23 for _, y in rows[1]) == 2
    assert any(f["label"] is None for f in fx["files"])                          # an image without a label file
    keys = set(fx["reference_stats"]["overlap_pixels"])
    assert {"scrape_vs_pitting", "pitting_vs_scrape"} <= keys                     # both orders of one pair
    for f, ps in parsed:                                                          # no polygon revisits a vertex
        for _, pts in ps:
            body = [v for k, v in enumerate(pts) if k == 0 or v != pts[k - 1]]    # (a point repeated in place is none)
            body = body[:-1] if len(body) > 1 and body[0] == body[-1] else body
            assert len(set(body)) == len(body), f["name"]


def test_pillow_histogram_equals_the_kernel_rule_on_every_fixture_file(parsed):
    for f, polys in parsed:
        h, w = f["size"]
        assert R.histogram(polys, w, h, R.draw_pillow) == R.histogram(polys, w, h, R.draw_rule), f["name"]


def test_pillow_statistics_equal_the_reference(fx, parsed):
    files = [(f["split"], f["name"], R.class_masks(polys, f["size"][1], f["size"][0])) for f, polys in parsed]
    got, want = R.normalised(R.stats_from_masks(files)), fx["reference_stats"]
    assert set(got) == set(want)
    for block in want:
        assert got[block] == want[block], block                                   # ints and floats alike: exact


def test_overlap_stats_from_pillow_histograms_equals_the_reference(fx, parsed):
    records = [(f["split"], f["name"], GO.first_appearance(polys), R.histogram(polys, f["size"][1], f["size"][0]))
               for f, polys in parsed]
    got = R.normalised(GO.to_jsonable(GO.overlap_stats(records)))
    for block, want in fx["reference_stats"].items():
        assert got[block] == want, block
    assert set(got) - set(fx["reference_stats"]) == {"device_extras"}


def test_overlap_stats_pair_keys_follow_first_appearance():
    #        bins:  {}  {0} {1} {01} {2} {02} {12} {012}
    a = ("train", "a.png", [0, 1], [10, 5, 4, 3, 0, 0, 0, 0])
    b = ("train", "b.png", [1, 0], [20, 1, 2, 7, 0, 0, 0, 0])
    c = ("val", "c.png", [2, 0, 1], [1, 2, 3, 4, 5, 6, 7, 8])                     # all eight bins non-zero
    none = ("val", "none.png", [], [99, 0, 0, 0, 0, 0, 0, 0])                     # no polygon: not counted
    clean = ("test", "clean.png", [0, 2], [50, 6, 0, 0, 9, 0, 0, 0])              # two classes that do not touch
    s = GO.overlap_stats([a, b, c, none, clean])
    assert s["overlap_pixels"] == {"pitting_vs_spalling": 3 + (4 + 8), "spalling_vs_pitting": 7,
                                   "scrape_vs_pitting": 6 + 8, "scrape_vs_spalling": 7 + 8}
    assert list(s["overlap_pixels"]) == ["pitting_vs_spalling", "spalling_vs_pitting", "scrape_vs_pitting",
                                         "scrape_vs_spalling"]                    # c: pairs (2,0), (2,1), (0,1) in turn
    assert s["files_with_overlaps"]["pitting_vs_spalling"] == ["train/a.png", "val/c.png"]
    assert s["files_with_overlaps"]["spalling_vs_pitting"] == ["train/b.png"]
    pit = (5 + 3) + (1 + 7) + (2 + 4 + 6 + 8) + 6
    spa = (4 + 3) + (2 + 7) + (3 + 4 + 7 + 8)
    scr = (5 + 6 + 7 + 8) + 9
    assert s["total_pixels_per_class"] == {0: pit, 1: spa, 2: scr}
    assert s["summary"]["total_pixels_per_class_name"] == {"pitting": pit, "spalling": spa, "scrape": scr}
    assert s["summary"]["total_files_processed"] == 4 and s["summary"]["files_with_any_overlap"] == 3
    assert s["summary"]["percentage_files_with_overlap"] == 3 / 4 * 100
    assert s["overlap_percentages"]["spalling_vs_pitting_pct_of_spalling"] == (7 / spa) * 100
    assert s["overlap_percentages"]["spalling_vs_pitting_pct_of_pitting"] == (7 / pit) * 100
    d = [x for x in s["detailed_stats"] if x["file"] == "val/c.png"]
    assert [(x["class_a"], x["class_b"], x["overlap_pixels"]) for x in d] == [
        ("scrape", "pitting", 14), ("scrape", "spalling", 15), ("pitting", "spalling", 12)]
    assert d[0]["class_a_total"] == 26 and d[0]["class_b_total"] == 20 and d[0]["overlap_ratio_a"] == 14 / 26
    assert GO.to_jsonable(s)["total_pixels_per_class"] == {"0": pit, "1": spa, "2": scr}
    assert GO.to_jsonable(s)["summary"]["class_names"] == {"0": "pitting", "1": "spalling", "2": "scrape"}


def test_overlap_stats_without_files():
    s = GO.overlap_stats([("train", "none.png", [], [4, 0, 0, 0, 0, 0, 0, 0])])
    assert s["summary"]["total_files_processed"] == 0 and s["summary"]["percentage_files_with_overlap"] == 0
    assert s["overlap_pixels"] == {} and s["detailed_stats"] == [] and s["total_pixels_per_class"] == {}


def test_device_extras_from_a_full_histogram():
    hist = [1, 2, 3, 4, 5, 6, 7, 8]
    s = GO.overlap_stats([("val", "c.png", [2, 0, 1], hist, {0: 2, 1: 1, 2: 3}),
                          ("val", "d.png", [1], [10, 0, 5, 0, 0, 0, 0, 0], {1: 4})])
    x = s["device_extras"]
    assert x["overlap_matrix"] == [[0, 4 + 8, 6 + 8], [4 + 8, 0, 7 + 8], [6 + 8, 7 + 8, 0]]
    assert x["triple_overlap_pixels"] == 8
    assert x["pixels_per_class_after_priority"] == {"background": 1 + 10, "pitting": 2 + 6, "spalling": 3 + 4 + 7 + 8 + 5,
                                                    "scrape": 5}
    assert sum(x["pixels_per_class_after_priority"].values()) == sum(hist) + 15
    assert x["polygon_instances_per_class"] == {"pitting": 2, "spalling": 5, "scrape": 3}
    assert x == R.extras_from_histograms([hist, [10, 0, 5, 0, 0, 0, 0, 0]],
                                         [[(0, None)] * 2 + [(1, None)] + [(2, None)] * 3, [(1, None)] * 4])


def test_partial_parse_keeps_the_earlier_lines(tmp_path, capsys):
    p = tmp_path / "a.txt"
    p.write_text("0 0.1 0.1 0.5 0.1 0.5 0.5\n2 0.2 0.2 0.6 0.2 0.6 0.6\n1 0.1 0.2 abc 0.4 0.5 0.6\n1 0.1 0.1 0.5 0.1 0.5 0.5\n")
    assert G.parse_labelme_txt(str(p), 100, 50) == []                             # the dataset's rule, unchanged
    assert capsys.readouterr().out == ""
    kept = G.parse_labelme_txt(str(p), 100, 50, keep_partial=True)
    assert kept == [(0, [(10, 5), (50, 5), (50, 25)]), (2, [(20, 10), (60, 10), (60, 30)])]
    out = capsys.readouterr().out
    assert out.startswith("Warning: Could not parse label file") and "abc" in out
    p.write_text("x 0.1 0.1 0.5 0.1 0.5 0.5\n")
    assert G.parse_labelme_txt(str(p), 100, 50, keep_partial=True) == []
    assert GO.first_appearance(kept + [(0, [(1, 1), (2, 2), (3, 1)])]) == [0, 2]


def test_scan_reads_headers_and_labels_only(fx, tmp_path, capsys):
    root = tmp_path / "g"
    for sub in ("images/train", "labels/train"):
        (root / sub).mkdir(parents=True)
    from PIL import Image
    Image.new("RGB", (40, 30)).save(root / "images/train/b.png")
    Image.new("RGB", (40, 30)).save(root / "images/train/a.png")
    Image.new("RGB", (40, 30)).save(root / "images/train/unlabelled.png")
    (root / "labels/train/a.txt").write_text("5 0.1 0.1 0.5 0.1 0.5 0.5\n2 0.1 0.1 0.5 0.1 0.5 0.5\n")
    (root / "labels/train/b.txt").write_text("")
    entries = GO.scan(str(root), ["train", "val"])
    assert [(e[0], e[1], e[2]) for e in entries] == [("train", "a.png", (30, 40)), ("train", "b.png", (30, 40))]
    assert entries[0][3] == [(2, [(4, 3), (20, 3), (20, 15)])] and entries[1][3] == []
    out = capsys.readouterr().out
    assert out.count("raw class ids [5]") == 1 and "Skipping val split" in out
    ang = np.linspace(0, 2 * np.pi, 600, endpoint=False)
    xy = np.stack([0.5 + 0.4 * np.cos(ang), 0.5 + 0.4 * np.sin(ang)], 1).reshape(-1)
    (root / "labels/train/b.txt").write_text("1 " + " ".join(f"{v:.6f}" for v in xy) + "\n")
    with pytest.raises(ValueError, match="b.txt.*600 vertices"):
        GO.scan(str(root), ["train"])
    (root / "labels/train/b.txt").write_text("1 0.1 0.1 0.5 0.1 0.5 0.5\n")
    Image.new("L", (4097, 2)).save(root / "images/train/b.png")
    with pytest.raises(ValueError, match="b.png.*4097 pixels wide"):
        GO.scan(str(root), ["train"])


def test_cli_flags_match_reference():
    args = vars(CLI.parse_args([]))
    assert args["data_root"] == "datasets/Gear" and args["splits"] == ["train", "val", "test"]
    assert args["save_dir"] == "overlap_analysis"                                 # reference analyze_class_overlaps.py
    assert set(args) == {"data_root", "splits", "save_dir", "batch_size", "synthetic"}
    assert args["batch_size"] == 32 and args["synthetic"] is False
    assert CLI.parse_args(["--splits", "val"]).splits == ["val"]


def _tri(n_vertices=3):
    ang = np.linspace(0, 2 * np.pi, n_vertices, endpoint=False)
    return [(int(50 + 40 * np.cos(t)), int(50 + 40 * np.sin(t))) for t in ang]


def test_binding_refuses_bad_arguments_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library must not be reached")
    monkeypatch.setattr(A.L, "lib", no_library)
    tri = G.flatten_polygons([[(0, _tri())]])
    with pytest.raises(ValueError, match="4097 pixels wide"):
        A.polygon_class_histogram(tri, [(8, 4097)], device="cuda:0")
    with pytest.raises(ValueError, match="513 vertices"):
        A.polygon_class_histogram(G.flatten_polygons([[(1, [(i, i * i) for i in range(513)])]]), [(100, 100)],
                                  device="cuda:0")
    two = G.flatten_polygons([[(0, _tri())], [(1, _tri())]])
    two["images"] = two["images"][::-1].copy()
    with pytest.raises(ValueError, match="non-decreasing"):
        A.polygon_class_histogram(two, [(100, 100), (100, 100)], device="cuda:0")
    with pytest.raises(ValueError, match="at least one image"):
        A.polygon_class_histogram(G.flatten_polygons([]), [], device="cuda:0")
    with pytest.raises(ValueError, match="2\\^24"):
        A.polygon_class_histogram(G.flatten_polygons([[(0, [(0, 0), (1 << 24, 0), (5, 5)])]]), [(10, 10)],
                                  device="cuda:0")
