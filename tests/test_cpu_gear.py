"""Gear loader, label parsing and the polygon fill rule on the host (no GPU).

The fill rule below is a numpy restatement of what csrc/polygon.hip computes.  It reproduces every full-resolution mask
of tests/golden/gear_masks.npz (made by the reference's own mask builder, i.e. Pillow's ImageDraw.polygon) except the
``diverge_*`` cases: polygons that revisit a vertex, where the reconstructed corner rule is known to differ from Pillow
by a few pixels.  Those are pinned as strict xfails, so a completed rule shows up as an unexpected pass."""
import math
import os

import numpy as np
import pytest

from tiaozhanbei_unet_amd import gear_dataset as G
from tiaozhanbei_unet_amd import train_gear

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "gear_masks.npz")
F = np.float32


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


DIVERGENT = "diverge_"


def _cases(gold, divergent=None):
    """(index, name) of the fixture cases; divergent=False / True keeps only the exact / the known-divergent ones"""
    out = [(i, str(n)) for i, n in enumerate(gold["names"])]
    if divergent is None:
        return out
    return [(i, n) for i, n in out if n.startswith(DIVERGENT) == divergent]


# ------------------------------------------------------------------------------------------------ the fill rule
def _round_up(f):      # Draw.c ROUND_UP: float f + 0.5F, then floor
    return int(math.floor(F(f) + F(0.5))) if f >= 0 else -int(math.floor(F(abs(f)) + F(0.5)))


def _round_down(f):
    return int(math.ceil(F(f) - F(0.5))) if f >= 0 else -int(math.ceil(F(abs(f)) - F(0.5)))


def _roundf(f):        # C roundf: halves away from zero
    return F(math.floor(f + 0.5) if f >= 0 else -math.floor(-f + 0.5))


def fill_polygon(pts, w, h):
    """ImageDraw.polygon(pts, fill=1) on an h x w 8-bit image, restated."""
    m = np.zeros((h, w), np.uint8)
    n = len(pts)
    seg = [(pts[i], pts[i + 1]) for i in range(n - 1)]
    if pts[-1] != pts[0]:
        seg.append((pts[-1], pts[0]))
    x0 = np.array([a[0] for a, _ in seg]); y0 = np.array([a[1] for a, _ in seg])
    x1 = np.array([b[0] for _, b in seg]); y1 = np.array([b[1] for _, b in seg])
    ylo, yhi = np.minimum(y0, y1), np.maximum(y0, y1)
    horiz = ylo == yhi
    with np.errstate(divide="ignore", invalid="ignore"):
        dx = np.where(horiz, F(0), (x1 - x0).astype(F) / (y1 - y0).astype(F)).astype(F)
    poly_ymax = max(p[1] for p in pts)

    def xat(k, y):
        return F(F(F(y - y0[k]) * dx[k]) + F(x0[k]))

    for k in np.nonzero(horiz)[0]:                       # horizontal edges: drawn as lines
        if 0 <= y0[k] < h:
            a, b = max(min(x0[k], x1[k]), 0), min(max(x0[k], x1[k]), w - 1)
            if a <= b:
                m[y0[k], a:b + 1] = 1
    for y in range(max(int(ylo.min()), 0), min(int(yhi.max()), h - 1) + 1):
        xs = []
        for k in np.nonzero(~horiz & (ylo <= y) & (y <= yhi))[0]:
            x = xat(k, y)
            if y == yhi[k] and y < poly_ymax:            # the lower end of an edge counts twice
                xs += [x, x]
                continue
            if dx[k] != 0 and float(x).is_integer() and y in (ylo[k], yhi[k]):
                for o in range(k):                       # corner fix-up against an earlier edge
                    if horiz[o] or y not in (ylo[o], yhi[o]):
                        continue
                    if (dx[k] > 0 and dx[o] <= 0) or (dx[k] < 0 and dx[o] >= 0) or x != xat(o, y):
                        continue
                    y2 = y - 1 if y == yhi[k] else y + 1
                    if not ylo[o] <= y2 <= yhi[o]:
                        continue
                    a, b = xat(k, y2), xat(o, y2)
                    if x > F(a + F(1)) and x > F(b + F(1)):
                        x = F(_roundf(max(a, b)) + F(1))
                    elif x < F(a - F(1)) and x < F(b - F(1)):
                        x = F(_roundf(min(a, b)) - F(1))
                    break
            xs.append(x)
        xs.sort()
        for i in range(1, len(xs), 2):
            a, b = max(_round_up(xs[i - 1]), 0), min(_round_down(xs[i]), w - 1)
            if a <= b:
                m[y, a:b + 1] = 1
    return m


def class_mask(verts, offsets, classes, w, h):
    """OR per raw class, then priority: raw 1 -> 2 over raw 0 -> 1 over raw 2 -> 3; other raw classes ignored."""
    cover = {c: np.zeros((h, w), bool) for c in (0, 1, 2)}
    for p, c in enumerate(classes):
        if int(c) in cover:
            pts = [tuple(int(v) for v in xy) for xy in verts[offsets[p]:offsets[p + 1]]]
            cover[int(c)] |= fill_polygon(pts, w, h).astype(bool)
    out = np.zeros((h, w), np.uint8)
    out[cover[2]] = 3
    out[cover[0]] = 1
    out[cover[1]] = 2
    return out


def test_fixture_pins_pillow(gold):
    assert str(gold["pillow_version"]) == "12.2.0"
    names = [n for _, n in _cases(gold)]
    for needed in ("square", "triangle", "bowtie", "out_of_frame", "horizontal_edges", "vertical_edges", "collinear",
                   "repeated_points", "overlap_all_three", "malformed", "labelme_1920x1080_0"):
        assert needed in names
    sq = gold[f"{names.index('square')}_full"]
    assert int(sq.sum()) == 49 and sq[2:9, 2:9].all()                   # both boundary edges included


def _restated(gold, i):
    h, w = (int(v) for v in gold[f"{i}_size"])
    return class_mask(gold[f"{i}_verts"], gold[f"{i}_offsets"], gold[f"{i}_classes"], w, h)


def test_fill_rule_reproduces_every_full_resolution_mask(gold):
    for i, name in _cases(gold, divergent=False):
        got, ref = _restated(gold, i), gold[f"{i}_full"]
        assert np.array_equal(got, ref), f"{name}: {int((got != ref).sum())} pixels differ"


def test_known_divergence_is_small_and_on_revisited_vertex_rows(gold):
    """The gap of the reconstructed corner rule: a few pixels, only on rows through a vertex the polygon visits twice."""
    cases = _cases(gold, divergent=True)
    assert len(cases) >= 8
    for i, name in cases:
        got, ref = _restated(gold, i), gold[f"{i}_full"]
        diff = got != ref
        assert 0 < int(diff.sum()) <= 8, name
        verts = [tuple(v) for v in gold[f"{i}_verts"].tolist()]
        revisited_rows = {y for (x, y) in verts if verts.count((x, y)) > 1}
        assert set(np.nonzero(diff.any(1))[0].tolist()) <= revisited_rows, name


@pytest.mark.xfail(strict=True, reason="corner fix-up condition of Pillow's polygon fill not fully reconstructed")
def test_fill_rule_reproduces_known_divergent_masks(gold):
    for i, name in _cases(gold, divergent=True):
        assert np.array_equal(_restated(gold, i), gold[f"{i}_full"]), name


# ------------------------------------------------------------------------------------------------ parsing
def test_parser_matches_fixture_vertices(gold, tmp_path):
    for i, name in _cases(gold):
        h, w = (int(v) for v in gold[f"{i}_size"])
        path = tmp_path / f"{i}.txt"
        path.write_bytes(gold[f"{i}_label"].tobytes())
        polys = G.parse_labelme_txt(str(path), w, h)
        flat = G.flatten_polygons([[(c, p) for c, p in polys]])
        keep = np.isin(gold[f"{i}_classes"], (0, 1, 2))
        ref_polys = [(int(c), [tuple(v) for v in gold[f"{i}_verts"][gold[f"{i}_offsets"][p]:gold[f"{i}_offsets"][p + 1]].tolist()])
                     for p, c in enumerate(gold[f"{i}_classes"])]
        assert [(c, p) for c, p in polys] == ref_polys, name
        assert len(flat["classes"]) == int(keep.sum())


def test_parser_edge_cases(tmp_path):
    p = tmp_path / "a.txt"
    p.write_text("0 0.1 0.1 0.5\n1 0.1 0.1 0.5 0.1\n2 0.1 0.1 0.5 0.1 0.5 0.5 0.9\n\n")
    assert G.parse_labelme_txt(str(p), 100, 50) == [(2, [(10, 5), (50, 5), (50, 25)])]
    p.write_text("0 0.1 0.1 0.5 0.1 0.5 0.5\n1 0.1 0.2 abc 0.4 0.5 0.6\n")
    assert G.parse_labelme_txt(str(p), 100, 50) == []                  # any exception: no polygons at all
    p.write_text("0 -0.25 1.5 0.5 0.1 0.5 0.5\n")
    assert G.parse_labelme_txt(str(p), 100, 50) == [(0, [(-25, 75), (50, 5), (50, 25)])]   # truncation toward zero


# ------------------------------------------------------------------------------------------------ CLI contract
REFERENCE_TRAIN_FLAGS = {  # reference train.py:26-97, pinned here as data
    "data_root": "datasets/Gear", "image_size": 512, "model": "seg_unet", "bilinear": False, "dropout": 0.1,
    "epochs": 50, "batch_size": 8, "learning_rate": 1e-3, "weight_decay": 1e-4, "optimizer": "adam",
    "ce_weight": 1.0, "dice_weight": 1.0, "focal_weight": 0.0, "class_weights": None, "num_workers": 4,
    "device": "auto", "seed": 42, "save_dir": "outputs", "save_freq": 10, "resume": None, "val_freq": 5,
    "debug": False, "debug_samples": 20,
}


def test_train_gear_flags_match_reference():
    args = vars(train_gear.parse_args([]))
    for k, v in REFERENCE_TRAIN_FLAGS.items():
        assert args[k] == v, k
    assert set(args) - set(REFERENCE_TRAIN_FLAGS) == {"precision", "synthetic", "sync_mask"}
    assert args["precision"] == "fp32" and not args["synthetic"] and not args["sync_mask"]
    choices = {name: kw.get("choices") for name, kw in train_gear.FLAGS}
    assert choices["--model"] == ["unet", "seg_unet"] and choices["--optimizer"] == ["adam", "adamw", "sgd"]


def test_train_gear_refuses_cpu(capsys):
    with pytest.raises(SystemExit) as e:
        train_gear.main(["--device", "cpu"])
    assert "no CPU path" in str(e.value)


# ------------------------------------------------------------------------------------------------ dataset
def test_synthetic_tree_pairing_and_collate(tmp_path):
    root = G.write_synthetic_gear(str(tmp_path / "gear"))
    ds = G.GearDataset(root, "train", (64, 64), raw=True)
    assert len(ds) == 6                                              # the unlabelled image is skipped
    assert all(os.path.splitext(os.path.basename(i))[0] == os.path.splitext(os.path.basename(l))[0]
               for i, l in zip(ds.image_paths, ds.label_paths))
    assert ds.image_paths == sorted(ds.image_paths)
    assert ds.class_names == ["pitting", "spalling", "scrape"] and ds.num_classes == 4
    samples = [ds[i] for i in range(len(ds))]
    assert samples[0][1] == [] and samples[1][1] == []               # empty and malformed label files
    images, polys, sizes, paths = G.collate_raw(samples)
    assert isinstance(images, list) and len(sizes) == 6 and sizes[0] == tuple(samples[0][0].shape[:2])
    n_polys = sum(len(s[1]) for s in samples)
    assert len(polys["classes"]) == n_polys and polys["offsets"][-1] == len(polys["verts"])
    assert np.all(np.diff(polys["images"]) >= 0) and set(polys["images"].tolist()) <= set(range(2, 6))
    assert polys["verts"].shape[1] == 2


def test_class_count_follows_reference(tmp_path):
    root = tmp_path / "g"
    for sub in ("images/train", "labels/train"):
        (root / sub).mkdir(parents=True)
    from PIL import Image
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(root / "images/train/a.png")
    (root / "labels/train/a.txt").write_text("2 0.1 0.1 0.5 0.1 0.5 0.5\n5 0.1 0.1 0.5 0.1 0.5 0.5\n")
    ds = G.GearDataset(str(root), "train")
    assert ds.class_names == ["scrape"] and ds.num_classes == 2


def test_host_eval_sample_shapes(tmp_path):
    root = G.write_synthetic_gear(str(tmp_path / "gear"))
    ds = G.GearDataset(root, "val", (24, 40), raw=False)
    x, m, _ = ds[2]
    assert tuple(x.shape) == (3, 24, 40) and tuple(m.shape) == (24, 40) and str(m.dtype) == "torch.int64"


def test_oversized_polygon_is_refused_when_the_dataset_is_built(tmp_path):
    root = tmp_path / "g"
    for sub in ("images/train", "labels/train"):
        (root / sub).mkdir(parents=True)
    from PIL import Image
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(root / "images/train/big.png")
    ang = np.linspace(0, 2 * np.pi, 600, endpoint=False)
    xy = np.stack([0.5 + 0.4 * np.cos(ang), 0.5 + 0.4 * np.sin(ang)], 1).reshape(-1)
    (root / "labels/train/big.txt").write_text("1 " + " ".join(f"{v:.6f}" for v in xy) + "\n")
    with pytest.raises(ValueError, match="big.txt.*600 vertices"):
        G.GearDataset(str(root), "train")
