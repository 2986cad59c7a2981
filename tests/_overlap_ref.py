"""Host restatement of the Gear class-overlap analysis for the tests: Pillow draws every polygon, the drawings are OR-ed
per raw class, and the report comes from ``&`` and sums over the full masks -- the route the reference's
analyze_class_overlaps.py takes, written from its described behaviour.  Also the same histogram from the polygon
kernel's documented fill rule (test_cpu_gear.fill_polygon) and the loader of tests/golden/gear_overlaps.json."""
import json
import os

import numpy as np
from PIL import Image, ImageDraw

from test_cpu_gear import fill_polygon

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gear_overlaps.json")
NAMES = {0: "pitting", 1: "spalling", 2: "scrape"}


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def parse(text, w, h):
    """[(class, points)] of a label text with the overlap script's rule: what was parsed before an exception is kept."""
    polys = []
    try:
        for ln in text.splitlines():
            parts = ln.strip().split()
            if len(parts) < 5:
                continue
            cls = int(parts[0])
            c = [float(t) for t in parts[1:]]
            pts = [(int(c[i] * w), int(c[i + 1] * h)) for i in range(0, len(c) - 1, 2)]
            if len(pts) >= 3:
                polys.append((cls, pts))
    except Exception:
        pass
    return polys


def fixture_polys(fx):
    """[(file record, polygons)] of the fixture's labelled files"""
    return [(f, parse(f["label"], f["size"][1], f["size"][0])) for f in fx["files"] if f["label"] is not None]


def draw_pillow(pts, w, h):
    im = Image.new("L", (w, h), 0)
    ImageDraw.Draw(im).polygon(pts, fill=1)
    return np.array(im).astype(bool)


def draw_rule(pts, w, h):
    return fill_polygon(pts, w, h).astype(bool)


def class_masks(polys, w, h, draw=draw_pillow):
    """{raw class: bool mask} in order of first appearance, raw classes 0..2 only"""
    masks = {}
    for cls, pts in polys:
        if cls in NAMES:
            masks[cls] = masks.get(cls, np.zeros((h, w), bool)) | draw(pts, w, h)
    return masks


def histogram(polys, w, h, draw=draw_pillow):
    """hist[b] = pixels whose set of covering raw classes is exactly b"""
    code = np.zeros((h, w), np.int64)
    for cls, m in class_masks(polys, w, h, draw).items():
        code |= m.astype(np.int64) << cls
    return np.bincount(code.reshape(-1), minlength=8).tolist()


def collapse(hist):
    """[background, pitting, spalling, scrape] pixel counts after the priority rule raw 1 > raw 0 > raw 2"""
    h = [int(v) for v in hist]
    return [h[0], h[1] + h[5], h[2] + h[3] + h[6] + h[7], h[4]]


def stats_from_masks(files):
    """The reference's statistics blocks from [(split, name, {class: mask})], by pairwise mask algebra; keys as strings"""
    total, overlap, where, detailed = {}, {}, {}, []
    n_files = n_overlap = 0
    for split, name, masks in files:
        if not masks:
            continue
        n_files += 1
        for c, m in masks.items():
            total[c] = total.get(c, 0) + int(m.sum())
        ids, hit = list(masks), False
        for i, a in enumerate(ids):
            for b in ids[i + 1:]:
                ov = int((masks[a] & masks[b]).sum())
                if ov == 0:
                    continue
                hit = True
                key = f"{NAMES[a]}_vs_{NAMES[b]}"
                overlap[key] = overlap.get(key, 0) + ov
                where.setdefault(key, []).append(f"{split}/{name}")
                ta, tb = int(masks[a].sum()), int(masks[b].sum())
                detailed.append({"file": f"{split}/{name}", "class_a": NAMES[a], "class_b": NAMES[b], "overlap_pixels": ov,
                                 "class_a_total": ta, "class_b_total": tb, "overlap_ratio_a": ov / ta, "overlap_ratio_b": ov / tb})
        n_overlap += hit
    back = {v: k for k, v in NAMES.items()}
    pct = {}
    for key, ov in overlap.items():
        a, b = key.split("_vs_")
        pct[f"{key}_pct_of_{a}"] = ov / total[back[a]] * 100
        pct[f"{key}_pct_of_{b}"] = ov / total[back[b]] * 100
    return {"total_pixels_per_class": {str(k): v for k, v in total.items()}, "overlap_pixels": overlap,
            "overlap_percentages": pct, "files_with_overlaps": where, "detailed_stats": detailed,
            "summary": {"total_files_processed": n_files, "files_with_any_overlap": n_overlap,
                        "percentage_files_with_overlap": n_overlap / n_files * 100 if n_files else 0,
                        "class_names": {str(k): v for k, v in NAMES.items()},
                        "total_pixels_per_class_name": {NAMES[k]: v for k, v in total.items()}}}


def extras_from_histograms(hists, polys_per_file):
    """The device_extras block from per-file histograms (files with a polygon only) and their polygons"""
    matrix = [[0] * 3 for _ in range(3)]
    after = [0, 0, 0, 0]
    census = {n: 0 for n in NAMES.values()}
    triple = 0
    for hist, polys in zip(hists, polys_per_file):
        for a in range(3):
            for b in range(3):
                if a != b:
                    matrix[a][b] += sum(int(hist[m]) for m in range(8) if m >> a & 1 and m >> b & 1)
        after = [x + y for x, y in zip(after, collapse(hist))]
        triple += int(hist[7])
        for cls, _ in polys:
            if cls in NAMES:
                census[NAMES[cls]] += 1
    return {"overlap_matrix": matrix, "triple_overlap_pixels": triple,
            "pixels_per_class_after_priority": dict(zip(("background", "pitting", "spalling", "scrape"), after)),
            "polygon_instances_per_class": census}


def normalised(stats):
    """Statistics with the lists whose order follows the directory listing sorted, as the fixture stores them"""
    out = dict(stats)
    out["files_with_overlaps"] = {k: sorted(v) for k, v in stats["files_with_overlaps"].items()}
    out["detailed_stats"] = sorted(stats["detailed_stats"], key=lambda d: (d["file"], d["class_a"], d["class_b"]))
    return out
