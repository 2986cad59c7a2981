#!/usr/bin/env python3
"""Generate tests/golden/gear_overlaps.json by running the REFERENCE's class-overlap analysis itself (build container
only: it needs a checkout of the reference, which the GPU box does not have).

Imports the reference's ``analyze_class_overlaps.py`` (``seaborn`` -- absent from the image, used there only by the
charts -- is stubbed, as tools/make_goldens_gear.py stubs ``torchvision``), writes a Gear-layout tree
(``gear_dataset.write_synthetic_gear``'s default tree plus the hand-written files below) and calls the reference's
``calculate_overlaps`` on it.  Stored: per file the split, name, (h, w) and label text, and the reference's returned
statistics with every dict key a string, counts as ints and the lists whose order is ``os.listdir`` order sorted.  Only
data is stored, nothing of the reference's source text.

    python tools/make_goldens_overlaps.py --reference <path of the reference checkout>
"""
import argparse
import json
import os
import sys
import tempfile
import types

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "gear_overlaps.json")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
from tiaozhanbei_unet_amd.gear_dataset import write_synthetic_gear  # noqa: E402


def px(pts, w, h):
    """Normalised text for integer pixel points: the midpoint of the pixel's preimage, so int(t * size) lands on it."""
    def t(v, size):
        return (v + 0.5) / size if v >= 0 else (v - 0.5) / size      # int() truncates toward zero
    return " ".join(f"{t(x, w)!r} {t(y, h)!r}" for x, y in pts)


def line(cls, pts, w, h):
    return f"{cls} {px(pts, w, h)}"


def hand_written():
    """(split, stem, (h, w), label text): no polygon revisits a vertex (the kernel's known divergence from Pillow)."""
    out = []

    def add(split, stem, h, w, lines):
        out.append((split, stem, (h, w), "\n".join(lines) + "\n"))

    # first polygon scrape (raw 2), then pitting (raw 0): the pair key comes out as scrape_vs_pitting
    add("train", "hand_reverse_order", 30, 65, [line(2, [(3, 2), (40, 4), (44, 25), (5, 22)], 65, 30),
                                                line(0, [(20, 10), (63, 12), (60, 28), (24, 27)], 65, 30)])
    # the same two classes in the other order, so that both keys accumulate
    add("train", "hand_forward_order", 31, 64, [line(0, [(2, 3), (50, 2), (48, 20), (4, 24)], 64, 31),
                                                line(2, [(30, 8), (62, 9), (61, 29), (28, 30)], 64, 31)])
    # two valid overlapping polygons, a malformed line, a valid line that is never reached: the partial parse is kept
    add("train", "hand_partial_parse", 40, 64, [line(1, [(4, 4), (40, 6), (36, 30), (6, 33)], 64, 40),
                                                line(0, [(20, 12), (60, 10), (58, 38), (22, 36)], 64, 40),
                                                "2 0.1 0.2 oops 0.4 0.5 0.6",
                                                line(2, [(0, 0), (63, 0), (63, 39), (0, 39)], 64, 40)])
    add("val", "hand_one_class", 20, 63, [line(1, [(5, 2), (58, 9), (21, 18)], 63, 20)])
    # two pitting polygons overlap each other and both other classes: OR within a class, a triple overlap
    add("val", "hand_same_class_twice", 50, 257, [line(0, [(10, 5), (150, 8), (140, 40), (12, 44)], 257, 50),
                                                  line(0, [(100, 3), (250, 6), (245, 47), (95, 45)], 257, 50),
                                                  line(2, [(60, 15), (200, 12), (210, 35), (55, 38)], 257, 50),
                                                  line(1, [(120, 1), (135, 2), (170, 48), (110, 49)], 257, 50)])
    # partly outside the frame: coordinates below 0 and above 1
    add("val", "hand_out_of_frame", 35, 300, [line(0, [(-40, -9), (200, -6), (330, 20), (120, 50), (-25, 30)], 300, 35),
                                              line(1, [(150, 10), (340, 5), (310, 44), (160, 30)], 300, 35)])
    # a horizontal edge on row 0 and another on the last row
    add("test", "hand_edge_rows", 24, 48, [line(0, [(3, 0), (30, 0), (25, 14), (6, 12)], 48, 24),
                                           line(2, [(10, 23), (44, 23), (40, 8), (14, 6)], 48, 24)])
    add("test", "hand_width_1", 9, 1, [line(0, [(-2, 1), (3, 2), (-1, 7)], 1, 9),
                                       line(1, [(-3, 3), (2, 3), (2, 8), (-3, 8)], 1, 9)])
    add("test", "hand_height_1", 1, 70, [line(2, [(5, -3), (40, -2), (30, 4)], 70, 1),
                                         line(0, [(20, -2), (60, -1), (50, 3)], 70, 1)])
    add("test", "hand_height_2", 2, 33, [line(1, [(2, -4), (30, -3), (20, 5)], 33, 2),
                                         line(2, [(8, 1), (28, 1), (26, 6), (9, 5)], 33, 2)])
    return out


def plain(v):
    """numpy scalars -> Python numbers, dict keys -> strings"""
    if isinstance(v, dict):
        return {str(k): plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, np.integer):
        return int(v)
    if isinstance(v, np.floating):
        return float(v)
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (read-only)")
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
    import analyze_class_overlaps as ref          # the reference

    with tempfile.TemporaryDirectory() as tmp:
        root = write_synthetic_gear(os.path.join(tmp, "gear"))
        for split, stem, (h, w), text in hand_written():
            Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(os.path.join(root, "images", split, stem + ".png"))
            with open(os.path.join(root, "labels", split, stem + ".txt"), "w") as f:
                f.write(text)
        files = []
        for split in ("train", "val", "test"):
            for name in sorted(os.listdir(os.path.join(root, "images", split))):
                label = os.path.join(root, "labels", split, os.path.splitext(name)[0] + ".txt")
                with Image.open(os.path.join(root, "images", split, name)) as im:
                    w, h = im.size
                text = open(label).read() if os.path.exists(label) else None
                files.append({"split": split, "name": name, "size": [h, w], "label": text})
        stats = plain(dict(ref.calculate_overlaps(root)))
    for k in stats["files_with_overlaps"]:
        stats["files_with_overlaps"][k].sort()
    stats["detailed_stats"].sort(key=lambda d: (d["file"], d["class_a"], d["class_b"]))
    with open(OUT, "w") as f:
        json.dump({"pillow_version": PIL.__version__, "files": files, "reference_stats": stats}, f, indent=1)
    s = stats["summary"]
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.0f} kB): {len(files)} files, {s['total_files_processed']} counted, "
          f"{s['files_with_any_overlap']} with overlaps, pairs {sorted(stats['overlap_pixels'])}")


if __name__ == "__main__":
    main()
