#!/usr/bin/env python3
"""Generate tests/golden/gear_masks.npz by running the REFERENCE's Gear mask builder itself (build container only).

Imports /root/reference/src/gear_dataset.py (read-only; ``torchvision`` -- absent from the image, used there only by
the transform helpers -- is stubbed), writes seeded LabelMe label files, runs ``GearDataset._create_mask_from_labelme``
on each and resizes the result with ``Image.resize((w, h), NEAREST)`` as its target transform does.  Stored per case:
the label text bytes, the source size (h, w), the vertex arrays (``int(float(tok) * size)`` of the parsed tokens), the
full-resolution mask and the masks at 512 x 512 and at a non-square size.  Nothing from the reference's source text is
stored.  The fixtures travel to the GPU box; /root/reference does not.

    python tools/make_goldens_gear.py
"""
import os
import sys
import tempfile
import types

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "gear_masks.npz")
RESIZES = {"r512": (512, 512), "rns": (288, 512)}          # (h, w)
# cases on which csrc/polygon.hip's reconstructed corner rule is known to differ from Pillow (tests pin them as xfail)
KNOWN_DIVERGENT_PREFIX = "diverge_"
# two small dense blobs (random, 10..200 vertices, radius 5..20 px) in which int() truncation repeats vertices
BLOB_A = [(64, 66), (62, 66), (63, 67), (67, 68), (66, 70), (60, 67), (62, 70), (65, 72), (60, 70), (61, 74), (58,
          71), (61, 76), (57, 72), (55, 76), (54, 73), (54, 73), (55, 78), (55, 79), (50, 75), (49, 74), (49, 73),
          (48, 77), (47, 76), (46, 79), (44, 79), (43, 77), (44, 72), (43, 71), (41, 72), (43, 71), (41, 70), (41,
          70), (36, 73), (38, 70), (39, 68), (33, 70), (32, 68), (35, 65), (33, 62), (33, 62), (33, 57), (37, 58),
          (40, 58), (41, 56), (40, 55), (39, 52), (42, 55), (41, 46), (42, 46), (45, 53), (44, 48), (45, 50), (47,
          51), (48, 51), (48, 50), (48, 46), (49, 51), (51, 51), (51, 51), (57, 47), (57, 47), (55, 53), (57, 51),
          (55, 54), (59, 49), (61, 53), (59, 56), (59, 57), (60, 59), (63, 58), (61, 60), (62, 60)]
BLOB_B = [(25, 16), (26, 16), (27, 17), (25, 17), (24, 17), (26, 18), (26, 18), (23, 20), (22, 20), (23, 21), (24,
          24), (23, 23), (21, 21), (22, 24), (20, 21), (21, 26), (19, 23), (17, 25), (17, 25), (16, 24), (16, 26),
          (14, 26), (15, 25), (15, 23), (14, 21), (13, 22), (12, 23), (13, 21), (10, 21), (9, 21), (10, 19), (9, 19),
          (7, 19), (5, 20), (9, 17), (8, 17), (8, 17), (8, 16), (5, 17), (8, 16), (6, 16), (9, 15), (7, 14), (5, 14),
          (8, 14), (4, 12), (5, 10), (8, 11), (5, 10), (8, 8), (11, 10), (10, 7), (9, 5), (10, 4), (10, 4), (12, 7),
          (14, 6), (13, 4), (13, 4), (14, 6), (14, 4), (14, 4), (15, 3), (16, 5), (16, 2), (16, 3), (17, 3), (16, 6),
          (17, 5), (20, 5), (21, 3), (22, 5), (23, 6), (23, 7), (23, 8), (26, 8), (23, 9), (24, 9), (26, 9), (27, 11),
          (24, 12), (27, 12), (25, 14), (25, 14), (27, 14)]

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference/src")
_tv = types.ModuleType("torchvision")
_tv.transforms = types.ModuleType("torchvision.transforms")
sys.modules.setdefault("torchvision", _tv)
sys.modules.setdefault("torchvision.transforms", _tv.transforms)
import gear_dataset as ref  # noqa: E402  (the reference)


def px(pts, w, h):
    """Normalised text for integer pixel points: the midpoint of the pixel's preimage, so int(t * size) lands on it."""
    def t(v, size):
        return (v + 0.5) / size if v >= 0 else (v - 0.5) / size      # int() truncates toward zero
    return " ".join(f"{t(x, w)!r} {t(y, h)!r}" for x, y in pts)


def line(cls, pts, w, h):
    return f"{cls} {px(pts, w, h)}"


def blob(rng, cx, cy, r, nv, w, h):
    ang = np.sort(rng.uniform(0, 2 * np.pi, nv))
    rr = r * rng.uniform(0.55, 1.0, nv)
    return " ".join(f"{float((cx + a * np.cos(t)) / w)!r} {float((cy + a * np.sin(t)) / h)!r}" for a, t in zip(rr, ang))


def cases():
    rng = np.random.default_rng(20240611)
    w, h = 40, 30
    out = []

    def add(name, text, size=(h, w)):
        out.append((name, text, size))

    add("square", line(0, [(2, 2), (8, 2), (8, 8), (2, 8)], w, h))
    add("triangle", line(0, [(3, 3), (20, 5), (6, 25)], w, h))
    add("bowtie", line(1, [(2, 2), (20, 20), (20, 2), (2, 20)], w, h))
    add("out_of_frame", line(2, [(-10, -5), (50, 4), (30, 45), (-3, 20)], w, h))
    add("horizontal_edges", line(0, [(2, 5), (10, 5), (18, 5), (18, 12), (9, 12), (9, 20), (2, 20)], w, h))
    add("vertical_edges", line(1, [(5, 2), (5, 10), (5, 25), (12, 25), (12, 2)], w, h))
    add("collinear", line(0, [(3, 2), (5, 1), (7, 0)], w, h) + "\n" + line(2, [(1, 1), (10, 10), (20, 20)], w, h))
    add("repeated_points", line(1, [(4, 4), (4, 4), (15, 6), (15, 6), (8, 18), (4, 4)], w, h))
    add("single_point", line(0, [(7, 7), (7, 7), (7, 7)], w, h))
    add("flat_line", line(2, [(3, 9), (30, 9), (12, 9)], w, h))
    add("touching_corners", line(0, [(12, 6), (12, 9), (3, 3)], w, h) + "\n" + line(2, [(6, 3), (12, 0), (20, 3), (12, 6)], w, h))
    sq = [(4, 4), (24, 4), (24, 20), (4, 20)]
    sh = [(14, 10), (34, 10), (34, 27), (14, 27)]
    add("overlap_spalling_over_pitting", line(0, sq, w, h) + "\n" + line(1, sh, w, h))
    add("overlap_spalling_over_scrape", line(1, sq, w, h) + "\n" + line(2, sh, w, h))
    add("overlap_pitting_over_scrape", line(2, sq, w, h) + "\n" + line(0, sh, w, h))
    add("overlap_all_three", "\n".join([line(2, [(2, 2), (30, 2), (30, 26), (2, 26)], w, h), line(0, sq, w, h),
                                         line(1, [(10, 8), (20, 8), (15, 28)], w, h)]))
    add("ignored_raw_classes", line(3, sq, w, h) + "\n" + line(7, sh, w, h) + "\n" + line(2, [(0, 0), (6, 0), (0, 6)], w, h))
    add("short_lines_and_odd_coords", "\n".join([
        "0 0.1 0.1 0.5",                                                 # 4 tokens: skipped
        "1 0.1 0.1 0.5 0.1",                                             # 2 points: skipped
        line(2, [(5, 5), (25, 6), (15, 22)], w, h) + " 0.9",             # odd trailing coordinate dropped
        "", "   ",
        line(0, [(30, 2), (38, 2), (34, 12)], w, h)]))
    add("malformed", line(0, sq, w, h) + "\n1 0.1 0.2 abc 0.4 0.5 0.6\n" + line(2, sh, w, h))
    add("bad_class_token", line(0, sq, w, h) + "\nx 0.1 0.2 0.3 0.4 0.5 0.6\n")
    add("empty", "")
    # polygons that revisit a vertex: handled like Pillow ...
    for k, (pts, sw, sh_) in enumerate([([(11, 5), (14, 10), (3, 13), (14, 10), (9, 2), (7, 3)], 20, 16),
                                        ([(15, 13), (0, 8), (12, 2), (0, 8)], 18, 16),
                                        ([(11, 9), (14, 2), (1, 1), (1, 1), (6, 4), (9, -2), (1, 4)], 18, 14)]):
        add(f"revisit_{k}", line(k % 3, pts, sw, sh_), (sh_, sw))
    # ... and revisits where the reconstructed corner rule is known to differ from Pillow (KNOWN_DIVERGENT)
    for k, (pts, sw, sh_) in enumerate([([(10, 1), (15, 14), (10, 1), (1, 6)], 16, 14),
                                        ([(3, 13), (1, 0), (13, 9), (3, 13), (17, 4), (8, -2), (3, 5)], 20, 16),
                                        ([(10, 1), (-1, 5), (10, 1), (15, 4)], 14, 6),
                                        ([(2, 20), (3, 7), (15, 9), (3, 7)], 14, 21),
                                        ([(2, 4), (3, 6), (8, 1), (15, 3), (8, 1)], 15, 14),
                                        ([(7, 8), (2, 4), (7, 8), (9, 7)], 12, 12),
                                        (BLOB_A, 120, 100), (BLOB_B, 120, 100)]):
        add(f"diverge_{k}", line(k % 3, pts, sw, sh_), (sh_, sw))
    # small blobs: int() truncation makes repeated vertices and short edges
    sw, sh_ = 120, 100
    add("small_blobs", "\n".join(f"{k % 3} " + blob(rng, rng.uniform(-5, 125), rng.uniform(-5, 105), rng.uniform(2, 20),
                                                     int(rng.integers(10, 120)), sw, sh_) for k in range(40)), (sh_, sw))
    # medium frame: random blobs of all classes
    mw, mh = 160, 90
    add("medium_blobs", "\n".join(f"{k % 3} " + blob(rng, rng.uniform(10, 150), rng.uniform(5, 85), rng.uniform(8, 40),
                                                     int(rng.integers(10, 60)), mw, mh) for k in range(9)), (mh, mw))
    # LabelMe-like polygons of 10..200 vertices on 1920 x 1080 photographs, overlapping across classes
    bw, bh = 1920, 1080
    for c in range(2):
        lines = []
        for k in range(10):
            lines.append(f"{(k + c) % 3} " + blob(rng, rng.uniform(100, 1820), rng.uniform(80, 1000), rng.uniform(60, 320),
                                                  int(rng.integers(10, 201)), bw, bh))
        add(f"labelme_1920x1080_{c}", "\n".join(lines), (bh, bw))
    return out


def parse_vertices(text, w, h):
    """Vertex arrays as the reference computes them (int(float(tok) * size)); empty when the file raises anywhere."""
    verts, offsets, classes = [], [0], []
    try:
        for ln in text.splitlines():
            parts = ln.strip().split()
            if len(parts) < 5:
                continue
            cls = int(parts[0])
            c = [float(t) for t in parts[1:]]
            pts = [(int(c[i] * w), int(c[i + 1] * h)) for i in range(0, len(c) - 1, 2)]
            if len(pts) >= 3:
                verts += pts
                offsets.append(len(verts))
                classes.append(cls)
    except Exception:
        return np.zeros((0, 2), np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32)
    return np.asarray(verts, np.int32).reshape(-1, 2), np.asarray(offsets, np.int32), np.asarray(classes, np.int32)


def main():
    ds = ref.GearDataset.__new__(ref.GearDataset)
    ds.enable_priority_logging = False
    ds.priority_stats = {"files_processed": 0, "files_with_overlaps": 0,
                         "pixels_resolved": {"spalling_over_pitting": 0, "spalling_over_scrape": 0, "pitting_over_scrape": 0}}
    store = {"pillow_version": np.array(PIL.__version__)}
    names = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, (name, text, (h, w)) in enumerate(cases()):
            path = os.path.join(tmp, f"{i}.txt")
            with open(path, "w") as f:
                f.write(text)
            full = ds._create_mask_from_labelme(path, w, h)
            verts, offsets, classes = parse_vertices(text, w, h)
            store[f"{i}_label"] = np.frombuffer(text.encode(), dtype=np.uint8)
            store[f"{i}_size"] = np.array([h, w], np.int32)
            store[f"{i}_verts"], store[f"{i}_offsets"], store[f"{i}_classes"] = verts, offsets, classes
            store[f"{i}_full"] = full
            for key, (oh, ow) in RESIZES.items():
                store[f"{i}_{key}"] = np.array(Image.fromarray(full, mode="L").resize((ow, oh), Image.NEAREST))
            names.append(name)
            print(f"{i:2d} {name:32s} {h}x{w} polygons {len(classes)} mask classes {np.unique(full).tolist()}")
    store["names"] = np.array(names)
    store["resize_keys"] = np.array(list(RESIZES))
    store["resize_sizes"] = np.array(list(RESIZES.values()), np.int32)
    np.savez_compressed(OUT, **store)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.0f} kB), Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
