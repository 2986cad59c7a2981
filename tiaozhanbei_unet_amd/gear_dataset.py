"""Gear defect segmentation data (reference /root/reference/src/gear_dataset.py) for the HIP path.

The reference draws every LabelMe polygon into its own full-resolution PIL image on the host, ORs them per class,
resolves the class priority and resizes the mask with NEAREST (:112-201, :241-259).  Here loader workers only DECODE
the image and PARSE the label file (the same tokenising, the same ``int(float(tok) * size)`` truncation, the same
"any exception -> empty mask" rule); the polygons travel as a few flat int32 arrays and ``augment.polygon_masks_u8``
(csrc/polygon.hip) rasterises them on the GPU directly at the NEAREST sample points.  The masks equal the reference's
on every fixture case of tests/golden/gear_masks.npz except polygons that revisit a vertex, where the kernel's
reconstruction of Pillow's corner rule can differ by a few pixels on that vertex's row (the ``diverge_*`` cases).
The image transform is the existing ``augment.DeviceTransform`` with the Gear parameters (:238-262).

Differences from the reference, on purpose:
  - files are listed in sorted order (the reference uses ``os.listdir`` order, which depends on the file system);
  - the reference applies the random flip / rotation to the image only (its target transform has neither), so image
    and mask disagree on rotated samples.  ``GearPreprocess`` reproduces that by default; ``sync_mask=True`` applies
    the image's flip and rotation to the mask too (nearest, fill 0 = background), as Kolektor's ``GpuPreprocess`` does.
"""
from __future__ import annotations

import os

import numpy as np
import torch
from PIL import Image, ImageDraw
from torch.utils.data import DataLoader, Dataset

from .dataset import MEAN, STD, ShardSampler

IMAGE_EXTS = (".jpg", ".jpeg", ".png")
CLASS_ORDER = ["pitting", "spalling", "scrape"]          # raw ids 0, 1, 2 (reference :45-46)
CLASS_TO_IDX = {"background": 0, "pitting": 1, "spalling": 2, "scrape": 3}
PRIORITY = (1, 0, 2)                                    # spalling > pitting > scrape (raw ids, highest first)
RAW_TO_FINAL = {0: 1, 1: 2, 2: 3}


def parse_labelme_txt(path, w, h, keep_partial=False):
    """[(raw class id, [(x, y), ...])] of a LabelMe txt file at image size (w, h), parsed like the reference's
    ``_create_mask_from_labelme`` (:121-147): lines of fewer than 5 tokens are skipped, an odd trailing coordinate is
    dropped, polygons of fewer than 3 points are skipped, and any exception anywhere in the file yields NO polygons
    (the reference then returns an all-zero mask).  ``keep_partial=True`` is the rule of the reference's
    ``analyze_class_overlaps.py`` instead: its ``try`` encloses the loop and it returns what it has drawn, so the
    polygons of the lines before the exception are kept and the warning is printed."""
    polys = []
    try:
        with open(path, "r") as f:
            for line in f:
                line = line.strip()
                if not line:
                    continue
                parts = line.split()
                if len(parts) < 5:
                    continue
                class_id = int(parts[0])
                coords = [float(x) for x in parts[1:]]
                pts = []
                for i in range(0, len(coords), 2):
                    if i + 1 < len(coords):
                        pts.append((int(coords[i] * w), int(coords[i + 1] * h)))
                if len(pts) >= 3:
                    polys.append((class_id, pts))
    except Exception as e:
        if not keep_partial:
            return []
        print(f"Warning: Could not parse label file {path}: {e}")
    return polys


def label_class_names(path):
    """Class names a label file mentions, counted as the reference's ``_parse_label_file`` counts them (:95-110)."""
    found = set()
    try:
        with open(path, "r") as f:
            for line in f:
                parts = line.strip().split()
                if len(parts) >= 5 and parts[0].isdigit() and int(parts[0]) in (0, 1, 2):
                    found.add(CLASS_ORDER[int(parts[0])])
    except Exception as e:
        print(f"Warning: Could not parse label file {path}: {e}")
    return found


def _check_vertex_counts(path):
    """Refuse, when the dataset is built, a label file whose polygons the mask kernel cannot take (more than
    augment.POLY_MAX_VERTICES vertices), instead of failing in the middle of an epoch."""
    from .augment import POLY_MAX_VERTICES
    big = [len(pts) for cls, pts in parse_labelme_txt(path, 1, 1) if cls in RAW_TO_FINAL and len(pts) > POLY_MAX_VERTICES]
    if big:
        raise ValueError(f"{path}: polygon(s) of {max(big)} vertices; the GPU mask kernel takes at most "
                         f"{POLY_MAX_VERTICES} vertices per polygon")


def mask_from_polygons_pil(polys, w, h):
    """The reference's host mask (:112-201) from parsed polygons: Pillow draws each polygon, classes OR-ed, priority
    resolved.  A host comparator for tests and ``raw=False``; the training path uses the GPU kernel."""
    class_masks = {}
    for cls, pts in polys:
        im = Image.fromarray(np.zeros((h, w), dtype=np.uint8))
        ImageDraw.Draw(im).polygon(pts, fill=1)
        class_masks[cls] = class_masks.get(cls, np.zeros((h, w), dtype=np.uint8)) | np.array(im)
    final = np.zeros((h, w), dtype=np.uint8)
    for cls in reversed(PRIORITY):
        if cls in class_masks:
            final[class_masks[cls] == 1] = RAW_TO_FINAL[cls]
    return final


class GearDataset(Dataset):
    """``images/{split}/*.{jpg,jpeg,png}`` paired with ``labels/{split}/<stem>.txt`` (images without a label file are
    skipped).  ``raw=True``: samples are (decoded uint8 image [H, W, 3], parsed polygons, path) for ``collate_raw`` and
    ``GearPreprocess``; ``raw=False``: the reference's eval sample on the host (bilinear resize + normalise, Pillow mask
    + NEAREST resize, long)."""

    def __init__(self, root_dir, split="train", image_size=(512, 512), raw=True):
        self.root_dir, self.split, self.image_size, self.raw = root_dir, split, tuple(image_size), bool(raw)
        images_dir = os.path.join(root_dir, "images", split)
        labels_dir = os.path.join(root_dir, "labels", split)
        if not os.path.exists(images_dir):
            raise ValueError(f"Images directory not found: {images_dir}")
        if not os.path.exists(labels_dir):
            raise ValueError(f"Labels directory not found: {labels_dir}")
        self.image_paths, self.label_paths = [], []
        found = set()
        for name in sorted(os.listdir(images_dir)):
            if name.lower().endswith(IMAGE_EXTS):
                label = os.path.join(labels_dir, os.path.splitext(name)[0] + ".txt")
                if os.path.exists(label):
                    self.image_paths.append(os.path.join(images_dir, name))
                    self.label_paths.append(label)
                    found |= label_class_names(label)
                    _check_vertex_counts(label)
        self.class_names = [c for c in CLASS_ORDER if c in found]
        self.num_classes = len(self.class_names) + 1
        self.class_to_idx = dict(CLASS_TO_IDX)

    def __len__(self):
        return len(self.image_paths)

    def __getitem__(self, idx):
        img = Image.open(self.image_paths[idx]).convert("RGB")
        w, h = img.size
        polys = parse_labelme_txt(self.label_paths[idx], w, h)
        if self.raw:
            return torch.from_numpy(np.array(img, dtype=np.uint8)), polys, self.image_paths[idx]
        oh, ow = self.image_size
        mask = Image.fromarray(mask_from_polygons_pil(polys, w, h), mode="L").resize((ow, oh), Image.NEAREST)
        a = np.array(img.resize((ow, oh), Image.BILINEAR), dtype=np.uint8).astype(np.float32).transpose(2, 0, 1) / 255.0
        return torch.from_numpy((a - MEAN) / STD), torch.from_numpy(np.array(mask)).long(), self.image_paths[idx]


def flatten_polygons(polys_per_image):
    """The batch's polygons as flat arrays for ``augment.polygon_masks_u8``: ``verts`` int32 [V, 2], ``offsets`` [P + 1],
    ``classes`` [P], ``images`` [P].  Raw classes other than 0, 1, 2 are dropped here: the reference's priority loop never
    visits them (:169-199)."""
    verts, offsets, classes, images = [], [0], [], []
    for n, polys in enumerate(polys_per_image):
        for cls, pts in polys:
            if cls not in RAW_TO_FINAL:
                continue
            verts.extend(pts)
            offsets.append(len(verts))
            classes.append(cls)
            images.append(n)
    return {"verts": np.asarray(verts, dtype=np.int64).reshape(-1, 2), "offsets": np.asarray(offsets, dtype=np.int64),
            "classes": np.asarray(classes, dtype=np.int64), "images": np.asarray(images, dtype=np.int64)}


def collate_raw(samples):
    """(images, polys, sizes, paths) of ``raw`` samples: images stacked when they share a size, a list otherwise;
    ``polys`` = flatten_polygons(...); ``sizes`` = [(h, w)]."""
    imgs, polys, paths = zip(*samples)
    same = len({tuple(t.shape) for t in imgs}) == 1
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in imgs]
    return (torch.stack(imgs) if same else list(imgs)), flatten_polygons(polys), sizes, list(paths)


class GearPreprocess:
    """get_gear_transforms (reference :238-262) on the GPU for ``collate_raw`` batches.  Images: Resize (bilinear)
    [-> RandomHorizontalFlip -> RandomRotation(10) -> ColorJitter(0.2, 0.2, 0.2, 0.1) when ``train``] -> ToTensor ->
    Normalize.  Masks: the polygon kernel at the NEAREST sample points -> long [N, H, W].  ``sync_mask=False`` (default)
    is the reference: the mask gets neither flip nor rotation; ``sync_mask=True`` applies the image's flip and rotation
    to the mask (``augment.flip_rotate_u8``)."""

    def __init__(self, image_size=(512, 512), train=False, sync_mask=False, seed=0):
        from .augment import DeviceTransform
        self.train, self.sync_mask = bool(train), bool(sync_mask)
        self.tf = DeviceTransform(tuple(image_size), train=train, degrees=10.0, brightness=0.2, contrast=0.2,
                                  saturation=0.2, hue=0.1, seed=seed)

    def __call__(self, images_u8, polys, sizes, device="cuda", params=None):
        from . import augment as A
        n = len(sizes)
        if self.train and params is None:
            params = self.tf.draw(n)
        x = self.tf(images_u8, params if self.train else None, device=device)
        h, w = self.tf.size
        m = A.polygon_masks_u8(polys, sizes, h, w, device=x.device)
        if self.train and self.sync_mask:
            m = A.flip_rotate_u8(m.unsqueeze(-1), params["flips"], params["angles"])[..., 0]
        return x, m.long()


def get_gear_dataloaders(root_dir, batch_size=16, image_size=(512, 512), num_workers=4, rank=0, world=1, seed=0):
    """(train, val, test, num_classes) over ``raw`` datasets with ``collate_raw`` (reference :265-326); with
    ``world > 1`` the train loader draws from this rank's ``dataset.ShardSampler`` shard."""
    sets = [GearDataset(root_dir, s, image_size, raw=True) for s in ("train", "val", "test")]
    kw = dict(batch_size=batch_size, num_workers=num_workers, pin_memory=torch.cuda.is_available(), collate_fn=collate_raw)
    if world > 1:
        train = DataLoader(sets[0], sampler=ShardSampler(len(sets[0]), rank, world, True, seed), **kw)
    else:
        train = DataLoader(sets[0], shuffle=True, **kw)
    return train, DataLoader(sets[1], shuffle=False, **kw), DataLoader(sets[2], shuffle=False, **kw), sets[0].num_classes


def _synthetic_label_lines(rng, n_polys):
    """LabelMe-like lines: closed blobs of 10..40 vertices in normalised coordinates, classes 0, 1, 2 overlapping."""
    lines = []
    for k in range(n_polys):
        cls = k % 3
        nv = int(rng.integers(10, 41))
        cx, cy = rng.uniform(0.15, 0.85, 2)
        r = rng.uniform(0.08, 0.25) * rng.uniform(0.6, 1.0, nv)
        ang = np.sort(rng.uniform(0, 2 * np.pi, nv))
        xy = np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1).reshape(-1)
        lines.append(f"{cls} " + " ".join(f"{v:.6f}" for v in xy))
    return lines


def write_synthetic_gear(root_dir, sizes=((96, 160), (72, 128), (80, 80)), per_split=(6, 4, 4), seed=0):
    """A tiny Gear-layout tree for tests and ``--synthetic``: images of a few sizes (``sizes`` = (h, w)) with overlapping
    polygons of all three classes; in every split one image has an empty label file and one a malformed one (-> an
    all-background mask, as in the reference), and one image has no label file at all (skipped)."""
    rng = np.random.default_rng(seed)
    for split, count in zip(("train", "val", "test"), per_split):
        idir, ldir = os.path.join(root_dir, "images", split), os.path.join(root_dir, "labels", split)
        os.makedirs(idir, exist_ok=True)
        os.makedirs(ldir, exist_ok=True)
        for i in range(count):
            h, w = sizes[i % len(sizes)]
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            stem = f"gear_{split}_{i:03d}"
            Image.fromarray(img).save(os.path.join(idir, stem + ".png"))
            if i == 0:
                text = ""                                               # empty label: background only
            elif i == 1:
                text = "1 0.1 0.1 0.5 0.1 0.5 oops 0.1 0.5\n"           # malformed: the whole file yields no polygons
            else:
                text = "\n".join(_synthetic_label_lines(rng, int(rng.integers(3, 7)))) + "\n"
            with open(os.path.join(ldir, stem + ".txt"), "w") as f:
                f.write(text)
        Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(
            os.path.join(idir, f"gear_{split}_unlabelled.png"))
    return root_dir
