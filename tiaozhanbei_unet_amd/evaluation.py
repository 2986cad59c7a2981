"""Evaluation on the device, outside autograd: scores, confusion counts, AUROC / AUPRC, AUPRO, class regions, uint8 input."""
import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib as L
from ._hipcall import _ptr, _require_cuda, _stream, _workspace


def anomaly_score(reconstruction, original, l1=False):
    """(score map [N, H, W], image score [N]) of compute_anomaly_score (/root/reference/src/utils.py:205-215)."""
    _require_cuda(reconstruction, original)
    r = reconstruction.detach().contiguous().float()
    o = original.detach().contiguous().float()
    n, c = r.shape[0], r.shape[1]
    hw = int(r.numel() // (n * c))
    score = torch.empty((n,) + tuple(r.shape[2:]), dtype=torch.float32, device=r.device)
    img = torch.empty(n, dtype=torch.float32, device=r.device)
    lib = L.lib()
    ws = _workspace(lib.unet_anomaly_score_workspace(n, hw), r.device)
    L.check(lib.unet_anomaly_score(_ptr(r), _ptr(o), n, c, hw, 1 if l1 else 0, _ptr(score), _ptr(img), _ptr(ws), ws.numel(),
                                   _stream()), "unet_anomaly_score")
    return score, img


def threshold_confusion(pred, truth, thresholds, select=None, counts=None):
    """Confusion counts [K][4] = {tp, fp, fn, tn} (int64 DEVICE tensor; pass it back as ``counts`` to keep accumulating
    over batches, read it once at the end) of (pred > t) against (truth > 0.5) for each threshold, over the images with
    select[n] true (None: all): the pixel-metric epilogue of /root/reference/src/test.py:79-106 and
    src/train_utils.py:232-245 on the device (unet_threshold_confusion)."""
    _require_cuda(pred)
    p = pred.detach().contiguous().float()
    t = truth.detach().to(p.device).contiguous().float()
    if p.shape != t.shape or p.dim() < 2:
        raise ValueError("threshold_confusion: prediction / truth shapes differ")
    n = p.shape[0]
    per = p.numel() // n
    values = [float(v) for v in thresholds]
    if not values:
        raise ValueError("threshold_confusion: at least one threshold")
    sel = None if select is None else torch.as_tensor(select).to(device=p.device, dtype=torch.uint8).contiguous()
    if counts is None:
        counts = torch.zeros((len(values), 4), dtype=torch.int64, device=p.device)
    if tuple(counts.shape) != (len(values), 4):
        raise ValueError("threshold_confusion: counts must be [len(thresholds), 4]")
    for k in range(0, len(values), 8):           # the kernel takes up to 8 thresholds per pass over the maps
        thr = torch.tensor(values[k:k + 8], dtype=torch.float32, device=p.device)
        L.check(L.lib().unet_threshold_confusion(_ptr(p), _ptr(t), _ptr(sel), n, per, _ptr(thr), thr.numel(),
                                                 _ptr(counts[k:k + 8]), _stream()), "unet_threshold_confusion")
    return counts


def _select_runs(select, n, what):
    """(runs, device mask) of a per-image selection: a device mask goes to the kernels as it is (one run, all images); a
    host mask becomes one launch per run of selected images, so nothing is copied and nothing synchronises."""
    if select is None:
        return [(0, n)], None
    sel = torch.as_tensor(select)
    if sel.numel() != n:
        raise ValueError(f"{what}: select needs one entry per image")
    if sel.is_cuda:
        return [(0, n)], sel.reshape(-1).to(torch.uint8).contiguous()
    on = sel.reshape(-1).to(torch.bool).tolist() + [False]
    runs, start = [], None
    for i, v in enumerate(on):
        if v and start is None:
            start = i
        elif not v and start is not None:
            runs.append((start, i))
            start = None
    return runs, None


class BinaryAUC:
    """Pixel-level AUROC / AUPRC accumulated over batches: the roc_auc_score and auc(precision_recall_curve) that
    the reference src/utils.py:84-91 computes for calculate_pixel_metrics (:97-108), on the device.  A pixel is
    positive iff truth > 0.5; ties are float equality (-0.0 == +0.0).  ``update`` appends the selected pixels' scores
    as sort keys (unet_rank_auc_append) without synchronising; ``compute`` reads the counts once, sorts and ranks
    (unet_rank_auc).  No positives, no negatives or any NaN / inf score give 0.0 / 0.0, as calculate_metrics does when
    sklearn refuses.  The result depends only on the multiset of (score, label) pixels, bitwise."""

    def __init__(self):
        self._chunks = []                     # (keys, capacity, counts): one exactly-sized key chunk per update

    def update(self, pred, truth, select=None):
        """pred / truth: device tensors of equal shape [N, ...]; select: host or device bool per image (None: all)."""
        _require_cuda(pred)
        p = pred.detach().contiguous().float()
        t = truth.detach().to(p.device).contiguous().float()
        if p.shape != t.shape or p.dim() < 2:
            raise ValueError("BinaryAUC.update: prediction / truth shapes differ")
        n = p.shape[0]
        per = p.numel() // n
        runs, sel = _select_runs(select, n, "BinaryAUC.update")
        cap = sum(b - a for a, b in runs) * per
        if cap == 0:
            return
        keys = torch.empty(cap, dtype=torch.int32, device=p.device)
        counts = torch.zeros(3, dtype=torch.int64, device=p.device)
        lib = L.lib()
        for a, b in runs:
            L.check(lib.unet_rank_auc_append(_ptr(p[a:b]), _ptr(t[a:b]), _ptr(sel), b - a, per, _ptr(keys), cap,
                                             _ptr(counts), _stream()), "unet_rank_auc_append")
        self._chunks.append((keys, cap, counts))

    def compute(self):
        """{"auroc", "auprc", "positives", "negatives", "nonfinite"} over every pixel passed to update."""
        totals = [0, 0, 0]
        if self._chunks:
            per_chunk = torch.stack([c for _, _, c in self._chunks]).tolist()      # the one read of the counts
            totals = [sum(c[i] for c in per_chunk) for i in range(3)]
        n_pos, n_neg, nonfinite = totals
        res = {"auroc": 0.0, "auprc": 0.0, "positives": n_pos, "negatives": n_neg, "nonfinite": nonfinite}
        if nonfinite or not n_pos or not n_neg:
            return res
        lib = L.lib()
        nbytes = lib.unet_rank_auc_workspace(n_pos, n_neg)
        if nbytes == 0:
            raise RuntimeError(f"BinaryAUC: {n_pos + n_neg} pixels, at most 2^31 - 1 are supported")
        dev = self._chunks[0][0].device
        pos = torch.cat([k[:c[0]] for (k, _, _), c in zip(self._chunks, per_chunk)])          # copies: the sort
        neg = torch.cat([k[cap - c[1]:] for (k, cap, _), c in zip(self._chunks, per_chunk)])  # is in place
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(2, dtype=torch.float64, device=dev)
        L.check(lib.unet_rank_auc(_ptr(pos), n_pos, _ptr(neg), n_neg, _ptr(out), _ptr(ws), nbytes, _stream()),
                "unet_rank_auc")
        res["auroc"], res["auprc"] = out.tolist()
        return res


SMOOTH_MAX_RADIUS = 32          # UNET_SMOOTH_MAX_RADIUS of include/unet_hip.h


class GaussianSmoother:
    """Gaussian smoothing of anomaly maps and their per-image peak in one launch (unet_smooth_maps): what
    scipy.ndimage.gaussian_filter(map, sigma, mode="reflect", truncate=truncate) computes plane by plane, in fp32.
    radius = int(truncate * sigma + 0.5) (scipy's rule); the taps exp(-0.5 (k / sigma)^2), k = 0 .. radius, are normalised
    over the full 2 radius + 1 window in float64 and then rounded to fp32 (``taps``; ``taps64`` keeps the float64 ones).
    sigma == 0 is radius 0 with taps [1]: a bit-exact copy and the plain per-image maximum."""

    def __init__(self, sigma, truncate=4.0):
        import math
        self.sigma, self.truncate = float(sigma), float(truncate)
        for name, v in (("sigma", self.sigma), ("truncate", self.truncate)):
            if not math.isfinite(v) or v < 0.0:
                raise ValueError(f"GaussianSmoother: {name} {v} must be finite and >= 0")
        limit = (SMOOTH_MAX_RADIUS + 0.5) / self.truncate if self.truncate > 0 else math.inf
        if self.truncate * self.sigma + 0.5 >= SMOOTH_MAX_RADIUS + 1:
            raise ValueError(f"GaussianSmoother: sigma {self.sigma} at truncate {self.truncate} needs a radius above "
                             f"{SMOOTH_MAX_RADIUS}; the largest sigma that fits is below {limit:g}")
        self.radius = int(self.truncate * self.sigma + 0.5)
        k = np.arange(self.radius + 1, dtype=np.float64)
        g = np.exp(-0.5 * (k / self.sigma) ** 2) if self.radius > 0 else np.ones(1)
        self.taps64 = g / (g[0] + 2.0 * g[1:].sum())
        self.taps = self.taps64.astype(np.float32)
        self._host = (C.c_float * (self.radius + 1))(*self.taps.tolist())

    def __call__(self, maps):
        """maps: CUDA tensor [N, H, W] or [N, 1, H, W] of any float dtype -> (smoothed fp32 of the same shape, image_max
        [N] fp32).  Does not synchronise."""
        _require_cuda(maps)
        if not maps.is_floating_point() or maps.dim() not in (3, 4) or (maps.dim() == 4 and maps.shape[1] != 1):
            raise ValueError(f"GaussianSmoother: float maps [N, H, W] or [N, 1, H, W], got {maps.dtype} {tuple(maps.shape)}")
        x = maps.detach().contiguous().float()
        n, h, w = x.shape[0], x.shape[-2], x.shape[-1]
        out = torch.empty_like(x)
        peak = torch.empty(n, dtype=torch.float32, device=x.device)
        L.check(L.lib().unet_smooth_maps(_ptr(x), _ptr(out), n, h, w, self._host, self.radius, _ptr(peak), _stream()),
                "unet_smooth_maps")
        return out, peak


def _image_planes(t, what):
    """[N, H, W] view of a [N, ..., H, W] tensor with one plane per image ([N, W]: one row)."""
    if t.dim() < 2:
        raise ValueError(f"{what}: needs [N, ...] maps")
    n, w = t.shape[0], t.shape[-1]
    h = t.shape[-2] if t.dim() >= 3 else 1
    if n == 0 or t.numel() != n * h * w:
        raise ValueError(f"{what}: one H x W plane per image, got {tuple(t.shape)}")
    return t.reshape(n, h, w)


def label_regions(truth, select=None, _runs=None):
    """8-connected regions of the defective pixels (truth > 0.5) of each image of truth [N, (1,) H, W], over the images
    with select[n] true (None: all): (labels, sizes, counts), all DEVICE tensors.  labels (int32, truth's shape) = 1 +
    the smallest linear index y * W + x of the pixel's region, sizes (int32) = the region's pixel count at each of its
    pixels, both 0 elsewhere; counts (int64 [3]) = {regions, defective pixels, ok pixels} of the selected images.
    scipy.ndimage.label(mask, np.ones((3, 3))) on the device (unet_label_regions); does not synchronise."""
    _require_cuda(truth)
    t = _image_planes(truth.detach().contiguous().float(), "label_regions")
    n, h, w = t.shape
    runs, sel = _runs if _runs is not None else _select_runs(select, n, "label_regions")
    lib = L.lib()
    labels = torch.zeros((n, h, w), dtype=torch.int32, device=t.device)
    sizes = torch.zeros((n, h, w), dtype=torch.int32, device=t.device)
    counts = torch.zeros(3, dtype=torch.int64, device=t.device)
    for a, b in runs:
        nbytes = lib.unet_label_regions_workspace(b - a, h, w)
        if nbytes == 0:
            raise RuntimeError(f"label_regions: {b - a} x {h} x {w} is not supported (n < 65536, at most 2^31 - 1 pixels)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=t.device)
        L.check(lib.unet_label_regions(_ptr(t[a:b]), _ptr(sel), b - a, h, w, _ptr(labels[a:b]), _ptr(sizes[a:b]),
                                       _ptr(counts), _ptr(ws), nbytes, _stream()), "unet_label_regions")
    return labels.reshape(truth.shape), sizes.reshape(truth.shape), counts


class RegionOverlapAUC:
    """AUPRO accumulated over batches: the area below the per-region-overlap curve of the MVTec AD evaluation up to a
    false-positive rate of ``fpr_limit``, divided by it.  A pixel is defective iff truth > 0.5, a region is an
    8-connected component of defective pixels of one image, and every region weighs the same: a defective pixel lifts
    the curve by 1 / (regions * its region's size).  ``update`` labels the batch's regions (unet_label_regions) and
    appends the selected pixels as sort keys and (key, size) elements (unet_region_auc_append) without synchronising;
    only those and the counts are kept.  ``compute`` reads the counts once, sorts and integrates (unet_region_auc).
    No region, no ok pixel or any NaN / inf score give 0.0.  The result depends only on the multiset of (score, region
    size) pixels, bitwise."""

    def __init__(self, fpr_limit=0.3):
        self.fpr_limit = float(fpr_limit)
        if not 0.0 < self.fpr_limit <= 1.0:
            raise ValueError(f"RegionOverlapAUC: fpr_limit {fpr_limit} is not in (0, 1]")
        self._chunks = []                     # (slots, capacity, counts[6]): one exactly-sized chunk per update
        self._max_region = 1

    def update(self, pred, truth, select=None):
        """pred / truth: device tensors of equal shape [N, (1,) H, W]; select: host or device bool per image."""
        _require_cuda(pred)
        p = pred.detach().contiguous().float()
        t = truth.detach().to(p.device).contiguous().float()
        if p.shape != t.shape:
            raise ValueError("RegionOverlapAUC.update: prediction / truth shapes differ")
        p = _image_planes(p, "RegionOverlapAUC.update")
        n, per = p.shape[0], p.shape[1] * p.shape[2]
        runs, sel = _select_runs(select, n, "RegionOverlapAUC.update")
        cap = sum(b - a for a, b in runs) * per
        if cap == 0:
            return
        _, sizes, regions = label_regions(t, _runs=(runs, sel))
        sizes = sizes.reshape(p.shape)
        slots = torch.empty(cap, dtype=torch.int64, device=p.device)
        counts = torch.zeros(3, dtype=torch.int64, device=p.device)
        lib = L.lib()
        for a, b in runs:
            L.check(lib.unet_region_auc_append(_ptr(p[a:b]), _ptr(sizes[a:b]), _ptr(sel), b - a, per, _ptr(slots), cap,
                                               _ptr(counts), _stream()), "unet_region_auc_append")
        self._chunks.append((slots, cap, torch.cat([counts, regions])))
        self._max_region = max(self._max_region, per)

    def compute(self):
        """{"aupro", "pro_at_limit", "fpr_limit", "regions", "defective", "ok", "nonfinite"} over every update."""
        totals = [0] * 6
        if self._chunks:
            per_chunk = torch.stack([c for _, _, c in self._chunks]).tolist()      # the one read of the counts
            totals = [sum(c[i] for c in per_chunk) for i in range(6)]
        n_pos, n_neg, nonfinite, regions, defective, ok = totals
        res = {"aupro": 0.0, "pro_at_limit": 0.0, "fpr_limit": self.fpr_limit, "regions": regions,
               "defective": defective, "ok": ok, "nonfinite": nonfinite}
        if nonfinite or not regions or not ok:
            return res
        lib = L.lib()
        nbytes = lib.unet_region_auc_workspace(n_pos, n_neg)
        if nbytes == 0:
            raise RuntimeError(f"RegionOverlapAUC: {n_pos + n_neg} pixels, at most 2^31 - 1 are supported")
        dev = self._chunks[0][0].device
        pos = torch.cat([s[:c[0]] for (s, _, _), c in zip(self._chunks, per_chunk)])          # copies: the sort
        neg = torch.cat([s.view(torch.int32)[2 * cap - c[1]:]                                 # destroys its input
                         for (s, cap, _), c in zip(self._chunks, per_chunk)])
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(2, dtype=torch.float64, device=dev)
        L.check(lib.unet_region_auc(_ptr(pos), n_pos, _ptr(neg), n_neg, regions, self._max_region, self.fpr_limit,
                                    _ptr(out), _ptr(ws), nbytes, _stream()), "unet_region_auc")
        res["aupro"], res["pro_at_limit"] = out.tolist()
        return res


def _class_maps(labels, what):
    """uint8 [N, H, W] device maps of integer label maps; values outside 0..254 become 255 (background)."""
    _require_cuda(labels)
    t = labels.detach()
    if t.dtype != torch.uint8:
        if t.is_floating_point() or t.dtype == torch.bool:
            raise ValueError(f"{what}: integer label maps, got {t.dtype}")
        t = t.long()
        t = torch.where((t >= 0) & (t < 255), t, torch.full_like(t, 255)).to(torch.uint8)
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{what}: [N, H, W] label maps, got {tuple(t.shape)}")
    return t.contiguous()


def _class_regions_error(what, n, h, w, num_classes):
    return RuntimeError(f"{what}: {n} x {h} x {w} maps of {num_classes} classes are not supported (n < 65536, at most "
                        "2^31 - 1 pixels, 2..255 classes)")


def label_class_regions(labels_u8, num_classes):
    """Class regions of integer label maps [N, H, W]: a pixel has class c iff its value is c with 1 <= c < num_classes
    (0 and every value >= num_classes, 255 among them, are background), and a class region is an 8-connected component
    of pixels of one class in one image.  Returns (region, sizes, counts), DEVICE tensors: region (int32 [N, H, W]) =
    1 + the smallest linear index y * W + x of the pixel's region, sizes (int32) = the region's pixel count at each of
    its pixels, both 0 on background; counts (int64 [N, num_classes]) = regions per image and class.  Per class,
    scipy.ndimage.label(map == c, np.ones((3, 3))) on the device (unet_label_class_regions); does not synchronise."""
    t = _class_maps(labels_u8, "label_class_regions")
    n, h, w = t.shape
    c = int(num_classes)
    lib = L.lib()
    nbytes = lib.unet_label_class_regions_workspace(n, h, w, c) if 0 <= c < 2 ** 31 else 0
    if nbytes == 0:
        raise _class_regions_error("label_class_regions", n, h, w, num_classes)
    region = torch.empty((n, h, w), dtype=torch.int32, device=t.device)
    sizes = torch.empty((n, h, w), dtype=torch.int32, device=t.device)
    counts = torch.zeros((n, c), dtype=torch.int64, device=t.device)
    ws = _workspace(nbytes, t.device)
    L.check(lib.unet_label_class_regions(_ptr(t), n, h, w, c, _ptr(region), _ptr(sizes), _ptr(counts), _ptr(ws),
                                         ws.numel(), _stream()), "unet_label_class_regions")
    return region, sizes, counts


FRAGMENT_FIELDS = ("image", "class", "root", "group", "size")
MAX_MERGE_GAP = 32              # the largest gap of unet_group_class_regions


def _record_buffer(cap, fields, device):
    """(out, records, count): a DEVICE int64 buffer of ``cap`` records of ``fields`` fields followed by their count, its
    two parts as views, the count zeroed"""
    out = torch.empty(cap * fields + 1, dtype=torch.int64, device=device)
    out[-1:].zero_()
    return out, out[:-1], out[-1:]


def _host_records(host, cap, fields, by, too_many):
    """the records of a ``_record_buffer`` read to the host, sorted by the columns ``by``, the most significant first"""
    k = int(host[-1])
    if k > cap:
        raise RuntimeError(too_many)                   # cannot happen
    rec = host[:-1].reshape(cap, fields)[:k]
    return np.ascontiguousarray(rec[np.lexsort(tuple(rec[:, col] for col in reversed(by)))])


def _group_labelled(t, region, sizes, c, gap, min_pixels, image_base, cap):
    """unet_group_class_regions on labelled maps: (group, group_sizes, counts, DEVICE int64 buffer of ``cap`` records of
    FRAGMENT_FIELDS followed by their count); does not synchronise."""
    n, h, w = t.shape
    lib = L.lib()
    group, group_sizes = torch.empty_like(region), torch.empty_like(sizes)
    counts = torch.zeros((n, c), dtype=torch.int64, device=t.device)
    out, records, count = _record_buffer(cap, len(FRAGMENT_FIELDS), t.device)
    ws = _workspace(lib.unet_group_class_regions_workspace(n, h, w, c), t.device)
    L.check(lib.unet_group_class_regions(_ptr(t), _ptr(region), _ptr(sizes), n, h, w, c, gap, min_pixels, image_base,
                                         _ptr(group), _ptr(group_sizes), _ptr(counts), _ptr(records), cap, _ptr(count),
                                         _ptr(ws), ws.numel(), _stream()), "unet_group_class_regions")
    return group, group_sizes, counts, out


def _merge_gap(what, merge_gap):
    g = int(merge_gap)
    if not 0 <= g <= MAX_MERGE_GAP:
        raise ValueError(f"{what}: merge_gap {merge_gap} is outside 0..{MAX_MERGE_GAP}")
    return g


def _min_pixels_and_base(what, min_pixels, image_base):
    if min_pixels < 1:
        raise ValueError(f"{what}: min_pixels {min_pixels} is below 1")
    if image_base < 0:
        raise ValueError(f"{what}: image_base {image_base} is negative")


def group_class_regions(labels_u8, region, sizes, num_classes, gap, min_pixels=1, image_base=0):
    """Which class regions belong to one defect.  ``labels_u8``, ``region`` and ``sizes`` are what ``label_class_regions``
    takes and makes.  A fragment is a region with at least ``min_pixels`` pixels (smaller regions are dropped first: they
    link nothing and join nothing); two fragments of one image and one class are linked iff they hold pixels p, q with
    (py - qy)^2 + (px - qx)^2 <= gap^2, ``gap`` in 1..32; a group is a connected component of the link graph, so linking
    is transitive.  Returns (group, group_sizes, counts, fragments): group (int32 [N, H, W], DEVICE) = 1 + the smallest
    fragment root of the pixel's group, group_sizes (int32, DEVICE) = the group's pixel count at each of its pixels, both
    0 on background and on dropped regions, so the pair stands in for (region, sizes) wherever those go; counts (int64
    [N, num_classes], DEVICE) = groups per image and class; fragments = an int64 [F, 5] numpy array of FRAGMENT_FIELDS,
    one row per fragment, ``image`` = image_base + the map's index, ``group`` = its group's root, sorted by (image,
    group, root).  ``gap=1`` gives every fragment its own group (unet_group_class_regions; integers throughout, so the
    outputs are a function of the inputs alone).  Two host reads: the number of region roots, which bounds the fragments
    from above and sizes the buffer, and the records with their count."""
    what = "group_class_regions"
    t = _class_maps(labels_u8, what)
    _require_cuda(region, sizes)
    if region.dtype != torch.int32 or sizes.dtype != torch.int32 or region.shape != t.shape or sizes.shape != t.shape \
            or region.device != t.device or sizes.device != t.device:
        raise ValueError(f"{what}: region and sizes are the int32 tensors that label_class_regions made of the labels")
    n, h, w = t.shape
    c, gap, min_pixels, image_base = int(num_classes), int(gap), int(min_pixels), int(image_base)
    lib = L.lib()
    nbytes = lib.unet_group_class_regions_workspace(n, h, w, c) if 0 <= c < 2 ** 31 else 0
    if nbytes == 0 or image_base + n >= 2 ** 31:
        raise _class_regions_error(what, n, h, w, num_classes)
    if not 1 <= gap <= MAX_MERGE_GAP:
        raise ValueError(f"{what}: gap {gap} is outside 1..{MAX_MERGE_GAP}")
    _min_pixels_and_base(what, min_pixels, image_base)
    region, sizes = region.contiguous(), sizes.contiguous()
    per = h * w
    index = torch.arange(1, per + 1, dtype=torch.int32, device=t.device).reshape(1, h, w)
    cap = max(int((region == index).sum()), 1)         # the region roots: every fragment is one
    group, group_sizes, counts, out = _group_labelled(t, region, sizes, c, gap, min_pixels, image_base, cap)
    return group, group_sizes, counts, _host_records(out.cpu().numpy(), cap, len(FRAGMENT_FIELDS), (0, 3, 2),
                                                     f"{what}: more fragments than regions")


RECORD_FIELDS = ("image", "class", "root", "size", "hit")


def _matcher_args(name, num_classes, min_pixels):
    """(num_classes, min_pixels) of a matcher's constructor, refused outside 2..255 classes and below one pixel"""
    c, mp = int(num_classes), int(min_pixels)
    if not 2 <= c <= 255:
        raise ValueError(f"{name}: {num_classes} classes, 2..255 are supported")
    if mp < 1:
        raise ValueError(f"{name}: min_pixels {min_pixels} is below 1")
    return c, mp


class ClassRegionMatcher:
    """Defect-level matching of predicted against true label maps, accumulated over batches.  Regions are those of
    ``label_class_regions``; a predicted region is kept iff it has at least ``min_pixels`` pixels.  ``hit`` of a truth
    region = its pixels whose predicted class is the region's and whose predicted region is kept; ``hit`` of a kept
    predicted region = its pixels whose truth class is its class (unet_match_class_regions; integers throughout).

    ``update`` labels truth and prediction in one call, matches them and keeps only the batch's two record buffers and
    its counts; it does not synchronise.  The buffers have to hold one record per pixel when they are made (the device
    alone knows how many regions there are), so the record counts travel to pinned host memory behind the kernels, and a
    later ``update`` trims every buffer whose counts have arrived, without waiting.  ``compute`` reads everything back
    once."""

    def __init__(self, num_classes, min_pixels=1):
        self.num_classes, self.min_pixels = _matcher_args("ClassRegionMatcher", num_classes, min_pixels)
        self.images = 0
        self._chunks = []          # [truth records, pred records, class counts [2n, C], host counts, event or None]

    def _trim(self, wait):
        for ch in self._chunks:
            if ch[4] is None or not (wait or ch[4].query()):
                continue
            if wait:
                ch[4].synchronize()
            kt, kp = ch[3].tolist()
            if kt > ch[0].shape[0] or kp > ch[1].shape[0]:
                raise RuntimeError("ClassRegionMatcher: more records than pixels")      # cannot happen
            ch[0], ch[1], ch[4] = ch[0][:kt].clone(), ch[1][:kp].clone(), None

    def update(self, pred_labels, truth):
        """pred_labels / truth: integer device label maps of equal shape [N, H, W] (the uint8 argmax of
        ``metrics.per_image_stats(..., labels=True)`` and the loaders' masks; values outside 0..254 become 255)."""
        p = _class_maps(pred_labels, "ClassRegionMatcher.update")
        t = _class_maps(truth.to(p.device), "ClassRegionMatcher.update")
        if p.shape != t.shape:
            raise ValueError("ClassRegionMatcher.update: prediction / truth shapes differ")
        self._trim(wait=False)
        n, h, w = p.shape
        c, dev = self.num_classes, p.device
        region, sizes, class_counts = label_class_regions(torch.cat([t, p]), c)      # one pass labels both
        lib = L.lib()
        nbytes = lib.unet_match_class_regions_workspace(n, h, w, c)
        if nbytes == 0 or self.images + n >= 2 ** 31:
            raise _class_regions_error("ClassRegionMatcher.update", n, h, w, c)
        cap = n * h * w
        records = [torch.empty((cap, len(RECORD_FIELDS)), dtype=torch.int32, device=dev) for _ in range(2)]
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        ws = _workspace(nbytes, dev)
        L.check(lib.unet_match_class_regions(_ptr(t), _ptr(region[:n]), _ptr(sizes[:n]), _ptr(p), _ptr(region[n:]),
                                             _ptr(sizes[n:]), n, h, w, c, self.min_pixels, self.images,
                                             _ptr(records[0]), _ptr(records[1]), cap, _ptr(counts), _ptr(ws),
                                             ws.numel(), _stream()), "unet_match_class_regions")
        host = torch.empty(2, dtype=torch.int64, pin_memory=True)
        host.copy_(counts, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self._chunks.append([records[0], records[1], class_counts, host, done])
        self.images += n

    def compute(self):
        """{"truth", "pred"}: int32 [K, 5] numpy records (image, class, root index y * W + x, size, hit), the image index
        counted over all updates, sorted by (image, root index); {"truth_counts", "pred_counts"}: int64
        [images, num_classes] regions per image and class (pred_counts before the min_pixels rule); "images"."""
        c, f = self.num_classes, len(RECORD_FIELDS)
        empty = np.zeros((0, f), np.int32)
        res = {"truth": empty, "pred": empty.copy(), "truth_counts": np.zeros((0, c), np.int64),
               "pred_counts": np.zeros((0, c), np.int64), "images": self.images}
        if not self._chunks:
            return res
        self._trim(wait=True)
        parts = [ch[0].reshape(-1) for ch in self._chunks] + [ch[1].reshape(-1) for ch in self._chunks]
        parts += [ch[2].to(torch.int32).reshape(-1) for ch in self._chunks]          # a count is below 2^31 pixels
        flat = torch.cat(parts).cpu().numpy()                                       # the one read-back
        kt = sum(ch[0].shape[0] for ch in self._chunks) * f
        kp = sum(ch[1].shape[0] for ch in self._chunks) * f
        for key, rec in (("truth", flat[:kt]), ("pred", flat[kt:kt + kp])):
            rec = rec.reshape(-1, f)
            res[key] = np.ascontiguousarray(rec[np.lexsort((rec[:, 2], rec[:, 0]))])
        at, tc, pc = kt + kp, [], []
        for ch in self._chunks:
            n = ch[2].shape[0] // 2
            both = flat[at:at + 2 * n * c].reshape(2, n, c).astype(np.int64)
            tc.append(both[0]); pc.append(both[1])
            at += 2 * n * c
        res["truth_counts"], res["pred_counts"] = np.concatenate(tc), np.concatenate(pc)
        return res


DEFECT_FIELDS = ("image", "class", "root", "size", "x0", "y0", "x1", "y1", "sum_x", "sum_y", "conf_sum_q", "conf_max_q")


def describe_class_regions(labels, num_classes, conf=None, min_pixels=1, image_base=0, merge_gap=0):
    """One record per class region of integer label maps [N, H, W] that has at least ``min_pixels`` pixels: an int64
    [K, 12] numpy array of DEFECT_FIELDS, sorted by (image, root).  Regions are those of ``label_class_regions``;
    ``image`` = image_base + the map's index, ``root`` = the smallest linear index y * W + x of the region, ``x0 .. y1``
    its inclusive bounding box, ``sum_x`` / ``sum_y`` the sums of its pixels' coordinates.  ``conf``: float device tensor
    [N, H, W] (the confidence of ``sheets.seg_confidence``), summed over the region as q(v) = rint(clamp(v, 0, 1) * 65536)
    in ``conf_sum_q`` with its maximum in ``conf_max_q``; both 0 without it (unet_describe_class_regions; integers
    throughout, so the array is a function of the inputs alone).  Two host reads: the region counts, which bound the
    records from above and size the buffer, and the records with their count.

    ``merge_gap`` >= 1 (at most 32) groups the regions first (``group_class_regions`` with this ``min_pixels``): a record
    then describes a group, ``root`` is the group's root, and the return value is (records, fragments), the second
    ``group_class_regions``' table, whose ``group`` column names the record a fragment went into.  0 changes nothing."""
    got = _checked_region_records("describe_class_regions", labels, num_classes, conf, min_pixels, image_base,
                                  merge_gap=merge_gap)
    return got.records if got.fragments is None else (got.records, got.fragments)


def _conf_like(what, conf, shape, device):
    """the fp32 contiguous ``conf``, refused unless it is a float tensor of the labels' ``shape`` on their ``device``"""
    if not torch.is_tensor(conf) or not conf.is_floating_point() or tuple(conf.shape) != shape:
        raise ValueError(f"{what}: conf is a float tensor {shape}, like the labels")
    _require_cuda(conf)
    if conf.device != device:
        raise ValueError(f"{what}: labels and conf share one device")
    return conf.detach().float().contiguous()


def _describe_args(what, labels, num_classes, conf, min_pixels, image_base):
    """(uint8 maps, fp32 conf or None, num_classes, min_pixels, image_base) of ``describe_class_regions``' arguments,
    refused as it refuses them; nothing is launched"""
    _require_cuda(labels)
    c, min_pixels, image_base = int(num_classes), int(min_pixels), int(image_base)
    lib = L.lib()
    if labels.dim() == 3 and labels.numel():           # refused by its shape alone, before anything is converted
        n, h, w = labels.shape
        nbytes = lib.unet_describe_class_regions_workspace(n, h, w, c) if 0 <= c < 2 ** 31 else 0
        if nbytes == 0 or image_base + n >= 2 ** 31:
            raise _class_regions_error(what, n, h, w, num_classes)
    t = _class_maps(labels, what)
    _min_pixels_and_base(what, min_pixels, image_base)
    cf = None if conf is None else _conf_like(what, conf, tuple(t.shape), t.device)
    return t, cf, c, min_pixels, image_base


def _describe_labelled(t, region, sizes, cf, c, min_pixels, image_base, cap):
    """unet_describe_class_regions on maps that are labelled already: the DEVICE int64 buffer of ``cap`` records of
    DEFECT_FIELDS followed by their count."""
    n, h, w = t.shape
    lib = L.lib()
    out, records, count = _record_buffer(cap, len(DEFECT_FIELDS), t.device)
    ws = _workspace(lib.unet_describe_class_regions_workspace(n, h, w, c), t.device)
    L.check(lib.unet_describe_class_regions(_ptr(t), _ptr(region), _ptr(sizes), _ptr(cf), n, h, w, c, min_pixels,
                                            image_base, _ptr(records), cap, _ptr(count), _ptr(ws), ws.numel(), _stream()),
            "unet_describe_class_regions")
    return out


from .defects import SHAPE_HEAD, direction_table  # noqa: E402  (numpy only: the host side of these records)


def shape_fields(directions=32):
    """the field names of a shape record with ``directions`` directions: SHAPE_HEAD, pmin_k, pmax_k"""
    d = int(directions)
    return SHAPE_HEAD + tuple(f"pmin_{k}" for k in range(d)) + tuple(f"pmax_{k}" for k in range(d))


SHAPE_FIELDS = shape_fields(32)


def _measure_args(what, labels, min_pixels, image_base, directions):
    """the direction table int32 [D, 2] once the shape, ``directions``, ``min_pixels`` and ``image_base`` are known to be
    ones unet_measure_class_regions takes; nothing is launched"""
    d, min_pixels, image_base = int(directions), int(min_pixels), int(image_base)
    if labels.dim() == 3 and labels.numel():
        n, h, w = labels.shape
        nbytes = L.lib().unet_measure_class_regions_workspace(n, h, w, d) if -2 ** 31 <= d < 2 ** 31 else 0
        if nbytes == 0 or image_base + n >= 2 ** 31:
            raise RuntimeError(f"{what}: {n} x {h} x {w} maps with {directions} directions are not supported (n < 65536, "
                               "at most 2^31 - 1 pixels, sides up to 16384, an even number of 2..32 directions)")
    _min_pixels_and_base(what, min_pixels, image_base)
    return direction_table(d)


def measure_class_regions(labels, num_classes, min_pixels=1, image_base=0, directions=32, merge_gap=0):
    """One shape record per class region of integer label maps [N, H, W] that has at least ``min_pixels`` pixels: an
    int64 [K, 11 + 2 directions] numpy array of ``shape_fields(directions)`` (SHAPE_FIELDS at the default 32), sorted by
    (image, root).  The regions, ``image``, ``root`` and ``size`` are ``describe_class_regions``': with equal arguments the
    rows of the two align one to one.  ``sum_xx`` / ``sum_yy`` / ``sum_xy``: sums of x x, y y, x y over the region's
    pixels in frame coordinates; ``q1, q2, qd, q3, q4``: its bit-quad counts (2 x 2 windows of the region's own mask with
    one member, two edge-adjacent, two diagonal, three, four); ``pmin_k`` / ``pmax_k``: the extremes of x c_k + y s_k for
    ``defects.direction_table(directions)``.  ``defects.shape_measures`` turns a record into lengths
    (unet_measure_class_regions; integers throughout, so the array is a function of the inputs alone).  Sides up to
    16384, an even number of 2..32 directions.  Two host reads: the region counts and the records with their count.

    ``merge_gap`` >= 1 measures groups as ``describe_class_regions`` describes them and returns (records, fragments); a
    group's bit-quads are those of the union of its fragments, so its Euler number is fragments minus holes."""
    what = "measure_class_regions"                     # its own order of refusals, then the family's pipeline
    _require_cuda(labels)
    gap = _merge_gap(what, merge_gap)
    c = int(num_classes)
    if labels.dim() == 3 and labels.numel():
        n, h, w = labels.shape
        if (L.lib().unet_label_class_regions_workspace(n, h, w, c) if 0 <= c < 2 ** 31 else 0) == 0:
            raise _class_regions_error(what, n, h, w, num_classes)
    table = _measure_args(what, labels, min_pixels, image_base, directions)
    t = _class_maps(labels, what)
    got = _region_records(what, t, None, c, int(min_pixels), int(image_base), gap, False, table, False)
    return got.shapes if got.fragments is None else (got.shapes, got.fragments)


def _measure_labelled(region, sizes, min_pixels, image_base, cap, table):
    """unet_measure_class_regions on labelled maps: the DEVICE int64 buffer of ``cap`` records of
    ``shape_fields(len(table))`` followed by their count."""
    n, h, w = region.shape
    lib = L.lib()
    table = np.ascontiguousarray(table, np.int32)
    d = table.shape[0]
    out, records, count = _record_buffer(cap, len(SHAPE_HEAD) + 2 * d, region.device)
    ws = _workspace(lib.unet_measure_class_regions_workspace(n, h, w, d), region.device)
    L.check(lib.unet_measure_class_regions(_ptr(region), _ptr(sizes), n, h, w, min_pixels, image_base,
                                           table.ctypes.data, d, _ptr(records), cap, _ptr(count), _ptr(ws), ws.numel(),
                                           _stream()), "unet_measure_class_regions")
    return out


def describe_and_measure_class_regions(labels, num_classes, conf=None, min_pixels=1, image_base=0, directions=32,
                                       contours=False, merge_gap=0):
    """(``describe_class_regions``' records, ``measure_class_regions``' records) of one labelling: the maps are labelled
    once, both kernels run on that labelling, and the two record sets come to the host in one buffer, so the host reads
    stay two (the region counts, then the records).  The rows of the two arrays align.

    ``contours=True`` traces the same labelling too and returns (records, shape records, loops, points), the last two as
    ``trace_class_regions`` gives them: the edge counts come with the records, and the outlines are a third read.  With
    it ``directions=None`` leaves the shapes out (None in their place).

    ``merge_gap`` >= 1 groups the regions first (``group_class_regions`` with this ``min_pixels``); both kernels then run
    on the groups, and the returned tuple gains ``group_class_regions``' fragment table as its last element.  The
    outlines stay those of the FRAGMENT labelling with the same ``min_pixels`` (a loop's ``root`` is its fragment's, and
    every fragment has exactly one outer loop); ``polygons.outlines`` attributes them to groups through the table."""
    got = _checked_region_records("describe_and_measure_class_regions", labels, num_classes, conf, min_pixels, image_base,
                                  shaped=not (contours and directions is None), directions=directions, contours=contours,
                                  merge_gap=merge_gap)
    out = (got.records, got.shapes) + ((got.loops, got.points) if contours else ())
    return out if got.fragments is None else out + (got.fragments,)


class RegionRecords(NamedTuple):
    """What one labelling of class regions gave, by name: the numpy arrays that ``describe_class_regions``
    (``records``), ``measure_class_regions`` (``shapes``), ``trace_class_regions`` (``loops``, ``points``) and
    ``group_class_regions`` (``fragments``) return, None for what was not asked for."""
    records: Optional[np.ndarray] = None
    shapes: Optional[np.ndarray] = None
    loops: Optional[np.ndarray] = None
    points: Optional[np.ndarray] = None
    fragments: Optional[np.ndarray] = None


def class_region_records(labels, num_classes, conf=None, min_pixels=1, image_base=0, *, describe=True, directions=None,
                         contours=False, merge_gap=0):
    """The class-region records of integer label maps [N, H, W], every kind from ONE labelling, as ``RegionRecords``.
    ``describe`` fills ``records`` as ``describe_class_regions`` gives them (``conf``, ``min_pixels`` and ``image_base``
    are its arguments), ``directions`` (a number of Feret directions; None: no shapes) fills ``shapes`` as
    ``measure_class_regions`` gives them, ``contours`` fills ``loops`` and ``points`` as ``trace_class_regions`` gives
    them, and ``merge_gap`` >= 1 (at most 32) fills ``fragments`` with ``group_class_regions``' table: ``records`` and
    ``shapes`` are then those of the groups, while the outlines stay those of the fragments.  Everything not asked for is
    None, and the rows of ``records`` and ``shapes`` align.  Two host reads -- the region counts, then every record set in
    one buffer -- and with ``contours`` the outlines as a third.  Maps without a region give empty arrays."""
    return _checked_region_records("class_region_records", labels, num_classes, conf, min_pixels, image_base,
                                   describe=describe, shaped=directions is not None, directions=directions,
                                   contours=contours, merge_gap=merge_gap)


def _checked_region_records(what, labels, num_classes, conf, min_pixels, image_base, describe=True, shaped=False,
                            directions=None, contours=False, merge_gap=0):
    """``_region_records`` of arguments that are refused, under the name ``what``, in the order of
    ``describe_and_measure_class_regions``: the gap, ``describe_class_regions``' arguments, the directions, the outlines"""
    gap = _merge_gap(what, merge_gap)
    t, cf, c, min_pixels, image_base = _describe_args(what, labels, num_classes, conf, min_pixels, image_base)
    table = _measure_args(what, t, min_pixels, image_base, directions) if shaped else None
    if contours:
        _trace_args(what, t)
    if not (describe or shaped or contours or gap):
        raise ValueError(f"{what}: nothing was asked for")
    return _region_records(what, t, cf, c, min_pixels, image_base, gap, describe, table, contours)


def _read_parts(parts):
    """{name: host int64 array} of {name: DEVICE int64 buffer}, all of them in ONE read"""
    device = list(parts.values())
    host = (device[0] if len(device) == 1 else torch.cat(device)).cpu().numpy()      # one buffer needs no copy first
    return dict(zip(parts, np.split(host, np.cumsum([p.numel() for p in device])[:-1])))


def _region_records(what, t, cf, c, min_pixels, image_base, gap, describe, table, contours):
    """The pipeline behind every function of the family, on checked arguments: label, group if ``gap``, launch what was
    asked for (``describe``, a direction ``table``, ``contours``), read it all at once, sort on the host -> RegionRecords."""
    fd, ff = len(DEFECT_FIELDS), len(FRAGMENT_FIELDS)
    fs = 0 if table is None else len(SHAPE_HEAD) + 2 * len(table)
    region, sizes, counts = label_class_regions(t, c)
    cap = int(counts.sum())                            # every record is a region: there cannot be more
    if cap == 0:
        return RegionRecords(np.zeros((0, fd), np.int64) if describe else None,
                             np.zeros((0, fs), np.int64) if fs else None, *(_no_outlines() if contours else (None, None)),
                             np.zeros((0, ff), np.int64) if gap else None)
    whole, whole_sizes, parts = region, sizes, {}      # what is described and measured: the regions or their groups
    if gap:
        whole, whole_sizes, _, frag = _group_labelled(t, region, sizes, c, gap, min_pixels, image_base, cap)
    if describe:
        parts["records"] = _describe_labelled(t, whole, whole_sizes, cf, c, min_pixels, image_base, cap)
    if fs:
        parts["shapes"] = _measure_labelled(whole, whole_sizes, min_pixels, image_base, cap, table)
    if gap:
        parts["fragments"] = frag
    if contours:
        parts["edges"] = _count_edges(region, sizes, min_pixels)
    host = _read_parts(parts)
    too_many = f"{what}: more records than regions"
    rec = _host_records(host["records"], cap, fd, (0, 2), too_many) if describe else None
    shapes = _host_records(host["shapes"], cap, fs, (0, 1), too_many) if fs else None
    if describe and fs and (len(rec) != len(shapes) or (rec[:, [0, 2, 3]] != shapes[:, :3]).any()):
        raise RuntimeError(f"{what}: the two record sets differ")      # cannot happen
    fragments, loops, points = None, None, None
    if gap:
        fragments = _host_records(host["fragments"], cap, ff, (0, 3, 2), f"{what}: more fragments than regions")
    if contours:
        loops, points = _trace_counted(region, sizes, min_pixels, image_base, host["edges"].tolist(), what)
    return RegionRecords(rec, shapes, loops, points, fragments)


LOOP_FIELDS = ("image", "root", "leader", "n_points", "first_point", "area2")


def _no_outlines():
    return np.zeros((0, len(LOOP_FIELDS)), np.int64), np.zeros((0, 2), np.int32)


def _trace_args(what, region):
    """refuse, before anything is launched, maps that unet_trace_class_regions does not take"""
    if region.dim() != 3 or region.numel() == 0:
        raise ValueError(f"{what}: [N, H, W] maps, got {tuple(region.shape)}")
    n, h, w = region.shape
    if L.lib().unet_count_class_region_edges_workspace(n, h, w) == 0:
        raise RuntimeError(f"{what}: {n} x {h} x {w} maps cannot be traced (n < 65536, at most 2^29 pixels)")


def _count_edges(region, sizes, min_pixels):
    """unet_count_class_region_edges: the DEVICE int64 [3] counts {edges, loops, points}"""
    n, h, w = region.shape
    lib = L.lib()
    counts = torch.empty(3, dtype=torch.int64, device=region.device)
    ws = _workspace(lib.unet_count_class_region_edges_workspace(n, h, w), region.device)
    L.check(lib.unet_count_class_region_edges(_ptr(region), _ptr(sizes), n, h, w, min_pixels, _ptr(counts), _ptr(ws),
                                              ws.numel(), _stream()), "unet_count_class_region_edges")
    return counts


def _trace_counted(region, sizes, min_pixels, image_base, counted, what):
    """unet_trace_class_regions with buffers of the ``counted`` {edges, loops, points}: (loops, points) on the host, one
    read"""
    n, h, w = region.shape
    edges, n_loops, n_points = (int(v) for v in counted)
    if edges == 0:
        return _no_outlines()
    lib = L.lib()
    nbytes = lib.unet_trace_class_regions_workspace(n, h, w, edges)
    if nbytes == 0 or image_base + n >= 2 ** 31:
        raise RuntimeError(f"{what}: {edges} edges of {n} x {h} x {w} maps cannot be traced")
    out = torch.empty(n_loops * len(LOOP_FIELDS) + 3 + n_points, dtype=torch.int64, device=region.device)
    loops, counts, points = out[:n_loops * 6], out[n_loops * 6:n_loops * 6 + 3], out[n_loops * 6 + 3:]
    ws = _workspace(nbytes, region.device)
    L.check(lib.unet_trace_class_regions(_ptr(region), _ptr(sizes), n, h, w, min_pixels, image_base, edges, _ptr(loops),
                                         n_loops, _ptr(points), n_points, _ptr(counts), _ptr(ws), ws.numel(), _stream()),
            "unet_trace_class_regions")
    host = out.cpu().numpy()
    if host[n_loops * 6:n_loops * 6 + 3].tolist() != [edges, n_loops, n_points]:
        raise RuntimeError(f"{what}: the two stages count differently")      # cannot happen
    return (np.ascontiguousarray(host[:n_loops * 6].reshape(n_loops, 6)),
            np.ascontiguousarray(host[n_loops * 6 + 3:].view(np.int32).reshape(n_points, 2)))


def trace_class_regions(region, sizes, min_pixels=1, image_base=0):
    """The outlines of labelled class regions, traced on the device (csrc/contours.hip; the inverse of
    ``augment.polygon_masks_u8``).  ``region`` / ``sizes``: the int32 DEVICE tensors [N, H, W] of ``label_class_regions``; a
    region is traced iff it has at least ``min_pixels`` pixels, the keep rule of ``describe_class_regions``.  Returns
    (loops, points), numpy: loops int64 [L, 6] of LOOP_FIELDS -- ``image`` = image_base + the map's index, ``root`` = the
    region's smallest linear index (the ``root`` of the defect records), ``leader`` = the loop's smallest crack edge id,
    ``n_points`` / ``first_point`` = its rows of ``points``, ``area2`` = twice its signed area: > 0 for a region's one
    outer loop, < 0 for a hole -- in ascending (image, leader); points int32 [P, 2] = (x, y) pixel centres in walk
    order.  Pillow's ``ImageDraw.polygon`` of an outer loop's points fills the region with its holes closed
    (``polygons.outlines`` groups the loops by region).  Integers and prefix sums throughout: two runs give the same
    bytes.  At most 2^29 pixels.  Two host reads: {edges, loops, points}, which size the buffers, then the outlines."""
    _require_cuda(region, sizes)
    if region.dtype != torch.int32 or sizes.dtype != torch.int32 or region.shape != sizes.shape \
            or region.device != sizes.device:
        raise ValueError("trace_class_regions: region and sizes are the int32 tensors of label_class_regions")
    min_pixels, image_base = int(min_pixels), int(image_base)
    _trace_args("trace_class_regions", region)
    _min_pixels_and_base("trace_class_regions", min_pixels, image_base)
    region, sizes = region.contiguous(), sizes.contiguous()
    counted = _count_edges(region, sizes, min_pixels).tolist()
    return _trace_counted(region, sizes, min_pixels, image_base, counted, "trace_class_regions")


PAIR_FIELDS = ("image", "truth_root", "pred_root", "overlap")


def _pairs_on_device(truth_region, pred_region, image_base, what):
    """(DEVICE int32 buffer of ``record_cap`` records of PAIR_FIELDS followed by the int64 count and overflow, record_cap)
    of two region maps; (None, 0) where no pixel carries a pair.  One host read: the bound."""
    _require_cuda(truth_region, pred_region)
    for r in (truth_region, pred_region):
        if r.dtype != torch.int32 or r.dim() != 3 or r.numel() == 0:
            raise ValueError(f"{what}: int32 [N, H, W] region maps of label_class_regions, got {r.dtype} {tuple(r.shape)}")
    if truth_region.shape != pred_region.shape or truth_region.device != pred_region.device:
        raise ValueError(f"{what}: the two region maps differ in shape or device")
    image_base = int(image_base)
    _min_pixels_and_base(what, 1, image_base)          # pairs have no min_pixels
    tr, pr = truth_region.detach().contiguous(), pred_region.detach().contiguous()
    n, h, w = tr.shape
    if n >= 65536 or n * h * w >= 2 ** 31 or image_base + n >= 2 ** 31:
        raise RuntimeError(f"{what}: {n} x {h} x {w} maps are not supported (n < 65536, at most 2^31 - 1 pixels, image "
                           "indices below 2^31)")
    lib = L.lib()
    bound = torch.zeros(n, dtype=torch.int64, device=tr.device)
    L.check(lib.unet_region_pair_bound(_ptr(tr), _ptr(pr), n, h, w, _ptr(bound), _stream()), "unet_region_pair_bound")
    per_image = bound.tolist()                         # >= the distinct pairs of every image
    record_cap = sum(per_image)
    if record_cap == 0:
        return None, 0
    capacity = 1 << (2 * max(per_image) - 1).bit_length()      # the next power of two: a load factor of at most 1 / 2
    nbytes = lib.unet_region_pairs_workspace(n, capacity)
    if nbytes == 0:
        raise RuntimeError(f"{what}: {n} tables of {capacity} slots are not supported")
    f = len(PAIR_FIELDS)
    out = torch.empty(record_cap * f + 4, dtype=torch.int32, device=tr.device)      # 16 bytes a record: the tail is aligned
    tail = out[record_cap * f:].view(torch.int64)      # {count, overflow}
    tail.zero_()
    ws = _workspace(nbytes, tr.device)
    L.check(lib.unet_region_pairs(_ptr(tr), _ptr(pr), n, h, w, capacity, image_base, _ptr(out), record_cap, _ptr(tail),
                                  _ptr(tail[1:]), _ptr(ws), ws.numel(), _stream()), "unet_region_pairs")
    return out, record_cap


def _pair_records(host, record_cap, what):
    """the sorted int64 records of ``_pairs_on_device``'s buffer, read to the host"""
    f = len(PAIR_FIELDS)
    count, overflow = (int(v) for v in host[record_cap * f:].view(np.int64))
    if overflow != 0 or count > record_cap:
        raise RuntimeError(f"{what}: {overflow} pixels found no slot, {count} records for {record_cap}")     # cannot happen
    rec = host[:count * f].reshape(count, f).astype(np.int64)
    return np.ascontiguousarray(rec[np.lexsort((rec[:, 2], rec[:, 1], rec[:, 0]))])


def pair_class_regions(truth_region, pred_region, image_base=0):
    """The overlaps of two region labellings: one record of PAIR_FIELDS per pair of a region of ``truth_region`` and a
    region of ``pred_region`` (int32 [N, H, W] DEVICE ``region`` maps of ``label_class_regions``: 1 + root index, 0 on
    background) of the same image that share a pixel, whatever their classes; ``overlap`` = the shared pixels, ``image``
    = image_base + the map's index.  An int64 [K, 4] numpy array sorted by (image, truth_root, pred_root)
    (csrc/regionpairs.hip; integers throughout, so the array is a function of the two maps alone).  Two host reads: the
    bound on the pairs per image, which sizes the hash tables (the next power of two >= twice the largest) and the
    record buffer, and the records with their count."""
    out, record_cap = _pairs_on_device(truth_region, pred_region, image_base, "pair_class_regions")
    if out is None:
        return np.zeros((0, len(PAIR_FIELDS)), np.int64)
    return _pair_records(out.cpu().numpy(), record_cap, "pair_class_regions")


class DetectionMatcher:
    """Region records for detection curves over confidence, accumulated over batches: every truth region, every kept
    predicted region (at least ``min_pixels`` pixels) with its summed confidence, and the overlap of every pair of them
    that shares a pixel.  ``seg_detection`` turns the three record sets into recall / precision / false alarms as a
    function of the confidence a predicted region must reach, which ``ClassRegionMatcher``'s one ``hit`` per region
    cannot give.

    ``update`` labels truth and prediction in one call (``label_class_regions``), describes each half with that
    labelling (unet_describe_class_regions: truth without confidence and with every region, the prediction with ``conf``
    and ``min_pixels``) and pairs the two ``region`` halves (``pair_class_regions``' kernels).  Every update may have
    another (H, W).  It reads the region counts, the pair bound and the records back, so it SYNCHRONISES per update: that
    is acceptable for an evaluation pass, and it keeps nothing on the device.

    ``merge_gap`` >= 1 groups the PREDICTED half of the labelling (``group_class_regions`` with ``min_pixels``): a
    predicted record is then a group, and the pairs are those of the truth regions with the groups.  The truth half stays
    as labelled.  Dropped regions have id 0 in the grouped map and so make no pairs."""

    def __init__(self, num_classes, min_pixels=1, merge_gap=0):
        self.merge_gap = _merge_gap("DetectionMatcher", merge_gap)
        self.num_classes, self.min_pixels = _matcher_args("DetectionMatcher", num_classes, min_pixels)
        self.images = 0
        self.image_sizes = []
        self._truth, self._pred, self._pairs = [], [], []

    def update(self, pred_labels, conf, truth):
        """pred_labels / truth: integer device label maps of equal shape [N, H, W] (values outside 0..254 become 255);
        conf: float device tensor [N, H, W], the confidence of ``sheets.seg_confidence`` or of ``tiling.blend_tiles``."""
        what = "DetectionMatcher.update"
        p = _class_maps(pred_labels, what)
        t = _class_maps(truth.to(p.device), what)
        if p.shape != t.shape:
            raise ValueError(f"{what}: prediction / truth shapes differ")
        n, h, w = p.shape
        cf = _conf_like(what, conf, (n, h, w), p.device)
        c, base = self.num_classes, self.images
        if L.lib().unet_describe_class_regions_workspace(n, h, w, c) == 0 or base + n >= 2 ** 31:
            raise _class_regions_error(what, n, h, w, c)
        region, sizes, counts = label_class_regions(torch.cat([t, p]), c)      # one pass labels both
        cap_t, cap_p = counts.reshape(2, -1).sum(1).tolist()
        preg, psiz = region[n:], sizes[n:]
        if self.merge_gap and cap_p:
            preg, psiz, _, _ = _group_labelled(p, preg, psiz, c, self.merge_gap, self.min_pixels, base, cap_p)
        halves = []
        for maps, reg, siz, cfd, mp, cap in ((t, region[:n], sizes[:n], None, 1, cap_t),
                                             (p, preg, psiz, cf, self.min_pixels, cap_p)):
            halves.append(_describe_labelled(maps, reg, siz, cfd, c, mp, base, cap) if cap else None)
        pairs, record_cap = _pairs_on_device(region[:n], preg, base, what)
        empty = np.zeros((0, len(DEFECT_FIELDS)), np.int64)
        trec, prec = (empty if o is None else _host_records(o.cpu().numpy(), cap, len(DEFECT_FIELDS), (0, 2),
                                                            f"{what}: more records than regions")
                      for o, cap in zip(halves, (cap_t, cap_p)))
        prs = np.zeros((0, len(PAIR_FIELDS)), np.int64)
        if pairs is not None:
            prs = _pair_records(pairs.cpu().numpy(), record_cap, what)
            kept = (prec[:, 0] - base) * (h * w) + prec[:, 2]                   # the kept predicted regions of this update
            prs = prs[np.isin((prs[:, 0] - base) * (h * w) + prs[:, 2], kept)]
        self._truth.append(trec)
        self._pred.append(prec)
        self._pairs.append(prs)
        self.image_sizes.extend([(h, w)] * n)
        self.images += n

    def compute(self):
        """{"truth": int64 [Kt, 12], "pred": int64 [Kp, 12]} numpy records of DEFECT_FIELDS sorted by (image, root) (truth
        with conf_sum_q = conf_max_q = 0), "pairs": int64 [K, 4] of PAIR_FIELDS sorted by (image, truth_root, pred_root),
        without the pairs of predicted regions below ``min_pixels``, "image_sizes": [(H, W)] per image, "images".  The
        image index counts over all updates; a root index is y * W + x in its own image's width."""
        def cat(parts, fields):
            return np.concatenate(parts) if parts else np.zeros((0, len(fields)), np.int64)

        return {"truth": cat(self._truth, DEFECT_FIELDS), "pred": cat(self._pred, DEFECT_FIELDS),
                "pairs": cat(self._pairs, PAIR_FIELDS), "image_sizes": list(self.image_sizes), "images": self.images}


BOUNDARY_NONE = 1 << 30         # UNET_BOUNDARY_NONE of include/unet_hip.h
BOUNDARY_MAX_TOLERANCES = 4
BOUNDARY_HIST_BINS = 1025
BOUNDARY_FIELDS = (("image", "class", "t_pixels", "p_pixels", "t_boundary", "p_boundary")
                   + tuple(f"p_near{k}" for k in range(BOUNDARY_MAX_TOLERANCES))
                   + tuple(f"t_near{k}" for k in range(BOUNDARY_MAX_TOLERANCES))
                   + ("band_inter", "band_union", "p_dist_sum_q8", "t_dist_sum_q8", "p_dist_max_sq", "t_dist_max_sq"))


def _boundary_error(what, n, h, w, num_classes):
    return RuntimeError(f"{what}: {n} x {h} x {w} maps of {num_classes} classes are not supported (sides up to 4096, 2..32 "
                        "classes, n < 65536, fewer than 2^31 distances)")


def boundary_distance_sq(labels, num_classes):
    """Exact squared Euclidean distance to the class boundaries of integer label maps [N, H, W]: an int32
    [N, num_classes - 1, H, W] DEVICE tensor, [n, c - 1, y, x] = the minimum of (y - y')^2 + (x - x')^2 over the boundary
    pixels (y', x') of class c of image n, BOUNDARY_NONE in a plane whose image has none.  A pixel has class c iff its value
    is c, 1 <= c < num_classes (everything else is background); it is a boundary pixel of c iff at least one 4-neighbour
    inside the frame has another value, so the frame edge makes no boundary.  What
    rint(scipy.ndimage.distance_transform_edt(~boundary) ** 2) gives plane by plane (unet_boundary_distance_sq, integers
    throughout); does not synchronise."""
    c = int(num_classes)
    lib = L.lib()
    if torch.is_tensor(labels) and labels.dim() == 3 and labels.numel():      # refused by its shape, before any conversion
        n, h, w = labels.shape
        if not 0 <= c < 2 ** 31 or lib.unet_boundary_distance_sq_workspace(n, h, w, c) == 0:
            raise _boundary_error("boundary_distance_sq", n, h, w, num_classes)
    t = _class_maps(labels, "boundary_distance_sq")
    n, h, w = t.shape
    d2 = torch.empty((n, c - 1, h, w), dtype=torch.int32, device=t.device)
    ws = _workspace(lib.unet_boundary_distance_sq_workspace(n, h, w, c), t.device)
    L.check(lib.unet_boundary_distance_sq(_ptr(t), n, h, w, c, _ptr(d2), _ptr(ws), ws.numel(), _stream()),
            "unet_boundary_distance_sq")
    return d2


def boundary_band_width(h, w):
    """Boundary IoU's default band: 2 % of the image diagonal, at least one pixel"""
    import math
    return max(1, round(0.02 * math.sqrt(h * h + w * w)))


class BoundaryMatcher:
    """Outline accuracy of predicted against true label maps, accumulated over batches: one record of BOUNDARY_FIELDS per
    (image, foreground class) and a pooled histogram of boundary-to-boundary distances (unet_boundary_stats; integers
    throughout, so both are a function of the label maps alone).  ``p_*`` fields belong to the prediction, ``t_*`` to the
    truth: pixels and boundary pixels of the class; ``p_near{k}`` = predicted boundary pixels within ``tolerances[k]``
    pixels (Euclidean) of the truth's boundary of the class, ``t_near{k}`` the other way round, the slots past the last
    tolerance 0; ``band_inter`` / ``band_union`` = Boundary IoU's counts at the band width; ``p_dist_sum_q8`` = the sum over
    the predicted boundary pixels of floor(256 * distance to the truth's boundary) and ``p_dist_max_sq`` the largest
    squared distance among them, ``t_*`` the other way round.  Where the other map has no boundary of the class, a boundary
    pixel counts in ``p_boundary`` / ``t_boundary`` only: ``seg_boundaries`` reports it as unmatched.

    ``band_width`` = 0 means ``boundary_band_width(H, W)`` of the maps of each update (2 % of the diagonal, as the Boundary
    IoU paper has it), so images of different sizes get their own.  ``update`` makes one distance call for truth and
    prediction together and one statistics call, keeps the batch's records on the device and does not synchronise;
    ``compute`` reads everything back once."""

    def __init__(self, num_classes, tolerances=(1, 2, 4), band_width=0):
        self.num_classes = int(num_classes)
        if not 2 <= self.num_classes <= 32:
            raise ValueError(f"BoundaryMatcher: {num_classes} classes, 2..32 are supported")
        tol = list(tolerances)
        if not 1 <= len(tol) <= BOUNDARY_MAX_TOLERANCES:
            raise ValueError(f"BoundaryMatcher: 1..{BOUNDARY_MAX_TOLERANCES} tolerances, got {len(tol)}")
        for v in list(tol) + [band_width]:
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 4096:
                raise ValueError(f"BoundaryMatcher: tolerances and band_width are integers in 0..4096, got {v!r}")
        self.tolerances = tuple(int(v) for v in tol)
        self.band_width = int(band_width)
        self._tol_sq = (C.c_int32 * len(tol))(*[v * v for v in self.tolerances])
        self.images = 0
        self.band_widths, self.image_sizes = [], []      # per image
        self._records, self._hist = [], None

    def update(self, pred_labels, truth):
        """pred_labels / truth: integer device label maps of equal shape [N, H, W] (values outside 0..254 become 255)."""
        what = "BoundaryMatcher.update"
        if torch.is_tensor(pred_labels) and torch.is_tensor(truth) and pred_labels.shape != truth.shape:
            raise ValueError(f"{what}: prediction / truth shapes differ")
        p = _class_maps(pred_labels, what)
        t = _class_maps(truth.to(p.device), what)
        n, h, w = p.shape
        c, dev = self.num_classes, p.device
        if 2 * n >= 65536 or self.images + n >= 2 ** 31:
            raise _boundary_error(what, 2 * n, h, w, c)
        d2 = boundary_distance_sq(torch.cat([t, p]), c)       # one pass serves both
        band = self.band_width or boundary_band_width(h, w)
        if self._hist is None:
            self._hist = torch.zeros((c - 1, 2, BOUNDARY_HIST_BINS), dtype=torch.int64, device=dev)
        records = torch.zeros((n, c - 1, len(BOUNDARY_FIELDS)), dtype=torch.int64, device=dev)
        L.check(L.lib().unet_boundary_stats(_ptr(t), _ptr(p), _ptr(d2[:n]), _ptr(d2[n:]), n, h, w, c, self._tol_sq,
                                            len(self.tolerances), band * band, self.images, _ptr(records),
                                            _ptr(self._hist), _stream()), "unet_boundary_stats")
        self._records.append(records)
        self.band_widths.extend([band] * n)
        self.image_sizes.extend([(h, w)] * n)
        self.images += n

    def compute(self):
        """{"records": int64 [images * (num_classes - 1), 20] numpy records of BOUNDARY_FIELDS sorted by (image, class), the
        image index counted over all updates; "hist": int64 [num_classes - 1, 2, 1025], direction 0 = prediction to
        truth, 1 = truth to prediction, bin min(floor(distance), 1024); "band_widths" and "image_sizes" per image;
        "tolerances"; "images"}."""
        c, f = self.num_classes, len(BOUNDARY_FIELDS)
        res = {"records": np.zeros((0, f), np.int64), "hist": np.zeros((c - 1, 2, BOUNDARY_HIST_BINS), np.int64),
               "band_widths": list(self.band_widths), "image_sizes": list(self.image_sizes),
               "tolerances": self.tolerances, "images": self.images}
        if not self._records:
            return res
        flat = torch.cat([r.reshape(-1) for r in self._records] + [self._hist.reshape(-1)]).cpu().numpy()  # the one read-back
        rec = flat[:-self._hist.numel()].reshape(-1, f)
        res["records"] = np.ascontiguousarray(rec[np.lexsort((rec[:, 1], rec[:, 0]))])
        res["hist"] = flat[-self._hist.numel():].reshape(c - 1, 2, BOUNDARY_HIST_BINS).copy()
        return res


CALIBRATION_MAX_BINS = 64
CALIBRATION_MAX_TEMPERATURES = 32
CALIBRATION_SELECT = {"all": 0, "defects": 1}


class CalibrationMeter:
    """Calibration of the per-pixel confidence, accumulated over batches (csrc/calibration.hip): a reliability histogram of
    the confidence at ``temperature`` and the summed negative log-likelihood of softmax(logits / T) for every T of
    ``temperatures`` (up to 32), both over the same pixels.  A pixel whose target is ``ignore_index`` or outside
    0..num_classes-1 is skipped; ``select`` "defects" also leaves out the pixels whose target and label are both class 0
    (background is ~99 % of these data sets).  ``seg_calibration`` turns the result into ECE / MCE and a fitted temperature.

    ``update`` makes three launches -- the confidence at ``temperature`` (``sheets.seg_confidence``), the histogram
    (unet_reliability_histogram), the sweep (unet_temperature_sweep) -- into device accumulators and does not synchronise;
    ``update_confidence`` takes labels and confidence that exist already (``tiling.blend_tiles`` makes them) and runs the
    histogram alone.  ``compute`` reads everything back once."""

    def __init__(self, num_classes, bins=15, temperatures=(1.0,), temperature=1.0, ignore_index=None, select="all"):
        from .sheets import inverse_temperature
        self.num_classes, self.bins = int(num_classes), int(bins)
        if not 2 <= self.num_classes <= 8:
            raise ValueError(f"CalibrationMeter: {num_classes} classes, 2..8 are supported")
        if not 1 <= self.bins <= CALIBRATION_MAX_BINS:
            raise ValueError(f"CalibrationMeter: {bins} bins, 1..{CALIBRATION_MAX_BINS} are supported")
        self.temperatures = tuple(float(t) for t in temperatures)
        if not 1 <= len(self.temperatures) <= CALIBRATION_MAX_TEMPERATURES:
            raise ValueError(f"CalibrationMeter: {len(self.temperatures)} temperatures, 1..{CALIBRATION_MAX_TEMPERATURES} "
                             "are supported")
        self.inv_t = [inverse_temperature(t, "CalibrationMeter: temperature") for t in self.temperatures]
        self.temperature = float(temperature)
        inverse_temperature(self.temperature, "CalibrationMeter: temperature")
        if select not in CALIBRATION_SELECT:
            raise ValueError(f"CalibrationMeter: select is 'all' or 'defects', got {select!r}")
        self.select = select
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self._inv_t = (C.c_float * len(self.inv_t))(*self.inv_t)
        self._counts = None            # int64 [C * bins * 3 + 3]: the histogram, skipped, taken, non-finite
        self._nll = None               # float64 [K]

    def _accumulators(self, dev):
        if self._counts is None:
            self._counts = torch.zeros(self.num_classes * self.bins * 3 + 3, dtype=torch.int64, device=dev)
            self._nll = torch.zeros(len(self.temperatures), dtype=torch.float64, device=dev)
        elif self._counts.device != dev:
            raise ValueError("CalibrationMeter: every update must be on the same device")
        return self._counts, self._nll

    def _target(self, target, shape, dev, what):
        if not torch.is_tensor(target) or target.is_floating_point() or target.dtype == torch.bool \
                or tuple(target.shape) != shape:
            raise ValueError(f"{what}: the target is an integer tensor {shape}")
        return target.detach().to(device=dev, dtype=torch.int64).contiguous()

    def update_confidence(self, labels, conf, target):
        """labels uint8 / conf float32 / target integer DEVICE tensors (N, H, W): the histogram alone."""
        what = "CalibrationMeter.update_confidence"
        _require_cuda(labels, conf)
        if labels.dtype != torch.uint8 or labels.dim() != 3 or labels.numel() == 0:
            raise ValueError(f"{what}: labels are a uint8 (N, H, W) tensor, got {labels.dtype} {tuple(labels.shape)}")
        if not conf.is_floating_point() or conf.shape != labels.shape or conf.device != labels.device:
            raise ValueError(f"{what}: conf is a float tensor {tuple(labels.shape)} on the labels' device")
        n, h, w = labels.shape
        t = self._target(target, (n, h, w), labels.device, what)
        lab, cf = labels.detach().contiguous(), conf.detach().float().contiguous()
        counts, _ = self._accumulators(lab.device)
        cells = self.num_classes * self.bins * 3
        ign = -1 if self.ignore_index is None else self.ignore_index       # a negative target is skipped anyway
        L.check(L.lib().unet_reliability_histogram(_ptr(lab), _ptr(cf), _ptr(t), n, h * w, self.num_classes, self.bins, ign,
                                                   CALIBRATION_SELECT[self.select], _ptr(counts), _ptr(counts[cells:]),
                                                   _stream()), "unet_reliability_histogram")

    def update(self, logits, target):
        """logits: float DEVICE tensor (N, num_classes, H, W); target: integer tensor (N, H, W)."""
        from .sheets import seg_confidence
        what = "CalibrationMeter.update"
        _require_cuda(logits)
        if logits.dim() != 4 or logits.shape[1] != self.num_classes or logits.numel() == 0:
            raise ValueError(f"{what}: logits are (N, {self.num_classes}, H, W), got {tuple(logits.shape)}")
        n, c, h, w = logits.shape
        x = logits.detach().float().contiguous()
        t = self._target(target, (n, h, w), x.device, what)
        labels, conf = seg_confidence(x, temperature=self.temperature)
        self.update_confidence(labels, conf, t)
        counts, nll = self._accumulators(x.device)
        lib = L.lib()
        k = len(self.inv_t)
        nbytes = lib.unet_temperature_sweep_workspace(n, h * w, k)
        if nbytes == 0:
            raise RuntimeError(f"{what}: {n} x {h} x {w} logits are not supported (n < 65536, at most 2^31 - 1 pixels an image)")
        ws = _workspace(nbytes, x.device)
        cells = c * self.bins * 3
        ign = -1 if self.ignore_index is None else self.ignore_index
        L.check(lib.unet_temperature_sweep(_ptr(x), _ptr(t), n, c, h * w, ign, CALIBRATION_SELECT[self.select], self._inv_t,
                                           k, _ptr(nll), _ptr(counts[cells + 1:]), _ptr(ws), ws.numel(), _stream()),
                "unet_temperature_sweep")

    def compute(self):
        """{"hist": int64 [num_classes, bins, 3] numpy {pixels, correct pixels, sum of q = rint(65536 conf)} by predicted
        class and bin, "skipped", "nll": float64 [K] summed over "counted" pixels, "nonfinite": pixels with a non-finite
        logit, set aside by the sweep, "temperatures", "temperature", "bins", "select"}."""
        c, b, k = self.num_classes, self.bins, len(self.temperatures)
        res = {"hist": np.zeros((c, b, 3), np.int64), "skipped": 0, "nll": np.zeros(k, np.float64), "counted": 0,
               "nonfinite": 0, "temperatures": self.temperatures, "temperature": self.temperature, "bins": b,
               "select": self.select}
        if self._counts is None:
            return res
        flat = torch.cat([self._counts, self._nll.view(torch.int64)]).cpu().numpy()      # the one read-back
        cells = c * b * 3
        res["hist"] = flat[:cells].reshape(c, b, 3).copy()
        res["skipped"], res["counted"], res["nonfinite"] = (int(v) for v in flat[cells:cells + 3])
        res["nll"] = flat[cells + 3:].view(np.float64).copy()
        return res


def preprocess_u8(images_u8, flips=None, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """uint8 [N, H, W, 3] device batch -> normalised fp32 NCHW (ToTensor + Normalize, optional per-sample horizontal
    flip): /root/reference/src/dataset.py:134-146, src/kolektorsdd_dataset.py:133-150, on the GPU."""
    _require_cuda(images_u8)
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3:
        raise ValueError("preprocess_u8 expects a uint8 [N, H, W, 3] tensor")
    images_u8 = images_u8.contiguous()
    n, h, w, _ = images_u8.shape
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=images_u8.device)
    fl = None
    if flips is not None:
        fl = flips.to(device=images_u8.device, dtype=torch.uint8).contiguous()
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s_ = (C.c_float * 3)(*[float(v) for v in std])
    L.check(L.lib().unet_preprocess_u8(_ptr(images_u8), _ptr(fl), _ptr(out), n, h, w, m, s_, _stream()),
            "unet_preprocess_u8")
    return out
