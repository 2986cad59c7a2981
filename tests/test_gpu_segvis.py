"""GPU tests of the segmentation prediction sheets (csrc/segvis.hip through ops.seg_confidence and
ops.render_seg_sheet) against tests/_segvis_ref.py -- labels byte for byte, the confidence within a float64 bound whose
terms are written out, the sheets byte for byte -- and of the two visualiser CLIs end to end.  The confidence cases
print their figures as `REF64 segconf` lines (run with -s).
"""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch

import _ref64 as R64
import _segvis_ref as S
from tiaozhanbei_unet_amd import _lib as L
from tiaozhanbei_unet_amd import ops
from tiaozhanbei_unet_amd.metrics import image_prediction_stats, per_image_stats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24                                           # one fp32 rounding


# ------------------------------------------------------------------------------------------------ confidence
N_CONF = 3
# the issue's shapes (none has hw % 4 == 0: scalar accesses, 26 blocks at 33 x 65) and one that takes the 16-byte path
CONF_SHAPES = [(7, 13), (33, 65), (1, 1), (16, 20)]


def _logits(kind, c, h, w):
    rng = np.random.default_rng(1000 * c + 10 * h + w)
    z = (rng.standard_normal((N_CONF, c, h, w)) * 4.0).astype(np.float32)           # N(0, 4^2)
    if kind == "tie":                                   # classes 1 and 3 share the maximum, exactly, on half the pixels
        top = (z.max(axis=1) + np.float32(1.0)).astype(np.float32)
        where = rng.random((N_CONF, h, w)) < 0.5
        where[0, 0, 0] = True
        z[:, 1] = np.where(where, top, z[:, 1])
        z[:, 3] = np.where(where, top, z[:, 3])
    elif kind == "pm80":
        z = np.where(rng.random(z.shape) < 0.5, np.float32(80.0), np.float32(-80.0)).astype(np.float32)
        z[0, :, 0, 0] = -80.0
        z[0, 0, 0, 0] = 80.0                             # one class at +80, the others 160 below: conf = 1
    return z


def _derived(c):
    """the derived terms of S.conf_bound (subtraction through exp, C - 1 additions, one division), relative to conf"""
    return c * np.exp(-1.0) * U + (c - 1) * U + U


def _check_conf(out, z, what):
    """out (fp32 values of the formula) against float64 with the bound of S.conf_bound through the scheme of
    _ref64.assert_measured: allowed = max(4 x host error, 2^-22) [expf, measured] + the derived terms, all relative to
    the float64 confidence.  Returns (worst err / bound, host error, kernel error, allowed)."""
    c = z.shape[1]
    ref = torch.from_numpy(S.conf64(z))
    host = torch.from_numpy(S.conf32(z))
    worst = R64.assert_measured(out, (ref, ref), host, what, extra=_derived(c))
    host_rel, kernel_rel, allowed = R64.MEASURED[what]
    total, terms = S.conf_bound(c, host_rel)
    assert abs(total - allowed) <= 1e-12 * allowed and set(terms) == {"subtraction", "additions", "division", "expf"}
    return worst, host_rel, kernel_rel, allowed


CONF_CASES = [("normal", c, h, w) for c in (2, 4, 8) for h, w in CONF_SHAPES] + \
             [("tie", 4, 33, 65), ("tie", 4, 16, 20), ("pm80", 4, 33, 65), ("pm80", 4, 16, 20)]


@pytest.mark.parametrize("kind, c, h, w", CONF_CASES, ids=[f"{k}-c{c}-{h}x{w}" for k, c, h, w in CONF_CASES])
def test_confidence_and_labels_against_float64(kind, c, h, w):
    z = _logits(kind, c, h, w)
    zd = torch.from_numpy(z).to(DEV)
    labels, conf = ops.seg_confidence(zd)
    assert labels.dtype == torch.uint8 and conf.dtype == torch.float32
    assert tuple(labels.shape) == (N_CONF, h, w) == tuple(conf.shape)
    want = S.labels64(z)                                # float64 argmax, the first maximum
    assert np.array_equal(labels.cpu().numpy(), want)
    assert torch.equal(labels, per_image_stats(zd, labels=True)["labels"])
    what = f"segconf {kind} c{c} {h}x{w}"
    worst, host_rel, kernel_rel, allowed = _check_conf(conf, z, what)
    print(f"REF64 {what}: host err {host_rel / U:.2f} u, kernel err {kernel_rel / U:.2f} u, allowed {allowed / U:.2f} u "
          f"(derived {_derived(c) / U:.2f} u), worst err / bound {worst:.3f}")
    # either output alone gives the same bytes
    only_l, none_c = ops.seg_confidence(zd, conf=False)
    none_l, only_c = ops.seg_confidence(zd, labels=False)
    assert none_c is None and none_l is None and torch.equal(only_l, labels) and torch.equal(only_c, conf)

    # the checks have teeth: the restatements with the defects named in the docstrings fail them
    if kind == "tie":
        planted = S.labels64(z, last_wins=True)
        assert (want[0, 0, 0], planted[0, 0, 0]) == (1, 3) and not np.array_equal(planted, want)
    if kind == "pm80":
        assert float(conf[0, 0, 0]) == 1.0
        with pytest.raises(AssertionError):
            _check_conf(torch.from_numpy(S.conf32(z, subtract_max=False)), z, what + " (planted: no max subtraction)")


def test_confidence_refuses_unsupported_class_counts():
    for c in (1, 9):
        with pytest.raises(RuntimeError, match="2..8 classes"):
            ops.seg_confidence(torch.zeros((2, c, 8, 8), device=DEV))
    with pytest.raises(ValueError):
        ops.seg_confidence(torch.zeros((2, 3, 8, 8), device=DEV), labels=False, conf=False)


# ------------------------------------------------------------------------------------------------ sheet
C_SHEET = 4
MAP_SPECIALS = [-0.5, 0.0, 1.0, 1.5, np.nan, np.inf, -np.inf, 0.5, 0.999, 3.0 / 256.0]
_inputs_cache = {}


def _sheet_inputs(n, h, w):
    """images with out-of-range and NaN pixels, labels with 0, C - 1 and 255, a map with the special values; computed
    once per shape and shared (never modified)."""
    key = (n, h, w)
    if key not in _inputs_cache:
        rng = np.random.default_rng(n * 10000 + h * 100 + w)
        images = (rng.standard_normal((n, 3, h, w)) * 1.5).astype(np.float32)      # both clamps are hit
        images[0, 0, 0, 0], images[n - 1, 2, h - 1, w - 1], images[0, 1, 1, 1] = np.nan, 1e30, -1e30
        truth = rng.integers(0, C_SHEET, (n, h, w)).astype(np.uint8)
        truth.reshape(n, -1)[:, :3] = (0, C_SHEET - 1, 255)
        pred = rng.integers(0, C_SHEET, (n, h, w)).astype(np.uint8)
        pred.reshape(n, -1)[:, -3:] = (255, 0, C_SHEET - 1)
        amap = rng.random((n, h, w)).astype(np.float32)
        amap.reshape(n, -1)[:, :len(MAP_SPECIALS)] = np.array(MAP_SPECIALS, np.float32)
        host = {"images": images, "truth": truth, "pred": pred, "map": amap}
        _inputs_cache[key] = (host, {k: torch.from_numpy(v).to(DEV) for k, v in host.items()})
    return _inputs_cache[key]


def _columns(t, names, alpha=0.4):
    make = {"image": lambda: ("image",), "classes": lambda: ("classes", t["truth"]),
            "classes_pred": lambda: ("classes", t["pred"]), "overlay": lambda: ("overlay", t["pred"], alpha),
            "overlay_truth": lambda: ("overlay", t["truth"], alpha), "lut": lambda: ("lut", t["map"])}
    return [make[k]() for k in names]


FOUR = ("image", "classes", "overlay", "lut")
PALETTE = S.class_palette(C_SHEET, "scaled")
VIRIDIS = S.viridis_lut()


def _both(n, h, w, names, gutter, per_row, alpha=0.4):
    host, dev = _sheet_inputs(n, h, w)
    got = ops.render_seg_sheet(dev["images"], _columns(dev, names, alpha), gutter=gutter, per_row=per_row,
                               palette=torch.from_numpy(PALETTE), lut=torch.from_numpy(VIRIDIS))
    want = S.render_seg_sheet(host["images"], _columns(host, names, alpha), gutter=gutter, per_row=per_row,
                              palette=PALETTE, lut=VIRIDIS)
    return got, want


@pytest.mark.parametrize("per_row", [1, 2, 5])
@pytest.mark.parametrize("gutter", [0, 4])
@pytest.mark.parametrize("h, w", [(5, 7), (16, 16), (9, 34)])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_sheet_bytes_equal_restatement(n, h, w, gutter, per_row):
    got, want = _both(n, h, w, FOUR, gutter, per_row)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape == S.sheet_shape(n, 4, h, w, gutter, per_row)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("h, w", [(16, 16), (9, 34)])
@pytest.mark.parametrize("names", [("image",), ("classes",), ("overlay",), ("lut",), FOUR + ("classes_pred", "overlay_truth",
                                                                                               "lut", "image")],
                         ids=["image", "classes", "overlay", "lut", "k8"])
def test_each_panel_kind_alone_and_eight_panels(names, h, w):
    got, want = _both(3, h, w, names, 4, 2)
    assert tuple(got.shape) == S.sheet_shape(3, len(names), h, w, 4, 2)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("alpha", [0.0, 0.4, 1.0])
def test_overlay_alphas(alpha):
    for h, w in ((16, 16), (5, 7)):
        got, want = _both(3, h, w, ("overlay", "overlay_truth"), 4, 1, alpha)
        assert np.array_equal(got.cpu().numpy(), want)
        if alpha == 0.0:
            image, _ = _both(3, h, w, ("image", "image"), 4, 1)
            assert torch.equal(got, image)


def test_planted_pixels_draw_what_the_rules_say():
    host, dev = _sheet_inputs(3, 9, 34)
    got = ops.render_seg_sheet(dev["images"], _columns(dev, FOUR), gutter=0, palette=torch.from_numpy(PALETTE),
                               lut=torch.from_numpy(VIRIDIS)).cpu().numpy()
    w = 34
    assert got[0, 0, 0] == 0                                                         # a NaN channel draws 0
    assert got[1, 1, 1] == 0 and got[-1, w - 1, 2] == 255                            # -1e30 and 1e30 clamp
    assert got[0, w + 0].tolist() == PALETTE[0].tolist() and got[0, w + 1].tolist() == PALETTE[C_SHEET - 1].tolist()
    assert got[0, w + 2].tolist() == [255, 255, 255]                                 # label 255: white
    lut_row = got[0, 3 * w:3 * w + len(MAP_SPECIALS)]
    for x, i in ((0, 0), (1, 0), (2, 255), (3, 255), (7, 128), (8, 255), (9, 3)):
        assert lut_row[x].tolist() == VIRIDIS[i].tolist(), x
    assert (lut_row[4:7] == 255).all()                                               # NaN, +inf, -inf: white


def test_int64_masks_are_converted():
    host, dev = _sheet_inputs(3, 9, 34)
    mask = host["truth"].astype(np.int64)
    mask.reshape(3, -1)[:, 5:9] = (-1, 256, 300, 255)
    got = ops.render_seg_sheet(dev["images"], [("classes", torch.from_numpy(mask).to(DEV)),
                                               ("overlay", torch.from_numpy(mask).to(DEV), 0.4)],
                               palette=torch.from_numpy(PALETTE))
    want = S.render_seg_sheet(host["images"], [("classes", mask), ("overlay", mask, 0.4)], palette=PALETTE)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want[0, 5:9] == 255).all()


def test_default_tables_are_the_index_palette_and_viridis():
    host, dev = _sheet_inputs(3, 16, 16)
    got = ops.render_seg_sheet(dev["images"], _columns(dev, FOUR))
    want = S.render_seg_sheet(host["images"], _columns(host, FOUR), palette=S.class_palette(10, "index"), lut=S.viridis_lut())
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("h, w, gutter", [(16, 16, 4), (9, 34, 4), (5, 7, 0)])
def test_image_panel_equals_the_mvtec_sheet(h, w, gutter):
    _, dev = _sheet_inputs(3, h, w)
    ours = ops.render_seg_sheet(dev["images"], [("image",)], gutter=gutter)
    theirs = ops.render_sheet([("image", dev["images"])], gutter=gutter)
    assert torch.equal(ours, theirs)


def test_non_default_stream():
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        got, want = _both(5, 9, 34, FOUR, 4, 2)
        z = _logits("normal", 4, 33, 65)
        labels, conf = ops.seg_confidence(torch.from_numpy(z).to(DEV))
    stream.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(labels.cpu().numpy(), S.labels64(z))
    _check_conf(conf, z, "segconf on a side stream")


MARGIN = 256
SENTINEL = 0xA5


@pytest.mark.parametrize("n, h, w, gutter, per_row", [(5, 9, 34, 4, 2), (3, 5, 7, 0, 2), (3, 16, 16, 4, 5)])
def test_every_sheet_byte_is_written_and_nothing_beyond(n, h, w, gutter, per_row):
    host, dev = _sheet_inputs(n, h, w)
    rows, cols, _ = S.sheet_shape(n, 4, h, w, gutter, per_row)
    nbytes = rows * cols * 3
    buf = torch.full((nbytes + 2 * MARGIN,), SENTINEL, dtype=torch.uint8, device=DEV)
    descs = (L.SegPanel * 4)(L.SegPanel(L.SEG_PANEL_IMAGE, 0, None, None),
                             L.SegPanel(L.SEG_PANEL_CLASSES, 0, dev["truth"].data_ptr(), None),
                             L.SegPanel(L.SEG_PANEL_OVERLAY, 102, dev["pred"].data_ptr(), None),
                             L.SegPanel(L.SEG_PANEL_LUT, 0, None, dev["map"].data_ptr()))
    pal, lut = torch.from_numpy(PALETTE).to(DEV), torch.from_numpy(VIRIDIS).to(DEV)
    mean, std = (ctypes.c_float * 3)(*ops.IMAGENET_MEAN), (ctypes.c_float * 3)(*ops.IMAGENET_STD)
    L.check(L.lib().unet_seg_render_sheet(ctypes.c_void_p(dev["images"].data_ptr()), descs, 4, n, h, w, gutter, per_row,
                                          mean, std, ctypes.c_void_p(pal.data_ptr()), ctypes.c_void_p(lut.data_ptr()),
                                          ctypes.c_void_p(buf.data_ptr() + MARGIN), None), "unet_seg_render_sheet")
    torch.cuda.synchronize()
    assert bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[-MARGIN:] == SENTINEL).all())
    want = S.render_seg_sheet(host["images"], _columns(host, FOUR), gutter=gutter, per_row=per_row, palette=PALETTE,
                              lut=VIRIDIS)
    assert np.array_equal(buf[MARGIN:-MARGIN].cpu().numpy().reshape(rows, cols, 3), want)


# ------------------------------------------------------------------------------------------------ CLIs
def _fresh_checkpoint(path, n_classes, seed):
    from tiaozhanbei_unet_amd import SegmentationUNet
    from tiaozhanbei_unet_amd.train_utils import get_optimizer
    from tiaozhanbei_unet_amd.utils import save_checkpoint
    torch.manual_seed(seed)
    model = SegmentationUNet(3, n_classes, precision="fp32").to(DEV)
    save_checkpoint(model, get_optimizer(model), 0, 0.0, str(path))
    return model


def _recompute(model, batches, num_samples):
    """what the CLI holds after its pass, computed here from the same checkpoint and batches"""
    model.eval()
    keep = {k: [] for k in ("images", "masks", "labels", "conf", "confusion", "mean", "std")}
    with torch.no_grad():
        for x, m in batches:
            out = model(x)
            labels, conf = ops.seg_confidence(out)
            st = per_image_stats(out, m)
            for k, t in zip(keep, (x, m, labels, conf, st["confusion"], st["conf_mean"], st["conf_std"])):
                keep[k].append(t)
    return {k: torch.cat(v)[:num_samples] for k, v in keep.items()}


def _png(path):
    from PIL import Image
    return np.array(Image.open(path).convert("RGB"))


def _check_json(save, paths, got, class_names, mode, panels, grid):
    vis = json.load(open(save / "visualizations.json"))
    n = len(paths)
    assert [c["name"] for c in vis["classes"]] == class_names
    assert [c["rgb"] for c in vis["classes"]] == S.class_palette(len(class_names), mode)[:len(class_names)].tolist()
    assert vis["panels"] == panels and vis["grid"] == grid and len(vis["samples"]) == n
    for i, e in enumerate(vis["samples"]):
        assert os.path.basename(e["image_path"]) == os.path.basename(paths[i])
        want = image_prediction_stats(got["confusion"][i], float(got["mean"][i]), float(got["std"][i]), class_names)
        assert e["stats"] == want
    dist = json.load(open(save / "class_distribution.json"))
    pixels = n * got["labels"].shape[1] * got["labels"].shape[2]
    assert dist["class_names"] == class_names and dist["samples"] == n
    assert sum(dist["ground_truth"]) == pixels and sum(dist["prediction"]) == pixels
    total = got["confusion"].sum(0).cpu().numpy()
    assert dist["ground_truth"] == total.sum(1).tolist() and dist["prediction"] == total.sum(0).tolist()
    return vis


def test_visualize_gear_cli_round_trip(tmp_path):
    from tiaozhanbei_unet_amd import gear_dataset as G
    from tiaozhanbei_unet_amd import visualize_gear
    size, seed, num_samples, bs = 64, 42, 4, 3
    root = G.write_synthetic_gear(str(tmp_path / "gear"), seed=seed)         # the tree --synthetic writes, again
    ckpt = tmp_path / "run" / "model.pth"
    os.makedirs(ckpt.parent)
    model = _fresh_checkpoint(ckpt, 4, seed=1)
    visualize_gear.main(["--checkpoint", str(ckpt), "--synthetic", "--seed", str(seed), "--image_size", str(size),
                         "--batch_size", str(bs), "--num_workers", "0", "--num_samples", str(num_samples),
                         "--grid_size", "1", "3"])
    save = ckpt.parent / "visualizations"                                    # the default: beside the checkpoint

    ds = G.GearDataset(root, "test", (size, size), raw=True)
    pre = G.GearPreprocess((size, size), train=False)
    samples = [ds[i] for i in range(len(ds))]
    batches = []
    for i in range(0, len(samples), bs):
        images, polys, sizes, _ = G.collate_raw(samples[i:i + bs])
        batches.append(pre(images, polys, sizes, device=DEV))
    got = _recompute(model, batches, num_samples)
    n = min(num_samples, len(ds))
    names = ["background"] + ds.class_names
    palette = ops.class_palette(4, "index")
    panels = ["overlay_truth", "overlay_prediction"]
    vis = _check_json(save, ds.image_paths[:n], got, names, "index", {"individual": panels, "grid": panels},
                      {"file": "predictions_grid.png", "grid_size": [1, 3], "samples": 3})
    for i, e in enumerate(vis["samples"]):
        assert e["file"] == f"prediction_{i:03d}_{os.path.basename(ds.image_paths[i]).split('.')[0]}.png"
        want = ops.render_seg_sheet(got["images"][i:i + 1], [("overlay", got["masks"][i:i + 1], 0.4),
                                                             ("overlay", got["labels"][i:i + 1], 0.4)], palette=palette)
        assert np.array_equal(_png(save / e["file"]), want.cpu().numpy())
    grid = ops.render_seg_sheet(got["images"][:3], [("overlay", got["masks"][:3], 0.4), ("overlay", got["labels"][:3], 0.4)],
                                per_row=3, palette=palette)
    assert np.array_equal(_png(save / "predictions_grid.png"), grid.cpu().numpy())
    assert len(glob.glob(str(save / "prediction_*.png"))) == n and glob.glob(str(save / "visualization_*.log"))


def test_visualize_kolektorsdd_cli_round_trip(tmp_path):
    from tiaozhanbei_unet_amd import kolektorsdd_dataset as K
    from tiaozhanbei_unet_amd import visualize_kolektorsdd
    (h, w), seed, num_samples, bs = (96, 48), 42, 3, 2
    root = K.write_synthetic_kolektorsdd(str(tmp_path / "kol"), seed=seed)   # the tree --synthetic writes, again
    ckpt = tmp_path / "model.pth"
    model = _fresh_checkpoint(ckpt, 3, seed=2)
    save = tmp_path / "vis"
    visualize_kolektorsdd.main(["--checkpoint", str(ckpt), "--synthetic", "--seed", str(seed), "--image_height", str(h),
                                "--image_width", str(w), "--batch_size", str(bs), "--num_workers", "0", "--num_samples",
                                str(num_samples), "--grid_size", "2", "2", "--save_individual", "--save_grid",
                                "--show_confidence", "--save_dir", str(save)])

    ds = K.KolektorSDDDataset(root, "test", (h, w), raw=True)
    assert len(ds) >= num_samples
    pre = K.GpuPreprocess((h, w), train=False)
    samples = [ds[i] for i in range(len(ds))]
    batches = [pre(*K.collate_raw(samples[i:i + bs])[:2], device=DEV) for i in range(0, len(samples), bs)]
    got = _recompute(model, batches, num_samples)
    palette = ops.class_palette(3, "scaled")
    vis = _check_json(save, ds.image_paths[:num_samples], got, K.CLASS_NAMES, "scaled",
                      {"individual": ["image", "truth", "prediction", "confidence"], "grid": ["image", "truth", "prediction"]},
                      {"file": "predictions_grid.png", "grid_size": [2, 2], "samples": 3})
    for i, e in enumerate(vis["samples"]):
        assert e["file"] == f"prediction_{i:03d}_{os.path.basename(ds.image_paths[i]).split('.')[0]}.png"
        want = ops.render_seg_sheet(got["images"][i:i + 1], [("image",), ("classes", got["masks"][i:i + 1]),
                                                             ("classes", got["labels"][i:i + 1]),
                                                             ("lut", got["conf"][i:i + 1])], palette=palette)
        assert np.array_equal(_png(save / e["file"]), want.cpu().numpy())
    grid = ops.render_seg_sheet(got["images"], [("image",), ("classes", got["masks"]), ("classes", got["labels"])],
                                per_row=2, palette=palette)
    assert tuple(grid.shape) == S.sheet_shape(3, 3, h, w, 4, 2)
    assert np.array_equal(_png(save / "predictions_grid.png"), grid.cpu().numpy())
