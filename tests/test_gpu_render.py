"""The visualisation sheet on the device (ops.render_sheet / ops.panel_range -> csrc/render.hip) against the numpy
restatement of tests/_render_ref.py (pinned to matplotlib by test_cpu_render.py), byte for byte: odd sizes and widths
that are no multiple of the 4-pixel run (tails, unaligned rows), the vectorised path, all five panel kinds in one sheet,
the CLI's default shape, special planes, determinism, input forms, refusals, and the evaluation CLI's files."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _render_ref as R

pytestmark = pytest.mark.gpu


def _ops():
    from tiaozhanbei_unet_amd import ops
    return ops


def _inputs(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return {"image": (rng.standard_normal((n, 3, h, w)) * 1.5).astype(np.float32),     # N(0, 1.5): both clamps are hit
            "mask": (rng.random((n, 1, h, w)) > 0.7).astype(np.float32),
            "amap": rng.random((n, 1, h, w)).astype(np.float32) ** 3,
            "recon": (rng.standard_normal((n, 3, h, w)) * 0.5 + 0.5).astype(np.float32)}


def _columns(x, kinds, alpha=0.4):
    make = {"image": lambda: ("image", x["image"]), "gray": lambda: ("gray", x["mask"]),
            "hot": lambda: ("hot", x["amap"]), "unit": lambda: ("unit", x["recon"]),
            "overlay": lambda: ("overlay", x["image"], x["amap"], alpha)}
    return [make[k]() for k in kinds]


def _to_device(columns):
    return [tuple(torch.as_tensor(v).cuda() if isinstance(v, np.ndarray) else v for v in c) for c in columns]


FOUR = ("image", "gray", "hot", "unit")
ALL = ("image", "gray", "hot", "unit", "overlay")
CASES = {"3x5x7": (3, 5, 7, 4, FOUR), "1x1x1": (1, 1, 1, 4, FOUR), "2x64x96": (2, 64, 96, 4, FOUR),
         "4x33x130_g1_all_kinds": (4, 33, 130, 1, ALL), "20x256x256_cli_default": (20, 256, 256, 4, FOUR)}
_cache = {}


def _case(name):
    """(columns on the host, gutter, expected sheet): computed once per case."""
    if name not in _cache:
        n, h, w, g, kinds = CASES[name]
        cols = _columns(_inputs(n, h, w, seed=len(name) + n * h), kinds)
        _cache[name] = (cols, g, R.render_sheet(cols, gutter=g))
    return _cache[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_sheet_equals_reference(name):
    cols, g, want = _case(name)
    got = _ops().render_sheet(_to_device(cols), gutter=g)
    assert got.dtype == torch.uint8 and got.is_cuda and got.is_contiguous() and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("name", sorted(CASES))
def test_panel_range_equals_reference(name):
    cols, _, _ = _case(name)
    amap = dict((c[0], c[1]) for c in cols)["hot"]
    got = _ops().panel_range(torch.as_tensor(amap).cuda())
    assert got.dtype == torch.float32 and tuple(got.shape) == (amap.shape[0], 2)
    assert np.array_equal(got.cpu().numpy(), R.panel_range(amap))


def _special_planes():
    rng = np.random.default_rng(21)
    h, w = 19, 27
    base = rng.standard_normal((h, w)).astype(np.float32)
    bad = base.copy()
    bad[0, 0], bad[3, 5], bad[7, 7], bad[h - 1, w - 1] = np.nan, np.inf, -np.inf, np.nan
    ends = base.copy()
    ends[0, 0], ends[h - 1, w - 1] = 9.0, -9.0                         # the maximum first, the minimum last
    lo, hi = np.float64(np.float32(0.1)), np.float64(np.float32(0.7))
    border = np.resize((lo + np.arange(257) * (hi - lo) / 256).astype(np.float32), (h, w))
    exact = np.resize((-1.25 + np.arange(257) * (4.75 / 256)).astype(np.float32), (h, w))   # dyadic: exactly on the borders
    return np.stack([base, np.full((h, w), 0.3, np.float32), border, exact, bad, np.full((h, w), np.nan, np.float32),
                     ends, np.full((h, w), -0.0, np.float32)])[:, None]


@pytest.mark.parametrize("kind", ["gray", "hot", "overlay"])
def test_special_planes(kind):
    planes = _special_planes()
    n = planes.shape[0]
    image = _inputs(n, planes.shape[2], planes.shape[3], 22)["image"]
    cols = [("overlay", image, planes, 0.5)] if kind == "overlay" else [(kind, planes)]
    got = _ops().render_sheet(_to_device(cols), gutter=3).cpu().numpy()
    assert np.array_equal(got, R.render_sheet(cols, gutter=3))
    h = planes.shape[2]
    if kind != "overlay":
        const = got[1 * (h + 3):1 * (h + 3) + h]
        assert (const == ((10, 0, 0) if kind == "hot" else (0, 0, 0))).all()       # hi == lo: LUT[0]
        assert (got[5 * (h + 3):5 * (h + 3) + h] == 255).all()                      # no finite pixel
    rng_got = _ops().panel_range(torch.as_tensor(planes).cuda()).cpu().numpy()
    want = R.panel_range(planes)
    assert np.array_equal(rng_got, want, equal_nan=True)
    assert np.isnan(rng_got[5]).all() and tuple(rng_got[6]) == (-9.0, 9.0) and tuple(rng_got[7]) == (0.0, 0.0)


def test_repeated_calls_are_identical():
    cols, g, _ = _case("4x33x130_g1_all_kinds")
    dev = _to_device(cols)
    a = _ops().render_sheet(dev, gutter=g)
    b = _ops().render_sheet(dev, gutter=g)
    assert torch.equal(a, b)
    amap = dev[2][1]
    assert torch.equal(_ops().panel_range(amap), _ops().panel_range(amap))


def test_render_does_not_synchronise():
    cols, g, want = _case("3x5x7")
    dev = _to_device(cols)
    _ops().render_sheet(dev, gutter=g)                                 # (the first call on a device uploads the tables)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _ops().render_sheet(dev, gutter=g)
        rng = _ops().panel_range(dev[2][1])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert np.array_equal(got.cpu().numpy(), want) and rng.shape == (3, 2)


def test_bf16_and_non_contiguous_inputs():
    x = _inputs(2, 12, 20, 31)
    dev = {k: torch.as_tensor(v).cuda() for k, v in x.items()}
    half = {k: v.to(torch.bfloat16) for k, v in dev.items()}
    ops = _ops()
    want = ops.render_sheet(_columns({k: v.float() for k, v in half.items()}, ALL))
    assert torch.equal(ops.render_sheet(_columns(half, ALL)), want)
    assert np.array_equal(want.cpu().numpy(), R.render_sheet(_columns({k: v.float().cpu().numpy() for k, v in half.items()}, ALL)))
    strided = {k: torch.as_tensor(np.ascontiguousarray(v.transpose(0, 1, 3, 2))).cuda().permute(0, 1, 3, 2)
               for k, v in x.items()}
    assert not strided["image"].is_contiguous()
    assert torch.equal(ops.render_sheet(_columns(strided, ALL)), ops.render_sheet(_columns(dev, ALL)))
    planes = dev["amap"][:, 0]                                          # (N, H, W) maps are taken too
    assert torch.equal(ops.render_sheet([("hot", planes)]), ops.render_sheet([("hot", dev["amap"])]))


def test_custom_mean_std_and_gutter_zero():
    x = _inputs(2, 6, 9, 41)
    mean, std = (0.5, 0.25, 0.125), (0.3, 0.2, 0.1)
    cols = _columns(x, ("image", "hot"))
    got = _ops().render_sheet(_to_device(cols), gutter=0, mean=mean, std=std)
    assert np.array_equal(got.cpu().numpy(), R.render_sheet(cols, gutter=0, mean=mean, std=std))


def test_refusals():
    ops = _ops()
    x = {k: torch.as_tensor(v).cuda() for k, v in _inputs(2, 6, 8, 51).items()}
    with pytest.raises(ValueError):
        ops.render_sheet([("image", x["image"]), ("hot", x["amap"][:, :, :5])])            # H differs
    with pytest.raises(ValueError):
        ops.render_sheet([("image", x["image"]), ("hot", x["amap"][:1])])                  # N differs
    with pytest.raises(ValueError):
        ops.render_sheet([("image", x["amap"])])                                           # one channel where three belong
    with pytest.raises(ValueError):
        ops.render_sheet([("hot", x["image"])])                                            # three where one belongs
    with pytest.raises(ValueError):
        ops.render_sheet([("hot", x["amap"])] * 9)                                         # K = 9
    with pytest.raises(ValueError):
        ops.render_sheet([])
    with pytest.raises(ValueError):
        ops.render_sheet([("overlay", x["image"], x["amap"], 1.5)])
    with pytest.raises(ValueError):
        ops.render_sheet([("viridis", x["amap"])])
    with pytest.raises(ValueError):
        ops.render_sheet([("hot", x["amap"])], gutter=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_sheet([("image", x["image"].cpu())])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.panel_range(x["amap"].cpu())


def test_c_abi_status_codes():
    """K > 8 and a sheet of 2^31 bytes or more are refused with UNET_ERR_UNSUPPORTED before anything is launched."""
    from tiaozhanbei_unet_amd import _lib as L
    lib = L.lib()
    amap = torch.zeros((1, 1, 4, 4), device="cuda")
    keys = torch.zeros(2 * 9, dtype=torch.int32, device="cuda")
    luts = torch.zeros((2, 256, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros(16 * 9 * 3 + 64, dtype=torch.uint8, device="cuda")
    descs = (L.Panel * 9)(*[L.Panel(L.PANEL_HOT, 0, None, amap.data_ptr()) for _ in range(9)])
    mean, std = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.unet_render_range(descs, 9, 1, 4, 4, p(keys), None) == -2
    assert lib.unet_render_sheet(descs, 9, 1, 4, 4, 0, mean, std, p(keys), p(luts), p(out), None) == -2
    assert b"at most 8" in lib.unet_last_error()
    # 32768 x 21846 x 3 = 2^31 + 65536 bytes
    assert lib.unet_render_sheet(descs, 1, 1, 32768, 21846, 0, mean, std, p(keys), p(luts), p(out), None) == -2
    assert lib.unet_render_sheet(descs, 1, 1, 4, 4, -1, mean, std, p(keys), p(luts), p(out), None) == -1
    bad = (L.Panel * 1)(L.Panel(L.PANEL_IMAGE, 0, None, amap.data_ptr()))                  # an image panel without rgb
    assert lib.unet_render_range(bad, 1, 1, 4, 4, p(keys), None) == -1
    torch.cuda.synchronize()


def _cli_tree(tmp_path, model_name):
    from tiaozhanbei_unet_amd import AnomalyUNet, UNet
    from tiaozhanbei_unet_amd.dataset import write_synthetic_mvtec
    from tiaozhanbei_unet_amd.utils import save_checkpoint
    root = write_synthetic_mvtec(str(tmp_path / "data"), "bottle", n_train=2, n_good=3, n_bad=4, size=64)
    torch.manual_seed(0)
    model = (AnomalyUNet(3, False) if model_name == "anomaly_unet" else UNet(3, 1, False)).cuda()
    ck = str(tmp_path / "model.pth")
    save_checkpoint(model, torch.optim.Adam(model.parameters()), 0, 0.0, ck)
    argv = ["--data_root", root, "--category", "bottle", "--model", model_name, "--checkpoint", ck, "--batch_size", "3",
            "--image_size", "64", "--num_workers", "0", "--output_dir", str(tmp_path / "test_out")]
    return root, model, ck, argv


@pytest.mark.parametrize("model_name,overlay", [("anomaly_unet", None), ("unet", None), ("anomaly_unet", 0.5)])
def test_cli_writes_the_sheet(tmp_path, model_name, overlay):
    """test.main --save_visualizations: visualizations.png decodes to the sheet of the samples visualizations.json names,
    rendered by the reference restatement from a second test_model pass."""
    from PIL import Image
    from tiaozhanbei_unet_amd import test as test_cli
    from tiaozhanbei_unet_amd.dataset import get_dataloaders
    from tiaozhanbei_unet_amd.utils import load_checkpoint
    root, model, ck, argv = _cli_tree(tmp_path, model_name)
    np.random.seed(5)
    extra = [] if overlay is None else ["--vis_overlay_alpha", str(overlay)]
    out = test_cli.main(argv + ["--save_visualizations", "--max_vis_samples", "3"] + extra)
    k = (4 if model_name == "anomaly_unet" else 3) + (overlay is not None)
    png = np.asarray(Image.open(os.path.join(out, "visualizations.png")))
    assert png.dtype == np.uint8 and png.shape == (3 * 64 + 2 * 4, k * 64 + (k - 1) * 4, 3)
    side = json.load(open(os.path.join(out, "visualizations.json")))
    names = ["original", "mask_true", "anomaly_map"] + (["reconstruction"] if model_name == "anomaly_unet" else []) \
        + (["overlay"] if overlay is not None else [])
    assert side["columns"] == names and side["gutter"] == 4 and len(side["rows"]) == 3
    assert len({r["index"] for r in side["rows"]}) == 3

    _, loader = get_dataloaders(root, "bottle", 3, 64, 0, device_preprocess=True)
    load_checkpoint(model, None, ck, torch.device("cuda"))
    res = test_cli.test_model(model, loader, torch.device("cuda"), pixel_thresholds=[0.3, 0.5, 0.7])
    idx = [r["index"] for r in side["rows"]]
    detail = json.load(open(os.path.join(out, "detailed_results.json")))
    for r in side["rows"]:
        i = r["index"]
        assert r["image_path"] == res["image_paths"][i] == detail["image_paths"][i]
        assert r["label"] == int(res["labels"][i]) and r["anomaly_type"] == res["anomaly_types"][i]
        assert r["prediction"] == detail["predictions"][i] and r["image_score"] == detail["anomaly_scores"][i]
    images = np.stack([res["images"][i].numpy() for i in idx])
    amaps = np.stack([res["anomaly_maps"][i] for i in idx])
    cols = [("image", images), ("gray", np.stack([res["masks_true"][i] for i in idx])), ("hot", amaps)]
    if model_name == "anomaly_unet":
        cols.append(("unit", np.stack([res["reconstructions"][i].float().numpy() for i in idx])))
    if overlay is not None:
        cols.append(("overlay", images, amaps, overlay))
    assert np.array_equal(png, R.render_sheet(cols, gutter=4))


def test_cli_without_the_flag_writes_neither_file(tmp_path):
    from tiaozhanbei_unet_amd import test as test_cli
    _, _, _, argv = _cli_tree(tmp_path, "unet")
    out = test_cli.main(argv + ["--max_vis_samples", "3", "--vis_overlay_alpha", "0.5"])
    assert os.path.exists(os.path.join(out, "test_metrics.json"))
    assert not os.path.exists(os.path.join(out, "visualizations.png"))
    assert not os.path.exists(os.path.join(out, "visualizations.json"))
