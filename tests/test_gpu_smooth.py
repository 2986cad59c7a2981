"""The map-smoothing kernel (csrc/smooth.hip: unet_smooth_maps, evaluation.GaussianSmoother) against the float64
restatement tests/_smooth_ref.py, element by element within its derived bound (2K + 2) u A, its per-image maximum
against the smoothed map's own amax bit for bit, and test.py's --map_sigma / --image_score round trip."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import _smooth_ref as R
from _rank_auc_ref import rank_auc64

pytestmark = pytest.mark.gpu

SIGMA_OF = {0: 0.0, 1: 0.25, 6: 1.5, 16: 4.0, 32: 8.0}          # radius -> sigma at truncate 4


def _smoother(radius):
    from tiaozhanbei_unet_amd.evaluation import GaussianSmoother
    s = GaussianSmoother(SIGMA_OF[radius])
    assert s.radius == radius
    return s


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _check(x, radius, out, peak, what=""):
    """out [n, h, w] against the restatement of x (both host fp32 tensors / device results), peak against out.amax."""
    taps = _smoother(radius).taps
    xs = x.detach().float().cpu().numpy().reshape(out.shape)
    got = out.detach().cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        want, bnd = R.smooth64(xs, taps), R.bound(xs, taps)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what          # +-inf where it is
    err = np.abs(got[fin] - want[fin])
    ratio = float((err / np.maximum(bnd[fin], 1e-300)).max()) if err.size and float(err.max()) > 0 else 0.0
    print(f"smooth {what} {tuple(out.shape)} r={radius}: max err {float(err.max()) if err.size else 0:.3e}, err / bound <= {ratio:.3f}")
    assert np.all(err <= bnd[fin]), what
    if peak is not None:
        amax = out.reshape(out.shape[0], -1).amax(1)
        nan = torch.isnan(amax).cpu()
        assert torch.equal(torch.isnan(peak).cpu(), nan), what
        assert torch.equal(_bits(peak)[~nan], _bits(amax)[~nan]), what


def _run(x, radius):
    out, peak = _smoother(radius)(x.cuda())
    assert out.dtype == torch.float32 and out.shape == x.shape and peak.shape == (x.shape[0],) and peak.dtype == torch.float32
    return out, peak


def _raw(src, dst, n, h, w, radius, image_max):
    """The C-ABI itself, on the current stream."""
    from tiaozhanbei_unet_amd import _lib
    s = _smoother(radius)
    _lib.check(_lib.lib().unet_smooth_maps(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), n, h, w, s._host, radius,
                                           C.c_void_p(image_max.data_ptr() if image_max is not None else 0),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "unet_smooth_maps")


# The kernel's tile is 32 rows x 64 columns.  (2, 69, 135) and (2, 69, 136): three tiles in each axis with ragged last
# tiles, on the scalar path (135 % 4 != 0) and the 16-byte path; (2, 37, 53): one ragged tile; (1, 3, 200) at radius 32:
# eleven folds of the 3 rows; (1, 1, 1) and (1, 5, 7) at radius 16: sides far below the radius; (3, 33, 66): w % 4 == 2.
CASES = [((1, 1, 1), 16), ((1, 5, 7), 16), ((2, 37, 53), 16), ((2, 69, 135), 16), ((2, 69, 136), 16), ((1, 3, 200), 32),
         ((2, 64, 64), 0), ((2, 64, 64), 1), ((2, 64, 64), 32), ((3, 33, 66), 6), ((4, 256, 256), 16), ((1, 1408, 512), 16)]


@pytest.mark.parametrize("shape, radius", CASES, ids=[f"{'x'.join(map(str, s))}-r{r}" for s, r in CASES])
def test_smoothed_map_and_peak(shape, radius):
    g = torch.Generator().manual_seed(shape[1] * 1000 + shape[2] + radius)
    x = torch.randn(shape, generator=g)
    out, peak = _run(x, radius)
    _check(x, radius, out, peak)
    if radius == 0:
        assert torch.equal(_bits(out), _bits(x))               # a bit-exact copy
        assert torch.equal(_bits(peak), _bits(x.reshape(shape[0], -1).amax(1)))
    out2, peak2 = _run(x, radius)                             # the same bits in every run
    assert torch.equal(_bits(out2), _bits(out)) and torch.equal(_bits(peak2), _bits(peak))


def test_unaligned_source_and_raw_calls():
    """src one float past a 16-byte boundary (the scalar path at a width that is a multiple of 4), image_max prefilled
    with +inf and with NaN, and image_max = NULL, through the C-ABI."""
    n, h, w, radius = 2, 37, 72, 16
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n * h * w + 1, generator=g).cuda()
    src = x[1:]
    assert src.data_ptr() % 16 == 4
    outs = []
    for fill in (float("inf"), float("nan"), None):
        dst = torch.empty((n, h, w), device="cuda")
        peak = None if fill is None else torch.full((n,), fill, device="cuda")
        _raw(src, dst, n, h, w, radius, peak)
        _check(src.reshape(n, h, w), radius, dst, peak, f"prefill {fill}")
        outs.append(dst)
    aligned, peak = _run(src.reshape(n, h, w).clone(), radius)      # the 16-byte path computes the same bits
    for o in outs:
        assert torch.equal(_bits(o), _bits(aligned))


def test_peak_in_corners_and_on_tile_seams():
    h, w, radius = 69, 136, 16
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (31, 63), (32, 64), (31, 64), (32, 63), (40, 127), (68, 64)]
    g = torch.Generator().manual_seed(11)
    x = torch.rand((len(spots), h, w), generator=g) - 1.0
    for i, (y, xx) in enumerate(spots):
        x[i, y, xx] = 1000.0
    out, peak = _run(x, radius)
    _check(x, radius, out, peak)
    where = out.reshape(len(spots), -1).argmax(1).cpu()
    assert [(int(p) // w, int(p) % w) for p in where] == spots
    assert bool((peak > 0).all())


def test_negative_zero_infinite_and_nan_planes():
    n, h, w, radius = 6, 40, 70, 6
    g = torch.Generator().manual_seed(5)
    x = torch.randn((n, h, w), generator=g)
    x[0] = -x[0].abs() - 0.5                                  # all negative: the peak is below zero
    x[1] = -0.0
    x[2, 33, 65] = float("inf")
    x[3, 2, 3] = float("nan")
    x[4, 39, 0] = float("-inf")
    out, peak = _run(x, radius)
    _check(x, radius, out, peak)
    peak = peak.cpu()
    assert float(peak[0]) < 0 and float(peak[1]) == 0.0
    assert bool((out[1] == 0).all())
    assert float(peak[2]) == float("inf") and bool(torch.isnan(peak[3])) and bool(torch.isfinite(peak[[0, 1, 4, 5]]).all())
    assert int(torch.isnan(out[3]).sum()) == (2 + radius + 1) * (3 + radius + 1) and not bool(torch.isnan(out[[0, 1, 2, 4, 5]]).any())
    clean = x.clone()
    clean[2, 33, 65] = 0.0; clean[3, 2, 3] = 0.0; clean[4, 39, 0] = 0.0
    out_c, peak_c = _run(clean, radius)
    for i in (0, 1, 5):                                       # the other planes do not notice
        assert torch.equal(_bits(out[i]), _bits(out_c[i])) and torch.equal(_bits(peak[i]), _bits(peak_c[i]))


@pytest.mark.parametrize("radius", [0, 1, 16, 32])
def test_constant_planes(radius):
    values = [1.0, -3.7, 1e-3, 123456.789]
    x = torch.tensor(values).reshape(-1, 1, 1).expand(-1, 45, 77).contiguous()
    out, peak = _run(x, radius)
    k = 2 * radius + 1
    for i, c in enumerate(values):
        c32 = float(np.float32(c))
        dev = float((out[i].double() - c32).abs().max())
        print(f"constant {c32} r={radius}: max deviation {dev / (R.U * abs(c32)):.2f} u |c| (allowed {k})")
        assert dev <= k * R.U * abs(c32)
    assert torch.equal(_bits(peak), _bits(out.reshape(len(values), -1).amax(1)))


def test_smoother_takes_nchw_bf16_and_strided_maps():
    g = torch.Generator().manual_seed(9)
    x = torch.randn((3, 1, 41, 68), generator=g)
    out, peak = _run(x, 6)
    _check(x, 6, out.reshape(3, 41, 68), peak, "nchw")
    xb = x.to(torch.bfloat16)
    out_b, peak_b = _smoother(6)(xb.cuda())
    assert out_b.dtype == torch.float32 and out_b.shape == xb.shape
    _check(xb.float(), 6, out_b.reshape(3, 41, 68), peak_b, "bf16")
    wide = torch.randn((3, 68, 41), generator=g).cuda()
    xt = wide.transpose(1, 2)                                  # [3, 41, 68], not contiguous
    assert not xt.is_contiguous()
    out_t, peak_t = _smoother(6)(xt)
    assert out_t.shape == xt.shape
    _check(xt.contiguous(), 6, out_t.contiguous(), peak_t, "strided")


def test_smoother_does_not_synchronise():
    x = torch.randn((2, 1, 64, 96), device="cuda")
    s = _smoother(16)
    want, want_peak = s(x)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, peak = s(x)
        out_b, _ = s(x.to(torch.bfloat16))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(_bits(out), _bits(want)) and torch.equal(_bits(peak), _bits(want_peak))


# ---- the CLI
def _tree(tmp_path, monkeypatch, model_name):
    from tiaozhanbei_unet_amd import AnomalyUNet, UNet
    from tiaozhanbei_unet_amd.augment import DeviceTransform
    quirk = DeviceTransform.masks          # (the loader's masks are k / 255: scaled back to {0, 1}, as test_gpu_rank_auc.py does)
    monkeypatch.setattr(DeviceTransform, "masks", lambda self, m, device="cuda": quirk(self, m, device) * 255.0)
    from tiaozhanbei_unet_amd.dataset import write_synthetic_mvtec
    from tiaozhanbei_unet_amd.utils import save_checkpoint
    root = write_synthetic_mvtec(str(tmp_path / "data"), "bottle", n_train=2, n_good=3, n_bad=4, size=64)
    torch.manual_seed(0)
    model = (AnomalyUNet(3, False) if model_name == "anomaly_unet" else UNet(3, 1, False)).cuda()
    ck = str(tmp_path / "model.pth")
    save_checkpoint(model, torch.optim.Adam(model.parameters()), 0, 0.0, ck)
    base = ["--data_root", root, "--category", "bottle", "--model", model_name, "--checkpoint", ck, "--batch_size", "3",
            "--image_size", "64", "--num_workers", "0"]
    return root, model, ck, base


@pytest.mark.parametrize("model_name", ["anomaly_unet", "unet"])
def test_cli_smooths_the_map_and_scores_by_its_peak(tmp_path, monkeypatch, model_name):
    from tiaozhanbei_unet_amd import test as cli
    from tiaozhanbei_unet_amd.dataset import get_dataloaders
    from tiaozhanbei_unet_amd.utils import load_checkpoint
    root, model, ck, base = _tree(tmp_path, monkeypatch, model_name)
    out = cli.main(base + ["--output_dir", str(tmp_path / "smooth"), "--map_sigma", "2", "--image_score", "map_max"])
    tm = json.load(open(os.path.join(out, "test_metrics.json")))
    assert tm["postprocess"] == {"map_sigma": 2.0, "map_truncate": 4.0, "radius": 8, "image_score": "map_max"}
    assert (tm["args"]["map_sigma"], tm["args"]["image_score"]) == (2.0, "map_max")

    dev = torch.device("cuda")
    _, loader = get_dataloaders(root, "bottle", 3, 64, 0, device_preprocess=True)
    load_checkpoint(model, None, ck, dev)
    raw = cli.test_model(model, loader, dev, pixel_thresholds=[0.3, 0.5, 0.7])
    res = cli.test_model(model, loader, dev, pixel_thresholds=[0.3, 0.5, 0.7], map_sigma=2.0, image_score="map_max")
    taps = R.taps64(2.0).astype(np.float32)
    maps = raw["anomaly_maps"]
    want, bnd = R.smooth64(maps, taps), R.bound(maps, taps)
    assert res["anomaly_maps"].shape == maps.shape and res["anomaly_maps"].dtype == np.float32
    assert np.all(np.abs(res["anomaly_maps"].astype(np.float64) - want) <= bnd)
    n = len(res["labels"])
    assert np.array_equal(res["image_scores"], res["anomaly_maps"].reshape(n, -1).max(1))
    assert np.array_equal(res["anomaly_scores"], res["image_scores"])
    assert np.array_equal(res["predictions"], (res["image_scores"] > res["threshold"]).astype(int))
    if model_name == "unet":
        assert len(set(res["image_scores"].tolist())) > 1          # (the reconstruction score of this model is 0 everywhere)
        assert not raw["image_scores"].any()
    bad = res["labels"] == 1
    ref = rank_auc64(res["anomaly_maps"][bad], res["masks_true"][bad] > 0.5)
    assert ref["positives"] > 0 and ref["negatives"] > 0
    entry = next(iter(tm["pixel_metrics"].values()))
    for got in (res["pixel_auc"], entry):
        assert abs(got["auroc"] - ref["auroc"]) <= 1e-12 and abs(got["auprc"] - ref["auprc"]) <= 1e-12
    # sigma 0 with map_max: the raw map, scored by its plain maximum
    peak = cli.test_model(model, loader, dev, pixel_thresholds=[0.5], image_score="map_max")
    assert np.array_equal(peak["anomaly_maps"], maps)
    assert np.array_equal(peak["image_scores"], maps.reshape(n, -1).max(1))


def test_cli_default_flags_change_nothing(tmp_path, monkeypatch):
    from tiaozhanbei_unet_amd import evaluation, test as cli
    _, _, _, base = _tree(tmp_path, monkeypatch, "anomaly_unet")
    plain = cli.main(base + ["--output_dir", str(tmp_path / "a")])

    def refuse(*a, **k):
        raise AssertionError("the smoothing kernel was launched at the default flags")

    monkeypatch.setattr(evaluation.GaussianSmoother, "__call__", refuse)
    spelled = cli.main(base + ["--output_dir", str(tmp_path / "b"), "--map_sigma", "0", "--map_truncate", "4.0",
                               "--image_score", "reconstruction"])
    a, b = (json.load(open(os.path.join(d, "test_metrics.json"))) for d in (plain, spelled))
    assert "postprocess" not in a and "postprocess" not in b
    assert {k: v for k, v in a.items() if k != "args"} == {k: v for k, v in b.items() if k != "args"}
    assert a["args"]["map_sigma"] == 0.0 and a["args"]["image_score"] == "reconstruction"
    assert open(os.path.join(plain, "detailed_results.json")).read() == open(os.path.join(spelled, "detailed_results.json")).read()
