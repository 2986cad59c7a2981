"""Host side of the map smoothing (evaluation.GaussianSmoother, test.py --map_sigma / --map_truncate / --image_score,
the refusals of unet_smooth_maps) and the worth of tests/_smooth_ref.py, which tests/test_gpu_smooth.py holds the
kernel to: no GPU needed."""
import ctypes as C

import numpy as np
import pytest

import _smooth_ref as R

SIGMAS = {0.25: 1, 1.5: 6, 4.0: 16, 8.0: 32}          # sigma -> radius at truncate 4
SHAPES = [(5, 7), (1, 1), (3, 200), (37, 53)]


@pytest.mark.parametrize("sigma", sorted(SIGMAS))
def test_restatement_equals_scipy(sigma):
    ndimage = pytest.importorskip("scipy.ndimage")
    assert R.radius_of(sigma) == SIGMAS[sigma]
    rng = np.random.default_rng(int(sigma * 100))
    worst = 0.0
    for h, w in SHAPES:
        x = rng.standard_normal((2, h, w))
        want = np.stack([ndimage.gaussian_filter(p, sigma, mode="reflect", truncate=4.0) for p in x])
        worst = max(worst, float(np.abs(R.smooth64(x, R.taps64(sigma)) - want).max()))
    print(f"sigma {sigma}: max |restatement - scipy| = {worst:.2e}")
    assert worst <= 1e-12
    x = rng.standard_normal((9, 11))                  # another truncate: radius int(2.5 * 1.5 + 0.5) = 4
    assert R.radius_of(1.5, 2.5) == 4
    assert np.abs(R.smooth64(x, R.taps64(1.5, 2.5)) - ndimage.gaussian_filter(x, 1.5, mode="reflect", truncate=2.5)).max() <= 1e-12


def test_fold_is_the_reflect_border():
    assert R.fold(np.arange(-9, 13), 4).tolist() == [0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3]
    assert set(R.fold(np.arange(-40, 40), 1).tolist()) == {0}


def test_smoother_radius_and_taps():
    from tiaozhanbei_unet_amd import evaluation, ops
    assert ops.GaussianSmoother is evaluation.GaussianSmoother
    for sigma, radius in SIGMAS.items():
        s = evaluation.GaussianSmoother(sigma)
        assert s.radius == radius and s.taps.dtype == np.float32 and s.taps.shape == (radius + 1,)
        assert np.array_equal(s.taps64, R.taps64(sigma))
        assert np.array_equal(s.taps, R.taps64(sigma).astype(np.float32))          # the rounded float64 taps
        assert list(s._host) == s.taps.tolist()
        full = R.window(s.taps)
        assert np.array_equal(full, full[::-1]) and len(full) == 2 * radius + 1
        assert abs(float(full.astype(np.float64).sum()) - 1.0) <= (2 * radius + 1) * R.U
    z = evaluation.GaussianSmoother(0.0)
    assert z.radius == 0 and z.taps.tolist() == [1.0]
    assert evaluation.GaussianSmoother(3.0, truncate=0.0).taps.tolist() == [1.0]
    assert evaluation.GaussianSmoother(1.5, truncate=2.5).radius == 4
    assert evaluation.GaussianSmoother(8.124).radius == 32


@pytest.mark.parametrize("sigma, truncate", [(-1.0, 4.0), (float("nan"), 4.0), (float("inf"), 4.0), (1.0, -1.0),
                                             (1.0, float("nan")), (1.0, float("inf")), (8.2, 4.0), (4.0, 9.0)])
def test_smoother_refuses(sigma, truncate):
    from tiaozhanbei_unet_amd.evaluation import GaussianSmoother
    with pytest.raises(ValueError) as e:
        GaussianSmoother(sigma, truncate)
    if sigma == 8.2:
        assert "8.125" in str(e.value)              # the largest sigma that fits at truncate 4: radius 32 ends below it


def test_cli_flags():
    from tiaozhanbei_unet_amd import test as cli
    names = [n for n, _ in cli.FLAGS]
    assert names[-3:] == ["--map_sigma", "--map_truncate", "--image_score"]
    assert names[:-3] == ["--data_root", "--category", "--image_size", "--model", "--bilinear", "--checkpoint", "--batch_size",
                          "--num_workers", "--device", "--threshold", "--pixel_thresholds", "--output_dir",
                          "--save_visualizations", "--max_vis_samples", "--precision", "--pro_fpr_limit", "--binary_masks",
                          "--vis_overlay_alpha"]
    a = cli.parse_args(["--checkpoint", "x.pth"])
    assert (a.map_sigma, a.map_truncate, a.image_score) == (0.0, 4.0, "reconstruction")
    b = cli.parse_args(["--checkpoint", "x.pth", "--map_sigma", "4", "--map_truncate", "3", "--image_score", "map_max"])
    assert (b.map_sigma, b.map_truncate, b.image_score) == (4.0, 3.0, "map_max")
    assert cli.map_radius(2.0, 4.0) == 8


@pytest.mark.parametrize("flag, value", [("--map_sigma", "-1"), ("--map_sigma", "nan"), ("--map_sigma", "inf"),
                                         ("--map_sigma", "9"), ("--map_truncate", "-0.5"), ("--map_truncate", "nan"),
                                         ("--image_score", "mean")])
def test_cli_refuses(flag, value, capsys):
    from tiaozhanbei_unet_amd import test as cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--checkpoint", "x.pth", flag, value])
    assert flag in str(e.value) + capsys.readouterr().err


def test_test_model_keeps_its_signature():
    import inspect
    from tiaozhanbei_unet_amd import test as cli
    p = inspect.signature(cli.test_model).parameters
    assert list(p)[:7] == ["model", "test_loader", "device", "threshold", "pixel_thresholds", "pro_fpr_limit", "binary_masks"]
    for name, default in (("map_sigma", 0.0), ("map_truncate", 4.0), ("image_score", "reconstruction")):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default


# ---- the entry point's refusals: all come before any launch, so they need no GPU
def _call(**over):
    from tiaozhanbei_unet_amd import _lib
    lib = _lib.lib()
    keep = _call.keep
    if "src" not in keep:
        keep.update(src=(C.c_float * 64)(), dst=(C.c_float * 64)(), taps=(C.c_float * 40)(*([0.01] * 40)))
    a = dict(src=C.addressof(keep["src"]), dst=C.addressof(keep["dst"]), n=1, h=4, w=4, taps=C.addressof(keep["taps"]),
             radius=2, image_max=None, stream=None)
    a.update(over)
    rc = lib.unet_smooth_maps(a["src"], a["dst"], a["n"], a["h"], a["w"], a["taps"], a["radius"], a["image_max"], a["stream"])
    return rc, lib.unet_last_error()


_call.keep = {}


def _taps(*values):
    _call.keep[values] = (C.c_float * len(values))(*values)
    return C.addressof(_call.keep[values])


def test_entry_point_refusals():
    bad = {"null src": dict(src=None), "null dst": dict(dst=None), "null taps": dict(taps=None),
           "n < 0": dict(n=-1), "h < 0": dict(h=-1), "w < 0": dict(w=-3), "radius < 0": dict(radius=-1),
           "nan tap": dict(taps=_taps(0.5, float("nan"), 0.1)), "inf tap": dict(taps=_taps(0.5, 0.1, float("inf")))}
    for what, over in bad.items():
        rc, err = _call(**over)
        assert rc == -1 and b"unet_smooth_maps:" in err, (what, rc, err)
    rc, err = _call(n=-7)
    assert rc == -1 and b"-7" in err
    rc, err = _call(taps=_taps(0.5, 0.25, float("nan")))
    assert rc == -1 and b"tap 2" in err
    src = C.addressof(_call.keep["src"])
    for what, over in {"in place": dict(dst=src), "overlap, dst ahead": dict(dst=src + 4), "overlap, src ahead": dict(src=src + 60, dst=src)}.items():
        rc, err = _call(**over)
        assert rc == -1 and b"unet_smooth_maps:" in err and b"overlap" in err, (what, rc, err)
    # (every call here stops before a launch: the buffers are host memory)
    unsupported = {"radius 33": (dict(radius=33), b"33"), "2^31 elements": (dict(n=2, h=32768, w=32768), b"32768"),
                   "2^40 planes": (dict(n=1 << 40, h=1, w=1), str(1 << 40).encode())}
    for what, (over, token) in unsupported.items():
        rc, err = _call(**over)
        assert rc == -2 and b"unet_smooth_maps:" in err and token in err, (what, rc, err)
    for over in (dict(n=0), dict(h=0), dict(w=0), dict(n=0, radius=32), dict(n=1 << 40, h=0, w=5)):
        assert _call(**over)[0] == 0, over
    assert _call(radius=32, n=0)[0] == 0 and _call(radius=0, n=0)[0] == 0


@pytest.mark.parametrize("sigma", sorted(SIGMAS))
def test_bound_holds_for_a_naive_fp32_evaluation(sigma):
    """Guards the bound itself: plain left-to-right fp32 passes stay inside (2K + 2) u A at every element, with room."""
    taps32 = R.taps64(sigma).astype(np.float32)
    rng = np.random.default_rng(7)
    worst = 0.0
    for h, w in SHAPES + [(64, 96)]:
        x = rng.standard_normal((2, h, w)).astype(np.float32)
        if h > 4:
            x[1] = np.abs(x[1]) + 3.0                 # no cancellation: the error is largest relative to the bound
        err = np.abs(R.smooth32_naive(x, taps32).astype(np.float64) - R.smooth64(x, taps32))
        bnd = R.bound(x, taps32)
        assert np.all(bnd > 0)
        worst = max(worst, float((err / bnd).max()))
    print(f"sigma {sigma}: naive fp32 error / bound <= {worst:.3f}")
    assert worst <= 1.0
