"""Host side of the synthetic anomalies (augment.AnomalySynthesizer, train.py --synthetic_anomalies) and the worth of
tests/_synth_ref.py, the fp32 restatement that tests/test_gpu_synth.py holds the kernel to: no GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

import _synth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def noise_pairs():
    """(threshold, noise32, noise64) over the GPU test's own cases plus 200 random draws at sizes up to 64 x 64."""
    cases = R.noise_cases()
    r = np.random.default_rng(5)
    for _ in range(200):
        cases.append((int(r.integers(0, 1 << 32)), int(r.integers(1, 65)), int(r.integers(1, 65)), 1 << int(r.integers(0, 7)),
                      1 << int(r.integers(0, 7)), float(r.uniform(-0.2, 0.6))))
    return [(thr, R.noise32(s, h, w, cy, cx), R.noise64(s, h, w, cy, cx)) for s, h, w, cy, cx, thr in cases]


def test_fp32_reference_agrees_with_its_float64_variant(noise_pairs):
    """eps = the largest |noise32 - noise64|.  Bound from the formula, u = 2^-24, |gradient| = 1, |offset| < 1.5: a dot is
    two products, a sum and at most one rounded offset (< 8u in all); a lerp a + f (b - a) passes its inputs' errors on
    without growth (0 <= f <= 1) and adds three roundings of values below 3 (9u), twice in a row; the scale multiplies
    by sqrt 2 and rounds once more: (8 + 9 + 9) sqrt 2 u + 2u < 64u = 3.9e-6.  The masks of the two variants may then
    differ only where the float64 noise lies within eps of the threshold, and on at most 0.1 % of the pixels of a case."""
    eps = max(float(np.abs(n32.astype(np.float64) - n64).max()) for _, n32, n64 in noise_pairs)
    worst = max(float(np.abs(n64).max()) for _, _, n64 in noise_pairs)
    near = total = 0
    for thr, n32, n64 in noise_pairs:
        thr32 = np.float32(thr)
        differ = (n32 > thr32) != (n64 > np.float64(thr32))
        close = np.abs(n64 - np.float64(thr32)) <= eps
        assert not np.any(differ & ~close)
        assert close.sum() <= 1e-3 * close.size, (thr, n32.shape, int(close.sum()))
        near += int(close.sum())
        total += close.size
    print(f"REF64 synth: eps = max|noise32 - noise64| = {eps:.3e} over {len(noise_pairs)} cases, max|noise| = {worst:.4f}, "
          f"{near} of {total} pixels within eps of their threshold")
    assert eps <= 64 * 2.0 ** -24
    assert worst <= 1.5                       # "roughly [-1, 1]": sqrt 2 times a lerp of dots below sqrt(1/2) in the cell's middle


def test_reference_masks_cover_both_values():
    for name, case in R.CASES.items():
        if not case["mixed"]:
            continue
        n, h, w = case["shape"]
        f = {k: np.broadcast_to(np.asarray(v), (n,)) for k, v in case["fields"].items()}
        m = np.stack([R.noise32(int(f["seed"][i]), h, w, int(f["cells_y"][i]), int(f["cells_x"][i])) > np.float32(f["threshold"][i])
                      for i in range(n) if f["apply"][i]])
        assert m.any() and not m.all(), name


def test_host_tables_match_the_reference():
    """augment.py's per-axis tables (cell, t, fade) and gradient table are the reference's own, value for value."""
    from tiaozhanbei_unet_amd import augment as A
    dev = torch.device("cpu")
    for n in (1, 8, 17, 23, 136, 256):
        cell, tf = (t.numpy() for t in A._synth_axis_tables(n, dev))
        for lg in range(7):
            i, t = R.axis(n, 1 << lg)
            fade = t * t * t * (t * (t * np.float32(6) - np.float32(15)) + np.float32(10))
            assert np.array_equal(cell[lg], i) and np.array_equal(tf[lg, 0], t) and np.array_equal(tf[lg, 1], fade)
    gx, gy = R.gradients()
    assert np.array_equal(A._synth_gradients(dev).numpy(), np.stack([gx, gy], 1))


def test_descriptor_dtype_matches_the_header():
    from tiaozhanbei_unet_amd import augment as A
    text = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    body = re.search(r"typedef struct unet_synth_desc \{(.*?)\} unet_synth_desc;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        m = re.match(r"\s*(int32_t|uint32_t|float)\s+(.*)", decl.strip(), re.S)
        if m:
            names += [v.strip() for v in m.group(2).split(",")]
    assert list(A.SYNTH_DTYPE.names) == names
    assert A.SYNTH_DTYPE.itemsize == 4 * len(names) == 48
    assert all(A.SYNTH_DTYPE.fields[k][1] == 4 * i for i, k in enumerate(names))
    assert A.SYNTH_PERMS == R.PERMS


def test_draw_is_reproducible_and_inside_its_ranges():
    from tiaozhanbei_unet_amd.augment import AnomalySynthesizer
    a, b = AnomalySynthesizer(seed=7), AnomalySynthesizer(seed=7)
    pa = [a.draw(16, (24, 40)) for _ in range(3)]
    assert pa == [b.draw(16, (24, 40)) for _ in range(3)]
    assert pa[0] != pa[1] and pa[0] != AnomalySynthesizer(seed=8).draw(16, (24, 40))
    assert not any(AnomalySynthesizer(p=0.0, seed=1).draw(64, 32)["apply"])
    assert all(AnomalySynthesizer(p=1.0, seed=1).draw(64, 32)["apply"])
    s = AnomalySynthesizer(p=0.5, beta=(0.2, 0.6), seed=3)
    applied = 0
    for n, (h, w) in ((1, (5, 7)), (2, (1, 9)), (8, (17, 23)), (32, (64, 64))):
        for _ in range(50):
            d = s.draw(n, (h, w))
            assert all(len(v) == n for v in d.values())
            assert all(c in (1, 2, 4, 8, 16, 32, 64) for c in d["cells_y"] + d["cells_x"])
            assert all(0.2 <= v <= 0.6 for v in d["beta"])
            assert all(0 <= v < n for v in d["src"]) and all(0 <= v < 6 for v in d["perm"])
            assert all(0 <= v < h for v in d["shift_y"]) and all(0 <= v < w for v in d["shift_x"])
            assert all(0 <= v < 1 << 32 for v in d["seed"])
            assert not any(d["src"][i] == i and d["shift_y"][i] == 0 and d["shift_x"][i] == 0 for i in range(n))
            applied += sum(d["apply"])
            rec = s.table(d)
            assert rec.shape == (n,) and np.all(rec["threshold"] == np.float32(0.5))
            assert np.array_equal(rec["one_minus_beta"], np.float32(1) - rec["beta"])
    assert 0.4 < applied / (50 * (1 + 2 + 8 + 32)) < 0.6
    small = AnomalySynthesizer(max_cells_log2=2, seed=4).draw(200, 16)
    assert set(small["cells_y"]) | set(small["cells_x"]) == {1, 2, 4}
    assert len(set(AnomalySynthesizer(seed=4).draw(400, 16)["cells_y"])) == 7
    one = AnomalySynthesizer(p=1.0, seed=5).draw(1, (1, 1))          # nothing to shift to: left alone
    assert one["apply"] == [False]


def test_train_flags_default_to_off():
    from tiaozhanbei_unet_amd import train
    a = train.parse_args([])
    assert a.synthetic_anomalies == 0.0 and a.perlin_threshold == 0.5
    b = train.parse_args(["--synthetic_anomalies", "0.5", "--perlin_threshold", "0.4"])
    assert b.synthetic_anomalies == 0.5 and b.perlin_threshold == 0.4


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.k = torch.nn.Parameter(torch.ones(()))
        self.seen = []

    def forward(self, x):
        self.seen.append(x.detach().clone())
        return x * self.k, x[:, :1] * self.k


class _Opt:
    steps = 0

    def zero_grad(self, set_to_none=True):
        pass

    def step(self):
        self.steps += 1


def test_train_epoch_corrupt_hook_contract():
    """With ``corrupt`` the model sees the corrupted inputs, the criterion the clean images as target and the
    corruptor's masks; without it the loop hands the loader's own tensors on."""
    from tiaozhanbei_unet_amd.train_utils import train_epoch
    g = torch.Generator().manual_seed(0)
    batches = [{"image": torch.randn(2, 3, 4, 4, generator=g), "mask": torch.zeros(2, 1, 4, 4)} for _ in range(2)]
    calls = []

    def corrupt(images, masks):
        calls.append((images, masks))
        return images + 1.0, masks + 0.5

    def criterion(recon, amap, target, masks):
        seen.append((target.clone(), masks.clone()))
        loss = recon.mean()
        return {"total_loss": loss, "recon_loss": loss, "seg_loss": loss}

    for hook in (corrupt, None):
        model, opt, seen = _Stub(), _Opt(), []
        out = train_epoch(model, [dict(b) for b in batches], criterion, opt, torch.device("cpu"), 0, corrupt=hook)
        assert opt.steps == 2 and set(out) == {"total_loss", "recon_loss", "seg_loss"}
        for b, x, (target, masks) in zip(batches, model.seen, seen):
            assert torch.equal(target, b["image"])
            assert torch.equal(x, b["image"] + 1.0 if hook else b["image"])
            assert torch.equal(masks, b["mask"] + 0.5 if hook else b["mask"])
    assert len(calls) == 2 and torch.equal(calls[0][0], batches[0]["image"])
