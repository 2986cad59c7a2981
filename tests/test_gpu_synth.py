"""The synthetic-anomaly kernel (csrc/synth.hip through augment.synth_anomalies / AnomalySynthesizer) against
tests/_synth_ref.py, and the trainer's --synthetic_anomalies flag end to end.  Both sides compute in IEEE single
precision with every product and sum rounded once and in the same order, so the bound is equality, bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

import _synth_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_case(shape, fields, images, masks):
    from tiaozhanbei_unet_amd import augment as A
    desc = A.synth_table(shape[0], **fields)
    got, got_mask = A.synth_anomalies(dev(images), desc, dev(masks))
    want, want_mask = R.synthesize(images, desc, masks)
    return desc, got.cpu().numpy(), got_mask.cpu().numpy(), want, want_mask


@pytest.mark.parametrize("name", list(R.CASES))
def test_kernel_equals_the_fp32_reference_bit_for_bit(name):
    case = R.CASES[name]
    n, h, w = case["shape"]
    images, masks = R.case_inputs(name)
    desc, got, got_mask, want, want_mask = run_case(case["shape"], case["fields"], images, masks)
    assert got.shape == (n, 3, h, w) and got_mask.shape == (n, 1, h, w) and got.dtype == got_mask.dtype == np.float32
    assert np.array_equal(bits(got_mask), bits(want_mask)), name
    assert np.array_equal(bits(got), bits(want)), name
    if case["mixed"]:
        assert (want != images).any() and (want == images).any()
    for i in range(n):
        if not desc["apply"][i]:             # an image left alone: its own bits, and the mask that came in
            assert np.array_equal(bits(got[i]), bits(images[i]))
            assert np.array_equal(bits(got_mask[i]), bits(masks[i] if masks is not None else np.zeros((1, h, w), np.float32)))
        if desc["threshold"][i] == 2.0:
            assert not got_mask[i].any() and np.array_equal(bits(got[i]), bits(images[i]))
        if desc["threshold"][i] == -2.0:
            assert (got_mask[i] == 1.0).all()
    assert np.isin(got_mask, [0.0, 1.0] if masks is None else [0.0, np.float32(1.0 / 255.0), 1.0]).all()
    if masks is not None:                    # the max rule: nothing that came in is lost
        assert (got_mask >= masks).all() and (got_mask > masks).any()


def test_beta_zero_gives_the_donor_exactly():
    case = R.CASES["beta_zero"]
    images, _ = R.case_inputs("beta_zero")
    f = case["fields"]
    _, got, got_mask, _, _ = run_case(case["shape"], f, images, None)
    assert (got_mask == 1.0).all()
    for i in range(case["shape"][0]):
        donor = np.roll(images[f["src"][i]], (-f["shift_y"][i], -f["shift_x"][i]), axis=(1, 2))[list(R.PERMS[f["perm"][i]])]
        # (0 * x + 1 * donor: equal as values; a zero of either sign stays a zero)
        assert np.array_equal(got[i], donor)


def test_one_batch_past_the_grid_cap():
    from tiaozhanbei_unet_amd import augment as A
    n, h, w = R.PAST_CAP
    g = torch.Generator().manual_seed(3)
    images = torch.randn((n, 3, h, w), generator=g).numpy()
    masks = (torch.rand((n, 1, h, w), generator=g) < 0.1).float().numpy()
    desc, got, got_mask, want, want_mask = run_case(R.PAST_CAP, R.past_cap_fields(), images, masks)
    assert A.SYNTH_DTYPE == desc.dtype and not desc["apply"].all() and desc["apply"][-1]
    assert np.array_equal(bits(got_mask), bits(want_mask))
    assert np.array_equal(bits(got), bits(want))
    assert (got[-1] != images[-1]).any()     # the image beyond the first trip of the stride loop was reached


def test_bad_arguments_are_refused():
    from tiaozhanbei_unet_amd import augment as A
    x = torch.zeros((2, 3, 8, 8), device=DEV)
    ok = dict(apply=1, seed=1, cells_y=2, cells_x=2, threshold=0.5, beta=0.5, src=[1, 0], shift_y=1, shift_x=1, perm=0)
    desc = A.synth_table(2, **ok)
    A.synth_anomalies(x, desc)
    refused = (ValueError, RuntimeError)
    with pytest.raises(refused):
        A.synth_anomalies(x.cpu(), desc)
    with pytest.raises(refused):
        A.synth_anomalies(x.half(), desc)
    with pytest.raises(refused):
        A.synth_anomalies(x[0], desc)
    with pytest.raises(refused, match="channels"):
        A.synth_anomalies(torch.zeros((2, 4, 8, 8), device=DEV), desc)
    with pytest.raises(refused):
        A.synth_anomalies(x, desc[:1])
    with pytest.raises(refused):
        A.synth_anomalies(x, desc, torch.zeros((2, 1, 8, 4), device=DEV))
    for field, value in (("src", 2), ("src", -1), ("cells_y", 3), ("cells_x", 128), ("shift_y", 8), ("shift_x", -1), ("perm", 6)):
        with pytest.raises(RuntimeError, match="unet_synth_anomalies"):
            A.synth_anomalies(x, A.synth_table(2, **{**ok, field: value}))
    torch.cuda.synchronize()


def test_replay_and_seeding_are_bit_exact():
    from tiaozhanbei_unet_amd.augment import AnomalySynthesizer
    g = torch.Generator().manual_seed(9)
    images = torch.randn((5, 3, 24, 36), generator=g).to(DEV)
    masks = (torch.rand((5, 1, 24, 36), generator=g) < 0.1).float().to(DEV)
    s = AnomalySynthesizer(p=1.0, threshold=0.2, seed=12)
    params = s.draw(5, (24, 36))
    a, am = s(images, masks, params=params)
    b, bm = s(images, masks, params=params)
    assert torch.equal(a, b) and torch.equal(am, bm)
    want, want_mask = R.synthesize(images.cpu().numpy(), s.table(params), masks.cpu().numpy())
    assert np.array_equal(bits(a.cpu().numpy()), bits(want)) and np.array_equal(bits(am.cpu().numpy()), bits(want_mask))
    one, two = AnomalySynthesizer(p=0.7, seed=99), AnomalySynthesizer(p=0.7, seed=99)
    for _ in range(2):
        (c, cm), (d, dm) = one(images), two(images)
        assert torch.equal(c, d) and torch.equal(cm, dm)
    other, _ = AnomalySynthesizer(p=0.7, seed=100)(images)
    assert not torch.equal(other, c)
    assert not torch.equal(a, images) and images.data_ptr() != a.data_ptr()


def _train(tmp_path, name, *extra):
    from tiaozhanbei_unet_amd import train
    exp = train.main(["--synthetic", *extra, "--epochs", "1", "--image_size", "32", "--batch_size", "4", "--num_workers", "0",
                      "--save_dir", str(tmp_path / name)])
    return (json.load(open(os.path.join(exp, "args.json"))),
            json.load(open(os.path.join(exp, "results", "training_results.json"))))


def test_training_with_synthetic_anomalies_end_to_end(tmp_path):
    args, res = _train(tmp_path, "on", "--synthetic_anomalies", "1.0")
    assert args["synthetic_anomalies"] == 1.0 and args["perlin_threshold"] == 0.5
    losses = res["train_losses"] + res["val_losses"]
    print("losses with synthetic anomalies:", losses)
    assert len(res["train_losses"]) == 1 and len(res["val_losses"]) == 1 and all(np.isfinite(losses))


def test_flag_at_zero_trains_exactly_as_without_it(tmp_path):
    """Off is off: the losses of a run with ``--synthetic_anomalies 0.0`` equal those of a run without the flag (training
    is bitwise reproducible from its seed), and differ from a run with it on."""
    a0, r0 = _train(tmp_path, "zero", "--synthetic_anomalies", "0.0")
    a1, r1 = _train(tmp_path, "none")
    print("train / val losses:", r0["train_losses"], r0["val_losses"], "|", r1["train_losses"], r1["val_losses"])
    assert a0["synthetic_anomalies"] == a1["synthetic_anomalies"] == 0.0
    for k in ("train_losses", "val_losses", "best_val_loss", "total_params"):
        assert r0[k] == r1[k], k
