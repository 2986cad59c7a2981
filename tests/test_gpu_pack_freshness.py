"""The cached weight packs (ops.PackCache per model, the BatchNorm-folded packs of ops._folded) across a model's life:
after every event that changes weights, replaces Parameters, copies the model or switches between models, a WARM model
(caches built before the event) must compute exactly what a COLD one does -- a new instance of the same class and
precision, loaded from clones of the warm model's state_dict, that has never run.

The project is bitwise reproducible, so every comparison is torch.equal: no tolerances in this file.  Each model is
run three ways -- eval under no_grad (folded packs), eval with autograd + backward (PackCache forward and data-gradient
packs), training forward + backward -- and outputs, input gradients and every parameter gradient are compared.  Every
scenario first shows that it could fail: the caches are warm before the event, and the event changes the output."""
import copy
import gc
import pickle
import weakref

import pytest
import torch
import torch.nn as nn

from oracle import weights as W
from test_gpu_model import DEV, maxabs

pytestmark = pytest.mark.gpu

BOTH = ["fp32", "bf16"]
WARMUP = ("train", "eval", "nograd")       # ends on the eval forwards: nothing but the event invalidates their packs
PHASES = ("nograd", "eval", "train")


class _Narrow(nn.Module):
    """DoubleConv(3, 40) into Up(80, 24, transposed conv): every width narrow, no PackCache (ops.packed's fallback);
    the folded packs take the rows / split branch of ops._folded_pack."""

    def __init__(self, precision):
        super().__init__()
        import tiaozhanbei_unet_amd as P
        self.dc = P.DoubleConv(3, 40, precision=precision)
        self.up = P.Up(80, 24, bilinear=False, precision=precision)

    def forward(self, x, deep):
        return self.up(deep, self.dc(x))


def _ctor(kind, precision):
    import tiaozhanbei_unet_amd as P
    with torch.device(DEV):
        if kind == "unet":
            return P.UNet(3, 2, precision=precision)
        if kind == "anomaly":
            return P.AnomalyUNet(3, precision=precision)
        if kind == "seg":
            return P.SegmentationUNet(3, 4, precision=precision)
        if kind == "narrow":
            return _Narrow(precision)
        if kind == "dc":
            return P.DoubleConv(64, 128, precision=precision)
        if kind == "up":
            return P.Up(128, 64, bilinear=False, precision=precision)
    raise ValueError(kind)


_SHAPES = {"narrow": [(2, 3, 32, 32), (2, 80, 16, 16)], "dc": [(2, 64, 16, 16)], "up": [(2, 128, 8, 8), (2, 64, 16, 16)]}
_const = {}


def _inputs(kind):
    shapes = _SHAPES.get(kind, [(2, 3, 32, 32)])
    key = ("x", kind)
    if key not in _const:
        _const[key] = [W.make_input(f"fresh:x{i}", s).to(DEV) for i, s in enumerate(shapes)]
    return _const[key]


def _gy(i, out):
    key = ("gy", i, tuple(out.shape))
    if key not in _const:
        _const[key] = W.make_input(f"fresh:gy{i}", tuple(out.shape)).to(DEV)
    return _const[key].to(out.dtype)


def _new(kind, precision, seed):
    """A model with seeded non-trivial weights, BatchNorm affine parameters and running statistics (drawn on the GPU)."""
    m = _ctor(kind, precision)
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 4:
                b = float(p.shape[1] * p.shape[2] * p.shape[3]) ** -0.5
                p.uniform_(-b, b, generator=g)
            elif name.endswith("weight"):
                p.uniform_(0.5, 1.5, generator=g)
            else:
                p.uniform_(-0.3, 0.3, generator=g)
        for name, b in m.named_buffers():
            if name.endswith("running_mean"):
                b.uniform_(-0.2, 0.2, generator=g)
            elif name.endswith("running_var"):
                b.uniform_(0.5, 1.5, generator=g)
    return m


def _cold(warm, kind, precision):
    cold = _ctor(kind, precision)
    cold.load_state_dict({k: v.detach().clone() for k, v in warm.state_dict().items()})
    return cold


def _tuple(out):
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def _collect(res, phase, model, outs, xs):
    for i, o in enumerate(outs):
        res[f"{phase}:out{i}"] = o.detach().clone()
    for i, x in enumerate(xs):
        res[f"{phase}:dx{i}"] = x.grad.detach().clone()
    for name, p in model.named_parameters():
        if p.grad is not None:
            res[f"{phase}:d {name}"] = p.grad.detach().clone()


def _run(model, inputs, phases=PHASES, calls=None):
    """-> ({name: tensor}, {phase: ops.pack_weight calls during that phase's forward + backward})."""
    res, slow = {}, {}
    for phase in phases:
        model.train(phase == "train")
        torch.manual_seed(77)                          # (SegmentationUNet's bottleneck dropout draws in training mode)
        n0 = len(calls) if calls is not None else 0
        if phase == "nograd":
            with torch.no_grad():
                outs = _tuple(model(*inputs))
            _collect(res, phase, model, outs, [])
        else:
            model.zero_grad(set_to_none=True)
            xs = [x.detach().clone().requires_grad_(True) for x in inputs]
            outs = _tuple(model(*xs))
            torch.autograd.backward(outs, [_gy(i, o) for i, o in enumerate(outs)])
            _collect(res, phase, model, outs, xs)
            model.zero_grad(set_to_none=True)
            del xs
        del outs
        slow[phase] = (len(calls) - n0) if calls is not None else 0
    torch.cuda.synchronize()
    return res, slow


def _same(got, want, tag):
    assert set(got) == set(want), (tag, sorted(set(got) ^ set(want)))
    nonfinite = [k for k, v in want.items() if not bool(torch.isfinite(v).all())]
    assert not nonfinite, (tag, "the scenario itself overflowed", nonfinite[:5])
    bad = {k: maxabs(got[k], want[k]) for k in want if not torch.equal(got[k], want[k])}
    assert not bad, (tag, len(bad), dict(list(bad.items())[:8]))


@pytest.fixture
def calls(monkeypatch):
    """Every ops.pack_weight call: the one-launch-per-layer path ops.packed falls back to when the cache misses."""
    from tiaozhanbei_unet_amd import ops
    seen = []
    real = ops.pack_weight
    monkeypatch.setattr(ops, "pack_weight", lambda *a, **k: seen.append(a[1]) or real(*a, **k))
    return seen


def _expect_fresh(warm, kind, precision, inputs, calls, pre=None, cached=True, phases=PHASES, tag=""):
    """The warm model against a cold one, run the same way.  ``pre``: what the warm model gave before the event;
    ``cached``: a whole model with a PackCache -- its second forward after the event makes no single pack launch."""
    cold = _cold(warm, kind, precision)
    got, slow = _run(warm, inputs, phases, calls)
    want, slow_cold = _run(cold, inputs, phases, calls)
    _same(got, want, (tag, kind, precision))
    if pre is not None:
        assert not torch.equal(got["nograd:out0"], pre["nograd:out0"]), (tag, "the event did not change the output")
    if cached:
        assert slow["eval"] == 0 and slow_cold["eval"] == 0, (tag, "pack launches on a cache hit", slow, slow_cold)
    return got


def _warm(kind, precision, seed, calls):
    m = _new(kind, precision, seed)
    inputs = _inputs(kind)
    pre, _ = _run(m, inputs, WARMUP, calls)
    return m, inputs, pre


def _scaled_state(model, factor=1.5):
    out = {}
    for k, v in model.state_dict().items():
        v = v.detach().clone()
        if v.dim() == 4:
            v = v * factor
        elif k.endswith("running_mean"):
            v = v + 0.1
        out[k] = v
    return out


def _layers(m, kind):
    """(a conv weight's holder, a convT weight's holder, a BatchNorm with an affine pair, a BatchNorm to reset)."""
    if kind == "narrow":
        return m.dc.double_conv[3], m.up.up, m.up.conv.double_conv[1], m.dc.double_conv[4]
    return m.down2.maxpool_conv[1].double_conv[3], m.up2.up, m.up3.conv.double_conv[1], \
        m.down1.maxpool_conv[1].double_conv[4]


# ------------------------------------------------------------------ a. load_state_dict
@pytest.mark.parametrize("kind,precision", [("unet", "fp32"), ("unet", "bf16"), ("seg", "bf16"), ("narrow", "fp32"),
                                            ("narrow", "bf16")])
def test_load_state_dict_between_forwards(kind, precision, calls):
    m, inputs, pre = _warm(kind, precision, 1, calls)
    m.load_state_dict(_scaled_state(m))
    _expect_fresh(m, kind, precision, inputs, calls, pre, cached=kind != "narrow")


# ------------------------------------------------------------------ b. load_state_dict(assign=True)
@pytest.mark.parametrize("precision", BOTH)
def test_load_state_dict_assign_replaces_the_parameters(precision, calls):
    m, inputs, pre = _warm("unet", precision, 2, calls)
    conv, convt, _, _ = _layers(m, "unet")
    old = [weakref.ref(conv.weight), weakref.ref(convt.weight), weakref.ref(m.inc.double_conv[0].weight)]
    m.load_state_dict(_scaled_state(m), assign=True)
    assert all(r() is not w for r, w in zip(old, (conv.weight, convt.weight, m.inc.double_conv[0].weight)))
    del conv, convt
    _expect_fresh(m, "unet", precision, inputs, calls, pre)          # (includes: no pack launch in its second forward)
    _, slow = _run(m, inputs, ("nograd", "eval"), calls)
    assert slow == {"nograd": 0, "eval": 0}, slow
    gc.collect()
    assert [r() for r in old] == [None, None, None], "the replaced Parameters are still held (and repacked)"


# ------------------------------------------------------------------ c. torch optimisers with every BatchNorm frozen
def _frozen_step(m, inputs, make_opt):
    """One optimiser step with the model in eval() and autograd on: no layer runs a training forward."""
    m.eval()
    m.zero_grad(set_to_none=True)
    outs = _tuple(m(*[x.detach().clone().requires_grad_(True) for x in inputs]))
    torch.autograd.backward(outs, [_gy(i, o) / o.numel() for i, o in enumerate(outs)])
    before = [p.detach().clone() for p in m.parameters()]
    opt = make_opt(m)
    opt.step()
    assert any(not torch.equal(a, p) for a, p in zip(before, m.parameters())), "the step changed nothing"
    m.zero_grad(set_to_none=True)
    return opt


# Step sizes.  With every BatchNorm frozen nothing renormalises the activations, and a first Adam step moves all weights
# of an output channel the same way (the sign of its gradient; the inputs are post-ReLU): the channel's sum grows by
# lr * fan_in * mean|x| per layer, 4608 * lr in the deep layers, and that factor compounds over 18 layers.  lr = 5e-2
# (230 per layer) would leave fp32's range; 2e-4 keeps it near 1 while moving the deep weights (rms 0.0085) by 2.4 %,
# three to six bf16 ulps, so that every pack changes.  SGD: one group per tensor, each moved by 10 % of its norm.
ADAM_LR = 2e-4


def _sgd(m):
    groups = []
    for p in m.parameters():
        gn = float(p.grad.norm()) if p.grad is not None else 0.0
        if gn > 0.0 and gn == gn:
            groups.append({"params": [p], "lr": 0.1 * float(p.detach().norm()) / gn})
    return torch.optim.SGD(groups, lr=0.0)


def _adam(m):
    return torch.optim.Adam(m.parameters(), lr=ADAM_LR, foreach=True)


@pytest.mark.parametrize("opt", ["sgd", "adam_foreach"])
@pytest.mark.parametrize("kind,precision", [("unet", "fp32"), ("unet", "bf16"), ("narrow", "fp32"), ("narrow", "bf16")])
def test_torch_optimizer_step_in_eval_mode(kind, precision, opt, calls):
    m, inputs, pre = _warm(kind, precision, 3, calls)
    _frozen_step(m, inputs, _sgd if opt == "sgd" else _adam)
    _expect_fresh(m, kind, precision, inputs, calls, pre, cached=kind != "narrow")


@pytest.mark.parametrize("precision", BOTH)
def test_fused_adam_step_in_eval_mode(precision, calls):
    """FusedAdam writes through raw pointers; in eval() no training forward repacks either (AnomalyUNet: two streams)."""
    import tiaozhanbei_unet_amd as P
    m, inputs, pre = _warm("anomaly", precision, 4, calls)
    opt = _frozen_step(m, inputs, lambda mod: P.get_optimizer(mod, "adam", ADAM_LR, 0.0))
    assert type(opt).__name__ == "FusedAdam"
    _expect_fresh(m, "anomaly", precision, inputs, calls, pre)


# ------------------------------------------------------------------ d / e. in-place writes
TARGETS = ["conv", "convt", "gamma", "reset_stats"]


def _write(m, kind, target, through_data):
    conv, convt, bn, bn_reset = _layers(m, kind)
    pick = (lambda t: t.data) if through_data else (lambda t: t)
    with torch.no_grad():
        if target == "conv":
            pick(conv.weight).mul_(1.5)
        elif target == "convt":
            pick(convt.weight).mul_(1.5)
        elif target == "gamma":
            pick(bn.weight).mul_(1.5)
        elif through_data:
            bn_reset.running_mean.data.zero_()
            bn_reset.running_var.data.fill_(1.0)
        else:
            bn_reset.reset_running_stats()


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("precision", BOTH)
def test_in_place_write_under_no_grad(precision, target, calls):
    m, inputs, pre = _warm("unet", precision, 5, calls)
    _write(m, "unet", target, through_data=False)
    _expect_fresh(m, "unet", precision, inputs, calls, pre, tag=target)


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("precision", BOTH)
def test_write_through_data_followed_by_parameters_written(precision, target, calls):
    """The contract of parameters_written(): after it, a write that moved no version counter is seen.  (What happens
    without the call is not asserted.)"""
    import tiaozhanbei_unet_amd as P
    m, inputs, pre = _warm("unet", precision, 6, calls)
    versions = [p._version for p in m.parameters()]
    _write(m, "unet", target, through_data=True)
    assert versions == [p._version for p in m.parameters()]
    P.parameters_written()
    _expect_fresh(m, "unet", precision, inputs, calls, pre, tag=target)


# ------------------------------------------------------------------ f. set_precision back and forth
@pytest.mark.parametrize("precision", BOTH)
def test_set_precision_back_and_forth(precision, calls):
    import tiaozhanbei_unet_amd as P
    other = "bf16" if precision == "fp32" else "fp32"
    m, inputs, pre = _warm("unet", precision, 7, calls)
    P.set_precision(m, other)
    there = _expect_fresh(m, "unet", other, inputs, calls, tag="switched")
    assert not torch.equal(there["nograd:out0"], pre["nograd:out0"]), "the two precisions computed the same bits"
    _run(m, inputs, ("eval", "nograd"), calls)                 # the other precision's packs are warm, too
    P.set_precision(m, precision)
    with torch.no_grad():
        _layers(m, "unet")[0].weight.mul_(1.5)
        _layers(m, "unet")[1].weight.mul_(1.5)
    _expect_fresh(m, "unet", precision, inputs, calls, pre, tag="switched back")


# ------------------------------------------------------------------ g. deepcopy, AveragedModel
def test_deepcopy_after_a_forward_shares_no_cache(calls):
    kind, precision = "anomaly", "bf16"
    m, inputs, pre = _warm(kind, precision, 8, calls)
    c = copy.deepcopy(m)
    cold = _cold(m, kind, precision)
    want, _ = _run(cold, inputs, calls=calls)
    got_c, slow_c = _run(c, inputs, calls=calls)
    got_m, slow_m = _run(m, inputs, calls=calls)
    _same(got_c, want, "the copy")
    _same(got_m, want, "the original after being copied")
    assert slow_c["eval"] == 0 and slow_m["eval"] == 0, (slow_c, slow_m)
    _run(c, inputs, ("eval", "nograd"), calls)
    pre_c, _ = _run(m, inputs, ("eval", "nograd"), calls)       # both warm, same state (the runs above were the same)
    with torch.no_grad():
        for holder in (c.down2.maxpool_conv[1].double_conv[3], c.up2_seg.up, c.up3_recon.conv.double_conv[0]):
            holder.weight.mul_(1.5)
    cold_c, cold_m = _cold(c, kind, precision), _cold(m, kind, precision)
    got_c, _ = _run(c, inputs, calls=calls)
    got_m, _ = _run(m, inputs, calls=calls)
    _same(got_c, _run(cold_c, inputs, calls=calls)[0], "the changed copy")
    _same(got_m, _run(cold_m, inputs, calls=calls)[0], "the original next to a changed copy")
    for i in (0, 1):
        assert not torch.equal(got_c[f"nograd:out{i}"], pre_c[f"nograd:out{i}"]), "the change did not show"
        assert torch.equal(got_m[f"nograd:out{i}"], pre_c[f"nograd:out{i}"]), "the original followed its copy"


def _averaged_twice(calls):
    """AveragedModel of a warm UNet, itself warm, after its second update_parameters (the mean of w and 2 w)."""
    kind, precision = "unet", "bf16"
    m, inputs, _ = _warm(kind, precision, 9, calls)
    avg = torch.optim.swa_utils.AveragedModel(m)
    avg.update_parameters(m)
    pre, _ = _run(avg.module, inputs, WARMUP, calls)            # (on the parent commit: KeyError in PackCache._build)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 4:
                p.mul_(2.0)
    avg.update_parameters(m)
    assert int(avg.n_averaged) == 2
    assert maxabs(avg.module.up2.up.weight, m.up2.up.weight * 0.75) < 1e-6      # the mean of w and 2 w
    return avg, inputs, pre, kind, precision


def test_averaged_model_follows_its_updates(calls):
    """On the GPU, AveragedModel.update_parameters averages with torch._foreach_lerp_, and on torch 2.10 / ROCm that
    operator moves NO version counter there -- measured: 0 of 64 counters moved, no data pointer changed, the values did
    change (also for _foreach_lerp_ on a Parameter itself; _foreach_mul_, Tensor.lerp_ and the CPU _foreach_lerp_ do
    move it).  Watching the weights alone, all 44 packs of the cache stayed stale: the logits were off by 0.444 at
    max |logit| 0.483.  update_parameters also writes every buffer of the averaged model (copy_ or an in-place foreach
    op, which do move their counters): the cache watches those as witnesses of a rewritten model."""
    avg, inputs, pre, kind, precision = _averaged_twice(calls)
    _expect_fresh(avg.module, kind, precision, inputs, calls, pre)


def test_averaged_model_update_followed_by_parameters_written(calls):
    import tiaozhanbei_unet_amd as P
    avg, inputs, pre, kind, precision = _averaged_twice(calls)
    P.parameters_written()
    _expect_fresh(avg.module, kind, precision, inputs, calls, pre)


# ------------------------------------------------------------------ h. pickle
def test_pickle_round_trip_carries_no_packs(calls):
    kind, precision = "unet", "bf16"
    m, inputs, _ = _warm(kind, precision, 10, calls)
    assert "_packs" in m.__dict__
    assert "_packs" not in m.__reduce_ex__(2)[2]
    c = pickle.loads(pickle.dumps(m))
    assert "_packs" not in c.__dict__ and c.compute_dtype == m.compute_dtype
    cold = _cold(m, kind, precision)
    want, _ = _run(cold, inputs, calls=calls)
    got_c, slow_c = _run(c, inputs, calls=calls)
    got_m, _ = _run(m, inputs, calls=calls)
    _same(got_c, want, "the unpickled model")
    _same(got_m, want, "the original")
    assert slow_c["eval"] == 0, slow_c
    pre, _ = _run(c, inputs, ("eval", "nograd"), calls)
    with torch.no_grad():
        c.up2.up.weight.mul_(1.5)
        c.down2.maxpool_conv[1].double_conv[3].weight.mul_(1.5)
    _expect_fresh(c, kind, precision, inputs, calls, pre, tag="the unpickled model, changed")


# ------------------------------------------------------------------ i. two live models
def test_two_models_alternating(calls):
    """ops keeps ONE active cache (the model that ran last): forwards A, B, A, then a backward of A after a forward of
    B -- A's data-gradient packs are then looked up in B's cache, miss, and are packed from A's weights."""
    kind, precision = "anomaly", "bf16"
    a, b = _new(kind, precision, 11), _new(kind, precision, 12)
    inputs = _inputs(kind)
    cold = [_cold(a, kind, precision), _cold(b, kind, precision)]
    got = [{}, {}]
    for mod in (a, b):
        mod.eval()
    with torch.no_grad():
        first = _tuple(a(*inputs))
        _collect(got[1], "nograd", b, _tuple(b(*inputs)), [])
        _collect(got[0], "nograd", a, _tuple(a(*inputs)), [])
    assert all(torch.equal(x, y) for x, y in zip(first, (got[0]["nograd:out0"], got[0]["nograd:out1"])))
    assert not torch.equal(got[0]["nograd:out0"], got[1]["nograd:out0"])
    for phase in ("eval", "train"):
        graphs = []
        for mod in (a, b):
            mod.train(phase == "train")
            mod.zero_grad(set_to_none=True)
            xs = [x.detach().clone().requires_grad_(True) for x in inputs]
            graphs.append((mod, _tuple(mod(*xs)), xs))
        for res, (mod, outs, xs) in zip(got, graphs):
            torch.autograd.backward(outs, [_gy(i, o) for i, o in enumerate(outs)])
            _collect(res, phase, mod, outs, xs)
        del graphs
    for mod, cold_mod, res, name in zip((a, b), cold, got, "AB"):
        want, _ = _run(cold_mod, inputs, calls=calls)
        _same(res, want, f"model {name}, alternating")


# ------------------------------------------------------------------ j. ids recycled by a new model
def test_model_deleted_and_another_built(calls):
    kind, precision = "unet", "bf16"
    inputs = _inputs(kind)
    last = None
    for round_ in range(3):
        a = _new(kind, precision, 20 + round_)
        _run(a, inputs, WARMUP, calls)
        del a
        gc.collect()
        b = _new(kind, precision, 30 + round_)
        got = _expect_fresh(b, kind, precision, inputs, calls, last, tag=f"round {round_}")
        last = {"nograd:out0": got["nograd:out0"]}
        del b
        gc.collect()


# ------------------------------------------------------------------ k. blocks on their own after a model forward
@pytest.mark.parametrize("kind", ["dc", "up"])
def test_standalone_block_after_a_model_forward(kind, calls):
    import tiaozhanbei_unet_amd as P
    precision = "bf16"
    model, _, _ = _warm("unet", precision, 13, calls)           # leaves its cache active
    blk = _new(kind, precision, 14)
    inputs = _inputs(kind)
    pre, _ = _run(blk, inputs, WARMUP, calls)
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 4:
                p.mul_(1.5)
    got = _expect_fresh(blk, kind, precision, inputs, calls, pre, cached=False, tag="version moved")
    _run(blk, inputs, ("eval", "nograd"), calls)
    for p in blk.parameters():
        if p.dim() == 4:
            p.data.mul_(1.5)
    P.parameters_written()
    _expect_fresh(blk, kind, precision, inputs, calls, got, cached=False, tag="parameters_written")
    del model


def test_sub_block_of_a_model_called_on_its_own(calls):
    """model.up4.conv on its own runs no cache refresh: a pack of the model's cache may be used only while current."""
    import tiaozhanbei_unet_amd as P
    kind, precision = "unet", "bf16"
    m, inputs, _ = _warm(kind, precision, 15, calls)
    x = [W.make_input("fresh:sub", (2, 128, 16, 16)).to(DEV)]
    n0 = len(calls)
    pre, _ = _run(m.up4.conv, x, ("eval", "nograd"), calls)
    assert len(calls) == n0, "the sub-block did not use the model's current packs"
    with torch.no_grad():
        for p in m.up4.conv.parameters():
            if p.dim() == 4:
                p.mul_(1.5)
    cold = _cold(m, kind, precision)
    got, _ = _run(m.up4.conv, x, calls=calls)
    _same(got, _run(cold.up4.conv, x, calls=calls)[0], "version moved")
    assert not torch.equal(got["nograd:out0"], pre["nograd:out0"])
    _run(m, inputs, ("eval", "nograd"), calls)                  # the model's packs are current again
    pre, _ = _run(m.up4.conv, x, ("eval", "nograd"), calls)
    for p in m.up4.conv.parameters():
        if p.dim() == 4:
            p.data.mul_(1.5)
    P.parameters_written()
    cold = _cold(m, kind, precision)
    got, _ = _run(m.up4.conv, x, calls=calls)
    _same(got, _run(cold.up4.conv, x, calls=calls)[0], "parameters_written")
    assert not torch.equal(got["nograd:out0"], pre["nograd:out0"])


# ------------------------------------------------------------------ l / m. the package's own raw writers
def test_adam_step_on_one_weight_of_a_warm_model(calls):
    from tiaozhanbei_unet_amd import ops
    kind, precision = "unet", "bf16"
    m, inputs, pre = _warm(kind, precision, 16, calls)
    w = _layers(m, kind)[0].weight
    version, before = w._version, w.detach().clone()
    g = W.make_input("fresh:adam_g", tuple(w.shape)).to(DEV)
    ops.adam_step_(w.detach(), g, torch.zeros_like(g), torch.zeros_like(g), 1, 5e-2, 0.9, 0.999, 1e-8, 0.0)
    assert w._version == version and not torch.equal(w.detach(), before)
    _expect_fresh(m, kind, precision, inputs, calls, pre)


def test_data_parallel_broadcast_into_a_warm_replica(calls, monkeypatch):
    """What a non-source rank sees: GradientExchange.broadcast overwrites ``param.data`` of a model that already ran.
    (One process: the collective is replaced by a write of other values; two real ranks: tests/test_cpu_pack_cache.py.)"""
    from tiaozhanbei_unet_amd import ddp
    kind, precision = "unet", "bf16"
    m, inputs, pre = _warm(kind, precision, 17, calls)
    ex = ddp.GradientExchange(m.parameters())
    assert ex.world == 1
    ex.world = 2
    received = []

    def fake_broadcast(t, src=None, group=None):
        received.append(t)
        if t.is_floating_point():
            t.mul_(1.5 if t.dim() == 4 else 1.0).add_(0.0 if t.dim() == 4 else 0.05)

    monkeypatch.setattr(ddp.dist, "broadcast", fake_broadcast)
    versions = [p._version for p in m.parameters()]
    ex.broadcast(list(m.parameters()) + list(m.buffers()))
    assert len(received) == len(list(m.parameters())) + len(list(m.buffers()))
    assert versions == [p._version for p in m.parameters()]
    _expect_fresh(m, kind, precision, inputs, calls, pre)
