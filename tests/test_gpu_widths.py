"""GPU checks of DoubleConv / Down / Up / OutConv at channel widths that are not multiples of 64 (padded storage with
zero pad lanes) against the CPU oracle: training and eval, frozen BatchNorm, pad lanes, the pass-through of a narrow
tensor between blocks, and a narrow U-Net trained for a few steps."""
import pytest
import torch
import torch.nn as nn

from oracle import unet_oracle as O
from oracle import weights as W
from test_gpu_model import DEV, l2rel, maxabs

pytestmark = pytest.mark.gpu

# (kind, args, input shapes): the Up skip is an odd 17x19 frame (centre pad), 64x96 elsewhere
BLOCKS = [
    ("double_conv", (3, 32), [(4, 3, 64, 96)]),
    ("double_conv", (3, 16), [(4, 3, 64, 96)]),
    ("double_conv", (40, 96, 48), [(4, 40, 64, 96)]),
    ("down", (96, 160), [(4, 96, 64, 96)]),
    ("up", (160, 80, False), [(4, 160, 8, 9), (4, 80, 17, 19)]),
    ("up", (192, 96, True), [(4, 96, 8, 9), (4, 96, 17, 19)]),
    ("outconv", (48, 2), [(4, 48, 64, 96)]),
]
IDS = [f"{k}_{'_'.join(map(str, a))}" for k, a, _ in BLOCKS]
BOUNDS = {"fp32": (1e-4, 2e-4, 1e-4), "bf16": (1.2e-2, 3e-2, 2e-2)}      # forward (of max), gradients (L2-rel), stats


def _inputs(kind, shapes):
    """Post-ReLU-like inputs already on the bf16 grid (what neighbouring layers hand over; as tests/test_gpu_round4.py)."""
    return [W.make_input(f"w:{kind}:{i}", s).clamp_min(-0.5).bfloat16().float() for i, s in enumerate(shapes)]


def _grad(kind, shape):
    return W.make_input(f"w:{kind}:gy", shape).bfloat16().float()


def _make(kind, args, precision):
    import tiaozhanbei_unet_amd as P
    cls = {"double_conv": P.DoubleConv, "down": P.Down, "up": P.Up, "outconv": P.OutConv}[kind]
    m = cls(*args, precision=precision)
    state = W.make_state(W.block_spec(kind, *args), 0)
    m.load_state_dict(state)
    return m.to(DEV), state


def _oracle(kind, args, state, xs, training, new_stats=None):
    if kind == "double_conv":
        return O.double_conv(state, "", xs[0], training, new_stats)
    if kind == "down":
        return O.down(state, "", xs[0], training, new_stats)
    if kind == "up":
        return O.up(state, "", xs[0], xs[1], training, args[2], new_stats)
    return O.out_conv(state, "", xs[0])


def _unprefixed(state):
    """The oracle addresses keys as f"{prefix}.name": with prefix "" a block's keys are ".name"."""
    return {"." + k: v for k, v in state.items()}


def _reference(kind, args, state, xs, training, gy, precision):
    work = {k: (v.clone().requires_grad_(True) if O.is_trainable(k) else v.clone()) for k, v in _unprefixed(state).items()}
    xr = [x.clone().requires_grad_(True) for x in xs]
    new_stats = {}
    ctx = O.bf16_storage() if precision == "bf16" else torch.enable_grad()
    with ctx:
        y = _oracle(kind, args, work, xr, training, new_stats)
        y.backward(gy)
    return y.detach(), [x.grad for x in xr], {k[1:]: v.grad for k, v in work.items() if v.requires_grad}, \
        {k[1:]: v for k, v in new_stats.items()}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,args,shapes", BLOCKS, ids=IDS)
def test_narrow_block_training_step(kind, args, shapes, precision):
    m, state = _make(kind, args, precision)
    m.train()
    xs = _inputs(kind, shapes)
    xg = [x.to(DEV).requires_grad_(True) for x in xs]
    y = m(*xg)
    gy = _grad(kind, tuple(y.shape))
    yr, dxr, gr, sr = _reference(kind, args, state, xs, True, gy, precision)
    fwd, grad, stat = BOUNDS[precision]
    assert tuple(y.shape) == tuple(yr.shape)
    assert maxabs(y, yr) < fwd * max(1.0, float(yr.abs().max())), maxabs(y, yr)
    y.backward(gy.to(DEV))
    for x, r in zip(xg, dxr):
        assert tuple(x.grad.shape) == tuple(r.shape) and l2rel(x.grad, r) < grad, l2rel(x.grad, r)
    for k, p in m.named_parameters():
        assert tuple(p.grad.shape) == tuple(p.shape) and l2rel(p.grad, gr[k]) < grad, (k, l2rel(p.grad, gr[k]))
    for k, b in m.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == 1, k
        else:
            assert tuple(b.shape) == tuple(sr[k].shape) and maxabs(b, sr[k]) < stat, (k, maxabs(b, sr[k]))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,args,shapes", BLOCKS, ids=IDS)
def test_narrow_block_eval_and_frozen_bn(kind, args, shapes, precision):
    m, state = _make(kind, args, precision)
    xs = _inputs(kind, shapes)
    fwd, grad, _ = BOUNDS[precision]
    m.eval()
    with torch.no_grad():                                       # folded BatchNorm
        y = m(*[x.to(DEV) for x in xs])
    gy = _grad(kind, tuple(y.shape))
    yr, dxr, gr, _ = _reference(kind, args, state, xs, False, gy, precision)
    assert maxabs(y, yr) < fwd * max(1.0, float(yr.abs().max())), maxabs(y, yr)
    # frozen BatchNorm: eval statistics inside an autograd graph (the fine-tuning pattern)
    xg = [x.to(DEV).requires_grad_(True) for x in xs]
    y = m(*xg)
    assert maxabs(y, yr) < fwd * max(1.0, float(yr.abs().max())), maxabs(y, yr)
    y.backward(gy.to(DEV))
    for x, r in zip(xg, dxr):
        assert l2rel(x.grad, r) < grad, l2rel(x.grad, r)
    for k, p in m.named_parameters():
        assert l2rel(p.grad, gr[k]) < grad, (k, l2rel(p.grad, gr[k]))
    for k, b in m.named_buffers():
        if not k.endswith("num_batches_tracked"):
            assert torch.equal(b.cpu(), state[k]), k               # eval leaves the running statistics alone


def test_image_layer_kernel_runs_for_a_narrow_first_block(monkeypatch):
    from tiaozhanbei_unet_amd import ops
    calls = []
    real = ops.FirstConvBnRelu.apply
    monkeypatch.setattr(ops.FirstConvBnRelu, "apply", lambda *a: calls.append(1) or real(*a))
    m, state = _make("double_conv", (3, 32), "bf16")
    m.train()
    x = W.make_input("w:first", (2, 3, 32, 48))                # width a multiple of 16
    assert ops.first_layer_ok(x.to(DEV), m.double_conv[0], torch.bfloat16)
    y = m(x.to(DEV))
    y.backward(torch.ones_like(y))
    assert calls == [1]
    assert m.double_conv[0].weight.grad.shape == (32, 3, 3, 3)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pad_lanes_stay_zero_and_narrow_tensors_pass_through(precision, monkeypatch):
    import tiaozhanbei_unet_amd as P
    from tiaozhanbei_unet_amd import ops
    a = P.DoubleConv(40, 48, precision=precision).to(DEV).train()
    b = P.Down(48, 80, precision=precision).to(DEV).train()
    packs = []
    real = ops.PackInput.apply
    monkeypatch.setattr(ops.PackInput, "apply", lambda *args: packs.append(1) or real(*args))
    x = W.make_input("w:chain", (2, 40, 32, 32)).to(DEV)
    ya = a(x)
    pa = ops.to_operator_layout(ya, ya.dtype)
    assert pa.shape[1] == 64 and pa.data_ptr() == ya.data_ptr()       # recovered without a copy
    assert len(packs) == 1                                            # the caller's NCHW input only
    yb = b(ya)
    assert len(packs) == 1                                            # ya went through as its padded tensor
    pb = ops.to_operator_layout(yb, yb.dtype)
    assert tuple(yb.shape) == (2, 80, 16, 16) and pb.shape[1] == 128
    assert torch.count_nonzero(pa[:, 48:]) == 0 and torch.count_nonzero(pb[:, 80:]) == 0
    grads = []
    pa.register_hook(lambda g: grads.append(g))
    yb.backward(W.make_input("w:chain:gy", tuple(yb.shape)).to(DEV))
    assert grads and grads[0].shape[1] == 64 and torch.count_nonzero(grads[0][:, 48:]) == 0
    assert torch.count_nonzero(grads[0][:, :48]) > 0
    # a user-modified view is not mistaken for the padded tensor: it goes through PackInput
    with torch.no_grad():
        yc = a(x)
        yc.mul_(1.0)
    assert ops.to_operator_layout(yc, yc.dtype).data_ptr() != yc.data_ptr()


class NarrowUNet(nn.Module):
    """The reference UNet's attribute layout at base width 24 (24, 48, 96, 192, 384): some levels are multiples of 64,
    some are padded; Up(192, 96) and Up(96, 48) put a narrow skip in front of the up-sampled tensor."""

    def __init__(self, precision):
        super().__init__()
        import tiaozhanbei_unet_amd as P
        c = [24, 48, 96, 192, 384]
        self.inc = P.DoubleConv(3, c[0], precision=precision)
        for i in range(4):
            setattr(self, f"down{i + 1}", P.Down(c[i], c[i + 1], precision=precision))
        for i in range(4):
            setattr(self, f"up{i + 1}", P.Up(c[4 - i], c[3 - i], False, precision=precision))
        self.outc = P.OutConv(c[0], 1, precision=precision)

    def forward(self, x):
        x1 = self.inc(x)
        x2 = self.down1(x1)
        x3 = self.down2(x2)
        x4 = self.down3(x3)
        x5 = self.down4(x4)
        y = self.up1(x5, x4)
        y = self.up2(y, x3)
        y = self.up3(y, x2)
        y = self.up4(y, x1)
        return self.outc(y)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_narrow_unet_training_steps(precision):
    from tiaozhanbei_unet_amd.train_utils import get_optimizer
    m = NarrowUNet(precision)
    state = W.make_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, 0)
    m.load_state_dict(state)
    m = m.to(DEV).train()
    x = W.make_input("w:net:x", (2, 3, 64, 64))
    gy = W.make_input("w:net:gy", (2, 1, 64, 64)).bfloat16().float()
    # bf16: eighteen layers of bf16 storage and flipped ReLU gates between the first layer's weight gradient and the loss
    fwd, grad, stat = (1e-3, 2e-3, 1e-3) if precision == "fp32" else (3e-2, 0.25, 2e-2)

    work = {k: (v.clone().requires_grad_(True) if O.is_trainable(k) else v.clone()) for k, v in state.items()}
    new_stats = {}
    with (O.bf16_storage() if precision == "bf16" else torch.enable_grad()):
        yr = O.unet_forward(work, x, True, False, new_stats)
        yr.backward(gy)
    y = m(x.to(DEV))
    assert maxabs(y, yr) < fwd * max(1.0, float(yr.abs().max())), maxabs(y, yr)
    y.backward(gy.to(DEV))
    for k, p in m.named_parameters():
        assert l2rel(p.grad, work[k].grad) < grad, (k, l2rel(p.grad, work[k].grad))
    for k, b in m.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == 1
        else:
            assert maxabs(b, new_stats[k]) < stat, (k, maxabs(b, new_stats[k]))

    # three optimiser steps of get_optimizer("adam") against the oracle's adam_step on the same gradients
    opt = get_optimizer(m, "adam")
    params = {k: state[k].clone() for k in state if O.is_trainable(k)}
    opt_state = {}
    for step in range(3):
        if step:
            opt.zero_grad(set_to_none=True)
            y = m(x.to(DEV))
            y.backward(gy.to(DEV))
        grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
        before = {k: p.detach().cpu().clone() for k, p in m.named_parameters()}
        opt.step()
        want = O.adam_step(before, grads, opt_state)
        for k, p in m.named_parameters():
            assert maxabs(p, want[k]) < 1e-6 + 1e-5 * float(want[k].abs().max()), (step, k, maxabs(p, want[k]))
        params = want
    assert set(params) == {k for k, _ in m.named_parameters()}
