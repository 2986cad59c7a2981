"""Kernel name -> launch count of five small runs, as JSON: what a change to the Python glue must leave as it is.
  python tools/launch_census.py [--tree DIR] > census.json      (DIR: another built checkout, e.g. the parent commit)
(a) one training step of AnomalyUNet(3) bf16 at 2x3x64x64, (b) the same in fp32, (c) one training step of a UNet of
widths 24..384 (none a multiple of 64 below 192) at 2x3x32x48 with transposed convolutions and the fused head, (d) / (e)
one eval-mode forward of (a) / (c) under torch.no_grad() (the folded BatchNorm packs)."""
import json
import os
import sys

import torch

here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else here))
import tiaozhanbei_unet_amd as P                                # noqa: E402
from tiaozhanbei_unet_amd import ops                            # noqa: E402

dev = torch.device("cuda:0")


def narrow_unet(precision):
    c = [24, 48, 96, 192, 384]                                  # the widths of tests/test_gpu_widths.py
    m = P.UNet(3, 1, False, precision=precision)
    m.inc = P.DoubleConv(3, c[0], precision=precision)
    for i in range(4):
        setattr(m, f"down{i + 1}", P.Down(c[i], c[i + 1], precision=precision))
        setattr(m, f"up{i + 1}", P.Up(c[4 - i], c[3 - i], False, precision=precision))
    m.outc = P.OutConv(c[0], 1, precision=precision)
    return m


def census(fn):
    torch.cuda.synchronize()
    ops.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        ops.prof_collect()
        ops.prof_enable(False)
    return {k: v["launches"] for k, v in sorted(ops.prof_kernels().items())}


def train_step(model, x, loss):
    def run():
        loss(model(x)).backward()
    return run


def eval_forward(model, x):
    def run():
        with torch.no_grad():
            model(x)
    return run


torch.manual_seed(0)
crit = P.CombinedLoss()
out = {}
x = torch.randn(2, 3, 64, 64, device=dev)
mask = (torch.rand(2, 1, 64, 64, device=dev) < 0.1).float()
for name, precision in (("a_anomaly_bf16_train", "bf16"), ("b_anomaly_fp32_train", "fp32")):
    model = P.AnomalyUNet(3, precision=precision).to(dev).train()
    out[name] = census(train_step(model, x, lambda o: crit(o[0], o[1], x, mask)["total_loss"]))
    if precision == "bf16":
        out["d_anomaly_bf16_eval"] = census(eval_forward(model.eval(), x))
xn = torch.randn(2, 3, 32, 48, device=dev)
model = narrow_unet("bf16").to(dev).train()
out["c_narrow_bf16_train"] = census(train_step(model, xn, lambda o: o.square().mean()))
out["e_narrow_bf16_eval"] = census(eval_forward(model.eval(), xn))
print(json.dumps(out, indent=1, sort_keys=True))
