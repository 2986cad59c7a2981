"""What every module that calls libunet_hip.so shares: dtype codes, stream and pointer marshalling, operator-layout
allocation, the per-stream scratch arena, the View2 descriptor, profiling.  Imports nothing of the package but ``_lib``."""
import ctypes as C
from typing import Optional

import torch

from . import _lib as L

_DT = {torch.float32: L.UNET_F32, torch.bfloat16: L.UNET_BF16}
BN_EPS = 1e-5


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "tiaozhanbei_unet_amd runs only on an AMD GPU through libunet_hip.so; got a "
                f"{t.device} tensor (there is deliberately no CPU fallback)")


def _nhwc_empty(n, c, h, w, dtype, device):
    return torch.empty((n, c, h, w), dtype=dtype, device=device, memory_format=torch.channels_last)


def _is_nhwc(t: torch.Tensor) -> bool:
    """Dense NHWC in memory (strides of size-1 dims are irrelevant)."""
    n, c, h, w = t.shape
    want = (h * w * c, 1, w * c, c)
    return all(sz == 1 or st == wt for sz, st, wt in zip(t.shape, t.stride(), want))


def _as_nhwc(t: torch.Tensor, dtype) -> torch.Tensor:
    """Activation/gradient in the operators' layout.  (Only reached for tensors produced outside
    these operators, e.g. a test's upstream gradient.)"""
    if t.dtype == dtype and _is_nhwc(t):
        return t
    out = _nhwc_empty(*t.shape, dtype, t.device)
    out.copy_(t)
    return out


_workspaces = {}


def _workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch arena per (device, stream): reuse is stream-ordered, so every compute stream has
    its own arena (the two decoders of AnomalyUNet run on two streams)."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def _views(items) -> "L.View2":
    arr = L.View2()
    for i, it in enumerate(items):
        if it is None:
            arr[i] = L.View(None, 0, 0, 0, 0, 0)
        else:
            t, oy, ox = it
            arr[i] = L.View(t.data_ptr(), t.shape[1], t.shape[2], t.shape[3], oy, ox)
    return arr


def _pad64(c: int) -> int:
    return (c + 63) // 64 * 64


# ----------------------------------------------------------------------------- profiling
def prof_enable(on: bool) -> None:
    L.check(L.lib().unet_prof_enable(int(on)), "unet_prof_enable")


def prof_collect():
    ms = (C.c_double * L.K_COUNT)()
    launches = (C.c_int64 * L.K_COUNT)()
    flops = (C.c_double * L.K_COUNT)()
    L.check(L.lib().unet_prof_collect(ms, launches, flops), "unet_prof_collect")
    return {L.KCLASS_NAMES[i]: {"ms": ms[i], "launches": launches[i], "flops": flops[i]}
            for i in range(L.K_COUNT)}


def prof_kernels():
    """Per-kernel breakdown of the brackets consumed by the last prof_collect(): {kernel name: ms, launches, flops}."""
    out, i = {}, 0
    lib = L.lib()
    while True:
        name, ms, n, fl = C.c_char_p(), C.c_double(), C.c_int64(), C.c_double()
        if lib.unet_prof_kernel_stats(i, C.byref(name), C.byref(ms), C.byref(n), C.byref(fl)) != 0:
            break
        by = C.c_double()
        lib.unet_prof_kernel_bytes(i, C.byref(by))
        out[name.value.decode()] = {"ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value}
        i += 1
    return out
