"""ctypes binding of libunet_hip.so (C-ABI declared in include/unet_hip.h).

The header is the one statement of every entry point's signature: SIGNATURES (name -> restype, argtypes) is read from
its declarations when first asked for, by lib() or by name, and a new entry point needs nothing here.  Importing this
module reads no file.  The structures and enum values below are needed at import, so they restate the header by hand;
tests/test_cpu_abi.py holds them to it.

The library is the ONLY compute path of this package: there is no CPU or eager
PyTorch fallback.  If the shared object is missing or a call fails, a RuntimeError
is raised -- loudly -- instead of silently computing something else.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UNET_HIP_LIB") or os.path.join(_HERE, "libunet_hip.so")   # (override: diagnostic builds)
CSRC = os.path.join(_HERE, "csrc")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "unet_hip.h")

UNET_F32, UNET_BF16 = 0, 1
PACK_CONV_FWD, PACK_CONV_DGRAD, PACK_CONVT_FWD, PACK_CONVT_DGRAD = 0, 1, 2, 3
(K_CONV_FWD, K_CONV_DGRAD, K_CONV_WGRAD, K_CONVT_FWD, K_CONVT_DGRAD, K_CONVT_WGRAD, K_BN, K_POOL,
 K_HEAD, K_LOSS, K_PACK, K_OTHER, K_COUNT) = range(13)
KCLASS_NAMES = ["conv3x3_fwd", "conv3x3_dgrad", "conv3x3_wgrad", "convt_fwd", "convt_dgrad",
                "convt_wgrad", "bn", "pool_upsample", "head", "loss", "pack_layout", "other"]


class View(C.Structure):
    """struct unet_view"""
    _fields_ = [("ptr", C.c_void_p), ("c", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("off_y", C.c_int32), ("off_x", C.c_int32)]


View2 = View * 2


class RemapDesc(C.Structure):
    """struct unet_remap_desc"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32),
                ("inner", C.c_int32), ("prows", C.c_int32), ("pcols", C.c_int32), ("split", C.c_int32),
                ("op", C.c_int32), ("reserved", C.c_int32)]


REMAP_PAD, REMAP_UNPAD = 0, 1


class Panel(C.Structure):
    """struct unet_panel"""
    _fields_ = [("kind", C.c_int32), ("alpha8", C.c_int32), ("rgb", C.c_void_p), ("map", C.c_void_p)]


PANEL_IMAGE, PANEL_UNIT, PANEL_GRAY, PANEL_HOT, PANEL_OVERLAY = range(5)


class SegPanel(C.Structure):
    """struct unet_seg_panel"""
    _fields_ = [("kind", C.c_int32), ("alpha8", C.c_int32), ("labels", C.c_void_p), ("map", C.c_void_p)]


SEG_PANEL_IMAGE, SEG_PANEL_CLASSES, SEG_PANEL_OVERLAY, SEG_PANEL_LUT = range(4)


class CropDesc(C.Structure):
    """struct unet_crop_desc"""
    _fields_ = [("image", C.c_int32), ("a", C.c_int32 * 6), ("reserved", C.c_int32)]


CROP_NEAREST, CROP_BILINEAR = 0, 1


class PasteDesc(C.Structure):
    """struct unet_paste_desc"""
    _fields_ = [("image", C.c_int32), ("b", C.c_int32 * 6), ("box", C.c_int32 * 4), ("dst", C.c_int32 * 4),
                ("reserved", C.c_int32)]


class MergeView(C.Structure):
    """struct unet_merge_view"""
    _fields_ = [("logits", C.c_void_p), ("h", C.c_int32), ("w", C.c_int32), ("flip_x", C.c_int32), ("flip_y", C.c_int32)]


_SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double,
            "size_t": C.c_size_t}
_DECLARATION = re.compile(r"((?:\bconst\s+)?\b\w+[\s*]+)(unet_[a-z0-9_]+)\s*\(([^;{()]*)\)\s*;")


def _ctype(spec: str, is_param: bool):
    """One return type, or one parameter with or without its name, through the closed table; None outside it."""
    words = re.sub(r"\bconst\b|\*|\[\d*\]", " ", spec).split()
    if "*" in spec or "[" in spec:
        if is_param and words:
            return C.POINTER(View) if words[0] == "unet_view" else C.c_void_p
        return C.c_char_p if "".join(spec.split()) == "constchar*" else None
    return _SCALARS.get(words[0]) if 1 <= len(words) <= 1 + is_param else None


def read_signatures(header: str) -> dict:
    """name -> (restype, argtypes) of every `ret unet_name(params);` in the text of a header.  A type outside the
    table above is never guessed: it is an error that quotes the declaration, for whoever adds the type to extend it."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)     # preprocessor lines, macros among them
    signatures = {}
    for decl in _DECLARATION.finditer(text):
        ret, name, params = decl.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        specs = [(ret, False)] + [(p, True) for p in params]
        types = [_ctype(spec, is_param) for spec, is_param in specs]
        if None in types:
            raise RuntimeError(f"no ctypes type for `{specs[types.index(None)][0].strip()}` in the declaration "
                               f"`{' '.join(decl.group(0).split())}`: extend the table of _lib.py")
        signatures[name] = (types[0], types[1:])
    return signatures


@functools.lru_cache(maxsize=None)
def _signatures() -> dict:
    if not os.path.exists(HEADER):
        raise RuntimeError(
            f"unet_hip.h not found at {HEADER}: it is the one statement of the library's signatures, and the binding "
            "of libunet_hip.so reads every restype and argtypes from it.")
    with open(HEADER) as f:
        return read_signatures(f.read())


def __getattr__(name):
    if name == "SIGNATURES":        # name -> (restype, argtypes): every symbol the header declares, read on first use
        return _signatures()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


_lib = None


def build(force: bool = False) -> str:
    """Compile libunet_hip.so for gfx950 with hipcc (csrc/Makefile).  Cross-compiles without a GPU."""
    if force or not os.path.exists(LIB_PATH) or _stale():
        subprocess.run(["make", "-C", CSRC, "-j8"], check=True, stdout=subprocess.DEVNULL)
    return LIB_PATH


def _stale() -> bool:
    if not os.path.isdir(CSRC):
        return False
    t = os.path.getmtime(LIB_PATH)
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(HEADER)
    return any(os.path.exists(s) and os.path.getmtime(s) > t for s in srcs)


def lib():
    """The loaded library; raises if it cannot be loaded (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libunet_hip.so not found at {LIB_PATH}: the HIP extension is the only compute path of "
                "tiaozhanbei_unet_amd (no CPU/eager fallback). Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C tiaozhanbei_unet_amd/csrc`.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _signatures().items():
            fn = getattr(handle, name)      # AttributeError if the .so does not export it
            fn.restype, fn.argtypes = res, args
        if handle.unet_abi_version() != 1:
            raise RuntimeError("libunet_hip.so: ABI version mismatch")
        _lib = handle
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().unet_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (status {rc}): {msg}")
