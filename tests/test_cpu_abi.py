"""The seam between include/unet_hip.h and the ctypes binding (no GPU): _lib.read_signatures on small header texts, a
hand-pinned witness for rows of the real header where a mix-up is possible, the binding of every declared symbol, and
the structures and enum values that _lib.py restates by hand, each held to the header by a parser of this file's own."""
import ctypes
import functools
import os
import re
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_void_p

import pytest

from conftest import ROOT
from tiaozhanbei_unet_amd import _lib
from tiaozhanbei_unet_amd._lib import View

HEADER = os.path.join(ROOT, "include", "unet_hip.h")


def test_reader_maps_each_form_of_declaration():
    got = _lib.read_signatures("""
        /* a block comment that names int32_t unet_not_declared(double x); */
        // and a line comment: float unet_neither(void);
        #define UNET_MAX 8
        #define UNET_CALL(x) \\
            int32_t unet_in_a_macro(int32_t x);
        typedef struct unet_view { void* ptr; int32_t c; } unet_view;
        static inline int32_t pad64(int32_t c) { return (c + 63) / 64 * 64; }
        static inline int32_t unet_inline_helper(int32_t c) { return pad64(c); }
        int32_t unet_pointers(const float* src, void* dst, const char** name, int64_t* counts, const uint8_t* select);
        int32_t unet_arrays(const int32_t hw[2], float taps[], const unet_view src[2], const unet_view* dst, unet_view* v);
        int32_t unet_widths(int64_t pixels, int32_t c, int64_t, int32_t);
        int32_t unet_reals(float lr, double beta1, double beta2, float eps);
        size_t unet_bytes(size_t have, const int32_t n);
        const char* unet_text(void);
        const char *unet_text2( );
        int32_t
        unet_spread(int32_t dtype,   /* the compute dtype, not a double */
                    const void* x,   // NHWC; int64_t strides
                    int64_t pixels,
                    void* stream);
    """)
    pv = POINTER(View)
    assert got == {
        "unet_pointers": (c_int32, [c_void_p] * 5),
        "unet_arrays": (c_int32, [c_void_p, c_void_p, pv, pv, pv]),
        "unet_widths": (c_int32, [c_int64, c_int32, c_int64, c_int32]),
        "unet_reals": (c_int32, [c_float, c_double, c_double, c_float]),
        "unet_bytes": (c_size_t, [c_size_t, c_int32]),
        "unet_text": (c_char_p, []),
        "unet_text2": (c_char_p, []),
        "unet_spread": (c_int32, [c_int32, c_void_p, c_int64, c_void_p]),
    }
    assert list(got) == ["unet_pointers", "unet_arrays", "unet_widths", "unet_reals", "unet_bytes", "unet_text",
                         "unet_text2", "unet_spread"]                      # (header order)


@pytest.mark.parametrize("decl, culprit", [
    ("int32_t unet_odd(int32_t n, uint32_t seed, void* stream);", "uint32_t seed"),       # an unknown scalar
    ("int32_t unet_odd(unsigned int n);", "unsigned int n"),
    ("int32_t unet_odd(unet_view v);", "unet_view v"),                                    # a structure by value
    ("uint64_t unet_odd(void);", "uint64_t"),                                             # an unknown return type
    ("void* unet_odd(int32_t n);", "void*"),                                              # a pointer that is no text
    ("char* unet_odd(void);", "char*"),
])
def test_reader_refuses_a_type_outside_its_table(decl, culprit):
    """Never a guess: the error quotes the type and the whole declaration."""
    with pytest.raises(RuntimeError) as e:
        _lib.read_signatures("int32_t unet_fine(int32_t n);\n" + decl.replace(", ", ",\n    "))
    assert f"`{culprit}`" in str(e.value) and f"`{decl}`" in str(e.value), str(e.value)


def test_witness_rows_of_the_real_header():
    """SIGNATURES comes from the header, so comparing the two compares the header with itself.  These rows were written
    by hand, position by position, for the declarations that mix 32- and 64-bit integers, float and double, size_t
    and the two unet_view positions: a reader that confuses any pair of them fails here."""
    i, l, f, d, z, p, pv = c_int32, c_int64, c_float, c_double, c_size_t, c_void_p, POINTER(View)
    witness = {
        "unet_adam_multi": (i, [p, p, i, f, d, d, f, f, f, i, i, p]),
        "unet_adam_step": (i, [p, p, p, p, l, f, d, d, f, f, f, i, p]),
        "unet_region_auc": (i, [p, l, p, l, l, l, d, p, p, z, p]),
        "unet_bn_finalize_partials": (i, [p, i, l, i, p, p, p, p, f, f, p, p, p, p, p]),
        "unet_seg_loss": (i, [p, p, i, i, l, p, l, i, f, f, f, f, f, p, p, p, z, p]),
        "unet_conv3x3": (i, [i, i, i, i, pv, p, i, pv, i, i, i, p]),
        "unet_last_error": (c_char_p, []),
        "unet_conv3x3_wgrad_workspace": (z, [i, i, i, i, i]),
        "unet_rank_auc_workspace": (z, [l, l]),
    }
    for name, row in witness.items():
        assert _lib.SIGNATURES[name] == row, name


def test_every_declared_symbol_is_bound_with_its_signature():
    lib = _lib.lib()
    assert len(_lib.SIGNATURES) >= 136
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_header_is_read_once_and_a_missing_one_is_named(monkeypatch, tmp_path):
    """The parse happens on first use and once per process, whoever asks first; without the header both lib() and
    SIGNATURES say which path they looked for."""
    reads = []
    real = _lib.read_signatures
    monkeypatch.setattr(_lib, "read_signatures", lambda text: reads.append(1) or real(text))
    monkeypatch.setattr(_lib, "_lib", None)                 # (a first lib() call; the loaded handle comes back below)
    _lib._signatures.cache_clear()
    try:
        first = _lib.SIGNATURES
        assert _lib.SIGNATURES is first and len(reads) == 1
        handle = _lib.lib()
        assert _lib.lib() is handle and len(reads) == 1
        assert handle.unet_abi_version() == 1

        gone = str(tmp_path / "include" / "unet_hip.h")
        monkeypatch.setattr(_lib, "HEADER", gone)
        monkeypatch.setattr(_lib, "_lib", None)
        _lib._signatures.cache_clear()
        with pytest.raises(RuntimeError, match="unet_hip.h not found at " + re.escape(gone)):
            _lib.SIGNATURES
        with pytest.raises(RuntimeError, match="unet_hip.h not found at " + re.escape(gone)):
            _lib.lib()
    finally:
        _lib._signatures.cache_clear()
    with pytest.raises(AttributeError):
        _lib.NO_SUCH_NAME


# ---- the mirrors _lib.py keeps by hand: needed at import, so not derived, but held to the header here -----------------

@functools.lru_cache(maxsize=None)
def _header_blocks():
    """(structs, enums) of the real header: {struct name: [(field, ctypes type)]} and {enum name: {enumerator: value}}."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(HEADER).read(), flags=re.S)
    scalars = {"int32_t": c_int32, "int64_t": c_int64, "uint32_t": ctypes.c_uint32, "float": c_float,
               "double": c_double}
    structs = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S):
        fields = structs[name] = []
        for statement in filter(None, (s.strip() for s in body.split(";"))):
            base, declarators = re.match(r"((?:const\s+)?\w+[\s*]+)(.*)$", statement, flags=re.S).groups()
            for declarator in declarators.split(","):
                field, length = re.match(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*$", declarator).groups()
                ctype = c_void_p if "*" in base else scalars[base.replace("const", "").strip()]
                fields.append((field, ctype * int(length) if length else ctype))
    enums = {}
    for name, body in re.findall(r"enum\s+(\w+)\s*\{(.*?)\}", text, flags=re.S):
        values, following = {}, 0
        for enumerator in filter(None, (e.strip() for e in body.split(","))):
            key, _, value = (part.strip() for part in enumerator.partition("="))
            values[key] = following = int(value, 0) if value else following
            following += 1
        enums[name] = values
    return structs, enums


def _c_sizeof(fields):
    """sizeof by the C rule, worked out apart from ctypes: every member at a multiple of its own alignment, the whole a
    multiple of the largest alignment."""
    end, widest = 0, 1
    for _, ctype in fields:
        align = ctypes.sizeof(getattr(ctype, "_type_", ctype) if hasattr(ctype, "_length_") else ctype)
        end = -(-end // align) * align + ctypes.sizeof(ctype)
        widest = max(widest, align)
    return -(-end // widest) * widest


MIRRORS = {"unet_view": _lib.View, "unet_remap_desc": _lib.RemapDesc, "unet_panel": _lib.Panel,
           "unet_seg_panel": _lib.SegPanel, "unet_crop_desc": _lib.CropDesc, "unet_paste_desc": _lib.PasteDesc,
           "unet_merge_view": _lib.MergeView}


@pytest.mark.parametrize("struct", sorted(MIRRORS))
def test_structure_mirrors_the_header(struct):
    declared = _header_blocks()[0][struct]
    mirror = MIRRORS[struct]
    assert mirror._fields_ == declared                       # names, order, types; `int32_t a[6]` is c_int32 * 6
    assert ctypes.sizeof(mirror) == _c_sizeof(declared)
    assert not hasattr(mirror, "_pack_")


def test_header_parser_of_this_file_reads_what_it_should():
    """The parser above on forms whose answer is known without it."""
    structs, enums = _header_blocks()
    assert structs["unet_view"] == [("ptr", c_void_p), ("c", c_int32), ("h", c_int32), ("w", c_int32),
                                    ("off_y", c_int32), ("off_x", c_int32)]
    assert structs["unet_crop_desc"] == [("image", c_int32), ("a", c_int32 * 6), ("reserved", c_int32)]
    assert _c_sizeof(structs["unet_view"]) == 32 and _c_sizeof(structs["unet_paste_desc"]) == 64
    assert _c_sizeof(structs["unet_adam_chunk"]) == 16 and _c_sizeof(structs["unet_adam_desc"]) == 40
    assert enums["unet_status"] == {"UNET_OK": 0, "UNET_ERR_BAD_ARG": -1, "UNET_ERR_UNSUPPORTED": -2,
                                    "UNET_ERR_WORKSPACE": -3, "UNET_ERR_LAUNCH": -4}
    assert enums["unet_kclass"]["UNET_K_CONV_FWD"] == 0 and enums["unet_kclass"]["UNET_K_CONV_DGRAD"] == 1
    assert enums["unet_kclass"]["UNET_K_COUNT"] == 12        # (counted on from the one explicit value)


@pytest.mark.parametrize("enum, prefix", [("unet_dtype", "UNET_"), ("unet_pack_mode", "PACK_"), ("unet_kclass", "K_"),
                                          ("unet_remap_op", "REMAP_"), ("unet_panel_kind", "PANEL_"),
                                          ("unet_seg_panel_kind", "SEG_PANEL_")])
def test_constants_restate_the_header_enum(enum, prefix):
    """Both ways: every constant of _lib.py with the prefix is an enumerator with that value, and every enumerator is
    restated."""
    declared = {key[len("UNET_"):] if prefix != "UNET_" else key: value
                for key, value in _header_blocks()[1][enum].items()}
    restated = {key: value for key, value in vars(_lib).items()
                if key.startswith(prefix) and key.isupper() and type(value) is int}
    assert restated == declared and len(declared) >= 2


def test_kernel_class_names_cover_the_classes():
    assert len(_lib.KCLASS_NAMES) == _lib.K_COUNT == _header_blocks()[1]["unet_kclass"]["UNET_K_COUNT"]
