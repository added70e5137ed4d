"""The C-ABI library loads (no GPU needed) and exports every symbol include/strongsort_hip.h declares."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from strongsort_yolo_amd import cheader, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "strongsort_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ss_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib.build()
    L = ctypes.CDLL(lib.SO_PATH)
    names = _declared()
    assert len(names) >= 25
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    assert sorted(names) == sorted(lib.EXPORTS)          # the ctypes binding covers the whole header
    assert "ss_cmc_estimate" in names and "ss_cmc_get_small" in names


def test_library_exports_only_declared_symbols():
    """Nothing under the ss_ prefix leaves the library that the header does not declare."""
    if shutil.which("nm") is None:
        pytest.skip("nm is not installed: the library's symbol table cannot be listed")
    lib.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], check=True, capture_output=True, text=True).stdout
    defined = sorted({line.split()[-1].split("@")[0] for line in out.splitlines() if line.split()[-1].startswith("ss_")})
    assert defined == _declared()


def test_config_struct_matches_header():
    src = open(os.path.join(ROOT, "include", "strongsort_hip.h")).read()
    body = src[src.index("typedef struct ss_config {"):src.index("} ss_config;")]
    fields = re.findall(r"^\s*(double|float|int)\s+(\w+);", body, flags=re.M)
    ctype = {"double": ctypes.c_double, "float": ctypes.c_float, "int": ctypes.c_int}
    assert [(n, ctype[t]) for t, n in fields] == [(n, t) for n, t in lib.ss_config._fields_]


def test_error_without_gpu_is_loud():
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from strongsort_yolo_amd.engine import TrackerEngine
    with pytest.raises(lib.SSError):
        TrackerEngine()


def test_host_side_entry_points_without_a_gpu():
    """Entry points that only compute on the host or validate arguments: callable on a CPU-only box."""
    lib.build()
    L = lib.load()
    assert L.ss_max_group_frames() == 32
    assert L.ss_cmc_get_small(None, 0, 0, None, 0, None, None) == lib.SS_ERR_INVALID                        # null context
    # band count of the LightConv chain launches: LDS form (16-row bands) below 96 images, the row-stream form sizes its bands
    # for one round of waves (32-wide: 3072 waves = images x bands x 2 chain groups), at least 8 rows per band
    assert L.ss_op_osnet_streams_bands(32, 64, 32, 16) == 4
    assert L.ss_op_osnet_streams_bands(512, 64, 32, 16) == 3
    assert L.ss_op_osnet_streams_bands(1024, 64, 32, 16) == 1
    assert L.ss_op_osnet_streams_bands(128, 64, 32, 16) == 8
    assert L.ss_op_osnet_streams_bands(512, 32, 16, 24) == 2
    assert L.ss_op_osnet_streams_bands(512, 16, 8, 32) == 2            # 8-wide maps: two images per wave, 256 units
    assert L.ss_op_osnet_streams_bands(32, 16, 8, 32) == 1             # below 96 images: the LDS form, whole 16-row bands
    assert L.ss_op_osnet_streams_bands(0, 64, 32, 16) < 0
    assert L.ss_op_set_valid_images(None, None, 0) == 0 and L.ss_op_set_valid_images(None, None, 5) == 0       # NULL count: off
    assert L.ss_op_set_option(b"pw_splitk", 1) == 0 and L.ss_op_set_option(b"no_such_switch", 1) == lib.SS_ERR_INVALID
    assert L.ss_op_conv_group_f16(None, 0, None) < 0                    # n out of range / no descriptors
    d = (lib.ss_conv_desc * 1)()
    assert L.ss_op_conv_group_f16(None, 1, d) < 0                       # null tensors
    assert L.ss_op_upcat_f16(None, None, None, None, 1, 4, 4, 8, 8, 1) < 0
    assert L.ss_op_sppf_pools_f16(None, None, None, 1, 40, 40, 8) < 0   # H*W > 1024 (and null tensors)
    assert L.ss_op_conv0_f16(None, None, None, None, None, 1, 8, 100, 16, 2) < 0
    assert L.ss_op32_conv_plan(1, 8, 8, 16, 16, 3, 1, None, None, None, None) < 0      # null results; with them it plans on the host: test_f32_ref_cpu.py


def test_pooling_depthwise_and_attention_entries_refuse_bad_extents_before_any_launch():
    """ss_op_maxpool_f16, ss_op_dwconv3x3_f16 and ss_op_psa_attention_f16 check their extents before they launch: dummy non-null pointers
    (never read: the refusal comes first) single out the argument that is refused.  A window wider than the padded map has no output -
    two negative extents used to multiply to a large positive element count - and 2 * pad > k lets a window lie wholly in the padding."""
    lib.build()
    L = lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    INV = lib.SS_ERR_INVALID
    pool = lambda N=1, H=4, W=4, C=8, k=3, s=1, pad=1, x=p, y=p: L.ss_op_maxpool_f16(None, x, y, N, H, W, C, k, s, pad)
    assert pool(x=None) == INV and pool(y=None) == INV                                      # (the null-argument calls, as before)
    for bad in (dict(N=0), dict(H=0), dict(W=0), dict(N=-1), dict(C=0), dict(C=12), dict(k=0), dict(s=0), dict(pad=-1),
                dict(k=3, pad=2),                          # 2 * pad > k: the corner window holds padding alone
                dict(H=2, W=2, k=5, pad=1),                # OH = OW = (2 + 2 - 5) / 1 + 1 = 0
                dict(H=1, W=1, k=7, pad=2),                # both extents negative: their product was a positive count
                dict(H=1, W=1, k=4, pad=1, s=2),           # (1 + 2 - 4) / 2 truncates to 0 in C: OH would read 1
                dict(H=4, W=1, k=5, pad=1)):               # one extent only
        assert pool(**bad) == INV, bad
    dw = lambda N=1, H=4, W=4, C=8, act=1, x=p, w=p, b=p, y=p: L.ss_op_dwconv3x3_f16(None, x, w, b, y, N, H, W, C, act)
    assert dw(x=None) == INV and dw(w=None) == INV and dw(b=None) == INV and dw(y=None) == INV
    for bad in (dict(N=0), dict(H=0), dict(W=0), dict(H=-3), dict(C=0), dict(C=12), dict(act=-1), dict(act=4)):
        assert dw(**bad) == INV, bad
    att = lambda B=1, N=16, heads=2: L.ss_op_psa_attention_f16(None, p, None, p, B, N, heads, 1.0)
    for bad in (dict(N=257), dict(N=0), dict(heads=0), dict(heads=65), dict(B=0)):
        assert att(**bad) == INV, bad


# ---- the binding is derived from the header (strongsort_yolo_amd/cheader.py): checked here with regular expressions of the test's own

_CTYPE = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong, "void": None,
          "const char*": ctypes.c_char_p, "const void*": ctypes.c_void_p, "void*": ctypes.c_void_p}


def _header_code():
    src = open(os.path.join(ROOT, "include", "strongsort_hip.h")).read()
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", src, flags=re.S)


def _prototypes():
    """name -> (return type, parameter texts) of every function declaration."""
    protos = {m.group(2): (" ".join(m.group(1).split()).replace(" *", "*"), [] if m.group(3).strip() == "void" else m.group(3).split(","))
              for m in re.finditer(r"^([A-Za-z][\w \t*]*?)\s*\b(ss_\w+)\s*\(([^()]*)\)\s*;", _header_code(), flags=re.M)}
    assert len(protos) >= 130 and "ss_cmc_get_small" in protos
    return protos


def test_every_function_has_the_declared_argument_count_and_return_type():
    lib.build()
    L = lib.load()
    protos = _prototypes()
    assert sorted(protos) == sorted(lib.EXPORTS)
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        assert fn.restype is _CTYPE[ret], (name, ret, fn.restype)
    assert ctypes.sizeof(L.ss_op_dwtab_bytes.restype) == 8 and ctypes.sizeof(L.ss_jpeg_encode_bound.restype) == 8


# sizes by natural alignment: ss_config 8 doubles + 5 ints = 84, padded to its 8-byte alignment; ss_byte_config 6 doubles + 6 ints;
# ss_conv_desc 4 pointers + 8 ints; ss_native_map 1 pointer + 3 long long + 3 ints = 44, padded to 48
@pytest.mark.parametrize("name,size", [("ss_config", 88), ("ss_byte_config", 72), ("ss_conv_desc", 64), ("ss_native_map", 48)])
def test_struct_matches_header_field_by_field(name, size):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header_code(), flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        t, names = re.fullmatch(r"((?:const )?(?:long long|\w+)\*?)\s+(\w+(?:\s*,\s*\w+)*)", decl).groups()
        fields += [(n.strip(), _CTYPE[t]) for n in names.split(",")]
    struct = getattr(lib, name)
    assert issubclass(struct, ctypes.Structure) and struct.__name__ == name
    assert fields == [(n, t) for n, t in struct._fields_]
    assert ctypes.sizeof(struct) == size


def test_constants_come_from_the_header():
    defines = {n: int(v) for n, v in re.findall(r"^#define (SS_\w+) \(?(-?\d+)\)?", _header_code(), flags=re.M)}
    assert len(defines) == 12
    for n, v in defines.items():
        assert getattr(lib, n if n == "SS_OK" or n.startswith("SS_ERR_") else n[3:]) == v, n


@pytest.mark.parametrize("text", [
    "int ss_f(ss_ctx* ctx, __half* d_x);",                 # a type the header does not use
    "int ss_f(wchar_t n);",
    "int ss_f(int a, int (*cb)(int));",                    # not flat
    "int ss_f(int a;",                                     # unbalanced parenthesis
    "int ss_f(int a));",
    "int ss_f(int);",                                      # a parameter without a name
    "int ss_f(ss_config cfg);",                            # a struct by value
    "int ss_f(int*** p);",
    "int ss_f(int a)",                                     # no semicolon
    "#define SS_X (1 << 3)",
    "typedef struct ss_s { int a[4]; } ss_s;",
    "typedef int ss_int;",
    "static int ss_x = 3;",
    "int ss_f(int a); int ss_f(int a);",                   # declared twice
])
def test_parser_raises_on_what_it_cannot_classify(text):
    prefix = "typedef struct ss_ctx ss_ctx;\ntypedef struct ss_config { int a; } ss_config;\n"
    assert cheader.Header(prefix + "int ss_f(ss_ctx* ctx, const ss_config* cfg, const float* d_x);").functions["ss_f"][1][2] is ctypes.c_void_p
    with pytest.raises(cheader.HeaderError):
        cheader.Header(prefix + text)


def test_typed_host_pointers_reject_the_wrong_array():
    """Host scalar pointers stay typed: ctypes refuses the call before the library sees it (no GPU call is made)."""
    lib.build()
    L = lib.load()
    assert L.ss_nms_set_classes.argtypes[1] == ctypes.POINTER(ctypes.c_int)
    with pytest.raises(ctypes.ArgumentError):
        L.ss_nms_set_classes(None, (ctypes.c_float * 4)(), 4)
    with pytest.raises(ctypes.ArgumentError):
        L.ss_gsi_smooth(None, 1, (ctypes.c_int * 2)(0, 1), (ctypes.c_int * 1)(), (ctypes.c_float * 4)(), None, 0.0, None, None)
    with pytest.raises(ctypes.ArgumentError):
        L.ss_op_conv_group_f16(None, 1, (lib.ss_native_map * 1)())
    assert L.ss_nms_set_classes(None, (ctypes.c_int * 4)(), 4) == lib.SS_ERR_INVALID      # the right type reaches the library: null context
