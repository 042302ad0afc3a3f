"""CPU: the ctypes binding is derived from include/flair_hip.h (flair_amd/_header.py) and every entry call is typed.

The struct layouts are compared with what a C compiler makes of the header, the prototype table with an independent regex
and with five prototypes written out here, and the refusals of ``_lib.call.flair_x(...)`` are exercised without a device."""
import ctypes
import glob
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

from flair_amd import _header, _lib, ops
from tests.test_abi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"flair_conv_params": 112, "flair_chain_params": 92, "flair_gn_params": 64, "flair_sampler_coefs": 56,
         "flair_attn_params": 48, "flair_tattn_params": 44, "flair_dcn_params": 52}


def _c_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [shutil.which("cc"), shutil.which("gcc"), shutil.which("clang")]
    found += sorted(glob.glob(os.path.join(rocm, "llvm", "bin", "clang")) + glob.glob(os.path.join(rocm, "lib", "llvm", "bin", "clang")))
    found = [c for c in found if c]
    assert found, "no C compiler (cc, gcc, clang or ROCm's clang) to check the struct layouts with"
    return found[0]


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    """sizeof and every offsetof of the 7 parameter structs, printed by a C program that includes the header, equal
    ctypes' (flair_sampler_coefs holds a long behind ten 4-byte fields, so padding is exercised)."""
    assert set(_header.STRUCTS) == set(SIZES)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "flair_hip.h"', 'int main(void) {']
    for name, cls in _header.STRUCTS.items():
        lines.append(f'    printf("{name} sizeof %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'    printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([_c_compiler(), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {(s, f): int(v) for s, f, v in (line.split() for line in out.splitlines())}
    want = {}
    for name, cls in _header.STRUCTS.items():
        want[(name, "sizeof")] = ctypes.sizeof(cls)
        for field, _ in cls._fields_:
            want[(name, field)] = getattr(cls, field).offset
    assert got == want
    assert {n: got[(n, "sizeof")] for n in SIZES} == SIZES


def test_struct_names_are_the_derived_classes():
    S = _header.STRUCTS
    assert _lib.ConvParams is ops.ConvParams is S["flair_conv_params"] and ops.ChainParams is S["flair_chain_params"]
    assert ops.GnParams is S["flair_gn_params"] and ops.SamplerCoefs is S["flair_sampler_coefs"]
    assert ops.AttnParams is S["flair_attn_params"] and ops.TAttnParams is S["flair_tattn_params"]
    assert ops.DcnParams is S["flair_dcn_params"]
    conv = dict(ops.ConvParams._fields_)
    assert conv["seg_c"] is ctypes.c_int * 4 and conv["res_ld"] is ctypes.c_int * 2 and conv["out_scale"] is ctypes.c_float
    assert dict(ops.SamplerCoefs._fields_)["frame_elems"] is ctypes.c_long and ops.SamplerCoefs.frame_elems.offset == 40


def test_every_declared_entry_is_typed():
    names = declared_symbols()
    assert sorted(_header.PROTOS) == names and len(names) == 75
    lib = _lib.lib()
    for name, (restype, params) in _header.PROTOS.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == len(params), name
        assert f.restype is restype, name
    assert {n for n, (r, _) in _header.PROTOS.items() if r is ctypes.c_size_t} == {
        "flair_conv_workspace_bytes", "flair_groupnorm_workspace_bytes", "flair_instnorm_workspace_bytes",
        "flair_image_metrics_workspace"}
    assert [n for n, (r, _) in _header.PROTOS.items() if r is ctypes.c_char_p] == ["flair_last_error"]


def test_five_prototypes_written_out_by_hand():
    """The type mapping, pinned without the parser: (name, ctypes type, pointed-to C type) per parameter."""
    i, l, f, d, z, v = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double, ctypes.c_size_t, ctypes.c_void_p
    S = _header.STRUCTS
    by_hand = {
        "flair_conv_nhwc": [("p", ctypes.POINTER(S["flair_conv_params"]), "flair_conv_params"), ("x", v, "void*"), ("w", v, "void"),
                            ("bias", v, "float"), ("frame_bias", v, "float"), ("res0", v, "void"), ("res1", v, "void"),
                            ("y", v, "void"), ("workspace", v, "void"), ("workspace_bytes", z, None), ("stream", v, None)],
        "flair_axpby_f32": [("x", v, "float"), ("y", v, "float"), ("a", f, None), ("b", f, None), ("lo", f, None), ("hi", f, None),
                            ("n", l, None), ("out", v, "float"), ("stream", v, None)],
        "flair_instnorm_nhwc": [("x", v, "float"), ("x_ld", i, None), ("F", i, None), ("H", i, None), ("W", i, None), ("C", i, None),
                                ("eps", d, None), ("act", i, None), ("y", v, "float"), ("y_ld", i, None), ("workspace", v, "void"),
                                ("workspace_bytes", z, None), ("stream", v, None)],
        "flair_slomo_blend": [("pair", v, "void"), ("pair_ld", i, None), ("flow", v, "void"), ("flow_ld", i, None), ("io", v, "void"),
                              ("io_ld", i, None), ("dtype", i, None), ("B", i, None), ("H", i, None), ("W", i, None),
                              ("c0", f, None), ("c1", f, None), ("c2", f, None), ("c3", f, None), ("t", d, None),
                              ("mean", v, "float"), ("out", v, "float"), ("out_batch_stride", l, None), ("stream", v, None)],
        "flair_corr_lookup": [("corr", v, "float*"), ("corr_t", v, "float*"), ("level_h", v, "int"), ("level_w", v, "int"),
                              ("levels", i, None), ("flow", v, "float"), ("flow_ld", i, None), ("B", i, None), ("h", i, None),
                              ("w", i, None), ("scale_corr", f, None), ("scale_corr_t", f, None), ("out", v, "float"),
                              ("out_ld", i, None), ("stream", v, None)],
    }
    lib = _lib.lib()
    for name, want in by_hand.items():
        restype, params = _header.PROTOS[name]
        assert restype is ctypes.c_int and [tuple(p) for p in params] == want, name
        assert list(getattr(lib, name).argtypes) == [t for _, t, _ in want], name


@pytest.mark.parametrize("text, word", [
    ("int flair_a(int n, unsigned m, hipStream_t stream);", "unsigned"),
    ("short flair_a(int n);", "short"),
    ("typedef struct { int a; char b; } flair_x_params;", "char b"),
    ("typedef struct { int a[N]; } flair_x_params;", "a[N]"),
    ("typedef union { int a; } flair_u;", "union"),
    ("int flair_a(int n)", "flair_a"),
    ("int flair_a(int n); int flair_a(int n);", "twice"),
])
def test_parser_raises_on_what_it_does_not_understand(text, word):
    good = 'extern "C" {\ntypedef struct { int a, b[2]; float c; } flair_x_params;\nint flair_b(const flair_x_params* p);\n%s\n}'
    structs, protos = _header.parse(good % "")
    assert list(structs) == ["flair_x_params"] and list(protos) == ["flair_b"]
    with pytest.raises(_header.HeaderError, match=re.escape(word)):
        _header.parse(good % text)


def test_unknown_struct_field_is_refused():
    for cls in _header.STRUCTS.values():
        p = cls()
        with pytest.raises(AttributeError):
            p.some_typo = 3
    p = ops.TAttnParams()
    p.head_dim = 64
    with pytest.raises(AttributeError):
        p.head_dims = 64


def _device_tensor(dtype):
    """Stands in for a tensor in HBM: call() looks at is_cuda, dtype and data_ptr() only."""
    return types.SimpleNamespace(is_cuda=True, dtype=dtype, data_ptr=lambda: 1 << 20)


def test_call_refusals():
    call, x = _lib.call, torch.zeros(8)
    with pytest.raises(_lib.FlairHipError, match="need tensors resident in HBM"):
        call.flair_axpby_f32(x, None, 1.0, 0.0, 0.0, 1.0, 8, x)
    f32, bf16 = _device_tensor(torch.float32), _device_tensor(torch.bfloat16)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_prelu_nhwc: slope must be float32, got bfloat16$"):
        call.flair_prelu_nhwc(f32, 4, None, 0, bf16, 4, 1, f32, 4)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_block_luma_sums: out must be int64, got float32$"):
        call.flair_block_luma_sums(_device_tensor(torch.uint8), 1, 8, 8, f32)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_face_mask_blur: parse_idx must be int32, got int64$"):
        call.flair_face_mask_blur(_device_tensor(torch.int64), 1, 8, 8, None, 0, None, 0, 2, 10, 255.0, None, None)
    with pytest.raises(AttributeError, match="flair_no_such_entry is not an entry"):
        call.flair_no_such_entry(x)
    for query in ("flair_abi_version", "flair_conv_variant", "flair_conv_workspace_bytes", "flair_last_error"):
        with pytest.raises(AttributeError, match="not an entry of flair_hip.h that launches"):
            getattr(call, query)
    with pytest.raises(TypeError, match="flair_corr_scale takes 3 arguments"):
        call.flair_corr_scale(f32, 8)


def test_a_void_pointer_takes_any_dtype_and_the_status_is_checked(monkeypatch):
    """Through call() to the library and back without a device: the entry refuses its arguments before it launches."""
    monkeypatch.setattr(_lib, "stream", lambda: None)
    bf16 = _device_tensor(torch.bfloat16)
    with pytest.raises(_lib.FlairHipError, match=r"^flair_flow_warp failed \(status -1\): .*x_ld"):
        _lib.call.flair_flow_warp(bf16, _lib.FLAIR_BF16, 4, _device_tensor(torch.float32), 2, 1, 8, 8, 8, False, bf16, 8)


def test_scalars_convert_through_argtypes():
    lib = _lib.lib()
    P = ctypes.c_void_p(1 << 20)
    with pytest.raises(ctypes.ArgumentError):
        lib.flair_corr_pool(P, 4, 8.0, 8, P, None)                 # a float for `int h`
    with pytest.raises(ctypes.ArgumentError):
        lib.flair_corr_scale(P, 4.0, 2.0, None)                    # a float for `long n`
    assert lib.flair_corr_scale(P, 4, 0, None) == -1 and b"divisor" in lib.flair_last_error()      # an int for `float divisor`
    assert lib.flair_corr_pool(P, 4, True, 8, P, None) == -1 and b"h = 1" in lib.flair_last_error()  # a flag is an int
    assert lib.flair_instnorm_workspace_bytes(2, 16, 18, 64) == 2 * 64 * 8 + 2 * 2 * 64 * 4        # size_t, not a truncated int


def test_ops_spells_no_binding_by_hand():
    """ops.py holds no struct mirror, no restype and no per-argument scalar wrapper; the one c_double is the FLOP count that
    flair_probe_matrix_rate writes."""
    src = open(os.path.join(ROOT, "flair_amd", "ops.py")).read()
    for word in ("ctypes.Structure", "restype", "c_float(", "c_long(", "c_size_t("):
        assert word not in src, word
    assert src.count("c_double(") == 1
    # what goes through lib() directly returns a value, not a status
    assert set(re.findall(r"\blib\(\)\.(flair_\w+)", src)) == {
        "flair_conv_variant", "flair_conv_workspace_bytes", "flair_groupnorm_workspace_bytes", "flair_instnorm_workspace_bytes",
        "flair_image_metrics_workspace"}
    assert not re.search(r"\bcheck\(", src)
