"""ctypes binding of libflair_hip.so, derived from the C ABI's own headers (include/flair_hip.h, the evaluation-only
include/flair_eval.h, the no-reference include/flair_noref.h, the identity score's include/flair_ident.h, the flow-warping
error's include/flair_temporal.h, the face score's include/flair_facescore.h, the video streams' include/flair_yuv.h and tiled
denoising's include/flair_tile.h, read by _header.py).

The library is the product path: there is no CPU or PyTorch fallback.  Loading fails
loudly (``FlairHipUnavailable``) when the shared object has not been built.  ``lib()`` is the
raw library with every declared entry typed (``argtypes`` / ``restype``); ``call.flair_x(...)`` launches
an entry on torch tensors and raises ``FlairHipError`` with the library's message on a non-zero status.
"""
import ctypes
import functools
import os

import torch  # noqa: F401  (must be imported first: the library binds to torch's HIP runtime)

from ._header import (EVAL_PROTOS, FACESCORE_PROTOS, IDENT_PROTOS, NOREF_PROTOS, PROTOS, STRUCTS, TEMPORAL_PROTOS, TILE_PROTOS,
                      YUV_PROTOS)

# every declared entry of the library: the sampling path's (flair_hip.h), the evaluation-only ones (flair_eval.h) and the
# no-reference scores (flair_noref.h)
ALL_PROTOS = {**PROTOS, **EVAL_PROTOS, **NOREF_PROTOS}
# ... and the identity score's (flair_ident.h), the flow-warping error's (flair_temporal.h), the face score's
# (flair_facescore.h), the video streams' (flair_yuv.h) and tiled denoising's (flair_tile.h), typed and launched like the others
# from tables of their own
_TYPED_PROTOS = {**ALL_PROTOS, **IDENT_PROTOS, **TEMPORAL_PROTOS, **FACESCORE_PROTOS, **YUV_PROTOS, **TILE_PROTOS}

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libflair_hip.so")

FLAIR_F32, FLAIR_BF16 = 0, 1
ACT_NONE, ACT_RELU, ACT_LRELU01, ACT_SILU, ACT_DCN_OFFSETS, ACT_LRELU02, ACT_GELU = 0, 1, 2, 3, 4, 5, 6

ConvParams = STRUCTS["flair_conv_params"]


class FlairHipUnavailable(RuntimeError):
    pass


class FlairHipError(RuntimeError):
    pass


_lib = None


def lib():
    """The loaded library; raises FlairHipUnavailable if it has not been built."""
    global _lib
    if _lib is None:
        global LIB_PATH
        if os.environ.get("FLAIR_HIP_LIB"):        # another build of the library, for same-box comparisons (tools/ab_libs.sh)
            LIB_PATH = os.environ["FLAIR_HIP_LIB"]
        if not os.path.exists(LIB_PATH):
            raise FlairHipUnavailable(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                f"g.build()'` (or `make -C flair_amd/csrc`). The HIP library is required; "
                f"there is no fallback path.")
        l = ctypes.CDLL(LIB_PATH)
        for name, (restype, params) in _TYPED_PROTOS.items():
            f = getattr(l, name)
            f.restype, f.argtypes = restype, [p.ctype for p in params]
        _lib = l
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().flair_last_error().decode("utf-8", "replace")
        raise FlairHipError(f"{what} failed (status {status}): {msg}")


def dtype_code(t):
    if t.dtype == torch.float32:
        return FLAIR_F32
    if t.dtype == torch.bfloat16:
        return FLAIR_BF16
    raise TypeError(f"unsupported activation dtype {t.dtype}")


def _address(t):
    if not t.is_cuda:
        raise FlairHipError("flair_amd ops need tensors resident in HBM (device='cuda'); "
                            "no CPU path exists")
    return t.data_ptr()


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return ctypes.c_void_p(0 if t is None else _address(t))


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# The entries that launch: status returned, `stream` last.  Per entry, the position, name and required tensor dtype (None
# behind a void*) of every data pointer, worked out once so that a call only walks this list.
_ELEM_DTYPE = {"float": torch.float32, "double": torch.float64, "int": torch.int32, "uint8_t": torch.uint8,
               "long long": torch.int64}
_LAUNCHES = {name: [(i, p.name, _ELEM_DTYPE.get(p.elem)) for i, p in enumerate(params[:-1])
                    if p.elem is not None and p.ctype is ctypes.c_void_p]
             for name, (restype, params) in _TYPED_PROTOS.items()
             if restype is ctypes.c_int and params and params[-1].name == "stream"}


def _launch(name, *args):
    fn = getattr(lib(), name)
    if len(args) != len(fn.argtypes) - 1:
        raise TypeError(f"{name} takes {len(fn.argtypes) - 1} arguments and the stream ({len(args)} given)")
    args = list(args)
    for i, pname, dtype in _LAUNCHES[name]:
        t = args[i]
        if hasattr(t, "data_ptr"):      # a tensor; None, host arrays and byref() go to ctypes as they are
            args[i] = _address(t)
            if dtype is not None and t.dtype != dtype:
                raise FlairHipError(f"{name}: {pname} must be {str(dtype)[6:]}, got {str(t.dtype)[6:]}")
    check(fn(*args, stream()), name)


class _Entries:
    """``call.flair_x(*args)`` launches entry flair_x of the header on torch's current stream.  ``args`` are the entry's
    arguments without the stream; a tensor stands for its device pointer (it must live in HBM and, behind a typed pointer
    such as ``const float*``, have that dtype) and None for NULL; numbers and flags convert through the entry's
    ``argtypes``.  Raises FlairHipError on a refusal here or a non-zero status of the library.  The entries that return
    a value instead of a status (size queries, flair_conv_variant, flair_abi_version) are called through ``lib()``.
    An attribute, not a string, so that a search for ``flair_x(`` finds the header, the C source and the Python callers."""

    def __getattr__(self, name):
        if name not in _LAUNCHES:
            raise AttributeError(f"{name} is not an entry of flair_hip.h that launches on a stream, nor one of flair_eval.h, flair_noref.h, flair_ident.h, flair_temporal.h, flair_facescore.h, flair_yuv.h or flair_tile.h")
        return functools.partial(_launch, name)


call = _Entries()


def image_metrics_workspace(N, H, W):
    """flair_image_metrics_workspace(N, H, W): bytes of workspace flair_image_metrics needs (0 for a shape it refuses)."""
    return lib().flair_image_metrics_workspace(N, H, W)


def image_metrics(a, b, N, H, W, out, ws, ws_bytes):
    """flair_image_metrics on torch's current stream; a, b, out, ws: ctypes pointers (ptr()).  Returns the status."""
    return lib().flair_image_metrics(a, b, N, H, W, out, ws, ws_bytes, stream())
