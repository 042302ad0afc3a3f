"""include/flair_hip.h read into ctypes: the parameter structs and every entry's prototype.

The header is the contract with libflair_hip.so; nothing of it is restated in Python.  ``STRUCTS`` maps a C struct name to
a ``ctypes.Structure`` class, ``PROTOS`` an entry name to ``(restype, [Param, ...])``; ``EVAL_PROTOS`` is the same table
of include/flair_eval.h, the evaluation-only entries of the same library, ``NOREF_PROTOS`` that of include/flair_noref.h,
the no-reference scores, ``IDENT_PROTOS`` that of include/flair_ident.h, the identity score, ``TEMPORAL_PROTOS`` that of
include/flair_temporal.h, the flow-warping error, ``FACESCORE_PROTOS`` that of include/flair_facescore.h, the face score's
crop, ``YUV_PROTOS`` that of include/flair_yuv.h, the video streams' colour conversion, and ``TILE_PROTOS`` that of
include/flair_tile.h, the gather and blend of tiled denoising.  Only the constructs the header uses
are understood, and anything else raises ``HeaderError`` with the offending text: a declaration is never skipped.
"""
import collections
import ctypes
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flair_hip.h")

SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
           "size_t": ctypes.c_size_t}
RETURNS = dict(SCALARS, **{"char*": ctypes.c_char_p})
POINTEES = {"void", "float", "double", "int", "uint8_t", "long long", "void*", "float*"}

# name, ctypes type, pointed-to C type (None for a scalar or a stream), e.g. ("bias", c_void_p, "float")
Param = collections.namedtuple("Param", "name ctype elem")


class HeaderError(RuntimeError):
    pass


def _ctype(text):
    """'const float* const*' -> 'float**': qualifiers dropped, stars attached."""
    return re.sub(r"\s*\*\s*", "*", " ".join(w for w in re.sub(r"\*", " * ", text).split() if w != "const"))


def _struct(name, body):
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(int|long|float)\s+(.+)", decl, re.S)
        if not m:
            raise HeaderError(f"struct {name}: cannot read the field declaration {decl!r}")
        for item in m.group(2).split(","):
            f = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", item.strip())
            if not f:
                raise HeaderError(f"struct {name}: cannot read the field {item!r} of {decl!r}")
            t = SCALARS[m.group(1)]
            fields.append((f.group(1), t * int(f.group(2)) if f.group(2) else t))
    # no instance __dict__: assigning a name that is not a field raises AttributeError instead of being dropped
    return type(name, (ctypes.Structure,), {"__slots__": (), "_fields_": fields})


def _param(entry, text, structs):
    m = re.fullmatch(r"(.+?)(\w+)", text.strip(), re.S)
    if not m:
        raise HeaderError(f"{entry}: cannot read the parameter {text!r}")
    t, name = _ctype(m.group(1)), m.group(2)
    if t in SCALARS:
        return Param(name, SCALARS[t], None)
    if t == "hipStream_t":
        return Param(name, ctypes.c_void_p, None)
    if t.endswith("*") and t[:-1] in structs:
        return Param(name, ctypes.POINTER(structs[t[:-1]]), t[:-1])
    if t.endswith("*") and t[:-1] in POINTEES:
        return Param(name, ctypes.c_void_p, t[:-1])
    raise HeaderError(f"{entry}: parameter type {m.group(1).strip()!r} of {text.strip()!r} is not understood")


def parse(text):
    """-> (structs, protos) of a header in the dialect of flair_hip.h."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"(?m)^\s*#.*$", "", text)
    text, n = re.subn(r'extern\s+"C"\s*\{', "", text)
    if n != 1 or not text.rstrip().endswith("}"):
        raise HeaderError('expected one extern "C" { ... } block around the declarations')
    text = text.rstrip()[:-1]
    structs, protos, pos = {}, {}, 0
    for m in re.finditer(r"\s*((?:[^;{}]|\{[^{}]*\})*?)\s*;", text):
        if m.start() != pos:
            break
        pos, stmt = m.end(), m.group(1)
        s = re.fullmatch(r"typedef\s+struct\s*\{(.*)\}\s*(\w+)", stmt, re.S)
        p = re.fullmatch(r"([\w\s\*]+?)\b(flair_\w+)\s*\((.*)\)", stmt, re.S)
        if s:
            structs[s.group(2)] = _struct(s.group(2), s.group(1))
        elif p:
            ret, name, args = _ctype(p.group(1)), p.group(2), p.group(3).strip()
            if ret not in RETURNS:
                raise HeaderError(f"{name}: return type {p.group(1).strip()!r} is not understood")
            if name in protos:
                raise HeaderError(f"{name} is declared twice")
            protos[name] = (RETURNS[ret], [] if args == "void" else [_param(name, a, structs) for a in args.split(",")])
        elif not re.fullmatch(r"typedef\s+enum\s*\{[^{}]*\}\s*\w+|typedef\s+struct\s+ihipStream_t\s*\*\s*hipStream_t", stmt):
            raise HeaderError(f"cannot read the declaration {' '.join(stmt.split())!r}")
    if text[pos:].strip():
        raise HeaderError(f"cannot read the header from {' '.join(text[pos:].split())[:120]!r} on")
    return structs, protos


with open(HEADER_PATH) as _f:
    STRUCTS, PROTOS = parse(_f.read())

# The evaluation-only ABI (include/flair_eval.h: LPIPS), same dialect and same library, in a table of its own: PROTOS stays
# exactly flair_hip.h.  It declares no struct and may not redeclare an entry of flair_hip.h.
EVAL_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "flair_eval.h")
with open(EVAL_HEADER_PATH) as _f:
    _eval_structs, EVAL_PROTOS = parse(_f.read())
if _eval_structs or set(EVAL_PROTOS) & set(PROTOS):
    raise HeaderError(f"flair_eval.h declares a struct or an entry of flair_hip.h: {sorted(_eval_structs) + sorted(set(EVAL_PROTOS) & set(PROTOS))}")

# The no-reference ABI (include/flair_noref.h: NIQE), on the same terms: a table of its own, no struct, no entry declared twice.
NOREF_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "flair_noref.h")
with open(NOREF_HEADER_PATH) as _f:
    _noref_structs, NOREF_PROTOS = parse(_f.read())
if _noref_structs or set(NOREF_PROTOS) & (set(PROTOS) | set(EVAL_PROTOS)):
    raise HeaderError("flair_noref.h declares a struct or an entry of another header: "
                      f"{sorted(_noref_structs) + sorted(set(NOREF_PROTOS) & (set(PROTOS) | set(EVAL_PROTOS)))}")

# The identity ABI (include/flair_ident.h: ArcFace similarity), on the same terms once more.
IDENT_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "flair_ident.h")
with open(IDENT_HEADER_PATH) as _f:
    _ident_structs, IDENT_PROTOS = parse(_f.read())
if _ident_structs or set(IDENT_PROTOS) & (set(PROTOS) | set(EVAL_PROTOS) | set(NOREF_PROTOS)):
    raise HeaderError("flair_ident.h declares a struct or an entry of another header: "
                      f"{sorted(_ident_structs) + sorted(set(IDENT_PROTOS) & (set(PROTOS) | set(EVAL_PROTOS) | set(NOREF_PROTOS)))}")

# The temporal ABI (include/flair_temporal.h: the flow-warping error), on the same terms.
TEMPORAL_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "flair_temporal.h")
with open(TEMPORAL_HEADER_PATH) as _f:
    _temporal_structs, TEMPORAL_PROTOS = parse(_f.read())
_older = set(PROTOS) | set(EVAL_PROTOS) | set(NOREF_PROTOS) | set(IDENT_PROTOS)
if _temporal_structs or set(TEMPORAL_PROTOS) & _older:
    raise HeaderError("flair_temporal.h declares a struct or an entry of another header: "
                      f"{sorted(_temporal_structs) + sorted(set(TEMPORAL_PROTOS) & _older)}")

# The face-score ABI (include/flair_facescore.h: the byte crop of the face-region scores), on the same terms.
FACESCORE_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "flair_facescore.h")
with open(FACESCORE_HEADER_PATH) as _f:
    _facescore_structs, FACESCORE_PROTOS = parse(_f.read())
_older = _older | set(TEMPORAL_PROTOS)
if _facescore_structs or set(FACESCORE_PROTOS) & _older:
    raise HeaderError("flair_facescore.h declares a struct or an entry of another header: "
                      f"{sorted(_facescore_structs) + sorted(set(FACESCORE_PROTOS) & _older)}")

# The video-stream ABI (include/flair_yuv.h: the colour conversion and chroma resampling of .y4m input and output), on the same terms.
YUV_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "flair_yuv.h")
with open(YUV_HEADER_PATH) as _f:
    _yuv_structs, YUV_PROTOS = parse(_f.read())
_older = _older | set(FACESCORE_PROTOS)
if _yuv_structs or set(YUV_PROTOS) & _older:
    raise HeaderError("flair_yuv.h declares a struct or an entry of another header: "
                      f"{sorted(_yuv_structs) + sorted(set(YUV_PROTOS) & _older)}")

# The tiling ABI (include/flair_tile.h: the gather and the feathered blend of tiled denoising), on the same terms.
TILE_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "flair_tile.h")
with open(TILE_HEADER_PATH) as _f:
    _tile_structs, TILE_PROTOS = parse(_f.read())
_older = _older | set(YUV_PROTOS)
if _tile_structs or set(TILE_PROTOS) & _older:
    raise HeaderError("flair_tile.h declares a struct or an entry of another header: "
                      f"{sorted(_tile_structs) + sorted(set(TILE_PROTOS) & _older)}")
