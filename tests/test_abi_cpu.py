"""CPU: the C-ABI library loads and exports every symbol include/flair_hip.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "flair_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(flair_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_hot_path():
    names = declared_symbols()
    for must in ("flair_conv_nhwc", "flair_groupnorm_nhwc", "flair_qkv_attention", "flair_temporal_attention",
                 "flair_dcn_align", "flair_flow_warp", "flair_timestep_embedding", "flair_sampler_update",
                 "flair_depthwise_filter", "flair_jpeg_roundtrip", "flair_last_error"):
        assert must in names


def test_library_exports_every_declared_symbol():
    from flair_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in declared_symbols() if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.flair_abi_version() >= 1


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from flair_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.FlairHipUnavailable, match="no fallback"):
        _lib.lib()


def test_argument_errors_are_reported_without_a_gpu():
    """Validation happens before any launch, so error plumbing is testable on CPU."""
    from flair_amd import _lib
    lib = _lib.lib()
    p = _lib.ConvParams()
    p.dtype = 7
    rc = lib.flair_conv_nhwc(ctypes.byref(p), (ctypes.c_void_p * 4)(1, 0, 0, 0), ctypes.c_void_p(16), None, None,
                             None, None, ctypes.c_void_p(16), None, ctypes.c_size_t(0), None)
    assert rc == -1 and b"bad dtype" in lib.flair_last_error()


def test_bcast_entry_validates_arguments():
    """flair_bcast_weights (the path's only collective) refuses a null blob / communicator with a message and
    does not touch RCCL for that (no GPU and no librccl needed here)."""
    import ctypes
    from flair_amd import _lib
    lib = _lib.lib()
    rc = lib.flair_bcast_weights(None, ctypes.c_size_t(0), 0, None, None)
    assert rc == -1 and b"flair_bcast_weights" in lib.flair_last_error()


# Functions of flair_amd/ops.py that launch nothing and so need no GPU test of their own: the K granularity of a dtype, the
# shape test in front of conv_chain, the host-side blend coefficients of SuperSloMo.
HOST_ONLY = {"k_align", "chain_supported", "slomo_coefficients"}


def test_every_ops_wrapper_is_called_by_a_gpu_test():
    """Every public function of flair_amd/ops.py (each ends in a call.flair_*(...) launch or prepares one) is called, as
    `ops.<name>(` or `<name>(`, in at least one test file that carries the gpu marker; a private one that calls the library
    is reached through a public one.  A new entry without a test of its own fails here."""
    import glob
    src = open(os.path.join(ROOT, "flair_amd", "ops.py")).read()
    bodies = dict(zip(re.findall(r"(?m)^def (\w+)\(", src), re.split(r"(?m)^def \w+\(", src)[1:]))
    launches = {n for n, b in bodies.items() if re.search(r"\b(?:lib\(\)|call)\.flair_\w+", b)}
    assert len(launches) > 60 and {"axpby_nhwc", "amt_multiflow_prepare", "amt_multiflow_combine"} <= launches
    assert HOST_ONLY <= set(bodies) and not HOST_ONLY & launches
    tests = [open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py")))]
    tests = [t for t in tests if re.search(r"\bpytest\.mark\.gpu\b", t)]
    assert len(tests) > 10

    def called(name, texts):
        pat = re.compile(r"(?:\bops\.|(?<![\w.]))%s\(" % re.escape(name))
        return any(pat.search(t) for t in texts)

    public = [n for n in bodies if not n.startswith("_") and n not in HOST_ONLY]
    missing = [n for n in public if not called(n, tests)]
    assert not missing, f"no gpu-marked test calls {missing}"
    private = [n for n in launches if n.startswith("_")]
    unreached = [n for n in private if not called(n, [b for m, b in bodies.items() if m != n and not m.startswith("_")])]
    assert not unreached, unreached


def test_dispatch_reads_no_environment():
    """Kernel choice depends on the arguments alone: no HIP source reads an environment variable and no model module
    reads os.environ (FLAIR_HIP_LIB, which picks the library file in flair_amd/_lib.py, is not a dispatch switch)."""
    import glob
    csrc = os.path.join(ROOT, "flair_amd", "csrc")
    hip = sorted(glob.glob(os.path.join(csrc, "*.hip"))) + sorted(glob.glob(os.path.join(csrc, "*.h")))
    py = sorted(glob.glob(os.path.join(ROOT, "flair_amd", "guided_diffusion", "*.py")))
    assert len(hip) > 1 and os.path.join(csrc, "common.h") in hip and py
    bad = [os.path.relpath(f, ROOT) for f in hip if re.search(r"\bgetenv\b", open(f).read())]
    bad += [os.path.relpath(f, ROOT) for f in py if re.search(r"\benviron\b", open(f).read())]
    assert not bad, bad
