"""CPU: the guarded-view helper of tests/util.py catches every kind of stray write, and the stride-taking entries refuse
strides below their channel count or granularity and misaligned pointers with their message, before any launch.
(Only parameters that must be refused reach an entry here: an accepted shape would launch.)"""
import ctypes

import pytest
import torch

from tests.util import IN_FILL, OUT_FILL, assert_untouched, guarded

# ------------------------------------------------------------------------------------------------ the helper itself


def _buf(dtype=torch.bfloat16, fill=OUT_FILL):
    buf, view = guarded(2, 3, 5, 8, dtype, "cpu", coff=8, ld=24, fill=fill)
    view.copy_(torch.arange(view.numel(), dtype=torch.float32).view(view.shape).to(dtype))
    return buf, view, buf.clone()


def test_guarded_layout():
    buf, view = guarded(2, 3, 5, 8, torch.float32, "cpu", coff=8, ld=24)
    assert tuple(buf.shape) == (4, 3, 5, 24) and tuple(view.shape) == (2, 3, 5, 8)
    assert view.stride() == (3 * 5 * 24, 5 * 24, 24, 1) and view.data_ptr() == buf[1, 0, 0, 8].data_ptr()
    assert torch.all(buf == OUT_FILL)
    assert torch.isnan(guarded(1, 2, 2, 4, torch.bfloat16, "cpu", fill=IN_FILL)[0]).all()
    assert OUT_FILL == float(torch.tensor(OUT_FILL, dtype=torch.bfloat16))      # exact in bf16


def test_view_writes_pass():
    buf, view, before = _buf()
    view.mul_(2)
    assert_untouched(buf, before, view)


@pytest.mark.parametrize("where", ["pad channel", "channel before", "guard frame before", "guard frame after"])
def test_flags_a_changed_guard(where):
    buf, view, before = _buf()
    idx = {"pad channel": (1, 2, 4, 16), "channel before": (2, 0, 0, 7), "guard frame before": (0, 1, 1, 9),
           "guard frame after": (3, 2, 4, 23)}[where]
    buf[idx] = 0.0
    with pytest.raises(AssertionError, match="outside the view"):
        assert_untouched(buf, before, view)


def test_flags_a_nan_sentinel_replaced_by_another_nan():
    buf, view, before = _buf(fill=IN_FILL)
    flat = buf.view(torch.int16)
    flat[0, 0, 0, 0] = 0x7FC1                                   # still NaN, another pattern
    assert torch.isnan(buf[0, 0, 0, 0])
    with pytest.raises(AssertionError, match="outside the view"):
        assert_untouched(buf, before, view)


def test_flags_a_changed_read_only_view():
    buf, view, before = _buf(fill=IN_FILL)
    assert_untouched(buf, before)
    view[1, 2, 3, 4] += 1
    with pytest.raises(AssertionError, match="read-only"):
        assert_untouched(buf, before)


# ------------------------------------------------------------------------------------------------ entry refusals
P16, P8, P2 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8), ctypes.c_void_p(4096 + 2)   # fake device pointers


def _lib():
    from flair_amd import _lib
    return _lib.lib()


def _refused(rc, *needles):
    assert rc == -1
    msg = _lib().flair_last_error()
    for n in needles:
        assert n.encode() in msg, msg
    return msg


def _conv_params(dtype=1, cout=64, segs=(64,), seg_ld=None, y_ld=None):
    from flair_amd import ops
    p = ops.ConvParams()
    p.dtype = dtype
    p.T, p.H, p.W = 1, 8, 8
    p.KT, p.KH, p.KW = 1, 3, 3
    p.Cout = cout
    p.nseg = len(segs)
    for i, c in enumerate(segs):
        p.seg_c[i] = c
        p.seg_ld[i] = seg_ld if seg_ld is not None else c
    p.y_ld = y_ld if y_ld is not None else cout
    p.stride = 1
    p.out_scale = 1.0
    return p


def _conv(p, x=P16, res0=None, res1=None, y=P16):
    arr = (ctypes.c_void_p * 4)(*([x] * p.nseg + [None] * (4 - p.nseg)))
    return _lib().flair_conv_nhwc(ctypes.byref(p), arr, P16, None, None, res0, res1, y, None, ctypes.c_size_t(0), None)


@pytest.mark.parametrize("dtype", [0, 1])
def test_conv_refuses_segment_strides(dtype):
    c = 64
    _refused(_conv(_conv_params(dtype, segs=(c,), seg_ld=c - (8 if dtype else 4))), "segment 0 stride/alignment")
    _refused(_conv(_conv_params(dtype, segs=(c,), seg_ld=c + (4 if dtype else 2))), "segment 0 stride/alignment")
    _refused(_conv(_conv_params(dtype, segs=(c,)), x=P8), "segment 0 stride/alignment")


@pytest.mark.parametrize("dtype,cout,y_ld", [
    (1, 64, 60),        # below Cout
    (1, 64, 68),        # 8-byte granular: Cout % 8 == 0 stores 16-byte pieces
    (0, 64, 66),        # f32: 8-byte granular
    (0, 36, 38),        # f32 Cout % 8 == 4: store_quad writes float4
    (1, 36, 38),        # bf16 Cout % 8 == 4: 4-byte granular
])
def test_conv_refuses_output_strides(dtype, cout, y_ld):
    _refused(_conv(_conv_params(dtype, cout=cout, y_ld=y_ld)), "output stride/alignment", f"y_ld = {y_ld}")


def test_conv_refuses_a_misaligned_output():
    _refused(_conv(_conv_params(1, cout=36, y_ld=36), y=P8), "output stride/alignment")


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("dtype,cout,res_ld,ptr", [
    (1, 64, 56, P16),   # below Cout
    (1, 64, 68, P16),   # 8-byte granular stride under 16-byte residual loads
    (1, 64, 64, P8),    # 8-byte aligned pointer under 16-byte residual loads
    (0, 64, 66, P16),
    (0, 64, 64, P8),
    (1, 36, 38, P16),   # bf16 Cout % 8 == 4: 8 bytes are enough, 4 are not
    (1, 36, 36, P2),
    (1, 36, 32, P16),
])
def test_conv_refuses_residual_strides(which, dtype, cout, res_ld, ptr):
    p = _conv_params(dtype, cout=cout)
    p.res_ld[which] = res_ld
    p.res_ld[1 - which] = cout
    res = [P16, P16]
    res[which] = ptr
    _refused(_conv(p, res0=res[0], res1=res[1]), f"res{which} stride/alignment", f"res_ld = {res_ld}")


def _chain_params(dtype=1, y_ld=64, res_ld=(0, 0), seg_ld=64):
    from flair_amd import ops
    p = ops.ChainParams()
    p.dtype = dtype
    p.T, p.H, p.W = 1, 8, 32
    p.C, p.CoutB = 64, 64
    p.nseg = 1
    p.seg_c[0], p.seg_ld[0] = 64, seg_ld
    p.y_ld = y_ld
    p.res_ld[0], p.res_ld[1] = res_ld
    p.out_scale = 1.0
    return p


def _chain(p, res0=None, res1=None, y=P16, x=P16):
    arr = (ctypes.c_void_p * 4)(x, None, None, None)
    return _lib().flair_conv_chain(ctypes.byref(p), arr, P16, None, P16, None, res0, res1, y, None)


@pytest.mark.parametrize("dtype", [0, 1])
def test_chain_refuses_strides(dtype):
    _refused(_chain(_chain_params(dtype, seg_ld=56)), "segment 0 stride/alignment")
    _refused(_chain(_chain_params(dtype, y_ld=56)), "flair_conv_chain", "y stride/alignment", "y_ld = 56")
    _refused(_chain(_chain_params(dtype, y_ld=66)), "flair_conv_chain", "y stride/alignment", "y_ld = 66")
    _refused(_chain(_chain_params(dtype), y=P8), "flair_conv_chain", "y stride/alignment")
    _refused(_chain(_chain_params(dtype, res_ld=(56, 0)), res0=P16), "flair_conv_chain", "res0 stride/alignment", "res0_ld = 56")
    _refused(_chain(_chain_params(dtype, res_ld=(64, 66)), res0=P16, res1=P16), "flair_conv_chain", "res1 stride/alignment",
             "res1_ld = 66")
    _refused(_chain(_chain_params(dtype, res_ld=(64, 0)), res0=P8), "flair_conv_chain", "res0 stride/alignment")


def _gn(dtype=1, C=64, c0=64, ld0=64, ld1=0, y_ld=64, raw_ld=0, x0=P16, x1=None, y=P16, raw=None):
    from flair_amd import ops
    p = ops.GnParams()
    p.dtype, p.C, p.c0, p.ld0, p.ld1, p.groups = dtype, C, c0, ld0, ld1, 32
    p.F, p.H, p.W, p.frames_per_stat, p.eps = 1, 4, 4, 1, 1e-5
    p.y_ld, p.raw_ld = y_ld, raw_ld
    return _lib().flair_groupnorm_nhwc(ctypes.byref(p), x0, x1, P16, P16, None, y, raw, P16, None)


@pytest.mark.parametrize("dtype", [0, 1])
def test_group_norm_refuses_strides(dtype):
    g = 8 if dtype else 4
    _refused(_gn(dtype, ld0=56), "strides/alignment")
    _refused(_gn(dtype, ld0=64 + g // 2), "strides/alignment")
    _refused(_gn(dtype, x0=P8), "strides/alignment")
    _refused(_gn(dtype, C=128, c0=64, ld1=56, x1=P16), "strides/alignment")
    _refused(_gn(dtype, C=128, c0=64, ld1=64, x1=P8), "strides/alignment")
    _refused(_gn(dtype, y_ld=56), "strides/alignment")
    _refused(_gn(dtype, y_ld=64 + g // 2), "strides/alignment")
    _refused(_gn(dtype, y=P8), "strides/alignment")
    _refused(_gn(dtype, raw_ld=56, raw=P16), "strides/alignment")
    _refused(_gn(dtype, raw_ld=64, raw=P8), "strides/alignment")


def _attn(ld, out_ld, d=64, q_off=0, dtype=1):
    from flair_amd import ops
    p = ops.AttnParams()
    p.dtype, p.frames, p.L, p.heads, p.head_dim = dtype, 1, 64, 1, d
    p.ld, p.out_ld = ld, out_ld
    p.q_off, p.k_off, p.v_off, p.head_stride = q_off, q_off + d, q_off + 2 * d, 3 * d
    p.scale = 0.125
    return _lib().flair_qkv_attention(ctypes.byref(p), P16, P16, None)


@pytest.mark.parametrize("d", [32, 64, 128])
def test_qkv_attention_refuses_strides(d):
    _refused(_attn(3 * d - 8, d, d), "exceed ld")
    _refused(_attn(3 * d, d - 8, d), "exceed ld")
    _refused(_attn(3 * d + 4, d, d), "multiples of 8")
    _refused(_attn(3 * d + 8, d + 4, d), "multiples of 8")
    _refused(_attn(3 * d + 8, d, d, q_off=4), "multiples of 8")


def _tattn(ld, out_ld, C=64, dtype=1):
    from flair_amd import ops
    p = ops.TAttnParams()
    p.dtype, p.T, p.H, p.W, p.C, p.window = dtype, 4, 2, 2, C, 5
    p.ld, p.out_ld, p.scale, p.head_dim = ld, out_ld, 0.125, 64
    return _lib().flair_temporal_attention(ctypes.byref(p), P16, P16, P16, None)


def test_temporal_attention_refuses_strides():
    _refused(_tattn(3 * 64 - 8, 64), "strides")
    _refused(_tattn(3 * 64 + 4, 64), "strides")
    _refused(_tattn(3 * 64, 68), "strides")


def _dcn(dtype=1, c=64, x_ld=(64, 64), raw_ld=432, y_ld=64, x0=P16, x1=P16, raw=P16):
    from flair_amd import ops
    p = ops.DcnParams()
    p.dtype, p.F, p.H, p.W, p.Cin, p.Cout, p.G = dtype, 1, 8, 8, 2 * c, c, 16
    p.x_ld[0], p.x_ld[1] = x_ld
    p.raw_ld, p.y_ld, p.max_residue_magnitude = raw_ld, y_ld, 10.0
    return _lib().flair_dcn_align(ctypes.byref(p), x0, x1, raw, None, None, P16, P16, P16, None)


@pytest.mark.parametrize("dtype", [0, 1])
def test_dcn_refuses_strides(dtype):
    g = 8 if dtype else 4
    _refused(_dcn(dtype, x_ld=(56, 64)), "strides/alignment")
    _refused(_dcn(dtype, x_ld=(64, 56)), "strides/alignment")
    _refused(_dcn(dtype, x_ld=(64 + g // 2, 64)), "strides/alignment")
    _refused(_dcn(dtype, x0=P8), "strides/alignment")
    _refused(_dcn(dtype, x1=P8), "strides/alignment")
    _refused(_dcn(dtype, raw=P8), "strides/alignment")
    _refused(_dcn(dtype, y_ld=60), "strides/alignment")
    _refused(_dcn(dtype, raw_ld=420), "raw_ld")
    _refused(_dcn(dtype, raw_ld=432 + g // 2), "raw_ld")


@pytest.mark.parametrize("dtype", [0, 1])
def test_elementwise_entries_refuse_strides(dtype):
    lib = _lib()
    g = 8 if dtype else 4
    P = ctypes.c_long(16)
    # add_act: ld below C, off-granule ld, misaligned pointer
    off = 64 + g // 2
    _refused(lib.flair_add_act_nhwc(P16, 56, None, 0, dtype, 64, P, 0, P16, 64, None), "flair_add_act_nhwc", "x0 stride/alignment",
             "x0_ld = 56")
    _refused(lib.flair_add_act_nhwc(P16, 64, P16, off, dtype, 64, P, 0, P16, 64, None), "flair_add_act_nhwc", "x1 stride/alignment",
             f"x1_ld = {off}")
    _refused(lib.flair_add_act_nhwc(P16, 64, None, 0, dtype, 64, P, 0, P8, 64, None), "flair_add_act_nhwc", "y stride/alignment")
    # maxpool
    _refused(lib.flair_maxpool3x3s2_nhwc(P16, 56, dtype, 1, 4, 4, 64, P16, 64, None), "flair_maxpool3x3s2_nhwc", "x stride/alignment",
             "x_ld = 56")
    _refused(lib.flair_maxpool3x3s2_nhwc(P16, 64, dtype, 1, 4, 4, 64, P16, off, None), "flair_maxpool3x3s2_nhwc", "y stride/alignment",
             f"y_ld = {off}")
    _refused(lib.flair_maxpool3x3s2_nhwc(P8, 64, dtype, 1, 4, 4, 64, P16, 64, None), "flair_maxpool3x3s2_nhwc", "x stride/alignment")
    # scale_pixels
    _refused(lib.flair_scale_pixels(P16, dtype, 56, 64, P, P16, None), "flair_scale_pixels", "x stride/alignment", "x_ld = 56")
    _refused(lib.flair_scale_pixels(P16, dtype, off, 64, P, P16, None), "flair_scale_pixels", "x stride/alignment", f"x_ld = {off}")
    _refused(lib.flair_scale_pixels(P8, dtype, 64, 64, P, P16, None), "flair_scale_pixels", "x stride/alignment")
    # flow_warp: flow_ld < 2 / odd, x / y strides off the vector granule
    _refused(lib.flair_flow_warp(P16, dtype, 64, P16, 1, 1, 4, 4, 64, 0, P16, 64, None), "flair_flow_warp")
    _refused(lib.flair_flow_warp(P16, dtype, 64, P16, 3, 1, 4, 4, 64, 0, P16, 64, None), "flair_flow_warp")
    _refused(lib.flair_flow_warp(P16, dtype, 64 + g // 2, P16, 2, 1, 4, 4, 64, 0, P16, 64, None), "flair_flow_warp")
    _refused(lib.flair_flow_warp(P16, dtype, 64, P16, 2, 1, 4, 4, 64, 0, P16, 64 + g // 2, None), "flair_flow_warp")
    # resize: strides below C
    f = ctypes.c_float(1.0)
    _refused(lib.flair_resize_nhwc(P16, dtype, 2, 1, 4, 4, 3, 0, 8, 8, P16, 4, f, f, None), "x_ld = 2")
    _refused(lib.flair_resize_nhwc(P16, dtype, 4, 1, 4, 4, 3, 0, 8, 8, P16, 2, f, f, None), "y_ld = 2")
    # layout / cast / affine / frame bias: the channel window must fit the stride
    _refused(lib.flair_nchw_f32_to_nhwc(P16, 1, 8, 2, 2, P16, dtype, 16, 12, None))
    _refused(lib.flair_nhwc_to_nchw_f32(P16, dtype, 16, 12, 1, 8, 2, 2, P16, None))
    _refused(lib.flair_cast_channels(P16, 4, 8, P, P16, dtype, 16, 12, None))
    _refused(lib.flair_cast_channels(P16, 4, 8, P, P16, dtype, 16, 0, None))        # src_ld < C
    _refused(lib.flair_add_frame_bias(P16, dtype, 56, 64, 1, P, P16, 64, None), "flair_add_frame_bias")
    _refused(lib.flair_add_frame_bias(P16, dtype, 64, 64, 1, P, P16, 56, None), "flair_add_frame_bias")


def test_affine_and_dwconv_refuse_strides():
    lib = _lib()
    P = ctypes.c_long(16)
    f = ctypes.c_float(0.0)
    _refused(lib.flair_affine_channels_f32(P16, 2, 3, P, f, f, f, f, P16, P16, P16, 4, None), "flair_affine_channels_f32")
    _refused(lib.flair_affine_channels_f32(P16, 4, 3, P, f, f, f, f, P16, P16, P16, 2, None), "flair_affine_channels_f32")
    _refused(lib.flair_dwconv_nhwc(P16, 4, 1, 4, 4, 8, 1, P16, P16, None, None, 8, 2, P16, 8, None), "x_ld = 4")
    _refused(lib.flair_dwconv_nhwc(P16, 10, 1, 4, 4, 8, 1, P16, P16, None, None, 8, 2, P16, 8, None), "x_ld = 10")
    _refused(lib.flair_dwconv_nhwc(P16, 8, 1, 4, 4, 8, 1, P16, P16, None, None, 8, 2, P16, 6, None), "y_ld = 6")
    _refused(lib.flair_dwconv_nhwc(P8, 8, 1, 4, 4, 8, 1, P16, P16, None, None, 8, 2, P16, 8, None), "flair_dwconv_nhwc")


# ------------------------------------------------------------------------------------------------ prior / warp / sampler
# The entries below move 16-byte pieces at p * ld + c0: every stride holds the C channels and is 16-byte granular, every
# tensor pointer is 16-byte aligned.  One refusal per argument, each naming it.
def _vsrpp(which, dtype, *, C=64, ld=None, ptr=None, pad_ld=None, second=True):
    """ld / ptr: {name: value} overrides of prop / feat2 / cond1 / cond2 (flowpad: ptr only)."""
    lib = _lib()
    ld, ptr = dict(ld or {}), dict(ptr or {})
    l = {n: ld.get(n, C) for n in ("prop", "feat2", "cond1", "cond2")}
    q = {n: ptr.get(n, P16) for n in ("prop", "feat2", "cond1", "cond2", "flowpad")}
    flow2 = P16 if second else None
    if which == "warp2":
        return lib.flair_vsrpp_warp2(q["prop"], l["prop"], q["feat2"] if second else None, l["feat2"] if second else 0, P16,
                                     flow2, dtype, 8, 8, C, q["cond1"], l["cond1"], q["cond2"] if second else None,
                                     l["cond2"] if second else 0, None)
    return lib.flair_vsrpp_prep(q["prop"], l["prop"], q["feat2"] if second else None, l["feat2"] if second else 0, P16,
                                flow2, dtype, 8, 8, C, q["cond1"], l["cond1"], q["cond2"] if second else None,
                                l["cond2"] if second else 0, P16 if second else None, q["flowpad"],
                                (32 if dtype else 16) if pad_ld is None else pad_ld, None)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("which", ["warp2", "prep"])
def test_vsrpp_entries_refuse_strides(which, dtype):
    g = 8 if dtype else 4
    fn = f"flair_vsrpp_{which}"
    for name in ("prop", "feat2", "cond1", "cond2"):
        _refused(_vsrpp(which, dtype, ld={name: 64 - g}), fn, f"{name} stride/alignment", f"{name}_ld = {64 - g}")
        _refused(_vsrpp(which, dtype, ld={name: 64 + g // 2}), fn, f"{name} stride/alignment", f"{name}_ld = {64 + g // 2}")
        _refused(_vsrpp(which, dtype, ptr={name: P8}), fn, f"{name} stride/alignment")
    # a first-order step has no feat2 / cond2, and still checks prop / cond1
    _refused(_vsrpp(which, dtype, ld={"prop": 64 - g}, second=False), fn, "prop stride/alignment")
    _refused(_vsrpp(which, dtype, ptr={"cond1": P8}, second=False), fn, "cond1 stride/alignment")
    _refused(_vsrpp(which, 2), fn, "bad dtype")
    _refused(_vsrpp(which, -1), fn, "bad dtype")


@pytest.mark.parametrize("dtype", [0, 1])
def test_vsrpp_prep_refuses_a_bad_flowpad(dtype):
    g = 8 if dtype else 4
    _refused(_vsrpp("prep", dtype, pad_ld=0), "flowpad stride/alignment", "pad_ld = 0")
    _refused(_vsrpp("prep", dtype, pad_ld=2), "flowpad stride/alignment", "pad_ld = 2")
    _refused(_vsrpp("prep", dtype, pad_ld=4 * g + g // 2), "flowpad stride/alignment", f"pad_ld = {4 * g + g // 2}")
    _refused(_vsrpp("prep", dtype, ptr={"flowpad": P8}), "flowpad stride/alignment")
    _refused(_vsrpp("prep", dtype, ptr={"flowpad": P2} if dtype else {"flowpad": P8}, second=False), "flowpad stride/alignment")


def _blend(dtype, C=64, x_ld=64, m_ld=64, y_ld=64, x=P16, m=P16, y=P16):
    return _lib().flair_gated_blend(x, x_ld, m, m_ld, P16, C, dtype, C, 2, ctypes.c_long(16), y, y_ld, None)


@pytest.mark.parametrize("dtype", [0, 1])
def test_gated_blend_refuses_strides(dtype):
    g = 8 if dtype else 4
    for name in ("x", "m", "y"):
        _refused(_blend(dtype, **{f"{name}_ld": 64 - g}), "flair_gated_blend", f"{name} stride/alignment", f"{name}_ld = {64 - g}")
        _refused(_blend(dtype, **{f"{name}_ld": 64 + g // 2}), "flair_gated_blend", f"{name} stride/alignment",
                 f"{name}_ld = {64 + g // 2}")
        _refused(_blend(dtype, **{name: P8}), "flair_gated_blend", f"{name} stride/alignment")
    _refused(_lib().flair_gated_blend(P16, 64, P16, 64, P16, 56, dtype, 64, 2, ctypes.c_long(16), P16, 64, None),
             "flair_gated_blend")                                                              # gate_ld below C


def _ln(dtype, C=64, x_ld=None, y_ld=None, y2_ld=None, x=P16, y=P16, y2=P16):
    ld = lambda v: C if v is None else v
    return _lib().flair_layernorm_nhwc(x, dtype, ld(x_ld), ctypes.c_long(7), C, P16, P16, ctypes.c_float(1e-5), y, ld(y_ld),
                                       P16 if y2 is not None else None, 7 if y2 is not None else 0, y2, ld(y2_ld), None)


@pytest.mark.parametrize("dtype", [0, 1])
def test_layernorm_refuses_strides(dtype):
    g = 8 if dtype else 4
    for name in ("x", "y", "y2"):
        _refused(_ln(dtype, **{f"{name}_ld": 64 - g}), "flair_layernorm_nhwc", f"{name} stride/alignment", f"{name}_ld = {64 - g}")
        _refused(_ln(dtype, **{f"{name}_ld": 64 + g // 2}), "flair_layernorm_nhwc", f"{name} stride/alignment")
        _refused(_ln(dtype, **{name: P8}), "flair_layernorm_nhwc", f"{name} stride/alignment")
    # without the second output its stride is not looked at, the others still are
    _refused(_ln(dtype, y2=None, y2_ld=0, y_ld=64 - g), "y stride/alignment")
    # one 16-byte piece per lane and four pieces: C <= 1024 (f32) / 2048 (bf16)
    limit = 64 * 4 * g
    _refused(_ln(dtype, C=limit + g), "flair_layernorm_nhwc", f"C={limit + g}", f"at most {limit}")
    _refused(_ln(dtype, C=limit, x_ld=limit - g), "x stride/alignment")          # the limit itself passes the C check


def _wide(dtype, *, L=35, heads=3, d=40, ld=None, out_ld=None, offs=None, head_stride=None, qkv=P16, out=P16):
    from flair_amd import ops
    C = heads * d
    p = ops.AttnParams()
    p.dtype, p.frames, p.L, p.heads, p.head_dim = dtype, 1, L, heads, d
    p.ld = 3 * C if ld is None else ld
    p.out_ld = C if out_ld is None else out_ld
    p.q_off, p.k_off, p.v_off = offs or (0, C, 2 * C)
    p.head_stride = d if head_stride is None else head_stride
    p.scale = 0.125
    return _lib().flair_attention_wide(ctypes.byref(p), qkv, out, None)


@pytest.mark.parametrize("dtype", [0, 1])
def test_attention_wide_refuses_strides(dtype):
    g = 8 if dtype else 4
    C = 120
    _refused(_wide(dtype, ld=3 * C - g), "flair_attention_wide", "exceed ld = %d" % (3 * C - g))
    _refused(_wide(dtype, ld=3 * C + g, offs=(0, C, 2 * C + 2 * g)), "flair_attention_wide", "exceed ld")   # v of the last head
    _refused(_wide(dtype, ld=3 * C, offs=(2 * C + g, C, 0)), "flair_attention_wide", "exceed ld")           # q the highest
    _refused(_wide(dtype, heads=1, d=C, ld=2 * C, head_stride=2 * C, offs=(0, C + g, C)), "exceed ld")      # k the highest
    _refused(_wide(dtype, ld=9 * C, head_stride=3 * C, offs=(0, 40, 80), out_ld=C - g), "flair_attention_wide",
             f"out_ld = {C - g}", f"heads * head_dim = {C}")
    _refused(_wide(dtype, out_ld=C + g // 2), "flair_attention_wide", f"out_ld = {C + g // 2}")
    _refused(_wide(dtype, qkv=P8), "flair_attention_wide", "16-byte aligned")
    _refused(_wide(dtype, out=P8), "flair_attention_wide", "16-byte aligned")
    _refused(_wide(dtype, ld=3 * C + g // 2), "flair_attention_wide", "multiples of")
    _refused(_wide(dtype, offs=(-g, C, 2 * C)), "flair_attention_wide", "exceed ld")


@pytest.mark.parametrize("dtype", [0, 1])
def test_sft_fuse_refuses_misaligned_pointers(dtype):
    lib = _lib()
    n = ctypes.c_long(64)
    w = ctypes.c_float(0.5)
    for i, name in enumerate(("dec", "scale", "shift", "y")):
        for bad in (P8, P2):
            a = [P16, P16, P16, P16]
            a[i] = bad
            _refused(lib.flair_sft_fuse(a[0], a[1], a[2], w, dtype, n, a[3], None), "flair_sft_fuse", f"{name} = ",
                     "16-byte aligned")


@pytest.mark.parametrize("dtype", [0, 1])
def test_flow_warp_refuses_strides(dtype):
    lib = _lib()
    g = 8 if dtype else 4

    def warp(x=P16, x_ld=64, y=P16, y_ld=64):
        return lib.flair_flow_warp(x, dtype, x_ld, P16, 2, 1, 4, 4, 64, 0, y, y_ld, None)
    _refused(warp(x_ld=64 - g), "flair_flow_warp", "x stride/alignment", f"x_ld = {64 - g}")
    _refused(warp(y_ld=64 - g), "flair_flow_warp", "y stride/alignment", f"y_ld = {64 - g}")
    _refused(warp(x_ld=64 + g // 2), "flair_flow_warp", "x stride/alignment")
    _refused(warp(y_ld=64 + g // 2), "flair_flow_warp", "y stride/alignment")
    _refused(warp(x=P8), "flair_flow_warp", "x stride/alignment")
    _refused(warp(y=P8), "flair_flow_warp", "y stride/alignment")


# ------------------------------------------------------------------------------------------------ the element type code
# Every entry that takes a dtype refuses a code that is neither FLAIR_F32 nor FLAIR_BF16, naming itself and the argument.
# The entries come from the header: a prototype with `int dtype`, or with a params struct that has a dtype field, so an
# entry added later is covered (a struct entry by failing the set comparison below until it gets a call).
def _header():
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flair_hip.h")
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    protos = {m.group(1): [a.strip() for a in m.group(2).split(",")]
              for m in re.finditer(r"^int (flair_\w+)\(([^)]*)\);", text, flags=re.M)}
    structs = {m.group(2) for m in re.finditer(r"typedef struct \{([^}]*)\} (flair_\w+);", text) if re.search(r"\bint dtype;", m.group(1))}
    return protos, structs


def _dtype_entries():
    protos, structs = _header()
    direct = sorted(n for n, args in protos.items() if "int dtype" in args)
    by_struct = sorted(n for n, args in protos.items() if any(a.split("*")[0].replace("const", "").strip() in structs for a in args))
    by_struct.remove("flair_conv_variant")          # reports the kernel choice for a shape; launches nothing, refuses nothing
    return direct, by_struct


# otherwise valid small arguments by parameter name: 64 channels in pixels 64 elements apart, one frame of 4 x 4 pixels
_INT_ARGS = {"C": 64, "D": 64, "F": 1, "B": 1, "T": 1, "N": 1, "frames": 1, "H": 4, "W": 4, "h": 4, "w": 4, "Hi": 4, "Wi": 4, "Ho": 8,
             "Wo": 8, "HW": 16, "mode": 0, "border": 0, "act": 0, "k0": 5, "k1": 9, "k2": 13, "out_c": 64, "pos_rows": 16,
             "gate_is_logit": 0, "add_x": 0}
_LONG_ARGS = {"P": 16, "HW": 16, "rows": 16, "n": 64, "out_batch_stride": 4096}


def _bad_dtype_call(name, args, code):
    call = []
    for a in args:
        kind, arg = a.rsplit(" ", 1)
        if "*" in a:
            call.append(P16)
        elif kind == "hipStream_t":
            call.append(None)
        elif arg == "dtype":
            call.append(code)
        elif kind == "long":
            call.append(ctypes.c_long(_LONG_ARGS[arg]))
        elif kind == "float":
            call.append(ctypes.c_float(1.0))
        elif kind == "double":
            call.append(ctypes.c_double(0.5))
        elif arg.endswith("ld"):
            call.append(64)
        elif arg.endswith("coff"):
            call.append(0)
        else:
            assert kind == "int", (name, a)
            call.append(_INT_ARGS[arg])
    return getattr(_lib(), name)(*call)


_STRUCT_CALLS = {
    "flair_conv_nhwc": lambda code: _conv(_conv_params(code)),
    "flair_conv_chain": lambda code: _chain(_chain_params(code)),
    "flair_groupnorm_nhwc": lambda code: _gn(code),
    "flair_qkv_attention": lambda code: _attn(192, 64, dtype=code),
    "flair_temporal_attention": lambda code: _tattn(192, 64, dtype=code),
    "flair_dcn_align": lambda code: _dcn(code),
    "flair_attention_wide": lambda code: _wide(code),
}


def test_the_header_lists_the_dtype_entries():
    direct, by_struct = _dtype_entries()
    assert len(direct) >= 26 and "flair_scale_pixels" in direct and "flair_resize_nhwc" in direct
    assert set(by_struct) == set(_STRUCT_CALLS)


@pytest.mark.parametrize("name", _dtype_entries()[0] + _dtype_entries()[1])
def test_entries_refuse_an_unknown_dtype(name):
    if name in _dtype_entries()[1]:
        assert name in _STRUCT_CALLS, f"{name} takes a params struct with a dtype: give it a call in _STRUCT_CALLS"
        rc = _STRUCT_CALLS[name](7)
    else:
        rc = _bad_dtype_call(name, _header()[0][name], 7)
    _refused(rc, name, "dtype")


# ------------------------------------------------------------------------------------------------ the finite input guard
def test_a_finite_guard_wins_an_arg_max_that_reads_past_n():
    """tests/test_gpu_prior_strides.py surrounds flair_argmax_codebook's logits with ARGMAX_FILL instead of NaN: `NaN > best`
    is false, so an arg-max that read one channel past N would never pick a NaN guard; it always picks this one."""
    from tests.util import ARGMAX_FILL
    assert ARGMAX_FILL == float(torch.tensor(ARGMAX_FILL, dtype=torch.bfloat16))      # exact in bf16
    for dtype in (torch.float32, torch.bfloat16):
        N = 37
        buf, view = guarded(1, 2, 3, N, dtype, "cpu", coff=8, ld=N + 16, fill=ARGMAX_FILL)
        logits = torch.randn(1, 2, 3, N, generator=torch.Generator().manual_seed(0)) * 50
        view.copy_(logits.to(dtype))
        rows = buf[1].reshape(6, -1).float()
        assert torch.equal(rows[:, 8:8 + N].argmax(1), logits.to(dtype).float().reshape(6, N).argmax(1))
        assert torch.all(rows[:, 8:8 + N + 1].argmax(1) == N)           # one channel too many: the guard wins, every row
        assert torch.all(rows[:, 7:8 + N].argmax(1) == 0)               # one channel before the view: likewise
        nan_buf, nan_view = guarded(1, 2, 3, N, dtype, "cpu", coff=8, ld=N + 16, fill=IN_FILL)
        nan_view.copy_(logits.to(dtype))
        r = nan_buf[1].reshape(6, -1).float()[:, 8:8 + N + 1]
        best = torch.full((6,), float("-inf"))
        pick = torch.zeros(6, dtype=torch.long)
        for n in range(N + 1):                                          # the kernel's `v > best` scan: NaN never wins
            win = r[:, n] > best
            best, pick = torch.where(win, r[:, n], best), torch.where(win, torch.full_like(pick, n), pick)
        assert torch.all(pick < N)


def test_flat_guard_flags_strays():
    from tests.util import assert_flat_untouched, flat_guarded
    buf, v, before = flat_guarded((2, 3, 4), torch.bfloat16, "cpu", OUT_FILL, torch.arange(24.0))
    assert buf.numel() == 24 + 128 and v.is_contiguous() and v.data_ptr() == buf[64:].data_ptr()
    v.mul_(2)
    assert_flat_untouched(buf, before, v)
    with pytest.raises(AssertionError, match="read-only"):
        assert_flat_untouched(buf, before)
    for i in (63, 64 + 24):
        b2 = buf.clone()
        b2[i] = 0.0
        with pytest.raises(AssertionError, match="outside the tensor"):
            assert_flat_untouched(b2, before, b2[64:88].view(2, 3, 4))
