"""Tensor-level wrappers over the C ABI (include/flair_hip.h).

Every function takes torch tensors that live in HBM, passes raw pointers / sizes to
libflair_hip.so on torch's current HIP stream and returns torch tensors.  Activations
are *clip tensors*: shape (T, H, W, C), C innermost, dtype float32 or bfloat16.
PyTorch only provides memory and streams here; no torch operator computes anything.
"""
import ctypes

import torch

from ._header import STRUCTS
from ._lib import ACT_DCN_OFFSETS, ACT_GELU, ACT_LRELU01, ACT_LRELU02, ACT_NONE, ACT_RELU, ACT_SILU, ConvParams, call, dtype_code, lib
from ._lib import check, ptr, stream  # noqa: F401  (for callers that drive lib() themselves)

__all__ = ["conv", "conv_chain", "group_norm", "nchw_to_clip", "clip_to_nchw", "timestep_embedding", "linear",
           "qkv_attention", "temporal_attention", "flow_warp", "flow_compose", "resize",
           "dcn_align", "dcn_raw_permutation", "scale_pixels", "predict_xstart", "sampler_update",
           "ACT_NONE", "ACT_RELU", "ACT_LRELU01", "ACT_SILU", "ACT_DCN_OFFSETS", "ACT_LRELU02", "ACT_GELU"]


# the parameter structs of the header (their layouts are derived from it: _header.py)
GnParams, SamplerCoefs, AttnParams = STRUCTS["flair_gn_params"], STRUCTS["flair_sampler_coefs"], STRUCTS["flair_attn_params"]
TAttnParams, DcnParams, ChainParams = STRUCTS["flair_tattn_params"], STRUCTS["flair_dcn_params"], STRUCTS["flair_chain_params"]


def _ld(t):
    """Pixel stride (elements) of a clip tensor or channel-slice view of one."""
    assert t.dim() == 4 and t.stride(3) == 1, "clip tensors are (T,H,W,C) with C innermost"
    ld = t.stride(2)
    assert t.stride(1) == ld * t.shape[2] and (t.shape[0] == 1 or t.stride(0) == ld * t.shape[1] * t.shape[2]), \
        "clip tensor must be dense over (T,H,W)"
    return ld


def _dense(t):
    """A per-channel parameter (bias, norm scale, flow): contiguous; that it is float32 is for the call to refuse, by name."""
    assert t is None or t.is_contiguous()
    return t


def k_align(dtype):
    """Channel granularity of a conv input segment (one 64-byte K step)."""
    return 32 if dtype == torch.bfloat16 else 16


def pad_channels(c, dtype):
    g = k_align(dtype)
    return (c + g - 1) // g * g


# --------------------------------------------------------------------------- conv
def conv(xs, weight, bias, cout, kernel, *, out=None, act=ACT_NONE, res0=None, res1=None,
         out_scale=1.0, stride=1, frame_bias=None, act_param=0.0, act_period=0, asym_pad=False, reflect_pad=False):
    """Y = act(conv(cat(xs), W) + bias) + res0 + res1, times out_scale.

    xs: one clip tensor or a list of up to 4 (channel-concatenated implicitly; each
    width a multiple of ``k_align``); weight: packed [cout][taps][sum C] in the
    activation dtype; kernel: (KT, KH, KW); out: optional (T,H,W,>=cout) view.
    """
    if isinstance(xs, torch.Tensor):
        xs = [xs]
    x0 = xs[0]
    T, H, W, _ = x0.shape
    p = ConvParams()
    p.dtype = dtype_code(x0)
    p.T, p.H, p.W = T, H, W
    p.KT, p.KH, p.KW = kernel
    p.Cout = cout
    p.nseg = len(xs)
    arr = (ctypes.c_void_p * 4)()
    for i, x in enumerate(xs):
        assert x.dtype == x0.dtype and x.shape[:3] == x0.shape[:3]
        p.seg_c[i] = x.shape[3]
        p.seg_ld[i] = _ld(x)
        arr[i] = x.data_ptr()
    p.stride = stride
    p.asym_pad = asym_pad
    p.reflect_pad = reflect_pad
    p.frame_bias_ld = frame_bias.stride(0) if frame_bias is not None else 0
    if frame_bias is not None:
        assert frame_bias.dtype == torch.float32 and frame_bias.stride(1) == 1 and frame_bias.shape[0] == T
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    if out is None:
        out = torch.empty((T, Ho, Wo, cout), dtype=x0.dtype, device=x0.device)
    assert tuple(out.shape[:3]) == (T, Ho, Wo) and out.shape[3] >= cout and out.dtype == x0.dtype
    p.y_ld = _ld(out)
    p.res_ld[0] = _ld(res0) if res0 is not None else 0
    p.res_ld[1] = _ld(res1) if res1 is not None else 0
    p.act = act
    p.act_param, p.act_period = act_param, act_period
    p.out_scale = out_scale
    assert weight.dtype == x0.dtype and weight.is_contiguous()
    e0 = _prof_begin()
    wsb = _conv_ws_bytes(p)
    ws = _workspace(wsb, x0.device, "conv") if wsb else None

    def launch(_keep=xs):       # the segment tensors reach the library as raw pointers: keep them alive with the closure
        call.flair_conv_nhwc(ctypes.byref(p), arr, weight, _dense(bias), frame_bias, res0, res1, out, ws, wsb)
    launch()
    if e0 is not None:
        cin = sum(x.shape[3] for x in xs)
        taps = kernel[0] * kernel[1] * kernel[2]
        esz = x0.element_size()
        flops = 2.0 * T * Ho * Wo * cout * cin * taps
        nbytes = esz * (cin * T * H * W + cout * T * Ho * Wo * (1 + (res0 is not None) + (res1 is not None))
                        + cout * taps * cin)
        _prof_end(e0, ("conv", lib().flair_conv_variant(ctypes.byref(p))), x0.dtype, flops, nbytes, launch,
                  ("conv", T, H, W, tuple(x.shape[3] for x in xs), cout, tuple(kernel), stride, act,
                   res0 is not None, res1 is not None, frame_bias is not None))
    return out


# bench.py sets PROFILE to a list to bracket every conv / GroupNorm / alignment / attention call with HIP
# events on the launch stream (roofline leg): entries are (family, dtype name, algorithmic FLOPs,
# algorithmic bytes, start event, end event).
PROFILE = None


def _prof_begin():
    if PROFILE is None:
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0


def _prof_end(e0, family, dtype, flops, nbytes, replay=None, sig=None):
    """replay: closure that re-issues the identical library call (its arguments stay alive with it), so that bench.py can
    time every distinct launch shape by hipGraph replay of back-to-back launches; sig: hashable shape signature."""
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    PROFILE.append((family, str(dtype), float(flops), float(nbytes), e0, e1, replay, sig))


def conv_variant(T, H, W, cins, cout, kernel, dtype=torch.bfloat16, stride=1, act=ACT_NONE):
    """Kernel variant flair_conv_nhwc dispatches this geometry to (flair_conv_variant); host-only.  The activation is part
    of the choice: GELU stays off the LDS-DMA kernels."""
    p = ConvParams()
    p.dtype = 1 if dtype == torch.bfloat16 else 0      # FLAIR_BF16 / FLAIR_F32
    p.T, p.H, p.W = T, H, W
    p.KT, p.KH, p.KW = kernel
    p.Cout = cout
    p.nseg = len(cins)
    for i, c in enumerate(cins):
        p.seg_c[i] = c
        p.seg_ld[i] = c
    p.stride = stride
    p.y_ld = cout
    p.act = act
    return lib().flair_conv_variant(ctypes.byref(p))


def _conv_ws_bytes(p):
    return lib().flair_conv_workspace_bytes(ctypes.byref(p))


def pack_conv_weight(w, seg_channels, dtype, cout_pad=None):
    """Reference layout (Cout, Cin, *k) f32 -> [Cout_pad][taps][sum padded seg] in `dtype`.

    ``seg_channels``: list of (real, padded) channel counts of the input segments, in
    concatenation order.  One-time repack at load (plain tensor plumbing).
    """
    cout, cin = w.shape[:2]
    taps = 1
    for k in w.shape[2:]:
        taps *= k
    w = w.reshape(cout, cin, taps).permute(0, 2, 1).float()  # cout, taps, cin
    parts, o = [], 0
    for real, padded in seg_channels:
        seg = w[:, :, o:o + real]
        if padded > real:
            seg = torch.cat([seg, seg.new_zeros(cout, taps, padded - real)], dim=2)
        parts.append(seg)
        o += real
    assert o == cin, (o, cin)
    w = torch.cat(parts, dim=2)
    if cout_pad is not None and cout_pad > cout:
        w = torch.cat([w, w.new_zeros(cout_pad - cout, taps, w.shape[2])], dim=0)
    return w.to(dtype).contiguous()


# ---------------------------------------------------------------- fused conv chains
def chain_supported(xs, c_mid):
    """Where the fused chain kernel is used: the geometry flair_conv_chain covers (W a multiple of 8, 64 or 128
    mid channels) AND a launch of at most ~2 workgroups per CU (per-frame calls of the recurrence).  Clip-level
    calls (thousands of tiles) stay on the two-launch path: there independent workgroups, two per CU, already
    overlap each other's fetch / MFMA / store phases, which one 135 KB workgroup per CU cannot."""
    x0 = xs[0] if isinstance(xs, (list, tuple)) else xs
    T, H, W, _ = x0.shape
    tiles = T * ((H + 7) // 8) * (W // 32 if W % 32 == 0 and T * ((H + 7) // 8) * (W // 32) >= 192 else W // 8)
    return c_mid in (64, 128) and W % 8 == 0 and tiles <= 512


def conv_chain(xs, wA, bA, actA, wB, bB, actB, c_mid, coutB, *, res0=None, res1=None, out_scale=1.0, out=None,
               act_param=0.0, act_period=0):
    """Y = (actB(conv3x3(actA(conv3x3(cat(xs), wA) + bA), wB) + bB) + res0 + res1) * out_scale in ONE launch
    (the c_mid-channel intermediate stays in LDS).  wA=None: no first stage; xs is the c_mid-channel input,
    staged once and kept resident while coutB output channels are produced (wide-output convolutions)."""
    if isinstance(xs, torch.Tensor):
        xs = [xs]
    x0 = xs[0]
    T, H, W, _ = x0.shape
    p = ChainParams()
    p.dtype = dtype_code(x0)
    p.T, p.H, p.W = T, H, W
    p.C, p.CoutB = c_mid, coutB
    p.nseg = len(xs)
    arr = (ctypes.c_void_p * 4)()
    for i, x in enumerate(xs):
        assert x.dtype == x0.dtype and x.shape[:3] == x0.shape[:3]
        p.seg_c[i] = x.shape[3]
        p.seg_ld[i] = _ld(x)
        arr[i] = x.data_ptr()
    if out is None:
        out = torch.empty((T, H, W, coutB), dtype=x0.dtype, device=x0.device)
    assert tuple(out.shape[:3]) == (T, H, W) and out.shape[3] >= coutB and out.dtype == x0.dtype
    p.y_ld = _ld(out)
    p.res_ld[0] = _ld(res0) if res0 is not None else 0
    p.res_ld[1] = _ld(res1) if res1 is not None else 0
    p.actA, p.actB = actA, actB
    p.act_param, p.act_period = act_param, act_period
    p.out_scale = out_scale
    assert wB.dtype == x0.dtype and wB.is_contiguous() and (wA is None or (wA.dtype == x0.dtype and wA.is_contiguous()))
    e0 = _prof_begin()

    def launch(_keep=xs):
        call.flair_conv_chain(ctypes.byref(p), arr, wA, _dense(bA), wB, _dense(bB), res0, res1, out)
    launch()
    if e0 is not None:
        cin = sum(x.shape[3] for x in xs)
        esz = x0.element_size()
        px = T * H * W
        flops = 2.0 * 9 * px * (c_mid * coutB + (cin * c_mid if wA is not None else 0))
        nbytes = esz * (px * (cin + coutB * (1 + (res0 is not None) + (res1 is not None)))
                        + 9 * c_mid * coutB + (9 * cin * c_mid if wA is not None else 0))
        _prof_end(e0, ("chain", 2 if wA is not None else 1, c_mid), x0.dtype, flops, nbytes, launch,
                  ("chain", T, H, W, tuple(x.shape[3] for x in xs), c_mid, coutB, wA is not None, res0 is not None,
                   res1 is not None))
    return out


# --------------------------------------------------------------------- group norm
_gn_ws = {}


def _workspace(nbytes, device, tag="gn"):
    key = (tag, device, torch.cuda.current_stream().cuda_stream)
    buf = _gn_ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _gn_ws[key] = buf
    return buf


def group_norm(x, gamma, beta, *, x1=None, groups=32, eps=1e-5, act=ACT_NONE, film=None,
               frames_per_stat=None, resample=0, out=None, want_raw=False):
    """act(GN(cat(x, x1)) * (1+scale) + shift) with optional 2x resampling.

    film: (F, >=2C) f32 rows (scale | shift) or None.  resample: 0 / 1 (avg-pool 2) /
    2 (nearest x2).  Returns y, or (y, raw) when ``want_raw``.
    """
    T, H, W, c0 = x.shape
    C = c0 + (x1.shape[3] if x1 is not None else 0)
    p = GnParams()
    p.dtype = dtype_code(x)
    p.C, p.c0 = C, c0
    p.ld0 = _ld(x)
    p.ld1 = _ld(x1) if x1 is not None else 0
    p.groups = groups
    p.F, p.H, p.W = T, H, W
    p.frames_per_stat = frames_per_stat or T
    p.eps = eps
    p.act = act
    p.resample = resample
    Ho, Wo = (H // 2, W // 2) if resample == 1 else ((H * 2, W * 2) if resample == 2 else (H, W))
    if out is None:
        out = torch.empty((T, Ho, Wo, C), dtype=x.dtype, device=x.device)
    raw = torch.empty((T, Ho, Wo, C), dtype=x.dtype, device=x.device) if want_raw else None
    p.y_ld = _ld(out)
    p.raw_ld = _ld(raw) if raw is not None else 0
    p.film_ld = film.stride(0) if film is not None else 0
    if film is not None:
        assert film.dtype == torch.float32 and film.stride(1) == 1 and film.shape[0] == T
    ws = _workspace(lib_ws_bytes(p), x.device)
    e0 = _prof_begin()

    def launch():
        call.flair_groupnorm_nhwc(ctypes.byref(p), x, x1, _dense(gamma), _dense(beta), film, out, raw, ws)
    launch()
    if e0 is not None:   # two-pass GroupNorm: the input is read twice, the output written once
        numel_in, numel_out = T * H * W * C, T * Ho * Wo * C
        _prof_end(e0, ("gn",), x.dtype, 8.0 * numel_in,
                  x.element_size() * (2 * numel_in + numel_out * (2 if want_raw else 1)), launch,
                  ("gn", T, H, W, C, c0, groups, p.frames_per_stat, act, resample, want_raw, film is not None))
    return (out, raw) if want_raw else out


def lib_ws_bytes(p):
    return lib().flair_groupnorm_workspace_bytes(ctypes.byref(p))


# ------------------------------------------------------------------ edge / small ops
def nchw_to_clip(src, dst, coff=0):
    """(N,C,H,W) f32 -> channels [coff, coff+C) of clip tensor dst (N,H,W,Cd)."""
    N, C, H, W = src.shape
    assert src.dtype == torch.float32 and src.is_contiguous()
    call.flair_nchw_f32_to_nhwc(src, N, C, H, W, dst, dtype_code(dst), _ld(dst), coff)
    return dst


def clip_to_nchw(src, C, coff=0, out=None):
    N, H, W, _ = src.shape
    if out is None:
        out = torch.empty((N, C, H, W), dtype=torch.float32, device=src.device)
    call.flair_nhwc_to_nchw_f32(src, dtype_code(src), _ld(src), coff, N, C, H, W, out)
    return out


def timestep_embedding(t, dim, max_period=10000.0, out=None, sin_first=False):
    """t: (N,) f32 device tensor -> (N, dim) f32 ([cos|sin], or [sin|cos] when sin_first)."""
    assert t.dtype == torch.float32 and t.is_contiguous()
    N = t.shape[0]
    if out is None:
        out = torch.empty((N, dim), dtype=torch.float32, device=t.device)
    call.flair_timestep_embedding(t, N, dim, max_period, sin_first, out)
    return out


def linear(x, w, b, *, act_in=ACT_NONE, act_out=ACT_NONE, out=None):
    """f32 (M<=32, K) @ (N, K)^T + b."""
    M, K = x.shape
    N = w.shape[0]
    assert x.dtype == torch.float32 and w.dtype == torch.float32 and x.is_contiguous() and w.is_contiguous()
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    call.flair_linear_f32(x, M, K, w, b, N, act_in, act_out, out, out.stride(0))
    return out


def qkv_attention(qkv, heads, *, new_order=False, out=None):
    """qkv: (F, H, W, 3C) clip tensor -> (F, H, W, C)."""
    F_, H, W, C3 = qkv.shape
    C = C3 // 3
    p = AttnParams()
    p.dtype = dtype_code(qkv)
    p.frames, p.L, p.heads, p.head_dim = F_, H * W, heads, C // heads
    p.ld = _ld(qkv)
    if out is None:
        out = torch.empty((F_, H, W, C), dtype=qkv.dtype, device=qkv.device)
    p.out_ld = _ld(out)
    d = C // heads
    if new_order:
        p.q_off, p.k_off, p.v_off, p.head_stride = 0, C, 2 * C, d
    else:
        p.q_off, p.k_off, p.v_off, p.head_stride = 0, d, 2 * d, 3 * d
    p.scale = 1.0 / (d ** 0.5)
    e0 = _prof_begin()

    def launch():
        call.flair_qkv_attention(ctypes.byref(p), qkv, out)
    launch()
    if e0 is not None:   # QK^T + AV: 4 * frames * heads * L^2 * d FLOPs; q, k, v read + out written
        L = H * W
        _prof_end(e0, ("attn", L), qkv.dtype, 4.0 * F_ * heads * L * L * d, qkv.element_size() * 4.0 * F_ * L * C,
                  launch, ("attn", F_, L, heads, d, new_order))
    return out


def temporal_attention(qkv, kpos, window, *, round_fp16, head_dim=64, out=None):
    """qkv: (T, H, W, 3C) clip tensor of q | k | v, C = heads * head_dim -> (T, H, W, C); softmax scale
    1/sqrt(head_dim) (flash_attn_func's default)."""
    T, H, W, C3 = qkv.shape
    C = C3 // 3
    p = TAttnParams()
    p.dtype = dtype_code(qkv)
    p.T, p.H, p.W, p.C, p.window = T, H, W, C, window
    p.ld = _ld(qkv)
    if out is None:
        out = torch.empty((T, H, W, C), dtype=qkv.dtype, device=qkv.device)
    p.out_ld = _ld(out)
    p.round_fp16 = round_fp16
    p.head_dim = head_dim
    p.scale = 1.0 / (head_dim ** 0.5)
    assert kpos.shape == (window - 1, C)
    call.flair_temporal_attention(ctypes.byref(p), qkv, _dense(kpos), out)
    return out


def flow_warp(x, flow, *, border=False, out=None):
    """x: (F,H,W,C) clip tensor; flow: (F,H,W,2) f32 (dx,dy)."""
    F_, H, W, C = x.shape
    assert flow.dtype == torch.float32 and flow.shape == (F_, H, W, 2)
    if out is None:
        out = torch.empty((F_, H, W, C), dtype=x.dtype, device=x.device)
    call.flair_flow_warp(x, dtype_code(x), _ld(x), flow, _ld(flow), F_, H, W, C, border, out, _ld(out))
    return out


def flow_compose(f1, f2, out=None):
    F_, H, W, _ = f1.shape
    assert f1.dtype == torch.float32 and f1.is_contiguous() and f2.is_contiguous()
    if out is None:
        out = torch.empty_like(f1)
    call.flair_flow_compose(f1, f2, F_, H, W, out)
    return out


RESIZE_BILINEAR, RESIZE_BILINEAR_AC, RESIZE_BICUBIC, RESIZE_AVGPOOL2, RESIZE_NEAREST = 0, 1, 2, 3, 4


def resize(x, size, mode, *, channels=None, out=None, scale_c0=1.0, scale_c1=1.0):
    F_, Hi, Wi, Cx = x.shape
    C = channels or Cx
    Ho, Wo = size
    if out is None:
        out = torch.zeros((F_, Ho, Wo, Cx), dtype=x.dtype, device=x.device)
    call.flair_resize_nhwc(x, dtype_code(x), _ld(x), F_, Hi, Wi, C, mode, Ho, Wo, out, _ld(out), scale_c0, scale_c1)
    return out


def dcn_raw_permutation(groups):
    """Index tensor taking the reference's conv_offset channel order (o1 | o2 | mask with
    group-major (g*9+k) indexing, unet_new.py:877-885) to the tap-major order flair_dcn_align
    reads (tap k owns channels [3Gk, 3G(k+1))): new[3Gk + 2g + e] = old[2*(g*9+k)+e],
    new[3Gk + 2G + g] = old[18G + g*9 + k].
    Applied to the OUTPUT channels of the last conv_offset convolution when it is packed."""
    G = groups
    perm = torch.empty(27 * G, dtype=torch.long)
    for k in range(9):
        for g in range(G):
            for e in range(2):
                perm[3 * G * k + 2 * g + e] = 2 * (g * 9 + k) + e
            perm[3 * G * k + 2 * G + g] = 18 * G + g * 9 + k
    return perm


def dcn_align(x0, x1, raw, flow1, flow2, weight, bias, cout, *, groups=16, max_mag=10.0, out=None, raw_activated=False):
    """raw: conv_offset output in TAP-MAJOR channel order (see dcn_raw_permutation); raw_activated: the producing
    convolution already applied ACT_DCN_OFFSETS (max_mag * tanh on the residues, sigmoid on the masks); 2: VQFR's
    DCNv2Pack (offsets as they are, sigmoid on the masks; no flows, x0 | x1 the channel halves of one input:
    see dcn_pack)."""
    F_, H, W, ch = x0.shape
    p = DcnParams()
    p.dtype = dtype_code(x0)
    p.F, p.H, p.W = F_, H, W
    p.Cin, p.Cout, p.G = 2 * ch, cout, groups
    p.x_ld[0], p.x_ld[1] = _ld(x0), _ld(x1)
    p.raw_ld = _ld(raw)
    if out is None:
        out = torch.empty((F_, H, W, cout), dtype=x0.dtype, device=x0.device)
    p.y_ld = _ld(out)
    p.max_residue_magnitude = max_mag
    p.raw_activated = raw_activated
    e0 = _prof_begin()

    def launch():
        call.flair_dcn_align(ctypes.byref(p), x0, x1, raw, flow1, flow2, weight, _dense(bias), out)
    launch()
    if e0 is not None:   # bytes = esz*(2c + 27G + c)*H*W; FLOPs = 2*9*2c*c*H*W + 9*2c*H*W*8
        px = F_ * H * W
        _prof_end(e0, ("dcn", cout), x0.dtype, px * (2.0 * 9 * 2 * ch * cout + 9.0 * 2 * ch * 8),
                  x0.element_size() * px * (2 * ch + 27 * groups + cout), launch,
                  ("dcn", F_, H, W, ch, cout, groups, flow2 is not None))
    return out


def dcn_pack(x, raw, weight, bias, cout, *, groups, out=None):
    """VQFR's DCNv2Pack.forward after conv_offset (vqfr.py:352-380): modulated deformable 3x3 convolution of the clip
    tensor x with the offsets of ``raw`` taken as they are and sigmoid(mask) (flair_dcn_align, raw_activated = 2).
    raw: conv_offset's output in tap-major order (dcn_raw_permutation), pixel stride 16-byte granular."""
    c = x.shape[3]
    assert c % 2 == 0
    return dcn_align(x[..., :c // 2], x[..., c // 2:], raw, None, None, weight, bias, cout, groups=groups, out=out,
                     raw_activated=2)


def scale_pixels(x, wmap):
    T, H, W, C = x.shape
    call.flair_scale_pixels(x, dtype_code(x), _ld(x), C, T * H * W, _dense(wmap))
    return x


# ------------------------------------------------------------------------ sampler
def predict_xstart(x, model_out, c_recip, c_recipm1, clip, out=None):
    N, C, H, W = x.shape
    Cm = model_out.shape[1]
    assert x.dtype == torch.float32 and x.is_contiguous() and model_out.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    call.flair_predict_xstart(x, model_out, N, C, Cm, H, W, c_recip, c_recipm1, clip, out)
    return out


def sampler_update(coefs, x, x0, restored, aux, z, prev_recon, out=None):
    if out is None:
        out = torch.empty_like(x)
    for t in (x, x0, restored, aux, z, prev_recon):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    call.flair_sampler_update(ctypes.byref(coefs), x, x0, restored, aux, z, prev_recon, x.numel(), out)
    return out


def affine_channels(x, C, a, b, lo, hi, sub, mul, out):
    """f32 clip tensors: out = (clamp(x*a+b, lo, hi) - sub[c]) * mul[c] on the first C channels."""
    T, H, W, _ = x.shape
    assert x.dtype == torch.float32 and out.dtype == torch.float32
    call.flair_affine_channels_f32(x, _ld(x), C, T * H * W, a, b, lo, hi, sub, mul, out, _ld(out))
    return out


def add_frame_bias(x, bias):
    T, H, W, C = x.shape
    assert bias.dtype == torch.float32 and bias.stride(1) == 1
    call.flair_add_frame_bias(x, dtype_code(x), _ld(x), C, T, H * W, bias, bias.stride(0))
    return x


def cast_channels(src, dst, coff=0):
    """src: (T,H,W,C) f32 -> channels [coff, coff+C) of clip tensor dst."""
    T, H, W, C = src.shape
    assert src.dtype == torch.float32
    call.flair_cast_channels(src, _ld(src), C, T * H * W, dst, dtype_code(dst), _ld(dst), coff)
    return dst


def axpby(x, y, a, b, out=None, lo=float("-inf"), hi=float("inf")):
    """out = clamp(a*x + b*y, lo, hi) on flat f32 tensors (y may be None)."""
    assert x.dtype == torch.float32 and x.is_contiguous() and (y is None or y.is_contiguous())
    if out is None:
        out = torch.empty_like(x)
    call.flair_axpby_f32(x, y, a, b, lo, hi, x.numel(), out)
    return out


def learned_range_variance(model_out, C, min_log, max_log, out=None):
    """out: optional (variance, log_variance) pair of contiguous (N,C,H,W) f32 tensors."""
    N, C2, H, W = model_out.shape
    if out is None:
        var = torch.empty((N, C, H, W), dtype=torch.float32, device=model_out.device)
        logvar = torch.empty_like(var)
    else:
        var, logvar = out
        assert all(t.dtype == torch.float32 and t.is_contiguous() and t.shape == (N, C, H, W) for t in out)
    call.flair_learned_range_variance(model_out, N, C, H, W, min_log, max_log, var, logvar)
    return var, logvar


# ------------------------------------------------------------------- degradation ops
def depthwise_filter(x, filt, *, pad, out_stride=1, out_offset=0, stuff=1, stuff_offset=0, out_hw=None,
                     reflect=False, out=None):
    """x: (N,C,H,W) f32; filt: (kh,kw) f32 device tensor shared by all planes; out: optional contiguous (N,C,*out_hw)."""
    N, C, H, W = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and filt.dtype == torch.float32 and filt.is_contiguous()
    Ho, Wo = out_hw
    if out is None:
        out = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (N, C, Ho, Wo)
    call.flair_depthwise_filter(x, N * C, H, W, filt, filt.shape[0], filt.shape[1], pad, out_stride, out_offset, stuff,
         stuff_offset, Ho, Wo, reflect, out)
    return out


def jpeg_roundtrip(x, q_luma, q_chroma, dct8, want_levels=False, entry="hw", out=None, levels=None, workspace=None):
    """x: (N,3,H,W) f32 in [-1,1], H and W multiples of 16; tables: python sequences / numpy arrays of 64 floats (host).
    want_levels: also return the quantised integer levels [luma (N,1,H,W), chroma (N,2,H/2,W/2)] (f32).
    entry: "hw" = flair_jpeg_roundtrip_hw (one launch, any H x W); "square" = the three-launch flair_jpeg_roundtrip
    with its workspace (H == W only).  The two agree bit for bit on squares (tests/test_gpu_rect.py) and "hw" is the
    faster one (43.6 against 76.0 us at 10 x 3 x 128 x 128), so it serves every shape.
    out, levels = (luma, chroma) and workspace (square entry): optional contiguous f32 tensors of those shapes to write to."""
    N, C, H, W = x.shape
    assert C == 3 and x.dtype == torch.float32 and x.is_contiguous()
    if H % 16 or W % 16:
        raise ValueError(f"jpeg_roundtrip: the codec works on whole 16x16 MCUs, got {H}x{W}")
    if entry not in ("hw", "square"):
        raise ValueError(f"jpeg_roundtrip: unknown entry {entry!r}")
    arr = ctypes.c_float * 64
    tables = [arr(*[float(v) for v in t]) for t in (q_luma, q_chroma, dct8)]
    if out is None:
        out = torch.empty_like(x)
    if levels is not None:
        want_levels = True
        luma, chroma = levels
    else:
        luma = torch.empty((N, 1, H, W), dtype=torch.float32, device=x.device) if want_levels else None
        chroma = torch.empty((N, 2, H // 2, W // 2), dtype=torch.float32, device=x.device) if want_levels else None
    for t, shape in ((out, (N, 3, H, W)), (luma, (N, 1, H, W)), (chroma, (N, 2, H // 2, W // 2)), (workspace, (N, 3, H, W))):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.shape == shape), (t.shape, shape)
    if entry == "square":
        if H != W:
            raise ValueError(f"jpeg_roundtrip: the square entry cannot take {H}x{W}")
        ws = torch.empty_like(x) if workspace is None else workspace
        call.flair_jpeg_roundtrip(x, N, H, *tables, ws, out, luma, chroma)
    else:
        call.flair_jpeg_roundtrip_hw(x, N, H, W, *tables, out, luma, chroma)
    return (out, [luma, chroma]) if want_levels else out


def matmul(a, b, out=None):
    """Batched f32 matmul; a: (B,M,K) or (M,K) shared; b: (B,K,N) or (K,N) shared; out: optional contiguous (B,M,N)."""
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous()
    batch = a.shape[0] if a.dim() == 3 else (b.shape[0] if b.dim() == 3 else 1)
    M, K = a.shape[-2:]
    N = b.shape[-1]
    assert b.shape[-2] == K
    if out is None:
        out = torch.empty((batch, M, N), dtype=torch.float32, device=a.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (batch, M, N)
    call.flair_matmul_f32(a, M * K if a.dim() == 3 else 0, b, K * N if b.dim() == 3 else 0, out, batch, M, N, K)
    return out


def gather_mac(x, outer, lin, inner, fov, w, out=None):
    """Resizer step: x viewed [outer][lin][inner] f32; fov int32 (taps,Lout); w f32 (taps,Lout); out: optional contiguous
    (outer, Lout, inner)."""
    taps, lout = fov.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and fov.dtype == torch.int32 and w.dtype == torch.float32
    if out is None:
        out = torch.empty((outer, lout, inner), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (outer, lout, inner)
    call.flair_gather_mac_f32(x, outer, lin, inner, fov.contiguous(), w.contiguous(), taps, lout, out)
    return out


def vsrpp_prep(prop, feat2, flow1, flow_prev, cond1, cond2, flow2_out, flowpad):
    """Fused alignment inputs of one BasicVSR++ step (see flair_vsrpp_prep).  One frame:
    prop/feat2/cond*: (1,H,W,c) clip tensors; flows: (1,H,W,2) f32; flowpad: (1,H,W,>=4)."""
    _, H, W, C = prop.shape
    second = flow_prev is not None
    e0 = _prof_begin()

    def launch():
        call.flair_vsrpp_prep(prop, _ld(prop), feat2 if second else None, _ld(feat2) if second else 0, _dense(flow1),
             _dense(flow_prev), dtype_code(prop), H, W, C, cond1, _ld(cond1), cond2 if second else None,
             _ld(cond2) if second else 0, flow2_out if second else None, flowpad, _ld(flowpad))
    launch()
    if e0 is not None:   # reads 1-2 features, writes 1-2 warped features + the 4-channel flow pad
        n = 2 if second else 1
        _prof_end(e0, ("prep",), prop.dtype, 0.0, prop.element_size() * H * W * (2.0 * n * C + flowpad.shape[3]) + 8.0 * H * W * n,
                  launch, ("prep", H, W, C, second))


def vsrpp_warp2(prop, feat2, flow1, flow2, cond1, cond2):
    """cond1 = warp(prop, flow1), cond2 = warp(feat2, flow2) in one launch (flair_vsrpp_warp2); flows precomposed."""
    _, H, W, C = prop.shape
    second = flow2 is not None
    e0 = _prof_begin()

    def launch():
        call.flair_vsrpp_warp2(prop, _ld(prop), feat2 if second else None, _ld(feat2) if second else 0, _dense(flow1),
             _dense(flow2) if second else None, dtype_code(prop), H, W, C, cond1, _ld(cond1), cond2 if second else None,
             _ld(cond2) if second else 0)
    launch()
    if e0 is not None:
        n = 2 if second else 1
        _prof_end(e0, ("prep",), prop.dtype, 0.0, prop.element_size() * H * W * 2.0 * n * C + 8.0 * H * W * n,
                  launch, ("warp2", H, W, C, second))


def add_act(x0, x1=None, act=ACT_NONE, out=None):
    """act(x0 + x1) on clip tensors (x1 may be None)."""
    T, H, W, C = x0.shape
    if out is None:
        out = torch.empty((T, H, W, C), dtype=x0.dtype, device=x0.device)
    call.flair_add_act_nhwc(x0, _ld(x0), x1, _ld(x1) if x1 is not None else 0, dtype_code(x0), C, T * H * W, act, out,
         _ld(out))
    return out


def dwconv(x, w_dw, b_dw, *, stride, pw=None, act=ACT_LRELU01, out=None):
    """MobileNet ``conv_dw`` block on an f32 clip tensor (flair_dwconv_nhwc): act(depthwise 3x3(x) + b_dw), then, when
    pw = (w_pw [Cout][C], b_pw [Cout]) is given, act(1x1 of that + b_pw) in the same launch.  w_dw: [9][C] f32 (BatchNorm folded);
    x has C = w_dw.shape[1] channels (padded to a multiple of 4); out: optional (T, ceil(H/s), ceil(W/s), >= Cout) view."""
    T, H, W, C = x.shape
    assert x.dtype == torch.float32 and tuple(w_dw.shape) == (9, C)
    w_pw, b_pw = pw if pw is not None else (None, None)
    cout = w_pw.shape[0] if w_pw is not None else C
    assert w_pw is None or tuple(w_pw.shape) == (cout, C)
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    if out is None:
        out = torch.empty((T, Ho, Wo, cout), dtype=torch.float32, device=x.device)
    assert tuple(out.shape[:3]) == (T, Ho, Wo) and out.shape[3] >= cout and out.dtype == torch.float32
    call.flair_dwconv_nhwc(x, _ld(x), T, H, W, C, stride, _dense(w_dw), _dense(b_dw), _dense(w_pw), _dense(b_pw), cout, act, out,
         _ld(out))
    return out


def dwconv7(x, w, b, *, out=None):
    """Depthwise 7x7 convolution, stride 1, zero padding 3 (flair_dwconv7_nhwc) of an f32 / bf16 clip tensor:
    w [49][C] f32 tap-major, b [C] f32 or None -> (T, H, W, C) in x's dtype (f32 accumulation)."""
    T, H, W, C = x.shape
    assert tuple(w.shape) == (49, C)
    if out is None:
        out = torch.empty((T, H, W, C), dtype=x.dtype, device=x.device)
    assert tuple(out.shape[:3]) == (T, H, W) and out.shape[3] >= C and out.dtype == x.dtype
    call.flair_dwconv7_nhwc(x, _ld(x), dtype_code(x), T, H, W, C, _dense(w), _dense(b), out, _ld(out))
    return out


def maxpool3x3s2(x, out=None):
    """nn.MaxPool2d(3, 2, 1) on a clip tensor."""
    T, H, W, C = x.shape
    if out is None:
        out = torch.empty((T, (H + 1) // 2, (W + 1) // 2, C), dtype=x.dtype, device=x.device)
    call.flair_maxpool3x3s2_nhwc(x, _ld(x), dtype_code(x), T, H, W, C, out, _ld(out))
    return out


# --------------------------------------------------------------------------- calibration launches (measurement only)
def probe_matrix_rate(iters, workgroups_per_cu=1, sink=None):
    """One launch of independent bf16 MFMA chains out of registers on every CU (flair_probe_matrix_rate); returns its FLOPs.
    The caller times it with events on the current stream."""
    if sink is None:
        sink = torch.zeros(4, dtype=torch.float32, device="cuda")
    flop = ctypes.c_double(0.0)
    call.flair_probe_matrix_rate(int(iters), int(workgroups_per_cu), sink, ctypes.byref(flop))
    return flop.value


def probe_stream_rate(src, dst, mode):
    """mode 0: read src, 1: write dst, 2: copy src -> dst (uint8 / any contiguous device tensors of equal size); returns the bytes moved."""
    n = dst.numel() * dst.element_size()
    if mode != 1:
        assert src.numel() * src.element_size() == n
    call.flair_probe_stream_rate(src if mode != 1 else None, dst, n, int(mode))
    return n * (2 if mode == 2 else 1)


def gated_blend(x, m, gate, out=None):
    """x + sigmoid(gate[f, c]) * (m - x); gate: (F, >=C) f32 logits."""
    T, H, W, C = x.shape
    assert gate.dtype == torch.float32 and gate.stride(1) == 1 and gate.shape[0] == T
    if out is None:
        out = torch.empty_like(x)
    call.flair_gated_blend(x, _ld(x), m, _ld(m), gate, gate.stride(0), dtype_code(x), C, T, H * W, out, _ld(out))
    return out


# --------------------------------------------------------------------------- CodeFormer prior pieces
def layer_norm(x, gamma, beta, *, eps=1e-5, pos=None, out=None, out_pos=None):
    """nn.LayerNorm over the channels of every pixel of a clip tensor.  With ``pos`` ((rows_per_frame, C) f32)
    also returns y + pos (broadcast over frames): -> y or (y, y_pos)."""
    F_, H, W, C = x.shape
    if out is None:
        out = torch.empty((F_, H, W, C), dtype=x.dtype, device=x.device)
    if pos is not None and out_pos is None:
        out_pos = torch.empty((F_, H, W, C), dtype=x.dtype, device=x.device)
    if pos is not None:
        assert pos.dtype == torch.float32 and pos.is_contiguous() and pos.shape == (H * W, C)
    call.flair_layernorm_nhwc(x, dtype_code(x), _ld(x), F_ * H * W, C, _dense(gamma), _dense(beta), eps, out, _ld(out), pos,
         H * W if pos is not None else 0, out_pos, _ld(out_pos) if pos is not None else 0)
    return out if pos is None else (out, out_pos)


def attention_wide(qkv, heads, head_dim, *, q_off, k_off, v_off, head_stride, out=None):
    """Attention over the H*W pixels of each frame with heads of any width (flair_attention_wide)."""
    F_, H, W, _ = qkv.shape
    p = AttnParams()
    p.dtype = dtype_code(qkv)
    p.frames, p.L, p.heads, p.head_dim = F_, H * W, heads, head_dim
    p.ld = _ld(qkv)
    if out is None:
        out = torch.empty((F_, H, W, heads * head_dim), dtype=qkv.dtype, device=qkv.device)
    p.out_ld = _ld(out)
    p.q_off, p.k_off, p.v_off, p.head_stride = q_off, k_off, v_off, head_stride
    p.scale = 1.0 / (head_dim ** 0.5)
    call.flair_attention_wide(ctypes.byref(p), qkv, out)
    return out


def argmax_codebook(logits, n_codes, codebook, *, forced_idx=None, out=None):
    """logits: (F,H,W,>=n_codes) clip tensor; codebook (n_codes, D) f32 -> (codes (F,H,W,D), idx (F*H*W,) int32)."""
    F_, H, W, _ = logits.shape
    D = codebook.shape[1]
    assert codebook.dtype == torch.float32 and codebook.is_contiguous() and codebook.shape[0] == n_codes
    if out is None:
        out = torch.empty((F_, H, W, D), dtype=logits.dtype, device=logits.device)
    idx = torch.empty((F_ * H * W,), dtype=torch.int32, device=logits.device)
    if forced_idx is not None:
        assert forced_idx.dtype == torch.int32 and forced_idx.is_contiguous() and forced_idx.numel() == idx.numel()
    call.flair_argmax_codebook(logits, dtype_code(logits), _ld(logits), F_ * H * W, n_codes, codebook, D, forced_idx, idx,
         out, _ld(out))
    return out, idx


def vq_nearest(z, codebook, *, forced_idx=None, out=None):
    """Nearest codebook row per pixel under the f32 squared distance (RestoreFormer's VectorQuantizer): z (F,H,W,D)
    clip tensor, codebook (N, D) f32 -> (codes (F,H,W,D) in z's dtype, idx (F*H*W,) int32).  ``forced_idx`` replaces
    the search (tests)."""
    F_, H, W, D = z.shape
    N = codebook.shape[0]
    assert codebook.dtype == torch.float32 and codebook.is_contiguous() and codebook.shape[1] == D
    if out is None:
        out = torch.empty((F_, H, W, D), dtype=z.dtype, device=z.device)
    idx = torch.empty((F_ * H * W,), dtype=torch.int32, device=z.device)
    if forced_idx is not None:
        assert forced_idx.dtype == torch.int32 and forced_idx.is_contiguous() and forced_idx.numel() == idx.numel()
    call.flair_vq_nearest_nhwc(z, dtype_code(z), _ld(z), F_ * H * W, D, codebook, N, forced_idx, idx, out, _ld(out))
    return out, idx


def adain(content, style, *, eps=1e-5, out=None):
    F_, H, W, C = content.shape
    assert style.shape == content.shape and style.dtype == content.dtype
    if out is None:
        out = torch.empty((F_, H, W, C), dtype=content.dtype, device=content.device)
    call.flair_adain_nhwc(content, _ld(content), style, _ld(style), dtype_code(content), F_, H * W, C, eps, out, _ld(out))
    return out


def sft_fuse(dec, scale, shift, w, out=None):
    """dec + w * (dec * scale + shift) on dense clip tensors."""
    assert dec.is_contiguous() and scale.is_contiguous() and shift.is_contiguous()
    assert dec.shape == scale.shape == shift.shape and dec.dtype == scale.dtype == shift.dtype
    if out is None:
        out = torch.empty_like(dec)
    call.flair_sft_fuse(dec, scale, shift, w, dtype_code(dec), dec.numel(), out)
    return out


# --------------------------------------------------------------------------- un-aligned prior branch (face crop / paste)
def _refuse(cond, what):
    if not cond:
        raise ValueError(what)


def warp_affine_cubic(src, minv, out_hw, *, border=(0.0, 0.0, 0.0), pre=False, post=False, src_index=None,
                      src_index_host=None):
    """cv2.warpAffine(INTER_CUBIC, BORDER_CONSTANT) per image (flair_warp_affine_cubic).  src: (N,C,Hs,Ws) f32 or f64
    (masks, C = 1); minv: (N, 6) float64 DEVICE tensor, the dst -> src matrices; -> (N,C,Hd,Wd) f32.
    ``src_index`` ((K,) int32 DEVICE tensor, with ``src_index_host``, the same K numbers as a host sequence, which is what
    gets range-checked): output k is cropped from src[src_index[k]] with minv[k] (flair_warp_affine_cubic_indexed),
    minv is (K, 6) and the result (K,C,Hd,Wd)."""
    if src_index is not None:
        return _warp_affine_cubic_indexed(src, minv, out_hw, border, pre, post, src_index, src_index_host)
    N, C, Hs, Ws = src.shape
    assert src.is_contiguous() and src.dtype in (torch.float32, torch.float64)
    assert minv.dtype == torch.float64 and minv.is_contiguous() and tuple(minv.shape) == (N, 6) and minv.is_cuda
    Hd, Wd = out_hw
    out = torch.empty((N, C, Hd, Wd), dtype=torch.float32, device=src.device)
    b = (ctypes.c_float * 4)(*([float(v) for v in border] + [0.0] * 4)[:4])
    call.flair_warp_affine_cubic(src, src.dtype == torch.float64, N, C, Hs, Ws, minv, Hd, Wd, b, pre, post, out)
    return out


def _warp_affine_cubic_indexed(src, minv, out_hw, border, pre, post, src_index, src_index_host):
    what = "flair_warp_affine_cubic_indexed"
    _refuse(src.dim() == 4 and src.dtype in (torch.float32, torch.float64) and src.is_contiguous(),
            f"{what}: src must be a contiguous (N,C,Hs,Ws) float32 or float64 tensor")
    Nsrc, C, Hs, Ws = src.shape
    _refuse(src_index.dim() == 1 and src_index.dtype == torch.int32 and src_index.is_contiguous(),
            f"{what}: src_index must be a contiguous (K,) int32 tensor")
    K = src_index.shape[0]
    _refuse(minv.dtype == torch.float64 and minv.is_contiguous() and tuple(minv.shape) == (K, 6),
            f"{what}: minv must be a contiguous ({K}, 6) float64 tensor")
    _refuse(src_index_host is not None and len(src_index_host) == K,
            f"{what}: src_index_host (the {K} indices on the host) is needed for the range check")
    _refuse(all(0 <= int(i) < Nsrc for i in src_index_host), f"{what}: src_index outside [0, {Nsrc})")
    Hd, Wd = out_hw
    out = torch.empty((K, C, Hd, Wd), dtype=torch.float32, device=src.device)
    b = (ctypes.c_float * 4)(*([float(v) for v in border] + [0.0] * 4)[:4])
    call.flair_warp_affine_cubic_indexed(src, src.dtype == torch.float64, Nsrc, src_index, K, C, Hs, Ws, minv, Hd, Wd, b,
         pre, post, out)
    return out


def face_paste(x0, faces, masks, minv, frame_start, frame_start_host, out=None):
    """Paste K restored faces into T frames through their blurred masks in one launch (flair_face_paste): per pixel and per
    face of the pixel's frame, in list order, v = v * (1 - m) + f * m with f / m the inverse cubic warps of the face / its
    f64 mask -- what warp_affine_cubic(face), warp_affine_cubic(mask) and face_blend give face by face, bit for bit.
    x0: (T,C,H,W) f32, C <= 4; faces: (K,C,h,w) f32; masks: (K,1,h,w) f64; minv: (K,6) f64; frame_start: (T+1,) int32 DEVICE
    tensor and ``frame_start_host`` the same numbers on the host (checked here: non-decreasing from 0 to K); K = 0 (faces,
    masks, minv None or empty) copies x0.  -> (T,C,H,W) f32, never x0's storage."""
    what = "flair_face_paste"
    _refuse(x0.dim() == 4 and x0.dtype == torch.float32 and x0.is_contiguous(), f"{what}: x0 must be a contiguous (T,C,H,W) float32 tensor")
    T, C, H, W = x0.shape
    K = 0 if faces is None else faces.shape[0]
    h = w = 0
    if K > 0:
        _refuse(faces.dim() == 4 and faces.dtype == torch.float32 and faces.is_contiguous() and faces.shape[1] == C,
                f"{what}: faces must be a contiguous (K,{C},h,w) float32 tensor")
        h, w = faces.shape[2:]
        _refuse(masks is not None and masks.dtype == torch.float64 and masks.is_contiguous() and tuple(masks.shape) == (K, 1, h, w),
                f"{what}: masks must be a contiguous ({K},1,{h},{w}) float64 tensor")
        _refuse(minv is not None and minv.dtype == torch.float64 and minv.is_contiguous() and tuple(minv.shape) == (K, 6),
                f"{what}: minv must be a contiguous ({K},6) float64 tensor")
    else:
        faces = masks = minv = None
    _refuse(frame_start.dtype == torch.int32 and frame_start.is_contiguous() and tuple(frame_start.shape) == (T + 1,),
            f"{what}: frame_start must be a contiguous ({T + 1},) int32 tensor")
    fs = [int(v) for v in frame_start_host]
    _refuse(len(fs) == T + 1 and fs[0] == 0 and fs[-1] == K and all(a <= b for a, b in zip(fs, fs[1:])),
            f"{what}: frame_start must be non-decreasing, start at 0 and end at K = {K} (got {fs})")
    if out is None:
        out = torch.empty_like(x0)
    _refuse(out.dtype == torch.float32 and out.is_contiguous() and out.shape == x0.shape, f"{what}: out must match x0")
    call.flair_face_paste(x0, T, C, H, W, faces, masks, minv, K, h, w, frame_start, out)
    return out


def face_mask_blur(parse_idx, N, H, W, lut, kern, *, repeats=2, edge=10, div=255.0):
    """lut[parse_idx] -> repeats x separable float64 Gaussian blur (reflect-101) -> edge zeroed, / div
    (flair_face_mask_blur).  parse_idx: (N*H*W,) int32; lut, kern: float64 DEVICE tensors -> (N,1,H,W) float64."""
    assert parse_idx.dtype == torch.int32 and parse_idx.is_contiguous() and parse_idx.numel() == N * H * W
    assert lut.dtype == torch.float64 and kern.dtype == torch.float64 and lut.is_cuda and kern.is_cuda
    tmp = torch.empty((N, 1, H, W), dtype=torch.float64, device=parse_idx.device)
    mask = torch.empty_like(tmp)
    call.flair_face_mask_blur(parse_idx, N, H, W, lut, lut.numel(), kern, kern.numel(), repeats, edge, div, tmp, mask)
    return mask


def face_blend(x0, face, mask):
    """x0 * (1 - mask) + face * mask; mask (N,1,H,W) f32 broadcast over the channels."""
    N, C, H, W = x0.shape
    assert x0.dtype == face.dtype == mask.dtype == torch.float32 and x0.is_contiguous() and face.is_contiguous()
    assert mask.is_contiguous() and tuple(mask.shape) == (N, 1, H, W) and face.shape == x0.shape
    out = torch.empty_like(x0)
    call.flair_face_blend(x0, face, mask, N, C, H, W, out)
    return out


# --------------------------------------------------------------------------- BiSeNet face parsing (parse.hip)
def global_avgpool(x, out=None):
    """F.avg_pool2d(x, x.size()[2:]) of a clip tensor (flair_global_avgpool_nhwc): (F, H, W, C) -> (F, C) float32 means."""
    F_, H, W, C = x.shape
    if out is None:
        out = torch.empty((F_, C), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.shape[0] == F_ and out.shape[1] >= C and out.stride(1) == 1
    call.flair_global_avgpool_nhwc(x, dtype_code(x), _ld(x), F_, H, W, C, out, out.stride(0))
    return out


def channel_gate(x, gate, *, logit=False, add_x=False, bias=None, add=None, out=None):
    """x * g (+ x) (+ bias) (+ add) on a clip tensor (flair_channel_gate_nhwc).  gate, bias: (F, C) float32 per (frame,
    channel); ``logit``: gate holds pre-sigmoid logits; ``add``: a clip tensor of x's shape and dtype.  out may be x."""
    F_, H, W, C = x.shape
    if out is None:
        out = torch.empty((F_, H, W, C), dtype=x.dtype, device=x.device)
    for t in (gate, bias):
        assert t is None or (t.dtype == torch.float32 and tuple(t.shape) == (F_, C) and t.stride(1) == 1)
    assert add is None or (add.dtype == x.dtype and add.shape == x.shape)
    assert out.dtype == x.dtype and tuple(out.shape[:3]) == (F_, H, W) and out.shape[3] >= C
    call.flair_channel_gate_nhwc(x, _ld(x), dtype_code(x), F_, H * W, C, gate, gate.stride(0), logit, add_x, bias,
         bias.stride(0) if bias is not None else 0, add, _ld(add) if add is not None else 0, out, _ld(out))
    return out


def upsample_argmax(logits, n_classes, size, table=None):
    """argmax over the classes of F.interpolate(logits, size, mode='bilinear', align_corners=True), first index on ties,
    without the enlarged tensor (flair_upsample_argmax_nhwc).  logits: (F, h, w, >= n_classes) clip tensor;
    table: optional (n_classes, D) float32 -> (idx (F, H, W) int32, table[idx] (F, H, W, D) float32 or None)."""
    F_, h, w, _ = logits.shape
    H, W = size
    idx = torch.empty((F_, H, W), dtype=torch.int32, device=logits.device)
    y, D = None, 0
    if table is not None:
        assert table.dtype == torch.float32 and table.is_contiguous() and table.shape[0] == n_classes
        D = table.shape[1]
        y = torch.empty((F_, H, W, D), dtype=torch.float32, device=logits.device)
    call.flair_upsample_argmax_nhwc(logits, dtype_code(logits), _ld(logits), F_, h, w, n_classes, H, W, table, D, idx, y, D)
    return idx, y


# --------------------------------------------------------------------------- YOLOv5-face detectors (detect.hip)
def maxpool2x2s2(x, out=None):
    """nn.MaxPool2d(2, 2, ceil_mode=True) on a clip tensor (flair_maxpool2x2s2_nhwc); out: optional (T, ceil(H/2), ceil(W/2),
    >= C) view, e.g. a channel slice of a wider buffer."""
    T, H, W, C = x.shape
    if out is None:
        out = torch.empty((T, (H + 1) // 2, (W + 1) // 2, C), dtype=x.dtype, device=x.device)
    assert tuple(out.shape) == (T, (H + 1) // 2, (W + 1) // 2, C) and out.dtype == x.dtype
    call.flair_maxpool2x2s2_nhwc(x, _ld(x), dtype_code(x), T, H, W, C, out, _ld(out))
    return out


def spp_maxpool(buf, C, ks):
    """SPP's three stride-1 max pools in place (flair_spp_maxpool_nhwc): reads channels [0, C) of the (T, H, W, >= 4C) clip
    tensor ``buf`` and writes MaxPool2d(ks[j], 1, ks[j] // 2) of them into channels [(j + 1) C, (j + 2) C), j = 0, 1, 2."""
    T, H, W, cb = buf.shape
    assert cb >= 4 * C and len(ks) == 3
    call.flair_spp_maxpool_nhwc(buf, _ld(buf), dtype_code(buf), T, H, W, C, int(ks[0]), int(ks[1]), int(ks[2]))
    return buf


def channel_interleave(a, b, out=None):
    """channel_shuffle(torch.cat((a, b), 1), 2) on clip tensors (flair_channel_interleave_nhwc): out[..., 2i] = a[..., i],
    out[..., 2i + 1] = b[..., i].  a, b: (T, H, W, C) views (any pixel stride); out: optional (T, H, W, 2C) view."""
    T, H, W, C = a.shape
    assert b.shape == a.shape and b.dtype == a.dtype
    if out is None:
        out = torch.empty((T, H, W, 2 * C), dtype=a.dtype, device=a.device)
    assert tuple(out.shape) == (T, H, W, 2 * C) and out.dtype == a.dtype
    call.flair_channel_interleave_nhwc(a, _ld(a), b, _ld(b), dtype_code(a), C, T * H * W, out, _ld(out))
    return out


def yolo_face_decode(x, na, stride, anchor_grid, z, row0, no=16):
    """Detect's inference decode of one level (flair_yolo_face_decode): x (B, ny, nx, >= na * 16) f32 head output ->
    rows [row0, row0 + na ny nx) of z (B, N, 16) f32.  anchor_grid: na (w, h) pairs in pixels (host floats)."""
    B, ny, nx, _ = x.shape
    assert x.dtype == torch.float32 and z.dtype == torch.float32 and z.is_contiguous() and z.dim() == 3 and z.shape[0] == B
    assert z.shape[2] == 16
    flat = [float(v) for pair in anchor_grid for v in pair]
    assert len(flat) == 2 * na
    arr = (ctypes.c_float * len(flat))(*flat)
    call.flair_yolo_face_decode(x, _ld(x), B, ny, nx, int(na), int(no), stride, arr, z, z.shape[1], row0)
    return z


def letterbox(src, new_hw, top_left, out_hw, *, pre=(1.0, 0.0, float("-inf"), float("inf")), scale=1.0, pad_value=114.0 / 255.0,
              out=None):
    """(B, 3, H, W) f32 NCHW frames -> (B, Ho, Wo, 16) f32 clip tensor (flair_letterbox_nhwc): the frames mapped to
    clamp(a x + b, lo, hi) (pre), resized to new_hw when that differs from (H, W), times ``scale``, placed at top_left in a
    field of ``pad_value``; channels 3..15 are zero."""
    B, C, H, W = src.shape
    assert C == 3 and src.dtype == torch.float32 and src.is_contiguous()
    Ho, Wo = out_hw
    if out is None:
        out = torch.empty((B, Ho, Wo, 16), dtype=torch.float32, device=src.device)
    assert tuple(out.shape) == (B, Ho, Wo, 16) and out.dtype == torch.float32
    a, b, lo, hi = pre
    call.flair_letterbox_nhwc(src, B, H, W, int(new_hw[0]), int(new_hw[1]), int(top_left[0]), int(top_left[1]), Ho, Wo,
         a, b, lo, hi, scale, pad_value, out, _ld(out))
    return out


# --------------------------------------------------------------------------- image metrics (metrics.hip)
def image_metrics(a, b, out=None):
    """Squared error and SSIM sums of two sets of written frames (flair_image_metrics): a, b (N, H, W, 3) uint8 dense RGB
    on the GPU, H, W >= 11 -> (N, 4) float64 device tensor, row n = [sum of squared byte differences (the exact integer),
    sum of the SSIM map of R, of G, of B over its (H - 10) x (W - 10) valid region].  flair_amd.metrics turns the rows into
    PSNR and mean SSIM.  The workspace comes from the library's size query."""
    _refuse(a.dim() == 4 and a.shape[3] == 3 and tuple(a.shape) == tuple(b.shape),
            f"image_metrics: two (N, H, W, 3) frame sets of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    _refuse(a.dtype == torch.uint8 and b.dtype == torch.uint8, f"image_metrics: uint8 frames, got {a.dtype} and {b.dtype}")
    _refuse(a.is_contiguous() and b.is_contiguous(), "image_metrics: dense (contiguous) frames")
    N, H, W, _ = a.shape
    if out is None:
        out = torch.empty((N, 4), dtype=torch.float64, device=a.device)
    _refuse(out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (N, 4), "image_metrics: out is a dense (N, 4) float64 tensor")
    nbytes = lib().flair_image_metrics_workspace(N, H, W)
    ws = _workspace(max(nbytes, 8), a.device, tag="metrics")
    call.flair_image_metrics(a, b, N, H, W, out, ws, nbytes)
    return out


# --------------------------------------------------------------------------- LPIPS (lpips.hip, include/flair_eval.h)
LPIPS_TAP_PARTS = 1024                      # FLAIR_LPIPS_TAP_PARTS: partials per frame, the tap kernel's workspace in closed form
LPIPS_TAP_WIDTHS = (64, 128, 192, 256, 384, 512)


def lpips_prepare(a, b, out=None):
    """Both (N, H, W, 3) uint8 frame sets -> one (2 N, H, W, 16) f32 clip tensor (flair_lpips_prepare): frames 0 .. N-1 are
    a's, the rest b's; channels 0 .. 2 = ((2 byte / 255 - 1) - shift) / scale, channels 3 .. 15 = 0.  a, b: dense, on the GPU,
    at any byte alignment; out: optional (2 N, H, W, >= 16) view."""
    _refuse(a.dim() == 4 and a.shape[3] == 3 and tuple(a.shape) == tuple(b.shape),
            f"lpips_prepare: two (N, H, W, 3) frame sets of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    _refuse(a.dtype == torch.uint8 and b.dtype == torch.uint8, f"lpips_prepare: uint8 frames, got {a.dtype} and {b.dtype}")
    _refuse(a.is_contiguous() and b.is_contiguous(), "lpips_prepare: dense (contiguous) frames")
    N, H, W, _ = a.shape
    if out is None:
        out = torch.empty((2 * N, H, W, 16), dtype=torch.float32, device=a.device)
    _refuse(tuple(out.shape[:3]) == (2 * N, H, W), f"lpips_prepare: out holds {tuple(out.shape[:3])} pixels, not {(2 * N, H, W)}")
    call.flair_lpips_prepare(a, b, N, H, W, out, _ld(out))
    return out


def lpips_tap(fa, fb, w, acc):
    """acc[f] += mean over the pixels of sum_c w_c (fa^ - fb^)^2, the features normalised per pixel over the channels
    (flair_lpips_tap).  fa, fb: (F, H, W, C) f32 clip views of one shape (any pixel stride), C one of LPIPS_TAP_WIDTHS; w: (C,)
    f32; acc: (F,) float64, accumulated over a trunk's five taps.  The same bits in every run and for every F."""
    _refuse(fa.dim() == 4 and tuple(fa.shape) == tuple(fb.shape), f"lpips_tap: two clip tensors of one shape, got {tuple(fa.shape)} and {tuple(fb.shape)}")
    F_, H, W, C = fa.shape
    _refuse(w.dim() == 1 and w.shape[0] == C and w.is_contiguous(), f"lpips_tap: w holds the {C} weights of the tap, got {tuple(w.shape)}")
    _refuse(acc.dim() == 1 and acc.shape[0] == F_ and acc.is_contiguous(), f"lpips_tap: acc is a dense ({F_},) float64 tensor")
    nbytes = F_ * LPIPS_TAP_PARTS * 8
    ws = _workspace(nbytes, fa.device, tag="lpips")
    call.flair_lpips_tap(fa, _ld(fa), fb, _ld(fb), F_, H * W, C, w, acc, ws, nbytes)
    return acc


def maxpool_valid(x, k, out=None):
    """nn.MaxPool2d(k, 2), no padding, floor mode, k = 2 or 3, on an f32 clip tensor (flair_maxpool_valid_s2_nhwc):
    (F, H, W, C) -> (F, (H - k) // 2 + 1, (W - k) // 2 + 1, C); out: optional view of that shape."""
    F_, H, W, C = x.shape
    Ho, Wo = (H - k) // 2 + 1, (W - k) // 2 + 1
    if out is None:
        out = torch.empty((F_, max(Ho, 0), max(Wo, 0), C), dtype=torch.float32, device=x.device)
    _refuse(tuple(out.shape) == (F_, max(Ho, 0), max(Wo, 0), C), f"maxpool_valid: out is {tuple(out.shape)}, not {(F_, Ho, Wo, C)}")
    call.flair_maxpool_valid_s2_nhwc(x, _ld(x), F_, H, W, C, int(k), out, _ld(out))
    return out


def alexnet_stem(x, w, bias, out=None):
    """relu(Conv2d(3, 64, 11, stride 4, padding 2)) of AlexNet on prepared frames (flair_alexnet_stem): x (F, H, W, >= 3) f32
    clip tensor, w (363, 64) f32 with row (ky * 11 + kx) * 3 + c, bias (64,) -> (F, (H - 7) // 4 + 1, (W - 7) // 4 + 1, 64)."""
    F_, H, W, _ = x.shape
    _refuse(tuple(w.shape) == (363, 64) and w.is_contiguous() and tuple(bias.shape) == (64,),
            f"alexnet_stem: w is (363, 64) and bias (64,), got {tuple(w.shape)} and {tuple(bias.shape)}")
    Ho, Wo = max((H - 7) // 4 + 1, 0), max((W - 7) // 4 + 1, 0)
    if out is None:
        out = torch.empty((F_, Ho, Wo, 64), dtype=torch.float32, device=x.device)
    _refuse(tuple(out.shape[:3]) == (F_, Ho, Wo) and out.shape[3] >= 64, f"alexnet_stem: out is {tuple(out.shape)}, not {(F_, Ho, Wo, 64)}")
    call.flair_alexnet_stem(x, _ld(x), F_, H, W, w, bias, out, _ld(out))
    return out


# --------------------------------------------------------------------------- NIQE (niqe.hip, include/flair_noref.h)
NIQE_BLOCK = 96                             # FLAIR_NIQE_BLOCK: block side at scale 1, half of it at scale 2
NIQE_HALF_UNIT = 2.0 ** -16                 # a value of the half-scale plane is y2 * NIQE_HALF_UNIT


def niqe_luma(u8, y1=None, y2=None):
    """Exact BT.601 luma of the top-left (96 nh, 96 nw) crop and 65536 x its MATLAB-bicubic half scale (flair_niqe_luma):
    u8 (N, H, W, 3) uint8 dense RGB on the GPU at any byte alignment, H, W >= 96 -> (y1 (N, 96 nh, 96 nw), y2 (N, 48 nh,
    48 nw)), both int32 and bit-exact; y1, y2: optional dense tensors of those shapes."""
    _refuse(u8.dim() == 4 and u8.shape[3] == 3, f"niqe_luma: (N, H, W, 3) frames, got {tuple(u8.shape)}")
    _refuse(u8.dtype == torch.uint8, f"niqe_luma: uint8 frames, got {u8.dtype}")
    _refuse(u8.is_contiguous(), "niqe_luma: dense (contiguous) frames")
    N, H, W, _ = u8.shape
    _refuse(min(H, W) >= NIQE_BLOCK, f"niqe_luma: frames of {H}x{W} hold no {NIQE_BLOCK}x{NIQE_BLOCK} block")
    Hc, Wc = H // NIQE_BLOCK * NIQE_BLOCK, W // NIQE_BLOCK * NIQE_BLOCK
    if y1 is None:
        y1 = torch.empty((N, Hc, Wc), dtype=torch.int32, device=u8.device)
    if y2 is None:
        y2 = torch.empty((N, Hc // 2, Wc // 2), dtype=torch.int32, device=u8.device)
    for name, t, shape in (("y1", y1, (N, Hc, Wc)), ("y2", y2, (N, Hc // 2, Wc // 2))):
        _refuse(t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == shape,
                f"niqe_luma: {name} is a dense {shape} int32 tensor, got {tuple(t.shape)} {t.dtype}")
    call.flair_niqe_luma(u8, N, H, W, y1, y2)
    return y1, y2


def niqe_moments(y, block, inv_scale, window, out=None, mscn=None):
    """The MSCN map of one scale and the 25 moments of each of its blocks (flair_niqe_moments): y (N, Hc, Wc) int32 dense, a
    pixel's value being y * inv_scale (1, or NIQE_HALF_UNIT for niqe_luma's y2); block 96 or 48, dividing Hc and Wc; window
    (7, 7) float64 on the GPU -> (N, (Hc / block) (Wc / block), 5, 5) float64: block j nh + i, maps M, M roll(M, (0,1)),
    (1,0), (1,1), (1,-1), moments c-, c+, s-, s+, a.  mscn: optional dense (N, Hc, Wc) float64 tensor that receives M.
    The same bits in every run, for every N and every position in the batch."""
    _refuse(y.dim() == 3 and y.dtype == torch.int32 and y.is_contiguous(), f"niqe_moments: y is a dense (N, Hc, Wc) int32 tensor, got {tuple(y.shape)} {y.dtype}")
    N, Hc, Wc = y.shape
    _refuse(block in (NIQE_BLOCK, NIQE_BLOCK // 2), f"niqe_moments: block = {block}, one of {NIQE_BLOCK} and {NIQE_BLOCK // 2}")
    _refuse(Hc % block == 0 and Wc % block == 0 and Hc and Wc, f"niqe_moments: the plane of {Hc}x{Wc} is not made of {block}x{block} blocks")
    _refuse(window.dtype == torch.float64 and window.is_contiguous() and tuple(window.shape) == (7, 7),
            f"niqe_moments: window is a dense (7, 7) float64 tensor, got {tuple(window.shape)} {window.dtype}")
    shape = (N, (Hc // block) * (Wc // block), 5, 5)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=y.device)
    _refuse(out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == shape, f"niqe_moments: out is a dense {shape} float64 tensor")
    _refuse(mscn is None or (mscn.dtype == torch.float64 and mscn.is_contiguous() and tuple(mscn.shape) == (N, Hc, Wc)),
            f"niqe_moments: mscn is a dense {(N, Hc, Wc)} float64 tensor")
    call.flair_niqe_moments(y, N, Hc, Wc, int(block), float(inv_scale), window, out, mscn)
    return out


# --------------------------------------------------------------------------- ArcFace identity (ident.hip, include/flair_ident.h)
IDENT_SIDE = 128                            # FLAIR_IDENT_SIDE: the network's input is 1 x 128 x 128
IDENT_EMBED_KCHUNK = 1024                   # FLAIR_IDENT_EMBED_KCHUNK: inputs per workgroup, the embed kernel's workspace in closed form


def ident_prepare(a, b=None, out=None):
    """One or two (N, H, W, 3) uint8 frame sets -> one (F, 128, 128, 16) f32 clip tensor (flair_ident_prepare), F = N without b
    and 2 N with it (a's frames first): channel 0 = the bilinear 128 x 128 resize of 0.2989 R + 0.5870 G + 0.1140 B on
    2 byte / 255 - 1, in double and rounded once; channels 1 .. 15 = 0.  a, b: dense, on the GPU, at any byte alignment; out:
    optional (F, 128, 128, >= 16) view."""
    _refuse(a.dim() == 4 and a.shape[3] == 3 and (b is None or tuple(a.shape) == tuple(b.shape)),
            f"ident_prepare: (N, H, W, 3) frame sets of one shape, got {tuple(a.shape)}" + ("" if b is None else f" and {tuple(b.shape)}"))
    _refuse(a.dtype == torch.uint8 and (b is None or b.dtype == torch.uint8), "ident_prepare: uint8 frames")
    _refuse(a.is_contiguous() and (b is None or b.is_contiguous()), "ident_prepare: dense (contiguous) frames")
    N, H, W, _ = a.shape
    F_ = N if b is None else 2 * N
    if out is None:
        out = torch.empty((F_, IDENT_SIDE, IDENT_SIDE, 16), dtype=torch.float32, device=a.device)
    _refuse(tuple(out.shape[:3]) == (F_, IDENT_SIDE, IDENT_SIDE), f"ident_prepare: out holds {tuple(out.shape[:3])} pixels, not {(F_, IDENT_SIDE, IDENT_SIDE)}")
    call.flair_ident_prepare(a, b, N, H, W, out, _ld(out))
    return out


def ident_embed(x, w, bias, out=None):
    """out[f][o] = bias[o] + sum_k w[o][k] x[f][k] with float64 products and sums, rounded to f32 once (flair_ident_embed).
    x: (F, K) f32 rows (any row stride), K a multiple of 4; w: (O, K) f32 dense; bias: (O,) f32; out: optional (F, O) f32 rows.
    The same bits in every run, for every F and every position in the batch."""
    _refuse(x.dim() == 2 and x.stride(1) == 1, f"ident_embed: x is (F, K) rows of floats, got {tuple(x.shape)}")
    F_, K = x.shape
    _refuse(w.dim() == 2 and w.shape[1] == K and w.is_contiguous(), f"ident_embed: w is a dense (O, {K}) tensor, got {tuple(w.shape)}")
    O = w.shape[0]
    _refuse(bias.dim() == 1 and bias.shape[0] == O and bias.is_contiguous(), f"ident_embed: bias holds {O} values, got {tuple(bias.shape)}")
    if out is None:
        out = torch.empty((F_, O), dtype=torch.float32, device=x.device)
    _refuse(out.dim() == 2 and tuple(out.shape) == (F_, O) and out.stride(1) == 1, f"ident_embed: out is ({F_}, {O}) rows of floats, got {tuple(out.shape)}")
    nbytes = -(-K // IDENT_EMBED_KCHUNK) * F_ * O * 8
    ws = _workspace(nbytes, x.device, tag="ident")
    call.flair_ident_embed(x, x.stride(0) if F_ > 1 else max(x.stride(0), K), F_, K, w, bias, O, out,
                           out.stride(0) if F_ > 1 else max(out.stride(0), O), ws, nbytes)
    return out


# --------------------------------------------------------------------------- flow-warping error (temporal.hip, include/flair_temporal.h)
WARP_TILE_H, WARP_TILE_W = 32, 64           # FLAIR_WARP_TILE_H / _W: the tile of one workgroup, the workspace in closed form


def _flow_pair(name, f, what):
    _refuse(f.dim() == 4 and f.shape[3] == 2 and f.dtype == torch.float32 and f.is_contiguous() and f.shape[0] >= 1,
            f"{name}: {what} is a dense (P, H, W, 2) float32 tensor with P >= 1, got {tuple(f.shape)} {f.dtype}")


def flow_occlusion(f, g, out=None):
    """The mask of include/flair_temporal.h, steps 1 to 5 (flair_flow_occlusion): f (the flow frame t -> t + 1) and g (the flow
    t + 1 -> t), dense (P, H, W, 2) f32 of (dx, dy) -> (P, H, W) uint8, 1 where a pixel is inside, not occluded and not on a
    motion boundary.  Float64 inside; out: an optional dense tensor of that shape."""
    _flow_pair("flow_occlusion", f, "f")
    _refuse(tuple(g.shape) == tuple(f.shape) and g.dtype == torch.float32 and g.is_contiguous(),
            f"flow_occlusion: g is a dense {tuple(f.shape)} float32 tensor like f, got {tuple(g.shape)} {g.dtype}")
    P, H, W, _ = f.shape
    if out is None:
        out = torch.empty((P, H, W), dtype=torch.uint8, device=f.device)
    _refuse(out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (P, H, W),
            f"flow_occlusion: out is a dense {(P, H, W)} uint8 tensor, got {tuple(out.shape)} {out.dtype}")
    call.flair_flow_occlusion(f, g, P, H, W, out)
    return out


def warp_error(a, f, mask, a2=None, out=None):
    """(S, N) of include/flair_temporal.h, steps 6 and 7, per frame pair (flair_warp_error): a (P + 1, H, W, 3) uint8 dense RGB on
    the GPU at any byte alignment, pair i being frames i and i + 1; f (P, H, W, 2) f32, the flow frame i -> i + 1; mask
    (P, H, W) uint8; a2: a second frame set like a, judged by the same f and mask -> (sets, P, 2) float64, sets = 1 or 2.
    The same bits in every run, for every P and every position in the batch."""
    _flow_pair("warp_error", f, "f")
    P, H, W, _ = f.shape
    for name, t in (("a", a), ("a2", a2)):
        _refuse(t is None or (t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == (P + 1, H, W, 3)),
                f"warp_error: {name} is a dense {(P + 1, H, W, 3)} uint8 tensor, one frame more than f has pairs" +
                ("" if t is None else f", got {tuple(t.shape)} {t.dtype}"))
    _refuse(a is not None, "warp_error: a is missing")
    _refuse(mask.dtype == torch.uint8 and mask.is_contiguous() and tuple(mask.shape) == (P, H, W),
            f"warp_error: mask is a dense {(P, H, W)} uint8 tensor, got {tuple(mask.shape)} {mask.dtype}")
    sets = 1 if a2 is None else 2
    if out is None:
        out = torch.empty((sets, P, 2), dtype=torch.float64, device=f.device)
    _refuse(out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (sets, P, 2),
            f"warp_error: out is a dense {(sets, P, 2)} float64 tensor, got {tuple(out.shape)} {out.dtype}")
    nbytes = sets * P * -(-H // WARP_TILE_H) * -(-W // WARP_TILE_W) * 16
    ws = _workspace(nbytes, f.device, tag="temporal")
    call.flair_warp_error(a, a2, f, mask, P, H, W, out, ws, nbytes)
    return out


# --------------------------------------------------------------------------- face-score crop (facecrop.hip, include/flair_facescore.h)
FACE_CROP_REACH = 32000                     # source pixels: beyond it lies the 16-bit saturation of the fixed-point form, left out


def face_crop_u8(a, minv, minv_host, src_index, src_index_host, out_hw, *, b=None, border=(135, 133, 132), out_a=None, out_b=None):
    """Aligned byte crops of the faces of one or two frame sets (flair_face_crop_u8): a (Nsrc, Hs, Ws, 3) uint8 dense RGB on the
    GPU at any byte alignment; b: a second frame set like a, cut with the same geometry; minv (K, 6) float64 DEVICE tensor, the
    dst -> src matrices, and ``minv_host`` the same numbers on the host; src_index (K,) int32 DEVICE tensor and
    ``src_index_host`` the same numbers on the host.  The host copies are what gets checked: an index outside [0, Nsrc) and a
    matrix that maps a corner of the crop beyond +-32 000 source pixels are refused before the launch.  -> out_a (K, Hd, Wd, 3)
    uint8 without b, (out_a, out_b) with it: the exact a = -0.75 cubic of include/flair_facescore.h with ``border`` (three
    bytes) outside the frame, rounded once.  The same bits in every run, for every K and every position in the batch."""
    import numpy as np
    what = "face_crop_u8"
    for name, t in (("a", a), ("b", b)):
        _refuse(t is None or (t.dim() == 4 and t.shape[3] == 3 and t.dtype == torch.uint8 and t.is_contiguous() and t.shape[0] >= 1),
                f"{what}: {name} is a dense (Nsrc, Hs, Ws, 3) uint8 tensor with Nsrc >= 1" + ("" if t is None else f", got {tuple(t.shape)} {t.dtype}"))
    _refuse(a is not None, f"{what}: a is missing")
    _refuse(b is None or tuple(b.shape) == tuple(a.shape), f"{what}: b is a frame set of a's shape {tuple(a.shape)}" + ("" if b is None else f", got {tuple(b.shape)}"))
    Nsrc, Hs, Ws, _ = a.shape
    _refuse(src_index.dim() == 1 and src_index.dtype == torch.int32 and src_index.is_contiguous(), f"{what}: src_index must be a contiguous (K,) int32 tensor")
    K = src_index.shape[0]
    _refuse(minv.dtype == torch.float64 and minv.is_contiguous() and tuple(minv.shape) == (K, 6), f"{what}: minv must be a contiguous ({K}, 6) float64 tensor")
    _refuse(src_index_host is not None and len(src_index_host) == K, f"{what}: src_index_host (the {K} indices on the host) is needed for the range check")
    _refuse(all(0 <= int(i) < Nsrc for i in src_index_host), f"{what}: src_index outside [0, {Nsrc})")
    Hd, Wd = (int(v) for v in out_hw)
    _refuse(Hd >= 1 and Wd >= 1, f"{what}: a crop of {Hd}x{Wd} pixels")
    m = np.asarray(minv_host, dtype=np.float64).reshape(-1, 6) if minv_host is not None and K else np.zeros((0, 6))
    _refuse(minv_host is not None and m.shape[0] == K, f"{what}: minv_host (the {K} matrices on the host) is needed for the range check")
    for k in range(K):
        corners = [(m[k, 0] * x + m[k, 1] * y + m[k, 2], m[k, 3] * x + m[k, 4] * y + m[k, 5]) for x in (0, Wd - 1) for y in (0, Hd - 1)]
        _refuse(all(abs(v) <= FACE_CROP_REACH for p in corners for v in p),                 # a not-a-number fails the comparison too
                f"{what}: matrix {k} maps a corner of the crop beyond +-{FACE_CROP_REACH} source pixels")
    _refuse(len(border) == 3 and all(int(v) == v and 0 <= int(v) <= 255 for v in border), f"{what}: border is three bytes, got {tuple(border)}")
    for name, t in (("out_a", out_a), ("out_b", out_b)):
        _refuse(t is None or (t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == (K, Hd, Wd, 3)),
                f"{what}: {name} is a dense {(K, Hd, Wd, 3)} uint8 tensor" + ("" if t is None else f", got {tuple(t.shape)} {t.dtype}"))
    _refuse(b is not None or out_b is None, f"{what}: out_b without b")
    if out_a is None:
        out_a = torch.empty((K, Hd, Wd, 3), dtype=torch.uint8, device=a.device)
    if b is not None and out_b is None:
        out_b = torch.empty((K, Hd, Wd, 3), dtype=torch.uint8, device=a.device)
    if K:
        call.flair_face_crop_u8(a, b, Nsrc, Hs, Ws, minv, src_index, K, Hd, Wd, (ctypes.c_uint8 * 3)(*(int(v) for v in border)), out_a, out_b)
    return out_a if b is None else (out_a, out_b)


# --------------------------------------------------------------------------- video streams (yuv.hip, include/flair_yuv.h)
YUV_FORMATS = {"420jpeg": 0, "420mpeg2": 1, "422": 2, "444": 3, "mono": 4}
YUV_MATRICES = {"bt601": 0, "bt709": 1}
YUV_RANGES = {"limited": 0, "full": 1}
from .y4m import payload_bytes as _yuv_payload_bytes  # noqa: E402  (W H + 2 wc hc: the size of one frame's payload)


def _yuv_ids(what, fmt, matrix, range_):
    _refuse(fmt in YUV_FORMATS, f"{what}: format {fmt!r}, one of {', '.join(YUV_FORMATS)}")
    _refuse(matrix in YUV_MATRICES, f"{what}: matrix {matrix!r}, one of {', '.join(YUV_MATRICES)}")
    _refuse(range_ in YUV_RANGES, f"{what}: range {range_!r}, one of {', '.join(YUV_RANGES)}")
    return YUV_FORMATS[fmt], YUV_MATRICES[matrix], YUV_RANGES[range_]


def yuv_to_rgb_u8(payload, hw, fmt, matrix, range_, *, planar=False, out=None):
    """The frames of a .y4m stream as RGB bytes (flair_yuv_to_rgb_u8): payload (N, P) uint8 on the GPU with dense rows, exactly
    the file's bytes Y | U | V of N frames of hw = (H, W) luma samples, at any byte alignment -> (N, H, W, 3) uint8, or
    (N, 3, H, W) with ``planar``.  fmt: 420jpeg, 420mpeg2, 422, 444 or mono; matrix: bt601 or bt709; range_: limited or full.
    The integer definition of include/flair_yuv.h: the same bits in every run."""
    what = "yuv_to_rgb_u8"
    ids = _yuv_ids(what, fmt, matrix, range_)
    H, W = (int(v) for v in hw)
    _refuse(H >= 1 and W >= 1, f"{what}: frames of {H}x{W} pixels")
    P = _yuv_payload_bytes(fmt, H, W)
    _refuse(payload.dim() == 2 and payload.dtype == torch.uint8 and payload.shape[1] == P and payload.is_contiguous(),
            f"{what}: payload is a dense (N, {P}) uint8 tensor for {fmt} frames of {H}x{W}, got {tuple(payload.shape)} {payload.dtype}")
    N = payload.shape[0]
    shape = (N, 3, H, W) if planar else (N, H, W, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=payload.device)
    _refuse(out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == shape, f"{what}: out is a dense {shape} uint8 tensor, got {tuple(out.shape)} {out.dtype}")
    if N:
        call.flair_yuv_to_rgb_u8(payload, N, H, W, *ids, int(bool(planar)), out)
    return out


def rgb_to_yuv_u8(rgb, fmt, matrix, range_, *, out=None):
    """RGB bytes as the payloads of a .y4m stream (flair_rgb_to_yuv_u8): rgb (N, H, W, 3) uint8 dense on the GPU -> (N, P) uint8,
    every row Y | U | V of one frame, the encode of include/flair_yuv.h (chroma footprints clamped to the frame, rounded once)."""
    what = "rgb_to_yuv_u8"
    ids = _yuv_ids(what, fmt, matrix, range_)
    _refuse(rgb.dim() == 4 and rgb.shape[3] == 3 and rgb.dtype == torch.uint8 and rgb.is_contiguous() and rgb.shape[1] >= 1 and rgb.shape[2] >= 1,
            f"{what}: rgb is a dense (N, H, W, 3) uint8 tensor, got {tuple(rgb.shape)} {rgb.dtype}")
    N, H, W, _ = rgb.shape
    P = _yuv_payload_bytes(fmt, H, W)
    if out is None:
        out = torch.empty((N, P), dtype=torch.uint8, device=rgb.device)
    _refuse(out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (N, P), f"{what}: out is a dense {(N, P)} uint8 tensor, got {tuple(out.shape)} {out.dtype}")
    if N:
        call.flair_rgb_to_yuv_u8(rgb, N, H, W, *ids, out)
    return out


# --------------------------------------------------------------------------- tiled denoising (tile.hip, include/flair_tile.h)
_tile_origin_arrays = {}


def _tile_origins(what, name, origins, t, L, device, cover):
    """A plan's origins along one axis as the int32 device array the kernels read, uploaded once per (device, origins).  The host
    list is checked first: every tile inside the axis and, for the blend (``cover``), every pixel under a tile."""
    key = tuple(int(o) for o in origins)
    _refuse(len(key) >= 1 and all(0 <= o <= L - t for o in key),
            f"{what}: {name} = {list(key)}: every tile of {t} pixels must lie inside the axis of {L}")
    if cover:
        reach = 0
        for o in sorted(key):
            _refuse(o <= reach, f"{what}: {name} = {list(key)} with tiles of {t} pixels leaves pixel {reach} of {L} uncovered")
            reach = max(reach, o + t)
        _refuse(reach >= L, f"{what}: {name} = {list(key)} with tiles of {t} pixels leaves pixel {reach} of {L} uncovered")
    k = (str(device), key)
    if k not in _tile_origin_arrays:
        if len(_tile_origin_arrays) >= 64:
            _tile_origin_arrays.clear()
        _tile_origin_arrays[k] = torch.tensor(key, dtype=torch.int32, device=device)
    return _tile_origin_arrays[k]


def _dense_f32(t):
    return t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()


def tile_gather(frame, oy, ox, tile_hw, out=None):
    """Whole frames -> overlapping tiles (flair_tile_gather_f32), a plain copy: frame (N, C, H, W) f32 dense on the GPU (a dense view
    at any offset will do); oy / ox: the tile rows' and columns' origins (host ints); tile_hw = (th, tw) -> (len(oy) len(ox) N, C, th,
    tw), the tile index major and row-major over (oy, ox): out[(r len(ox) + c) N + n] = frame[n, :, oy[r]:oy[r] + th, ox[c]:ox[c] + tw]."""
    what = "tile_gather"
    _refuse(_dense_f32(frame), f"{what}: frame is a dense (N, C, H, W) float32 tensor, got {tuple(frame.shape)} {frame.dtype}")
    N, C, H, W = frame.shape
    th, tw = (int(v) for v in tile_hw)
    _refuse(N >= 1 and C >= 1 and 1 <= th <= H and 1 <= tw <= W, f"{what}: tiles of {th}x{tw} of frames {tuple(frame.shape)}")
    dy, dx = _tile_origins(what, "oy", oy, th, H, frame.device, False), _tile_origins(what, "ox", ox, tw, W, frame.device, False)
    shape = (len(oy) * len(ox) * N, C, th, tw)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=frame.device)
    _refuse(_dense_f32(out) and tuple(out.shape) == shape, f"{what}: out is a dense {shape} float32 tensor, got {tuple(out.shape)} {out.dtype}")
    call.flair_tile_gather_f32(frame, N, C, H, W, dy, len(oy), dx, len(ox), th, tw, out)
    return out


def tile_blend(tiles, oy, ox, frame_hw, ramp, out=None):
    """Tiles -> whole frames with feathered weights (flair_tile_blend_f32; include/flair_tile.h holds the definition): tiles
    (len(oy) len(ox) N, C, th, tw) f32 dense on the GPU in tile_gather's order -> (N, C, H, W) for frame_hw = (H, W).  ``ramp``: the
    width in pixels over which a tile's weight rises from its inner edges (the plan's minimum overlap).  Any number of tiles may
    cover a pixel; every pixel must be covered.  The same bits in every run; a pixel under one tile is that tile's value."""
    what = "tile_blend"
    _refuse(_dense_f32(tiles), f"{what}: tiles is a dense (K N, C, th, tw) float32 tensor, got {tuple(tiles.shape)} {tiles.dtype}")
    KN, C, th, tw = tiles.shape
    H, W = (int(v) for v in frame_hw)
    K = len(oy) * len(ox)
    _refuse(K >= 1 and KN >= K and KN % K == 0 and C >= 1, f"{what}: {KN} tile planes for a plan of {len(oy)}x{len(ox)} tiles")
    _refuse(1 <= th <= H and 1 <= tw <= W, f"{what}: tiles of {th}x{tw} for frames of {H}x{W}")
    _refuse(int(ramp) >= 1, f"{what}: ramp = {ramp} pixels, at least 1")
    N = KN // K
    dy, dx = _tile_origins(what, "oy", oy, th, H, tiles.device, True), _tile_origins(what, "ox", ox, tw, W, tiles.device, True)
    shape = (N, C, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=tiles.device)
    _refuse(_dense_f32(out) and tuple(out.shape) == shape, f"{what}: out is a dense {shape} float32 tensor, got {tuple(out.shape)} {out.dtype}")
    call.flair_tile_blend_f32(tiles, N, C, H, W, dy, len(oy), dx, len(ox), th, tw, int(ramp), out)
    return out


# --------------------------------------------------------------------------- scene cuts (scenes.hip)
def block_luma_sums(u8, out=None):
    """Exact integer luma sums over an 8 x 8 grid of blocks per frame (flair_block_luma_sums): u8 (N, H, W, 3) uint8 dense RGB
    on the GPU, H, W >= 8 -> (N, 64) int64 device tensor, entry 8 a + b = sum of (77 R + 150 G + 29 B + 128) >> 8 over rows
    (a H) // 8 .. ((a + 1) H) // 8 and columns (b W) // 8 .. ((b + 1) W) // 8.  flair_amd.scenes turns the rows into distances."""
    _refuse(u8.dim() == 4 and u8.shape[3] == 3, f"block_luma_sums: (N, H, W, 3) frames, got {tuple(u8.shape)}")
    _refuse(u8.dtype == torch.uint8, f"block_luma_sums: uint8 frames, got {u8.dtype}")
    _refuse(u8.is_contiguous(), "block_luma_sums: dense (contiguous) frames")
    N, H, W, _ = u8.shape
    if out is None:
        out = torch.empty((N, 64), dtype=torch.int64, device=u8.device)
    _refuse(out.dtype == torch.int64 and out.is_contiguous() and tuple(out.shape) == (N, 64),
            "block_luma_sums: out is a dense (N, 64) int64 tensor")
    call.flair_block_luma_sums(u8, N, H, W, out)
    return out


# --------------------------------------------------------------------------- SuperSloMo frame interpolation (slomo.hip)
SLOMO_MEAN = (0.429, 0.431, 0.397)          # superslomo.py:250: the channel means of normalize()


def slomo_coefficients(k, factor):
    """t = k / factor and co_eff of superslomo.py:260-262 as Python doubles -> (t, [c0, c1, c2, c3])."""
    t = k / factor
    temp = -t * (1 - t)
    return t, [temp, t * t, (1 - t) * (1 - t), temp]


def slomo_warp_pack(pair, flow, coef, out=None):
    """Stage A of one intermediate frame (flair_slomo_warp_pack): pair (B, H, W, >= 6) normalised i0 | i1, flow (B, H, W, >= 4)
    f01 | f10, coef the four doubles of slomo_coefficients -> the interpolation UNet's input, (B, H, W, pad_channels(20))
    with zeros in the pad channels; out: optional view of that shape."""
    B, H, W, _ = pair.shape
    assert flow.dtype == pair.dtype and tuple(flow.shape[:3]) == (B, H, W)
    oc = pad_channels(20, pair.dtype)
    if out is None:
        out = torch.empty((B, H, W, oc), dtype=pair.dtype, device=pair.device)
    assert tuple(out.shape) == (B, H, W, oc) and out.dtype == pair.dtype
    call.flair_slomo_warp_pack(pair, _ld(pair), flow, _ld(flow), dtype_code(pair), B, H, W, *coef, out, _ld(out), oc)
    return out


def slomo_blend(pair, flow, io, coef, t, out, mean=SLOMO_MEAN):
    """Stage B of one intermediate frame (flair_slomo_blend): io (B, H, W, >= 5) is the interpolation UNet's output; out: a
    (B, 3, H, W) f32 view whose frames are dense, e.g. slot [:, k] of the (B, factor - 1, 3, H, W) result."""
    B, H, W, _ = pair.shape
    assert flow.dtype == pair.dtype and io.dtype == pair.dtype
    assert tuple(flow.shape[:3]) == (B, H, W) and tuple(io.shape[:3]) == (B, H, W)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 3, H, W) and out[0].is_contiguous()
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    call.flair_slomo_blend(pair, _ld(pair), flow, _ld(flow), io, _ld(io), dtype_code(pair), B, H, W, *coef, t, m, out,
         out.stride(0) if B > 1 else 3 * H * W)
    return out


# --------------------------------------------------------------------------- AMT-G frame interpolation (amt.hip)
CORR_TAPS = 49                              # (2 * 3 + 1) ** 2: AMT's lookup radius


def corr_volume(fa, fb_nchw, out=None):
    """BidirCorrBlock.corr (raft.py:201-209): fa (B, h, w, D) NHWC features of one frame, fb_nchw (B, D, h, w) the other
    frame's features channel-major -> (B * h * w, h, w) planes of fa^T fb / sqrt(D): flair_matmul_f32, then the division
    in place (flair_corr_scale)."""
    B, h, w, D = fa.shape
    assert tuple(fb_nchw.shape) == (B, D, h, w)
    vol = matmul(fa.reshape(B, h * w, D), fb_nchw.reshape(B, D, h * w), out=None if out is None else out.view(B, h * w, h * w))
    div = float(torch.sqrt(torch.tensor(D).float()))
    call.flair_corr_scale(vol, vol.numel(), div)
    return vol.view(B * h * w, h, w)


def corr_pool(vol, out=None):
    """F.avg_pool2d(vol, 2, stride=2) of (planes, h, w) f32 planes (flair_corr_pool); odd sizes floor."""
    P, h, w = vol.shape
    assert vol.dtype == torch.float32 and vol.is_contiguous()
    if h < 2 or w < 2:
        raise ValueError(f"corr_pool: planes of {h}x{w} hold no 2x2 window")
    if out is None:
        out = torch.empty((P, h // 2, w // 2), dtype=torch.float32, device=vol.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (P, h // 2, w // 2)
    call.flair_corr_pool(vol, P, h, w, out)
    return out


def corr_lookup(pyramid, pyramid_t, flow, scale_corr, scale_corr_t, out):
    """BidirCorrBlock.__call__ on coord + flow1 * scale_corr (pyramid) and coord + flow0 * scale_corr_t (pyramid_t)
    (flair_corr_lookup): the pyramids are lists of (B * h * w, lh, lw) f32 volumes, flow (B, h, w, >= 4) f32 flow0 | flow1,
    out a (B, h, w, >= 98 * levels) f32 clip view whose first 98 * levels channels are written: corr | corr_T."""
    B, h, w, _ = flow.shape
    n = len(pyramid)
    assert len(pyramid_t) == n and flow.dtype == torch.float32 and out.dtype == torch.float32
    assert tuple(out.shape[:3]) == (B, h, w) and out.shape[3] >= 2 * CORR_TAPS * n
    for v in list(pyramid) + list(pyramid_t):
        assert v.dtype == torch.float32 and v.is_contiguous() and v.dim() == 3 and v.shape[0] == B * h * w, tuple(v.shape)
    for a, b in zip(pyramid, pyramid_t):
        assert a.shape == b.shape
    pa = (ctypes.c_void_p * n)(*[v.data_ptr() for v in pyramid])
    pb = (ctypes.c_void_p * n)(*[v.data_ptr() for v in pyramid_t])
    lh = (ctypes.c_int * n)(*[v.shape[1] for v in pyramid])
    lw = (ctypes.c_int * n)(*[v.shape[2] for v in pyramid])
    e0 = _prof_begin()

    def launch(_keep=(pyramid, pyramid_t)):
        call.flair_corr_lookup(pa, pb, lh, lw, n, flow, _ld(flow), B, h, w, scale_corr, scale_corr_t, out, _ld(out))
    launch()
    if e0 is not None:      # algorithmic bytes: an 8 x 8 patch per level and direction read, 98 floats per level written
        _prof_end(e0, ("corr_lookup",), torch.float32, 2.0 * 7 * B * h * w * 2 * n * CORR_TAPS,
                  4.0 * B * h * w * (2 * n * (64 + CORR_TAPS) + 4), launch, ("corr_lookup", B, h, w, n))
    return out


def prelu(x0, slope, x1=None, out=None):
    """prelu(x0 (+ x1), slope[c]) on f32 clip tensors (flair_prelu_nhwc); slope: (>= C,) f32; out may be x0."""
    T, H, W, C = x0.shape
    assert x0.dtype == torch.float32 and slope.dtype == torch.float32 and slope.is_contiguous() and slope.numel() >= C
    assert x1 is None or (x1.dtype == torch.float32 and x1.shape == x0.shape)
    if out is None:
        out = torch.empty((T, H, W, C), dtype=torch.float32, device=x0.device)
    assert out.dtype == torch.float32 and out.shape == x0.shape
    call.flair_prelu_nhwc(x0, _ld(x0), x1, _ld(x1) if x1 is not None else 0, slope, C, T * H * W, out, _ld(out))
    return out


def depth_to_space2(x, C, out=None):
    """(F, H, W, >= 4 C) f32, channels parity-major -> (F, 2 H, 2 W, C) (flair_depth_to_space2_nhwc)."""
    F_, H, W, Cx = x.shape
    assert x.dtype == torch.float32 and Cx >= 4 * C
    if out is None:
        out = torch.empty((F_, 2 * H, 2 * W, C), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and tuple(out.shape[:3]) == (F_, 2 * H, 2 * W) and out.shape[3] >= C
    call.flair_depth_to_space2_nhwc(x, _ld(x), F_, H, W, C, out, _ld(out))
    return out


def deconv_as_conv3x3(w, b, cpad=None):
    """nn.ConvTranspose2d(Cin, Cout, 4, 2, 1) as a 3x3 convolution with 4 * cpad outputs (host-side, once per load).
    Output pixel (2 m + py, 2 n + px) sums input pixels (m + dy, n + dx), dy in {py - 1, py}, dx in {px - 1, px}, through
    kernel tap (py + 1 - 2 dy, px + 1 - 2 dx); parity (py, px) takes output channels [(2 py + px) cpad, ... + Cout) and the 3x3
    taps it does not use are zero (9/4 of the products; depth_to_space2 undoes the channel layout).
    w: (Cin, Cout, 4, 4), b: (Cout,) or None -> (4 cpad, Cin, 3, 3), (4 cpad,); cpad: Cout rounded up to a multiple of 4."""
    cin, cout, kh, kw = w.shape
    assert (kh, kw) == (4, 4), "deconv_as_conv3x3 restates ConvTranspose2d(kernel 4, stride 2, padding 1) only"
    cpad = cpad or (cout + 3) // 4 * 4
    w3 = w.new_zeros(4 * cpad, cin, 3, 3)
    b3 = w.new_zeros(4 * cpad)
    for py in (0, 1):
        for px in (0, 1):
            o = (2 * py + px) * cpad
            for dy in (py - 1, py):
                for dx in (px - 1, px):
                    w3[o:o + cout, :, dy + 1, dx + 1] = w[:, :, py + 1 - 2 * dy, px + 1 - 2 * dx].t()
            if b is not None:
                b3[o:o + cout] = b
    return w3, b3


def axpby_nhwc(x0, a, x1=None, b=0.0, out=None):
    """a * x0 + b * x1 on f32 clip views (flair_axpby_nhwc), products rounded before the sum; out may be x0 or x1."""
    T, H, W, C = x0.shape
    assert x0.dtype == torch.float32 and (x1 is None or (x1.dtype == torch.float32 and x1.shape == x0.shape))
    if out is None:
        out = torch.empty((T, H, W, C), dtype=torch.float32, device=x0.device)
    assert out.dtype == torch.float32 and out.shape == x0.shape
    call.flair_axpby_nhwc(x0, _ld(x0), a, x1, _ld(x1) if x1 is not None else 0, b, C, T * H * W, out, _ld(out))
    return out


def amt_multiflow_prepare(dec, up, out=None):
    """MultiFlowDecoder.forward behind its convblock (flair_amt_multiflow_prepare): dec (B, H, W, >= 40), up (B, H, W, >= 4)
    -> (B, H, W, 40) final flows | sigmoid mask | img_res."""
    B, H, W, _ = dec.shape
    assert dec.dtype == torch.float32 and up.dtype == torch.float32 and tuple(up.shape[:3]) == (B, H, W)
    if out is None:
        out = torch.empty((B, H, W, 40), dtype=torch.float32, device=dec.device)
    call.flair_amt_multiflow_prepare(dec, _ld(dec), up, _ld(up), B * H * W, out, _ld(out))
    return out


def amt_multiflow_combine(pair, prep, neg_mean, x=None, avg=None):
    """multi_flow_combine up to comb_block (flair_amt_multiflow_combine): pair (B, H, W, >= 6) mean-free frames, prep
    (B, H, W, >= 40), neg_mean (B, >= 1) f32 -> x (B, H, W, 16) comb_block's input, avg (B, H, W, 4) the mean prediction."""
    B, H, W, _ = pair.shape
    assert pair.dtype == torch.float32 and prep.dtype == torch.float32 and tuple(prep.shape[:3]) == (B, H, W)
    assert neg_mean.dtype == torch.float32 and neg_mean.shape[0] == B and neg_mean.stride(1) == 1
    if x is None:
        x = torch.empty((B, H, W, 16), dtype=torch.float32, device=pair.device)
    if avg is None:
        avg = torch.empty((B, H, W, 4), dtype=torch.float32, device=pair.device)
    call.flair_amt_multiflow_combine(pair, _ld(pair), prep, _ld(prep), neg_mean, neg_mean.stride(0), B, H, W, x, _ld(x),
         avg, _ld(avg))
    return x, avg


def instance_norm(x, act=ACT_NONE, eps=1e-5, out=None):
    """nn.InstanceNorm2d (no affine) + activation (none or ReLU) on an f32 clip tensor (flair_instnorm_nhwc)."""
    F_, H, W, C = x.shape
    assert x.dtype == torch.float32
    if out is None:
        out = torch.empty((F_, H, W, C), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.shape == x.shape
    nbytes = lib().flair_instnorm_workspace_bytes(F_, H, W, C)
    ws = _workspace(nbytes, x.device, "instnorm")
    call.flair_instnorm_nhwc(x, _ld(x), F_, H, W, C, eps, act, out, _ld(out), ws, nbytes)
    return out
