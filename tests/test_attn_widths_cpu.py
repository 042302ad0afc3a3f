"""CPU: attention head widths other than 64 -- the modules construct at the widths the kernels run and refuse the
others at construction; the C entries refuse unsupported widths with a message before any launch."""
import ctypes

import pytest
import torch


def test_temporal_attention_constructs_at_other_widths():
    from flair_amd.guided_diffusion.unet_new import TemporalAttention
    assert TemporalAttention(128, 5, num_head_channels=32).head_dim == 32
    assert TemporalAttention(256, 5, num_head_channels=128).head_dim == 128
    assert TemporalAttention(256, 7, num_heads=1).head_dim == 256
    assert TemporalAttention(96, 5, num_head_channels=96).head_dim == 96


@pytest.mark.parametrize("channels,width", [(96, 12), (528, 264), (64, 4)])
def test_temporal_attention_refuses_unsupported_widths(channels, width):
    from flair_amd.guided_diffusion.unet_new import TemporalAttention
    with pytest.raises(NotImplementedError, match="multiples of 8 from 8 to 256"):
        TemporalAttention(channels, 5, num_head_channels=width)


def test_attention_blocks_validate_width_at_construction():
    from flair_amd.guided_diffusion.unet_new import AttentionbottleBlock, AttentionBlock
    AttentionBlock(256, num_head_channels=32)
    AttentionBlock(256, num_head_channels=128, use_new_attention_order=True)
    AttentionbottleBlock(512, num_head_channels=128)
    AttentionBlock(256, num_heads=4)                      # num_head_channels=-1: width 64
    with pytest.raises(NotImplementedError, match="32, 64, 128"):
        AttentionBlock(96, num_head_channels=12)
    with pytest.raises(NotImplementedError, match="32, 64, 128"):
        AttentionbottleBlock(512, num_heads=3)           # 512 / 3 heads is no width at all


def test_sr3_unet_builds_at_its_default_head_width():
    """sr3.UNet with its own default head_dim=32 (the bicubic-task model) builds, with the oracle's names."""
    from flair_amd.guided_diffusion.sr3 import UNet
    from flair_amd.guided_diffusion.unet_new import TemporalAttention
    from oracle.sr3 import UNet as Oracle
    from tests.test_gpu_sr3 import SR3_SMALL
    cfg = {k: v for k, v in SR3_SMALL.items() if k != "head_dim"}
    o = Oracle(**cfg)
    m = UNet(**cfg)
    assert list(o.state_dict().keys()) == list(m.state_dict().keys())
    m.load_state_dict(o.state_dict(), strict=True)
    widths = {mod.head_dim for mod in m.modules() if isinstance(mod, TemporalAttention)}
    assert widths == {32}


def test_unet_model_builds_at_width_32():
    from flair_amd.guided_diffusion.unet_new import UNetModel
    from oracle.unet import UNetModel as Oracle
    from tests.test_gpu_unet import SMALL
    cfg = dict(SMALL, num_head_channels=32)
    o, m = Oracle(**cfg), UNetModel(**cfg)
    assert list(o.state_dict().keys()) == list(m.state_dict().keys())
    m.load_state_dict(o.state_dict(), strict=True)


def _lib():
    from flair_amd import _lib
    return _lib.lib()


def _tattn(C, head_dim):
    from flair_amd import ops
    p = ops.TAttnParams()
    p.dtype = 0
    p.T, p.H, p.W, p.C, p.window = 2, 4, 4, C, 5
    p.ld, p.out_ld, p.round_fp16, p.scale, p.head_dim = 3 * C, C, 0, 0.125, head_dim
    return p


@pytest.mark.parametrize("head_dim", [12, 264, 4])
def test_temporal_entry_refuses_unsupported_width(head_dim):
    lib = _lib()
    p = _tattn(24 * 11, head_dim)
    dummy = ctypes.c_void_p(16)
    rc = lib.flair_temporal_attention(ctypes.byref(p), dummy, ctypes.cast(dummy, ctypes.POINTER(ctypes.c_float)), dummy,
                                      None)
    assert rc == -1
    msg = lib.flair_last_error()
    assert f"head width {head_dim} unsupported".encode() in msg and b"8 to 256" in msg


def test_temporal_entry_zero_width_means_64():
    """A zero-filled head_dim (a caller built against ABI version 6) keeps the width-64 meaning: C = 96 is no
    whole number of such heads."""
    lib = _lib()
    p = _tattn(96, 0)
    dummy = ctypes.c_void_p(16)
    rc = lib.flair_temporal_attention(ctypes.byref(p), dummy, ctypes.cast(dummy, ctypes.POINTER(ctypes.c_float)), dummy,
                                      None)
    assert rc == -1 and b"head width=64" in lib.flair_last_error()
    assert lib.flair_abi_version() >= 7


def _qattn(L, d, heads=1):
    from flair_amd import ops
    p = ops.AttnParams()
    p.dtype = 0
    p.frames, p.L, p.heads, p.head_dim = 1, L, heads, d
    p.ld, p.out_ld = 3 * heads * d, heads * d
    p.q_off, p.k_off, p.v_off, p.head_stride = 0, d, 2 * d, 3 * d
    p.scale = 0.125
    return p


@pytest.mark.parametrize("dtype", [0, 1])
def test_qkv_entry_refuses_wide_head_beyond_lds_limit(dtype):
    """d = 48 has no MFMA kernel; flair_attention_wide holds it only while d + L <= 2048."""
    lib = _lib()
    p = _qattn(4096, 48)
    p.dtype = dtype
    rc = lib.flair_qkv_attention(ctypes.byref(p), ctypes.c_void_p(16), ctypes.c_void_p(16), None)
    assert rc == -1
    msg = lib.flair_last_error()
    assert b"head width 48 unsupported at L = 4096" in msg and b"32, 64 and 128" in msg and b"2048" in msg


@pytest.mark.parametrize("d", [12, 0, -8])
def test_qkv_entry_refuses_widths_that_are_no_multiple_of_8(d):
    lib = _lib()
    rc = lib.flair_qkv_attention(ctypes.byref(_qattn(64, d)), ctypes.c_void_p(16), ctypes.c_void_p(16), None)
    assert rc == -1 and f"head width {d} unsupported".encode() in lib.flair_last_error()


def test_qkv_entry_refuses_heads_beyond_the_row():
    lib = _lib()
    p = _qattn(256, 128, heads=2)
    p.ld = 3 * 128                                        # one head's q|k|v only
    rc = lib.flair_qkv_attention(ctypes.byref(p), ctypes.c_void_p(16), ctypes.c_void_p(16), None)
    assert rc == -1 and b"exceed ld" in lib.flair_last_error()


def test_tattn_params_mirror_the_header():
    """ops.TAttnParams appends head_dim after scale, as flair_tattn_params does."""
    from flair_amd import ops
    assert [f[0] for f in ops.TAttnParams._fields_][-2:] == ["scale", "head_dim"]
    assert ops.TAttnParams.head_dim.offset == 40 and ctypes.sizeof(ops.TAttnParams) == 44
