"""CPU: head widths 192 ... 1024 (multiples of 64) -- the entry refuses what lies outside that range and the other
rules with a message naming the range, before any launch; the modules build at their default one head per layer.
(An accepted shape would launch, so none is passed to the entry here.)"""
import ctypes

import pytest


def _lib():
    from flair_amd import _lib
    return _lib.lib()


def _qattn(L, d, heads=1, dtype=0):
    from flair_amd import ops
    p = ops.AttnParams()
    p.dtype = dtype
    p.frames, p.L, p.heads, p.head_dim = 1, L, heads, d
    p.ld, p.out_ld = 3 * heads * d, heads * d
    p.q_off, p.k_off, p.v_off, p.head_stride = 0, d, 2 * d, 3 * d
    p.scale = 0.125
    return p


def _refused(p):
    lib = _lib()
    rc = lib.flair_qkv_attention(ctypes.byref(p), ctypes.c_void_p(16), ctypes.c_void_p(16), None)
    assert rc == -1
    return lib.flair_last_error()


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("d", [1088, 200])
def test_qkv_entry_refuses_widths_outside_the_wide_range(dtype, d):
    """1088 is beyond 1024; 200 is a multiple of 8 but not of 64: neither has a kernel at L = 4096."""
    msg = _refused(_qattn(4096, d, dtype=dtype))
    assert f"head width {d} unsupported at L = 4096".encode() in msg
    assert b"multiples of 64 from 192 to 1024 at any L" in msg and b"32, 64 and 128" in msg and b"2048" in msg


@pytest.mark.parametrize("d", [192, 512, 1024])
def test_qkv_entry_refuses_wide_heads_beyond_the_row(d):
    p = _qattn(4096, d, heads=2)
    p.ld = 3 * d                                          # one head's q|k|v only
    assert b"exceed ld" in _refused(p)


def test_qkv_entry_refuses_wide_heads_beyond_the_output_row():
    p = _qattn(4096, 512, heads=2)
    p.out_ld = 512
    assert b"exceed ld" in _refused(p)


def test_attention_blocks_build_at_one_head():
    """The modules' defaults (num_heads=1, num_head_channels=-1) at the widths FLAIR's layers have."""
    from flair_amd.guided_diffusion.unet_new import AttentionbottleBlock, AttentionBlock
    assert AttentionBlock(256).num_heads == 1
    assert AttentionBlock(512, use_new_attention_order=True).num_heads == 1
    assert AttentionbottleBlock(512).num_heads == 1
    with pytest.raises(NotImplementedError, match="multiples of 64 from 192 to 1024"):
        AttentionBlock(96, num_head_channels=12)
