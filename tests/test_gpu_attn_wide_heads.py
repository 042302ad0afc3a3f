"""Spatial attention heads of width 192 ... 1024 (multiples of 64) on the GPU vs the CPU oracle, at any token count: the
channel-split MFMA kernel (bf16) and the row kernel (f32) behind flair_qkv_attention, the blocks at their default one
head per layer, and a UNetModel whose widest level has d = 192 at 4096 tokens (d + L > 2048: refused before these
kernels).  Measured errors go to parity_log; bf16 bounds are about 1.5x the largest error measured on an MI355X for
the group of cases (relative to max|ref|), f32 bounds sit at the accumulation-order floor.  Row clamping to L - 1, the
masked last tile, the cross-wave exchange and the online rescale of these kernels are checked bit for bit, within 1 ulp
and per element on inputs with a known softmax in test_gpu_attn_exact.py (all three (NW, CPW) builds)."""
import functools

import pytest
import torch

from tests.golden.weights import name_seeded_weights
from tests.util import from_clip, parity_log, to_clip

DTYPES = [torch.float32, torch.bfloat16]


def _ops():
    from flair_amd import ops
    return ops


def _check(err, ref_max, rel, what):
    bound = rel * ref_max + 1e-6
    parity_log(f"attn_wide_heads {what}: max|err| {err:.3e} (bound {bound:.3e}, max|ref| {ref_max:.3e})")
    assert err <= bound, f"{what}: max|err|={err:.3e} > {bound:.3e}"


# ------------------------------------------------------------------------------------------------ kernels
# (frames, H, W, heads, new order, padded ld): L = 64 (two heads, two frames, two query blocks, two KV tiles),
# L = 1000 (ragged last query block and KV tile, q/k/v and output rows padded), L = 4096 (refused before: d + L > 2048)
KCASES = [(2, 8, 8, 2, False, False), (1, 25, 40, 1, True, True), (1, 64, 64, 1, False, False)]
WIDTHS = [192, 256, 512, 1024]

# max|err| / max|ref| measured: f32 <= 2.0e-6 up to L = 1000 and 4.9e-6 at L = 4096 (accumulation order over 4096 keys,
# the CPU oracle's included), bf16 <= 3.2e-3 (bf16 output and P rounding)
KREL = {torch.float32: 1e-5, torch.bfloat16: 4.6e-3}


@functools.lru_cache(maxsize=None)
def _kernel_case(d, case):
    """bf16-representable inputs (so one oracle serves both dtypes) and the oracle's output."""
    from oracle.unet import qkv_attention_legacy, qkv_attention_new
    Fr, H, W, heads, new_order, _ = case
    C = heads * d
    g = torch.Generator().manual_seed(d + H)
    qkv = (torch.randn(Fr, 3 * C, H * W, generator=g) * 1.5).to(torch.bfloat16).float()
    ref = (qkv_attention_new if new_order else qkv_attention_legacy)(qkv, heads).reshape(Fr, C, H, W)
    return qkv.reshape(Fr, 3 * C, H, W), ref


def _run_kernel(qkv, heads, new_order, padded, dtype, dev):
    Fr, C3, H, W = qkv.shape
    C = C3 // 3
    x = to_clip(qkv, dtype, dev, pad_to=C3 + 72 if padded else None)[..., :C3]
    out = None
    if padded:
        out = torch.full((Fr, H, W, C + 40), float("nan"), dtype=dtype, device=dev)[..., :C]
    y = _ops().qkv_attention(x, heads, new_order=new_order, out=out)
    torch.cuda.synchronize()
    return from_clip(y)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("case", KCASES, ids=["L64", "L1000-padded-new", "L4096"])
def test_qkv_attention_wide_heads(dev, dtype, d, case):
    Fr, H, W, heads, new_order, padded = case
    qkv, ref = _kernel_case(d, case)
    got = _run_kernel(qkv, heads, new_order, padded, dtype, dev)
    err = (got - ref).abs().max().item()
    _check(err, ref.abs().max().item(), KREL[dtype], f"qkv d={d} L={H * W} {case} {str(dtype)[6:]}")


@pytest.mark.gpu
def test_qkv_attention_wide_heads_16384_tokens(dev):
    """d = 256 over 128 x 128 tokens (bf16): 256 fixed random query rows against the oracle over all keys."""
    d, H, W = 256, 128, 128
    L = H * W
    g = torch.Generator().manual_seed(16384)
    qkv = (torch.randn(1, 3 * d, H, W, generator=g) * 1.5).to(torch.bfloat16).float()
    got = _run_kernel(qkv, 1, False, False, torch.bfloat16, dev).reshape(d, L)
    rows = torch.randperm(L, generator=g)[:256]
    t = qkv.reshape(3 * d, L)
    q, k, v = t[:d, rows], t[d:2 * d], t[2 * d:]
    w = torch.softmax((q.t() @ k) / d ** 0.5, dim=-1)              # (256, L)
    ref = (w @ v.t()).t()                                          # (d, 256)
    err = (got[:, rows] - ref).abs().max().item()
    _check(err, ref.abs().max().item(), KREL[torch.bfloat16], "qkv d=256 L=16384 (256 rows) bfloat16")


# ------------------------------------------------------------------------------------------------ blocks
BLOCKS = [  # name, channels, S, new order, bottleneck
    ("AttentionBlock(256) 64x64", 256, 64, False, False),
    ("AttentionBlock(256) 64x64 new order", 256, 64, True, False),
    ("AttentionBlock(512) 32x32", 512, 32, False, False),
    ("AttentionBlock(512) 32x32 new order", 512, 32, True, False),
    ("AttentionbottleBlock(512) 32x32", 512, 32, False, True),
]

# f32 at the accumulation-order floor of 1024 / 4096 keys (the kernel cases' bound); bf16: test_gpu_attn_widths' block bound
BREL = {torch.float32: 1e-5, torch.bfloat16: 8.6e-3}


@functools.lru_cache(maxsize=None)
def _block_case(c, S, new_order, bottleneck):
    from oracle.unet import AttentionBlock as Oracle
    o = name_seeded_weights(Oracle(c, num_head_channels=-1, new_order=new_order, bottleneck=bottleneck)).eval()
    T = 2
    x = torch.randn(T, c, S, S, generator=torch.Generator().manual_seed(c + S))
    emb = torch.randn(T, 512, generator=torch.Generator().manual_seed(22)) if bottleneck else None
    with torch.no_grad():
        ref = o(x[None], emb)[0]
        film = o.emb_layers(emb).contiguous() if bottleneck else None
    return o.state_dict(), x, film, ref


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("blk", BLOCKS, ids=[b[0] for b in BLOCKS])
def test_attention_blocks_one_head_vs_oracle(dev, dtype, blk):
    """The blocks at their default arguments (num_heads=1, num_head_channels=-1): one head as wide as the block."""
    from flair_amd.guided_diffusion.unet_new import AttentionbottleBlock, AttentionBlock, Ctx
    name, c, S, new_order, bottleneck = blk
    sd, x, film, ref = _block_case(c, S, new_order, bottleneck)
    m = (AttentionbottleBlock if bottleneck else AttentionBlock)(c, use_new_attention_order=new_order)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev)
    m.pack(dtype, dev)
    ctx = Ctx(dtype, dev, x.shape[0])
    ctx.film_all = film.to(dev) if bottleneck else None
    got = from_clip(m.run(ctx, to_clip(x, dtype, dev)))
    err = (got - ref).abs().max().item()
    _check(err, ref.abs().max().item(), BREL[dtype], f"block {name} {str(dtype)[6:]}")


# ------------------------------------------------------------------------------------------------ model
# num_heads=2 with num_head_channels=-1 (the num_heads path of the defaults): input and output levels at 64 x 64 have
# 384 channels, so d = 192 over L = 4096 (refused before this kernel) and d = 192 over 1024 tokens at 32 x 32; the
# middle block has d = 256 over 256 tokens.  One head per layer (num_heads=1) would give the middle block's temporal
# attention a width of 512, beyond flair_temporal_attention's 256.  No recurrent (BasicVSR++) levels: its alignment
# does not run the 768 channels they would have here.
WIDE_CFG = dict(image_size=64, in_channels=6, model_channels=128, out_channels=6, num_res_blocks=1,
                attention_resolutions=(1, 2), rnn_resolutions=(), channel_mult=(3, 3, 4), use_fp16=False,
                num_heads=2, num_head_channels=-1, resblock_updown=True, use_scale_shift_norm=True,
                temporal_block=True, use_checkpoint=False)


@functools.lru_cache(maxsize=None)
def _model_case():
    from tests.test_gpu_unet import _inputs, build_pair
    o, m = build_pair(WIDE_CFG)
    T = 2
    x, lr, t = _inputs(T, 64)
    with torch.no_grad():
        ref = o(x, t, low_res_input=lr, num_frames=T, vsrpp_weights=1.0)
    return m, (x, lr, t), ref


@pytest.mark.gpu
def test_unet_wide_heads_vs_oracle(dev):
    from flair_amd.guided_diffusion.unet_new import AttentionBlock
    m, (x, lr, t), ref = _model_case()
    assert {mod.channels // mod.num_heads for mod in m.modules() if isinstance(mod, AttentionBlock)} == {192, 256}
    m = m.to(dev)
    m.convert_to_fp32()
    y = m(x.to(dev), t.to(dev), low_res_input=lr.to(dev), num_frames=x.shape[0], vsrpp_weights=1.0)
    torch.cuda.synchronize()
    rel = 2e-4                                            # test_unet_small_vs_oracle's f32 bound
    err = (y.cpu() - ref).abs().max().item() / ref.abs().max().item()
    parity_log(f"attn_wide_heads UNetModel {WIDE_CFG['channel_mult']} num_heads=2 float32: rel err {err:.3e} "
               f"(bound {rel:.0e})")
    assert err <= rel, err


@pytest.mark.gpu
def test_unet_wide_heads_hip_graph_replay_matches_eager(dev):
    """bf16: the captured forward (the wide-head launches inside the graph) replays bit-identically to eager."""
    m, (x, lr, t), _ = _model_case()
    m = m.to(dev)
    m.convert_to_fp16()
    T = x.shape[0]
    lr = lr.to(dev)
    cases = [((x + 0.01 * k).to(dev), torch.full((T,), tv, dtype=torch.long, device=dev))
             for k, tv in enumerate((371, 12))]
    eager = [m(xx, tt, low_res_input=lr, num_frames=T, vsrpp_weights=1.0).clone() for xx, tt in cases]
    m.enable_hip_graph()
    try:
        for (xx, tt), ref in zip(cases, eager):
            y = m(xx, tt, low_res_input=lr, num_frames=T, vsrpp_weights=1.0)
            torch.cuda.synchronize()
            assert torch.equal(y, ref)
        assert len(m._graphs) == 1
    finally:
        m.enable_hip_graph(False)
        m.convert_to_fp32()
