"""Attention at head widths other than 64 on the GPU vs the CPU oracle: the spatial MFMA / row kernels at d = 32 and
128, the temporal window kernel at d = 16 ... 256 (d = 96: lanes of the 16-lane group without channels), the blocks
built on them and the two models whose configurations use them (sr3.UNet's default head_dim=32, UNetModel with
num_head_channels=32).  Measured errors go to parity_log; every bound is about 1.5x the largest error measured on an
MI355X for its group of cases (relative to max|ref|), except the f32 spatial blocks (at the f32 accumulation floor)
and the models (the bounds of test_gpu_sr3 / test_gpu_unet).  These are max-norm bounds on randn data: the masked tail of
the last KV tile, the odd and even tile counts, the online rescale and the clamped windows are checked bit for bit, within
1 ulp and per element on inputs with a known softmax in test_gpu_attn_exact.py."""
import pytest
import torch

from tests.golden.weights import name_seeded_weights
from tests.util import from_clip, parity_log, rb, to_clip

DTYPES = [torch.float32, torch.bfloat16]


def _ops():
    from flair_amd import ops
    return ops


# (frames, H, W, heads): L = 256 with 64-query workgroups (NW = 2); L = 1024 with 128-query workgroups (NW = 4);
# L = 400 with a partly masked last KV tile and 128-query workgroups
QKV_CASES = [(16, 16, 16, 2), (16, 32, 32, 2), (5, 20, 20, 13)]


# max|err| / max|ref| measured: f32 <= 2.8e-6 (accumulation order), bf16 <= 3.1e-3 (bf16 output and P rounding)
QKV_REL = {torch.float32: 4e-6, torch.bfloat16: 4.6e-3}


def _check_qkv(got, ref, dtype, what):
    err = (got - ref).abs().max().item()
    bound = QKV_REL[dtype] * ref.abs().max().item() + 1e-6
    parity_log(f"attn_widths qkv {what} {str(dtype)[6:]}: max|err| {err:.3e} (bound {bound:.3e}, "
               f"max|ref| {ref.abs().max().item():.3e})")
    assert err <= bound, f"{what}: max|err|={err:.3e} > {bound:.3e}"


def _qkv_case(d, dtype, new_order, case, seed=11):
    from oracle.unet import qkv_attention_legacy, qkv_attention_new
    Fr, H, W, heads = case
    C = heads * d
    g = torch.Generator().manual_seed(seed)
    qkv = rb(torch.randn(Fr, 3 * C, H * W, generator=g) * 1.5, dtype)
    ref = (qkv_attention_new if new_order else qkv_attention_legacy)(qkv, heads).reshape(Fr, C, H, W)
    y = _ops().qkv_attention(to_clip(qkv.reshape(Fr, 3 * C, H, W), dtype, torch.device("cuda:0")), heads,
                             new_order=new_order)
    torch.cuda.synchronize()
    return from_clip(y), ref


@pytest.mark.gpu
@pytest.mark.parametrize("d", [32, 128])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("new_order", [False, True])
@pytest.mark.parametrize("case", QKV_CASES)
def test_qkv_attention_widths(dev, d, dtype, new_order, case):
    got, ref = _qkv_case(d, dtype, new_order, case)
    _check_qkv(got, ref, dtype, f"d={d} new_order={new_order} {case}")


@pytest.mark.gpu
@pytest.mark.parametrize("d", [32, 128])
def test_qkv_attention_widths_4096_tokens(dev, d):
    """One L = 4096 case per width (bf16, the kernels' 64-query workgroups over 64 / 128 KV tiles)."""
    got, ref = _qkv_case(d, torch.bfloat16, False, (1, 64, 64, 2))
    _check_qkv(got, ref, torch.bfloat16, f"d={d} L=4096")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_qkv_attention_wide_width_routes_to_wide_kernel(dev, dtype):
    """d = 48 (no MFMA kernel) runs on flair_attention_wide through the same entry while d + L <= 2048."""
    got, ref = _qkv_case(48, dtype, True, (2, 16, 16, 2))
    _check_qkv(got, ref, dtype, "d=48 (flair_attention_wide)")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [16, 32, 96, 128, 256])
@pytest.mark.parametrize("window", [5, 7])
def test_temporal_attention_widths(dev, dtype, d, window):
    from oracle.thirdparty import flash_attn_func
    T, H, W = 5, 4, 4
    heads = 2
    C = heads * d
    n = window - 1
    half = window // 2
    g = torch.Generator().manual_seed(5 + d)
    qkv = rb(torch.randn(T, 3 * C, H, W, generator=g), dtype)
    kpos = torch.randn(n, C, generator=g) * 0.3
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    offs = torch.tensor([j for j in range(-half, half + 1) if j != 0])
    idx = (torch.arange(T).view(T, 1) + offs.view(1, n)).clamp(0, T - 1)
    kw = k[idx] + kpos.view(1, n, C, 1, 1)             # T,n,C,H,W
    vw = v[idx]

    def tok(z):  # -> (T*H*W, n, heads, d)
        return z.permute(0, 3, 4, 1, 2).reshape(T * H * W, z.shape[1], heads, d)
    qq = tok(q[:, None])
    if dtype == torch.float32:   # reference rounds through fp16 (nn.py:370-386)
        o = flash_attn_func(qq.half(), tok(kw).half(), tok(vw).half()).float()
    else:
        o = flash_attn_func(qq, tok(kw), tok(vw))
    ref = o.reshape(T, H, W, C).permute(0, 3, 1, 2)
    y = _ops().temporal_attention(to_clip(qkv, dtype, dev), kpos.to(dev), window, round_fp16=(dtype == torch.float32),
                                  head_dim=d)
    torch.cuda.synchronize()
    err = (from_clip(y) - ref).abs().max().item()
    # f32 reproduces the reference's fp16 rounding: measured 0 .. 9.8e-4 (one fp16 ulp in [1, 2)) with max|ref| 2.6 .. 3.6;
    # bf16: max|err| / max|ref| <= 2.8e-3
    bound = 1.5e-3 if dtype == torch.float32 else 4.2e-3 * ref.abs().max().item()
    parity_log(f"attn_widths temporal d={d} window={window} {str(dtype)[6:]}: max|err| {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------------------------------------ blocks
def _clip_in(T, C, S, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, C, S, S, generator=g)


def _run_block(m, x, dtype, dev, film=None):
    from flair_amd.guided_diffusion.unet_new import Ctx
    m = m.to(dev)
    m.pack(dtype, dev)
    ctx = Ctx(dtype, dev, x.shape[0])
    ctx.film_all = film
    y = m.run(ctx, to_clip(x, dtype, dev))
    torch.cuda.synchronize()
    return from_clip(y)


BLOCKS = [  # name, channels, width, new order, bottleneck
    ("AttentionBlock d=32", 256, 32, False, False),
    ("AttentionBlock d=128 new order", 256, 128, True, False),
    ("AttentionbottleBlock d=128", 512, 128, False, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("blk", BLOCKS, ids=[b[0] for b in BLOCKS])
def test_attention_blocks_vs_oracle(dev, dtype, blk):
    from flair_amd.guided_diffusion.unet_new import AttentionbottleBlock, AttentionBlock
    from oracle.unet import AttentionBlock as Oracle
    name, c, d, new_order, bottleneck = blk
    o = name_seeded_weights(Oracle(c, num_head_channels=d, new_order=new_order, bottleneck=bottleneck)).eval()
    m = (AttentionbottleBlock if bottleneck else AttentionBlock)(c, num_head_channels=d,
                                                                 use_new_attention_order=new_order)
    m.load_state_dict(o.state_dict(), strict=True)
    T, S = 3, 16
    x = _clip_in(T, c, S, seed=21)
    emb = torch.randn(T, 512, generator=torch.Generator().manual_seed(22)) if bottleneck else None
    with torch.no_grad():
        ref = o(x[None], emb)[0]
        film = o.emb_layers(emb).to(dev).contiguous() if bottleneck else None
    got = _run_block(m, x, dtype, dev, film)
    # f32: measured <= 2.7e-7, bound at the f32 accumulation-order floor (the CPU oracle's sums change with its thread
    # count); bf16: measured <= 5.7e-3
    rel = 1e-6 if dtype == torch.float32 else 8.6e-3
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    parity_log(f"attn_widths block {name} {str(dtype)[6:]}: rel err {err:.3e} (bound {rel:.0e})")
    assert err <= rel, err


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_temporal_block_vs_oracle(dev, dtype):
    from flair_amd.guided_diffusion.unet_new import TemporalAttention, TemporalWrapper
    from oracle.unet import TemporalAttention as Oracle
    o = name_seeded_weights(Oracle(128, 5, num_head_channels=32)).eval()
    m = TemporalWrapper(TemporalAttention(128, 5, num_head_channels=32))
    m.wrapped_module.load_state_dict(o.state_dict(), strict=True)
    T, S = 6, 8
    x = _clip_in(T, 128, S, seed=23)
    with torch.no_grad():
        ref = o(x[None])[0]
    got = _run_block(m.wrapped_module, x, dtype, dev)
    rel = 1.2e-4 if dtype == torch.float32 else 7.2e-3    # measured 7.6e-5 (fp16 rounding of the reference) / 4.8e-3
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    parity_log(f"attn_widths block TemporalAttention d=32 {str(dtype)[6:]}: rel err {err:.3e} (bound {rel:.0e})")
    assert err <= rel, err


# ------------------------------------------------------------------------------------------------ models
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_sr3_default_head_dim_vs_oracle(dev, dtype):
    """sr3.UNet at its own default head_dim=32, with the tolerances of test_sr3_small_vs_oracle."""
    from flair_amd.guided_diffusion.sr3 import UNet
    from oracle.sr3 import UNet as Oracle
    from tests.test_gpu_sr3 import SR3_SMALL, inputs
    cfg = {k: v for k, v in SR3_SMALL.items() if k != "head_dim"}
    torch.manual_seed(0)
    o = name_seeded_weights(Oracle(**cfg)).eval()
    m = UNet(**cfg)
    m.load_state_dict(o.state_dict(), strict=True)
    m = m.eval()
    x, lr, level = inputs()
    with torch.no_grad():
        ref = o(x, level, low_res_input=lr, num_frames=4, vsrpp_weights=0.93)
    m = m.to(dev)
    if dtype == torch.bfloat16:
        m.convert_to_fp16()
    y = m(x.to(dev), level.to(dev), low_res_input=lr.to(dev), num_frames=4, vsrpp_weights=0.93)
    torch.cuda.synchronize()
    rel = 3e-4 if dtype == torch.float32 else 5e-2
    err = (y.cpu() - ref).abs().max().item() / ref.abs().max().item()
    parity_log(f"attn_widths sr3.UNet head_dim=32 {str(dtype)[6:]}: rel err {err:.3e} (bound {rel:.0e})")
    assert err <= rel, err


@pytest.mark.gpu
def test_unet_width_32_vs_oracle(dev):
    """The small UNetModel of test_gpu_unet with num_head_channels=32 (spatial and temporal blocks at d = 32), f32."""
    from tests.test_gpu_unet import SMALL, _inputs, build_pair
    o, m = build_pair(dict(SMALL, num_head_channels=32))
    T, S = 4, 32
    x, lr, t = _inputs(T, S)
    with torch.no_grad():
        ref = o(x, t, low_res_input=lr, num_frames=T, vsrpp_weights=1.0)
    m = m.to(dev)
    y = m(x.to(dev), t.to(dev), low_res_input=lr.to(dev), num_frames=T, vsrpp_weights=1.0)
    torch.cuda.synchronize()
    rel = 2e-4                                            # test_unet_small_vs_oracle's f32 bound; measured 6.5e-5
    err = (y.cpu() - ref).abs().max().item() / ref.abs().max().item()
    parity_log(f"attn_widths UNetModel num_head_channels=32 float32: rel err {err:.3e} (bound {rel:.0e})")
    assert err <= rel, err
