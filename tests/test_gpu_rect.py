"""Rectangular frames on the GPU: the one-launch JPEG codec, the operators, both networks' flow plumbing and the window
loop at H != W, each against the oracle that already defines it (oracle.degrade per 16x16 MCU, BlurOperator, two
SeparableSR, oracle.unet with a rectangular forward, the stock oracle.sr3, the oracle window loop)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RECT = [(16, 48), (48, 16), (32, 80)]


# ------------------------------------------------------------------------------------------ JPEG
def jpeg_image(seed, H, W):
    """The _jpeg_image recipe of tests/test_gpu_sampler.py at H x W."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(2, 3, 8, 8, generator=g) * 2 - 1
    return (F.interpolate(base, (H, W), mode="bilinear") + 0.1 * torch.randn(2, 3, H, W, generator=g)).clamp(-1, 1)


def to_tiles(x, t=16):
    """(N,C,H,W) -> (N*H/t*W/t, C, t, t), tiles in row-major order."""
    N, C, H, W = x.shape
    return x.reshape(N, C, H // t, t, W // t, t).permute(0, 2, 4, 1, 3, 5).reshape(-1, C, t, t)


def from_tiles(tiles, N, H, W):
    C, t = tiles.shape[1], tiles.shape[-1]
    return tiles.reshape(N, H // t, W // t, C, t, t).permute(0, 3, 1, 4, 2, 5).reshape(N, C, H, W)


def pre_rounding(x, qf):
    """_jpeg_pre_rounding of tests/test_gpu_sampler.py for any batch size: the oracle's luma / chroma values just
    before .round(), recomputed with its own helpers."""
    from oracle import degrade as odeg
    n, S = x.shape[0], x.shape[-1]
    xx = (x + 1) / 2 * 255
    m = torch.tensor([[0.299, 0.587, 0.114], [-0.1687, -0.3313, 0.5], [0.5, -0.4187, -0.0813]])
    ycc = torch.einsum("nchw,kc->nkhw", xx, m).clone()
    ycc[:, 1:] += 128
    q1, q2 = odeg.quant_tables(qf)
    D = odeg._dct_matrix()
    pre_l = odeg._unblocks(odeg._lin2d(odeg._blocks(ycc[:, 0:1]).reshape(-1, 8, 8) - 128, D).view(-1, 1, 8, 8) / q1, n, 1, S)
    pre_c = odeg._unblocks(odeg._lin2d(odeg._blocks(ycc[:, 1:, ::2, ::2]).reshape(-1, 8, 8) - 128, D).view(-1, 2, 8, 8) / q2,
                           n, 2, S // 2)
    return pre_l, pre_c


def oracle_per_mcu(x, qf):
    """The codec is independent per 16x16 MCU: the oracle on every tile, reassembled.
    Returns (decoded, luma levels, chroma levels, luma pre-rounding, chroma pre-rounding)."""
    from oracle import degrade as odeg
    N, _, H, W = x.shape
    tiles = to_tiles(x)
    luma, chroma = odeg.jpeg_encode(tiles, qf)
    dec = odeg.jpeg_decode([luma, chroma], qf)
    pre_l, pre_c = pre_rounding(tiles, qf)
    return (from_tiles(dec, N, H, W), from_tiles(luma, N, H, W), from_tiles(chroma, N, H // 2, W // 2),
            from_tiles(pre_l, N, H, W), from_tiles(pre_c, N, H // 2, W // 2))


def near_tie(pre):
    return ((pre - pre.floor()) - 0.5).abs() < 2e-3


def test_per_mcu_oracle_is_the_whole_image_oracle():
    """The reference used below: on a 48 x 48 image the tile-wise oracle equals the whole-image oracle exactly."""
    from oracle import degrade as odeg
    x = jpeg_image(5, 48, 48)
    dec, luma, chroma, _, _ = oracle_per_mcu(x, 30)
    ref_l, ref_c = odeg.jpeg_encode(x, 30)
    assert torch.equal(luma, ref_l) and torch.equal(chroma, ref_c)
    assert torch.equal(dec, odeg.jpeg_decode([ref_l, ref_c], 30))


@pytest.mark.parametrize("qf", [10, 60, 90])
@pytest.mark.parametrize("H,W", RECT)
def test_jpeg_rect_quantised_levels_bit_exact(dev, H, W, qf):
    """The rule of test_jpeg_quantised_levels_bit_exact on rectangular images: equal outside the oracle's own 2e-3 tie
    band, at most one level apart inside it, band share below 1 % per plane."""
    from flair_amd.guided_diffusion.jpeg import jpeg_encode
    x = jpeg_image(100 + qf, H, W)
    _, ref_luma, ref_chroma, pre_l, pre_c = oracle_per_mcu(x, qf)
    assert torch.equal(pre_l.round(), ref_luma) and torch.equal(pre_c.round(), ref_chroma)
    got_luma, got_chroma = (t.cpu() for t in jpeg_encode(x.to(dev), qf))
    for name, got, ref, pre in (("luma", got_luma, ref_luma, pre_l), ("chroma", got_chroma, ref_chroma, pre_c)):
        assert got.shape == ref.shape and torch.equal(got, got.round())
        band = near_tie(pre)
        print(f"jpeg levels {H}x{W} qf={qf} {name}: {int(band.sum())} of {band.numel()} in the band, "
              f"{int((got != ref).sum())} differ, max |diff| {(got - ref).abs().max().item()}")
        assert band.float().mean().item() < 0.01
        assert torch.equal(got[~band], ref[~band])
        assert (got - ref).abs().max().item() <= 1.0


@pytest.mark.parametrize("H,W,qf,seed", [(16, 48, 10, 9), (16, 48, 30, 8), (48, 16, 10, 3), (48, 16, 30, 12),
                                         (32, 80, 10, 21)])
def test_jpeg_rect_roundtrip_every_pixel(dev, H, W, qf, seed):
    """The form of test_jpeg_roundtrip_small_sizes_every_pixel: seeds whose oracle has no coefficient in the tie band
    (asserted first), so no level can flip and every pixel agrees to 1e-4."""
    from flair_amd.guided_diffusion.jpeg import jpeg_decode, jpeg_encode
    x = jpeg_image(seed, H, W)
    ref, _, _, pre_l, pre_c = oracle_per_mcu(x, qf)
    assert not near_tie(pre_l).any() and not near_tie(pre_c).any(), "the seed no longer avoids the .5 boundaries"
    got = jpeg_decode(jpeg_encode(x.to(dev), qf), qf).cpu()
    err = (got - ref).abs().max().item()
    print(f"jpeg round trip {H}x{W} qf={qf}: max|err| = {err:.3e}")
    assert err <= 1e-4


@pytest.mark.parametrize("S", [16, 48, 64])
def test_jpeg_hw_entry_equals_square_entry_bit_for_bit(dev, S):
    """flair_jpeg_roundtrip_hw and the three-launch flair_jpeg_roundtrip share their arithmetic: on squares the image
    and both level planes are identical -- what lets ops.jpeg_roundtrip send every shape to the one-launch entry."""
    from flair_amd import ops
    from flair_amd.guided_diffusion.jpeg import dct8_matrix, general_quant_matrix
    for qf in (10, 60, 90):
        x = jpeg_image(100 + qf, S, S).to(dev)
        q1, q2 = general_quant_matrix(qf)
        new, (nl, nc) = ops.jpeg_roundtrip(x, q1, q2, dct8_matrix().reshape(-1), want_levels=True, entry="hw")
        old, (ol, oc) = ops.jpeg_roundtrip(x, q1, q2, dct8_matrix().reshape(-1), want_levels=True, entry="square")
        assert torch.equal(new, old) and torch.equal(nl, ol) and torch.equal(nc, oc), qf
        assert torch.equal(ops.jpeg_roundtrip(x, q1, q2, dct8_matrix().reshape(-1)), old)


# ------------------------------------------------------------------------------------- operators
@pytest.mark.parametrize("H,W", [(32, 48), (48, 32)])
def test_blur_operator_rect_vs_oracle(dev, H, W):
    """The six comparisons and the 2e-5 of test_blur_operator_vs_oracle (pseudoSR_PyTorch is shape-agnostic: a pin)."""
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion import pseudoSR as psr
    from oracle import degrade as odeg
    g = torch.Generator().manual_seed(3)
    x = torch.rand(3, 3, H, W, generator=g) * 2 - 1
    lr = torch.rand(3, 3, H // 4, W // 4, generator=g) * 2 - 1
    kern = wl.synthetic_blur_kernel(sigma=1.8)
    o = odeg.BlurOperator(kern, 4)
    A = psr.pseudoSR(psr.Get_pseudoSR_Conf(4), upscale_kernel=kern, kernel_indx=10).WrapArchitecture_PyTorch().to(dev)
    for name, got, ref in [("down", A.DownscaleOP(x.to(dev)), o.down(x)),
                           ("inv", A.Conv_LR_with_Inv_hTh_OP(lr.to(dev)), o.inv(lr)),
                           ("up", A.Upscale_OP(lr.to(dev)), o.up(lr)),
                           ("a_pinv", A.A_pinv(lr.to(dev), x.to(dev)), o.a_pinv(lr, x)),
                           ("a_pinv_lr", A.A_pinv(lr.to(dev)), o.a_pinv(lr)),
                           ("a_forward", A.A(x.to(dev)), o.a_forward(x))]:
        assert got.shape == ref.shape, name
        err = (got.cpu() - ref).abs().max().item()
        assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (name, err)


@pytest.mark.parametrize("H,W", [(32, 64), (64, 32)])
def test_srconv_rect_vs_two_oracles(dev, H, W):
    """SRConv((H, W), stride 8): A = F_H X F_W^T and A_pinv = P_H Y P_W^T against the matrices of two
    oracle.degrade.SeparableSR (one per axis), at the bounds of test_srconv_vs_oracle_and_golden (5e-5, 5e-4, and
    1e-3 for the projection A A^+ A = A)."""
    from flair_amd.guided_diffusion.restore_util import SRConv
    from oracle import degrade as odeg
    f = 8
    taps = torch.from_numpy(odeg.bicubic_taps(f)).float()
    k = taps / taps.sum()
    oh, ow = odeg.SeparableSR(k, 3, H, f), odeg.SeparableSR(k, 3, W, f)
    fwd = lambda o: o.U @ torch.diag(o.sv) @ o.V[:, :o.s].t()                                        # noqa: E731
    pinv = lambda o: o.V[:, :o.s] @ torch.diag(torch.where(o.sv > 0, 1.0 / o.sv, torch.zeros_like(o.sv))) @ o.U.t()  # noqa: E731
    g = torch.Generator().manual_seed(6)
    img = torch.rand(2, 3, H, W, generator=g) * 2 - 1
    ref_y = fwd(oh) @ img.reshape(6, H, W) @ fwd(ow).t()
    ref_back = pinv(oh) @ ref_y @ pinv(ow).t()
    sr = SRConv(k, 3, (H, W), dev, stride=f)
    y = sr.A(img.reshape(2, -1).to(dev))
    assert y.shape == (2, 3 * (H // f) * (W // f))
    assert (y.cpu() - ref_y.reshape(2, -1)).abs().max().item() <= 5e-5
    back = sr.A_pinv(ref_y.reshape(2, -1).to(dev))
    assert back.shape == (2, 3 * H * W)
    assert (back.cpu() - ref_back.reshape(2, -1)).abs().max().item() <= 5e-4
    assert (sr.A(sr.A_pinv(y)) - y).abs().max().item() <= 1e-3
    # the spectrum is the outer product of the two axes' spectra (f64 SVD here, f32 in the oracle: 1e-5 on values <= 1)
    assert torch.equal(sr.singulars().cpu(), torch.outer(*sr.singulars_hw).reshape(-1).repeat_interleave(3))
    assert (sr.singulars().cpu() - torch.outer(oh.sv, ow.sv).reshape(-1).repeat_interleave(3)).abs().max().item() <= 1e-5


# ------------------------------------------------------------------------------------- UNetModel
def rect_oracle_class():
    """oracle.unet.UNetModel with the flow rule of rectangular clips: the level at down-sampling s takes the flows of
    the conditioning clip resized bicubically to (H/s, W/s), stored under W/s.  Only forward differs."""
    from oracle import unet as ou

    class RectOracle(ou.UNetModel):
        def forward(self, x, timesteps, low_res_input=None, num_frames=None, rnn_input=None,
                    enable_cross_frames=True, vsrpp_weights=None, **kwargs):
            H, W = x.shape[-2:]
            x = x.reshape(-1, num_frames, *x.shape[1:])
            x = torch.cat([x, low_res_input], dim=2)
            if rnn_input is None:
                rnn_input = low_res_input
            flows = {}
            for r in self.need_flows_res:
                s = self.image_size // r
                hw = (H // s, W // s)
                fi = rnn_input if tuple(rnn_input.shape[-2:]) == hw else \
                    ou.per_frame(rnn_input, lambda z: F.interpolate(z, hw, mode="bicubic"))
                flows[hw[1]] = self.compute_flow(fi)
            emb = self.time_embed(ou.timestep_embedding(timesteps, self.model_channels))
            h, hs = x, []
            for blk in self.input_blocks:
                h = blk(h, emb, flows, vsrpp_weights, enable_cross_frames)
                hs.append(h)
            h = self.middle_block(h, emb, flows, vsrpp_weights, enable_cross_frames)
            for blk in self.output_blocks:
                h = blk(torch.cat([h, hs.pop()], dim=2), emb, flows, vsrpp_weights, enable_cross_frames)
            h = F.silu(ou.group_norm_over_clip(h, self.out[0].wrapped_module))
            h = ou.per_frame(h, self.out[2].wrapped_module)
            return h.reshape(-1, *h.shape[2:])
    return RectOracle


def rect_oracle(cfg, seed=0):
    """The oracle half of build_pair of tests/test_gpu_unet.py, with the rectangular forward."""
    torch.manual_seed(seed)
    o = rect_oracle_class()(**cfg)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in o.parameters():
            if p.abs().sum() == 0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    return o.eval()


def hip_unet(cfg, state_dict):
    from flair_amd.guided_diffusion.unet_new import UNetModel
    m = UNetModel(**cfg)
    m.load_state_dict(state_dict, strict=True)
    return m.eval()


def unet_inputs(T, H, W, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, 3, H, W, generator=g)
    base = torch.rand(3, H, W, generator=g) * 2 - 1
    lr = torch.stack([torch.roll(base, shifts=(i, 2 * i), dims=(1, 2)) for i in range(T)])[None]
    lr = (lr + 0.05 * torch.randn(1, T, 3, H, W, generator=g)).clamp(-1, 1)
    return x, lr, torch.full((T,), 371, dtype=torch.long)


_unet_ref = {}


def unet_reference(T, H, W):
    """The oracle's stages and output for one shape, computed once and shared by the f32 and bf16 cases."""
    if (T, H, W) not in _unet_ref:
        from tests.test_gpu_unet import SMALL
        o = rect_oracle(dict(SMALL, image_size=W))
        x, lr, t = unet_inputs(T, H, W)
        stages = []
        hook = lambda name: (lambda mod, inp, out: stages.append((name, out.detach())))       # noqa: E731
        for i, b in enumerate(o.input_blocks):
            b.register_forward_hook(hook(f"input_blocks.{i}"))
        o.middle_block.register_forward_hook(hook("middle_block"))
        for i, b in enumerate(o.output_blocks):
            b.register_forward_hook(hook(f"output_blocks.{i}"))
        with torch.no_grad():
            ref = o(x, t, low_res_input=lr, num_frames=T, vsrpp_weights=1.0)
        _unet_ref[(T, H, W)] = (o.state_dict(), stages, ref)
    return _unet_ref[(T, H, W)]


def test_rect_oracle_equals_stock_oracle_on_a_square_clip():
    from oracle.unet import UNetModel as Stock
    from tests.test_gpu_unet import SMALL
    o = rect_oracle(SMALL)
    stock = Stock(**SMALL).eval()
    stock.load_state_dict(o.state_dict())
    x, lr, t = unet_inputs(2, 32, 32)
    with torch.no_grad():
        assert torch.equal(o(x, t, low_res_input=lr, num_frames=2, vsrpp_weights=1.0),
                           stock(x, t, low_res_input=lr, num_frames=2, vsrpp_weights=1.0))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,H,W", [(3, 32, 48), (2, 48, 32), (2, 40, 64)])
def test_unet_rect_vs_oracle(dev, T, H, W, dtype):
    """Per stage and for the output, at the 2e-4 (f32) / 5e-2 (bf16) of test_unet_small_vs_oracle."""
    from tests.test_gpu_unet import SMALL
    from tests.util import from_clip
    sd, stages, ref = unet_reference(T, H, W)
    m = hip_unet(dict(SMALL, image_size=W), sd).to(dev)
    if dtype == torch.bfloat16:
        m.convert_to_fp16()
    x, lr, t = unet_inputs(T, H, W)
    m._trace = []
    y = m(x.to(dev), t.to(dev), low_res_input=lr.to(dev), num_frames=T, vsrpp_weights=1.0)
    torch.cuda.synchronize()
    rel = 2e-4 if dtype == torch.float32 else 5e-2
    assert len(stages) == len(m._trace) and y.shape == ref.shape == (T, 6, H, W)
    report = []
    for (n1, a), (n2, b) in zip(stages, m._trace):
        assert n1 == n2
        a4 = a[0].float()
        report.append((n1, (from_clip(b) - a4).abs().max().item() / (a4.abs().max().item() + 1e-12)))
    err = (y.cpu() - ref).abs().max().item() / ref.abs().max().item()
    print(f"UNetModel {T}x{H}x{W} {dtype}: output {err:.2e}, worst stage {max(report, key=lambda r: r[1])}")
    bad = [r for r in report if r[1] > rel]
    assert not bad, f"stages beyond {rel}: {bad[:4]} (all: {report})"
    assert err <= rel, (err, report)


def test_unet_rect_hip_graph_replay_matches_eager(dev):
    """test_hip_graph_replay_matches_eager on a rectangular clip: capture, pure replays with new latents / timesteps,
    and a re-capture for a new conditioning clip, all bit-identical to eager launches."""
    from tests.test_gpu_unet import SMALL
    T, H, W = 3, 32, 48
    cfg = dict(SMALL, image_size=W)
    m = hip_unet(cfg, rect_oracle(cfg).state_dict()).to(dev)
    m.convert_to_fp16()
    cases, clips = [], {}
    for seed, tval in [(3, 371), (3, 12), (8, 940)]:
        x, lr, _ = unet_inputs(T, H, W, seed=seed)
        if seed not in clips:
            clips[seed] = lr.to(dev)
        cases.append(((x + 0.01 * tval).to(dev), clips[seed], torch.full((T,), tval, dtype=torch.long, device=dev)))
    eager = [m(x, t, low_res_input=lr, num_frames=T, vsrpp_weights=1.0).clone() for x, lr, t in cases]
    m.enable_hip_graph()
    graphs = []
    for (x, lr, t), ref in zip(cases, eager):
        y = m(x, t, low_res_input=lr, num_frames=T, vsrpp_weights=1.0)
        torch.cuda.synchronize()
        assert torch.equal(y, ref)
        assert len(m._graphs) == 1
        graphs.append(next(iter(m._graphs.values()))["graph"])
    assert graphs[0] is graphs[1] and graphs[2] is not graphs[0]
    m.enable_hip_graph(False)


# -------------------------------------------------------------------------------------- sr3.UNet
def sr3_inputs(T, H, W, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, 3, H, W, generator=g)
    base = torch.rand(3, H, W, generator=g) * 2 - 1
    lr = torch.stack([torch.roll(base, shifts=(i, 2 * i), dims=(1, 2)) for i in range(T)])[None]
    lr = (lr + 0.05 * torch.randn(1, T, 3, H, W, generator=g)).clamp(-1, 1)
    return x, lr, torch.full((T,), 0.83)


_sr3_ref = {}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,H,W", [(2, 64, 96), (2, 96, 64)])
def test_sr3_rect_vs_stock_oracle(dev, T, H, W, dtype):
    """The stock oracle.sr3 resizes the flow input to hidden.shape[-2:], so it is the reference as it stands;
    configuration and bounds (3e-4 f32, 5e-2 bf16) of tests/test_gpu_sr3.py."""
    from tests.test_gpu_sr3 import build_pair
    o, m = build_pair()
    x, lr, level = sr3_inputs(T, H, W)
    if (T, H, W) not in _sr3_ref:
        with torch.no_grad():
            _sr3_ref[(T, H, W)] = o(x, level, low_res_input=lr, num_frames=T, vsrpp_weights=0.93)
    ref = _sr3_ref[(T, H, W)]
    m = m.to(dev)
    if dtype == torch.bfloat16:
        m.convert_to_fp16()
    y = m(x.to(dev), level.to(dev), low_res_input=lr.to(dev), num_frames=T, vsrpp_weights=0.93)
    torch.cuda.synchronize()
    rel = 3e-4 if dtype == torch.float32 else 5e-2
    err = (y.cpu() - ref).abs().max().item() / ref.abs().max().item()
    print(f"sr3.UNet {T}x{H}x{W} {dtype}: {err:.2e}")
    assert y.shape == ref.shape and err <= rel, err


# ----------------------------------------------------------------------------------- window loop
def _tapes(N, h, w, H, W, L, OV, steps, seed):
    from flair_amd import video
    g = torch.Generator().manual_seed(seed)
    degraded = torch.rand(1, N, 3, h, w, generator=g)
    wins = video.window_indices(N, L, OV)
    tapes = [[torch.randn(len(i), 3, H, W, generator=g) for _ in range(steps)] for i in wins]
    qnoise = [torch.randn(len(i), 3, H, W, generator=g) for i in wins]
    return degraded, wins, tapes, qnoise


def _oracle_windows(degraded, wins, tapes, qnoise, H, W, OV, steps, tau, model, aux_model):
    """scripts/video_sample.py:371-485 on oracle.diffusion for H x W frames, as tests/test_gpu_unaligned_video.py
    assembles it; aux_model sees whole frames (the un-aligned composition is restated inside it)."""
    from flair_amd import workload as wl
    from oracle import degrade as odeg
    from oracle import diffusion as odiff
    hp = wl.TASKS["gaussian"]
    tab = odiff.Spaced(odiff.spaced_steps(1000, str(steps)), odiff.named_betas("face_blur", 1000))
    oblur = odeg.BlurOperator(wl.synthetic_blur_kernel(), 4)
    prev, ref = None, []
    for wi, idx in enumerate(wins):
        d = degraded[:, idx[0]:idx[-1] + 1]
        init = F.interpolate(d[0], (H, W), mode="area").clamp(0, 1)[None]
        d_n, init_n = (d - 0.5) / 0.5, (init - 0.5) / 0.5
        a = torch.from_numpy(tab.sqrt_alphas_cumprod).float()[tab.num_timesteps - 1]
        b = torch.from_numpy(tab.sqrt_one_minus_alphas_cumprod).float()[tab.num_timesteps - 1]
        rnn = F.interpolate(d_n[0], (H, W), mode="bicubic", align_corners=False).clamp(-1, 1)[None]
        sample = odiff.sample_loop(tab, model, a * init_n[0] + b * qnoise[wi],
                                   model_kwargs=dict(low_res_input=init_n, num_frames=len(idx), rnn_input=rnn),
                                   restore_fn=lambda x0, _d=d_n: oblur.a_pinv(_d[0], x0), aux_model=aux_model, w=hp["w"],
                                   tau=tau, rho=hp["rho"], noise_level=hp["noise_level"], zeta=hp["zeta"], prev_recon=prev,
                                   step_noise=tapes[wi])[None]
        if prev is not None:
            sample = sample[:, OV:]
        prev = sample[:, -OV:].clone()
        ref.append((sample.clamp(-1, 1) + 1) / 2)
    return torch.cat(ref, 1)[0]


def test_window_loop_rect_aligned_vs_oracle_loop(dev):
    """restore_video(size=(32, 48)): two windows sharing one frame, aligned, against the oracle loop at the 2e-3 of
    tests/test_gpu_unaligned_video.py; and the refusals of the pair mode come before any launch."""
    from flair_amd import video
    from flair_amd import workload as wl
    from tests.test_gpu_unaligned_video import _M, _blur_op, _toy_model
    N, H, W, L, OV, steps, tau = 4, 32, 48, 3, 1, 2, 0
    degraded, wins, tapes, qnoise = _tapes(N, H // 4, W // 4, H, W, L, OV, steps, 31)
    assert wins == [[0, 1, 2], [2, 3]]
    ref = _oracle_windows(degraded, wins, tapes, qnoise, H, W, OV, steps, tau, _toy_model, None)
    m = _M(degraded.to(dev))
    common = dict(tau=tau, length=L, overlap=OV, noise_fn=lambda wi, it, like: tapes[wi][it].to(dev),
                  q_noise_fn=lambda wi, like: qnoise[wi].to(dev))
    got = video.restore_video("gaussian", degraded.to(dev), m, wl.diffusion_for(steps), _blur_op(dev), size=(H, W), **common)
    torch.cuda.synchronize()
    assert got.shape == ref.shape == (N, 3, H, W) and m.calls == steps * len(wins)
    for i in range(N):
        err = (got[i].cpu() - ref[i]).abs().max().item()
        print(f"aligned window loop {H}x{W}, frame {i}: max|err| = {err:.3e}")
        assert err <= 2e-3, (i, err)
    m = _M(degraded.to(dev))
    with pytest.raises(ValueError, match=r"48x32.*12x8.*8x12"):          # the pair is (H, W): no implicit resize
        video.restore_video("gaussian", degraded.to(dev), m, wl.diffusion_for(steps), _blur_op(dev), size=(W, H), **common)
    assert m.calls == 0


def _rect_window(dev, helper, size, hw, **kw):
    """One window of three frames through video.restore_video with per-frame model and operator (tests/test_gpu_faces_all.py)."""
    from flair_amd import video
    from flair_amd import workload as wl
    from tests.test_gpu_faces_all import _W
    from tests.test_gpu_unaligned_video import _blur_op
    H, W = hw
    degraded, _, tapes, qnoise = _tapes(3, H // 4, W // 4, H, W, 3, 1, 2, 5)
    out = video.restore_video("gaussian", degraded.to(dev), _W(degraded.to(dev)), wl.diffusion_for(2), _blur_op(dev), size=size,
                              tau=0, length=3, overlap=1, noise_fn=lambda wi, it, like: tapes[wi][it].to(dev),
                              q_noise_fn=lambda wi, like: qnoise[wi].to(dev), face_helper=helper, **kw)
    torch.cuda.synchronize()
    return out, (degraded, tapes, qnoise)


def test_window_loop_rect_unaligned(dev):
    """size=(64, 96) with a 32-pixel face helper: the faces are cropped to the face size and pasted back into the
    rectangular frames.  faces="largest" equals faces="all", max_faces=1 bit for bit, and meets the composition
    crop -> prior -> parse / blur -> inverse warp -> blend restated with oracle.facewarp inside the oracle loop, at the
    2e-3 of tests/test_gpu_unaligned_video.py (the parser is a fixed map: no arg-max ties)."""
    import numpy as np
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    from flair_amd.guided_diffusion.retinaface_utils import estimate_affine_partial
    from oracle import facewarp as fw
    from tests.test_gpu_faces_all import BIG, MID, SMALL, _TPL, StubDetector, StubParser, _aux, _face, _frame_model
    H, W, FS = 64, 96, 32
    wide = _face(70.0, 30.0, 30.0, 0.95)                                   # a face in the part a square frame lacks
    per_frame = [[SMALL, BIG], [wide], [BIG, MID, SMALL]]
    det = StubDetector(per_frame)
    parser = StubParser(3, FS, dev)
    helper = FaceRestoreHelper(face_size=FS, device=dev, face_det=det, face_parse=parser)
    largest, (degraded, tapes, qnoise) = _rect_window(dev, helper, (H, W), (H, W), aux_model=_aux, aligned=False)
    capped, _ = _rect_window(dev, helper, (H, W), (H, W), aux_model=_aux, aligned=False, faces="all", max_faces=1)
    assert det.calls == [False, True] and largest.shape == (3, 3, H, W)
    assert torch.equal(largest, capped)
    plain, _ = _rect_window(dev, helper, (H, W), (H, W), aux_model=_aux, aligned=True)
    assert (plain - largest).abs().max().item() > 1e-2                     # the crops' prior is not the whole-frame prior
    mats = [estimate_affine_partial(d[5:15].reshape(5, 2), _TPL * (FS / 512.0)) for d in (BIG, wide, BIG)]   # largest per frame

    def oracle_prior(x0, t, img):
        crops = fw.get_crop_face_from_affine_matrices(x0, mats, face_size=(FS, FS))
        crops_t = fw.get_crop_face_from_affine_matrices(img, mats, face_size=(FS, FS))
        faces = _aux(crops, t, crops_t)
        f255 = (((faces.float() + 1.0) / 2.0).clamp(0, 1) * 255).permute(0, 2, 3, 1).contiguous().numpy()
        cmap = np.asarray(fw.MASK_COLORMAP, dtype=np.float64)
        v = x0.clone()
        for k in range(3):
            mask = fw.gaussian_blur(fw.gaussian_blur(cmap[parser.maps[k].numpy()], 101, 26), 101, 26)
            mask[:10, :] = 0
            mask[-10:, :] = 0
            mask[:, :10] = 0
            mask[:, -10:] = 0
            inv = fw.invert_affine(mats[k])
            f = torch.from_numpy(fw.warp_affine_cubic(f255[k], inv, (W, H)).astype(np.float32)).permute(2, 0, 1) / 255.0
            m = torch.from_numpy(fw.warp_affine_cubic(mask / 255.0, inv, (W, H)).astype(np.float32))[None]
            v[k] = fw.blend(v[k], ((f - 0.5) / 0.5).clamp(-1, 1), m)
        return v
    ref = _oracle_windows(degraded, [[0, 1, 2]], tapes, qnoise, H, W, 1, 2, 0, _frame_model, oracle_prior)
    for i in range(3):
        err = (largest[i].cpu() - ref[i]).abs().max().item()
        print(f"unaligned window loop {H}x{W}, frame {i}: max|err| = {err:.3e}")
        assert err <= 2e-3, (i, err)


def test_pair_mode_equals_int_mode_on_a_square(dev):
    """size=(64, 64) with a 64-pixel face helper: the pair mode (crop / paste_faces with face_frames = 0..T-1) gives the
    bits of the int mode (the reference's inverse_faces and blend), aligned or not."""
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    from tests.test_gpu_faces_all import BIG, MID, SMALL, StubDetector, StubParser, _aux
    S = 64
    helper = FaceRestoreHelper(face_size=S, device=dev, face_det=StubDetector([[SMALL, BIG], [MID], [BIG, MID, SMALL]]),
                               face_parse=StubParser(6, S, dev))
    for kw in (dict(aligned=False), dict(aligned=True)):
        a, _ = _rect_window(dev, helper, S, (S, S), aux_model=_aux, **kw)
        b, _ = _rect_window(dev, helper, (S, S), (S, S), aux_model=_aux, **kw)
        assert torch.equal(a, b), kw
