"""VQFR v2 prior on the MI355X: the two new kernel forms (flair_dwconv7_nhwc; flair_dcn_align with raw offsets,
raw_activated = 2) against PyTorch / the deformable-convolution oracle, the entries VQFR reuses at its shapes, the HIP
network against the reference's own output (tests/golden/g14_vqfr.npz) and the CPU restatement (tests/vqfr_cpu.py), the
sampler with the prior, and the command line with ``--prior vqfrv2`` on an unaligned window.

Code indices are an arg-max over 1024 logits per token: indices are compared where the fixture's top-2 margin is clear,
and the decoders are compared with the fixture's indices injected (``code_idx``)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import parity_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g14_vqfr.npz")


def _rel(a, b):
    return (a.float() - b.float()).abs().max().item() / max(b.float().abs().max().item(), 1e-12)


def _clip(t, dtype, extra, dev):
    """(F, C, H, W) -> an NHWC channel slice [extra, extra + C) of a wider (F, H, W, C + 2 extra) tensor on ``dev``."""
    F_, C, H, W = t.shape
    buf = torch.randn(F_, H, W, C + 2 * extra).to(dtype)
    buf[..., extra:extra + C] = t.permute(0, 2, 3, 1).to(dtype)
    return buf.to(dev)[..., extra:extra + C]


# ------------------------------------------------------------------------------------------- depthwise 7x7
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("F_,H,W,C", [(2, 13, 17, 64), (1, 9, 6, 512), (10, 16, 16, 512), (1, 64, 67, 128)])
def test_dwconv7_matches_conv2d(dev, dtype, F_, H, W, C):
    """Depthwise 7x7 (groups = C, padding 3, bias) on channel-slice views, into a channel slice of a wider output: against
    F.conv2d on the same (rounded) inputs in float64; the output's neighbouring channels untouched."""
    from flair_amd import ops
    g = torch.Generator().manual_seed(F_ * 1000 + H * W + C)
    x = torch.randn(F_, C, H, W, generator=g).to(dtype).double()
    w = torch.randn(C, 1, 7, 7, generator=g) / 7.0
    b = 0.1 * torch.randn(C, generator=g)
    ref = F.conv2d(x, w.double(), b.double(), padding=3, groups=C)
    vec = 8
    out = torch.full((F_, H, W, C + 2 * vec), 7.0, dtype=dtype, device=dev)
    y = ops.dwconv7(_clip(x, dtype, 8, dev), w.reshape(C, 49).t().contiguous().to(dev), b.to(dev),
                    out=out[..., vec:vec + C])
    torch.cuda.synchronize()
    got = y.cpu().permute(0, 3, 1, 2).double()
    tol = 2e-6 if dtype == torch.float32 else 8e-3
    assert _rel(got, ref) <= tol
    assert (out[..., :vec] == 7.0).all() and (out[..., vec + C:] == 7.0).all()


@pytest.mark.gpu
def test_dwconv7_refuses_bad_strides(dev):
    from flair_amd import ops
    from flair_amd._lib import FlairHipError
    w = torch.zeros(49, 64, device=dev)
    x = torch.zeros(1, 8, 8, 70, dtype=torch.bfloat16, device=dev)
    with pytest.raises(FlairHipError, match="x_ld"):
        ops.dwconv7(x[..., :64], w, None)                          # bf16 pixel stride 70: not 16-byte granular
    with pytest.raises(FlairHipError, match="aligned"):
        ops.dwconv7(torch.zeros(1, 8, 8, 72, dtype=torch.bfloat16, device=dev)[..., 4:68], w, None)
    with pytest.raises(FlairHipError, match="C = 60"):
        ops.dwconv7(torch.zeros(1, 8, 8, 60, dtype=torch.bfloat16, device=dev), torch.zeros(49, 60, device=dev), None)


# ------------------------------------------------------------------------------------------- deformable conv, raw offsets
def _dcn_case(dev, dtype, F_, H, W, C, G, kind, seed):
    from flair_amd import ops
    from oracle.thirdparty import deform_conv2d
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(F_, C, H, W, generator=g).to(dtype).double()
    wt = (torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5).to(dtype)
    b = 0.1 * torch.randn(C, generator=g)
    off = 2.5 * torch.randn(F_, 18 * G, H, W, generator=g)
    if kind == "integer":
        off = off.round()                                        # exactly integer: single-corner samples, frame edges
    elif kind == "large":
        off = off * 20.0                                         # tens of pixels: most samples outside the frame
    m = torch.randn(F_, 9 * G, H, W, generator=g)
    raw = torch.cat([off, m], dim=1).to(dtype)                   # the kernel reads the offsets in the activation dtype
    off, m = raw[:, :18 * G].double(), raw[:, 18 * G:].double()
    ref = deform_conv2d(x, off, wt.double(), b.double(), (1, 1), (1, 1), (1, 1), torch.sigmoid(m))
    cpad = (27 * G + 7) // 8 * 8
    rawp = torch.zeros(F_, H, W, cpad, dtype=dtype)
    rawp[..., :27 * G] = raw[:, ops.dcn_raw_permutation(G)].permute(0, 2, 3, 1)
    wpk = ops.pack_conv_weight(wt.float(), [(C, C)], dtype).to(dev)
    y = ops.dcn_pack(_clip(x, dtype, 32, dev), rawp.to(dev), wpk, b.to(dev), C, groups=G)
    torch.cuda.synchronize()
    return y.cpu().permute(0, 3, 1, 2).double(), ref


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("F_,H,W,C,G,kind", [
    (3, 33, 37, 64, 4, "random"),          # VQFR level 1 (odd size)
    (2, 16, 16, 512, 4, "random"),         # level 32: four cout slices of 128
    (2, 20, 24, 64, 8, "integer"),
    (2, 16, 16, 512, 8, "large"),
    (1, 128, 128, 128, 4, "random"),       # H*W >= 16384: the large-P tiles
    (2, 32, 32, 256, 4, "integer"),
])
def test_dcn_raw_offsets_match_oracle(dev, dtype, F_, H, W, C, G, kind):
    """flair_dcn_align, raw_activated = 2 (VQFR's DCNv2Pack): offsets as they are, sigmoid masks, x_main's two channel
    halves as the two inputs (channel-slice views), against torchvision.ops.deform_conv2d semantics in float64."""
    got, ref = _dcn_case(dev, dtype, F_, H, W, C, G, kind, seed=F_ * 7 + H + C + G)
    err = _rel(got, ref)
    parity_log(f"dcn raw offsets {dtype} F{F_} {H}x{W} c{C} G{G} {kind}: {err:.2e} rel-max")
    assert err <= (2e-5 if dtype == torch.float32 else 1.5e-2)


@pytest.mark.gpu
def test_dcn_raw_offsets_refusals(dev):
    """Flows with raw offsets, G = 4 in the other modes, a raw row that is not 16-byte granular: refused."""
    from flair_amd import ops
    from flair_amd._lib import FlairHipError
    x = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(64, 9, 64, dtype=torch.bfloat16, device=dev)
    raw = torch.zeros(1, 8, 8, 112, dtype=torch.bfloat16, device=dev)
    flow = torch.zeros(1, 8, 8, 2, device=dev)
    with pytest.raises(FlairHipError, match="no flows"):
        ops.dcn_align(x[..., :32], x[..., 32:], raw, flow, None, w, None, 64, groups=4, raw_activated=2)
    with pytest.raises(FlairHipError, match="G=4"):
        ops.dcn_align(x[..., :32], x[..., 32:], raw, None, None, w, None, 64, groups=4, raw_activated=1)
    with pytest.raises(FlairHipError, match="raw_ld"):
        ops.dcn_pack(x, torch.zeros(1, 8, 8, 108, dtype=torch.bfloat16, device=dev), w, None, 64, groups=4)


# ------------------------------------------------------------------------------------------- reused entries at VQFR's shapes
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reused_entries_at_vqfr_shapes(dev, dtype):
    """Bilinear (align_corners=False) inpfeat 512^2 -> 16^2 and offsets x2 (vector path), GroupNorm + SiLU over a two-part
    input, and the segment convolution of ResnetBlock(2c -> c)'s shortcut, against PyTorch."""
    from flair_amd import ops
    g = torch.Generator().manual_seed(5)
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    inp = torch.randn(2, 32, 512, 512, generator=g).to(dtype).float()
    for size in (16, 256):
        ref = F.interpolate(inp, size=(size, size), mode="bilinear", align_corners=False)
        got = ops.resize(_clip(inp, dtype, 0, dev).contiguous(), (size, size), ops.RESIZE_BILINEAR).cpu().permute(0, 3, 1, 2)
        assert _rel(got, ref) <= tol, size
    off = torch.randn(2, 128, 64, 64, generator=g).to(dtype).float()
    ref = F.interpolate(off, scale_factor=2, mode="bilinear", align_corners=False)
    got = ops.resize(_clip(off, dtype, 0, dev).contiguous(), (128, 128), ops.RESIZE_BILINEAR).cpu().permute(0, 3, 1, 2)
    assert _rel(got, ref) <= tol
    a, b = (torch.randn(2, 64, 24, 24, generator=g).to(dtype).float() for _ in range(2))
    gam, bet = 1 + 0.1 * torch.randn(128, generator=g), 0.1 * torch.randn(128, generator=g)
    ref = F.silu(F.group_norm(torch.cat([a, b], 1), 32, gam, bet, 1e-6))
    got = ops.group_norm(_clip(a, dtype, 0, dev).contiguous(), gam.to(dev), bet.to(dev), x1=_clip(b, dtype, 0, dev).contiguous(),
                         eps=1e-6, act=ops.ACT_SILU, frames_per_stat=1)
    assert _rel(got.cpu().permute(0, 3, 1, 2), ref) <= (1e-4 if dtype == torch.float32 else 2e-2)
    w = torch.randn(64, 128, 1, 1, generator=g) / 128 ** 0.5
    ref = F.conv2d(torch.cat([a, b], 1), w.to(dtype).float())
    got = ops.conv([_clip(a, dtype, 0, dev).contiguous(), _clip(b, dtype, 0, dev).contiguous()],
                   ops.pack_conv_weight(w, [(64, 64), (64, 64)], dtype).to(dev), None, 64, (1, 1, 1))
    assert _rel(got.cpu().permute(0, 3, 1, 2), ref) <= (1e-4 if dtype == torch.float32 else 2e-2)


# ------------------------------------------------------------------------------------------- the network
@pytest.fixture(scope="module")
def hip_model(dev):
    from flair_amd.guided_diffusion.vqfr import VQFRv2
    from tests import vqfr_cpu as ov
    net = VQFRv2(**ov.RELEASE)
    sd = ov.seeded_state_dict(net)
    return net.to(dev).eval(), sd


@pytest.mark.gpu
def test_hip_vqfr_matches_reference_fixture_f32(dev, hip_model):
    """f32 against g14: code indices where the logit margin is clear, the level-1 TextureWarpingModule (G = 4, c = 64 at
    512^2: output and offset at the stored pixels), main_dec with the fixture's codes."""
    from tests import vqfr_cpu as ov
    g = np.load(GOLD)
    model, _ = hip_model
    x = ov.vqfr_input(torch.from_numpy(g["x_u8"])).to(dev)
    trace = {}
    r = model(x, trace=trace)
    idx = r["quant_index"].cpu()
    clear = torch.from_numpy(g["margin"]) > 1e-3
    assert torch.equal(idx[clear], torch.from_numpy(g["idx"]).long()[clear])
    agree = (idx == torch.from_numpy(g["idx"]).long()).float().mean().item()
    warp, offset = (t.float().cpu().permute(0, 3, 1, 2) for t in trace["twm.Level_1"])
    tpix = torch.from_numpy(g["twm1_pix"])
    ref_idx = torch.from_numpy(g["idx"]).long()
    if agree < 1.0:                                 # the warps depend on the codes: inject the fixture's
        trace = {}
        model(x, code_idx=ref_idx, trace=trace)
        warp, offset = (t.float().cpu().permute(0, 3, 1, 2) for t in trace["twm.Level_1"])
    e_w = _rel(ov.take(warp, tpix), torch.from_numpy(g["twm1_out"]))
    e_o = _rel(ov.take(offset, tpix), torch.from_numpy(g["twm1_offset"]))
    dec = model(x, code_idx=ref_idx)["main_dec"].cpu()
    e_d = _rel(ov.take(dec, torch.from_numpy(g["dec_pix"])), torch.from_numpy(g["dec_sub"]))
    parity_log(f"vqfr f32 vs g14: codes {agree:.3f}, twm1 out {e_w:.2e} offset {e_o:.2e}, main_dec {e_d:.2e} rel-max")
    assert e_w <= 1e-3 and e_o <= 1e-3 and e_d <= 1e-3
    assert r["quant_logit"].shape == (2, 256, 1024) and r["enc_feat"].shape == (2, 256, 16, 16)
    assert "texture_dec" not in r


@pytest.mark.gpu
def test_hip_vqfr_batch_fidelity_and_bf16(dev, hip_model):
    """A face's result does not depend on its batch neighbour; fidelity_ratio scales the main branch as the CPU
    restatement does; bf16 with the fixture's codes within a stated bound."""
    from tests import vqfr_cpu as ov
    g = np.load(GOLD)
    model, sd = hip_model
    x = ov.vqfr_input(torch.from_numpy(g["x_u8"])).to(dev)
    ref_idx = torch.from_numpy(g["idx"]).long()
    both = model(x, code_idx=ref_idx)["main_dec"].cpu()
    other = x.clone()
    other[1] = -x[1]
    swapped = model(other, code_idx=ref_idx)["main_dec"].cpu()
    solo = model(x[:1], code_idx=ref_idx[:1])["main_dec"].cpu()
    assert (solo[0] - both[0]).abs().max().item() <= 1e-5 * both.abs().max().item()
    assert torch.equal(swapped[0], both[0])
    half = model(x[:1], 0.5, code_idx=ref_idx[:1])["main_dec"].cpu()
    ref_half = ov.vqfr_forward(sd, x[:1].cpu(), ov.RELEASE, fidelity_ratio=0.5, code_idx=ref_idx[:1])["main_dec"]
    assert _rel(half, ref_half) <= 1e-3
    try:
        model.convert_to_bf16()
        dec16 = model(x, code_idx=ref_idx)["main_dec"].cpu()
        idx16 = model(x)["quant_index"].cpu()
        torch.cuda.synchronize()
        assert torch.isfinite(dec16).all()
        err = _rel(dec16, both)
        agree = (idx16 == ref_idx).float().mean().item()
        parity_log(f"vqfr bf16 vs f32: code agreement {agree:.3f}, main_dec (fixture codes) {err:.2e} rel-max")
        assert err <= 8e-2 and agree > 0.5
    finally:
        model.dtype = torch.float32
        model._packed_key = None


@pytest.mark.gpu
def test_hip_vqfr_nearest_mode(dev):
    """The small "Nearest" network of g14 (G = 8, L2VectorQuantizer on flair_vq_nearest_nhwc)."""
    from flair_amd.guided_diffusion.vqfr import VQFRv2
    from tests import vqfr_cpu as ov
    g = np.load(GOLD)
    net = VQFRv2(**ov.SMALL_NEAREST)
    ov.vqfr_seeded_weights(net)
    net = net.to(dev).eval()
    x = ov.vqfr_input(torch.from_numpy(g["n_x_u8"])).to(dev)
    r = net(x)
    clear = torch.from_numpy(g["n_margin"]) > 1e-3
    assert torch.equal(r["quant_index"].cpu()[clear], torch.from_numpy(g["n_idx"]).long()[clear])
    dec = net(x, code_idx=torch.from_numpy(g["n_idx"]))["main_dec"].cpu()
    assert _rel(ov.take(dec, torch.from_numpy(g["n_dec_pix"])), torch.from_numpy(g["n_dec_sub"])) <= 1e-3
    assert "quant_logit" not in r


@pytest.mark.gpu
def test_sampler_steps_with_hip_vqfr(dev, hip_model):
    """gaussian_diffusion.py:471-496 with aligned=True, two steps on one 512x512 face (toy eps-model): the HIP sampler with
    the HIP prior (through workload.vqfr_aux) against the oracle loop with the CPU restatement as prior; the
    restatement's code indices are injected so that a near-tie cannot fork the trajectories."""
    from flair_amd import workload as wl
    from oracle import diffusion as odiff
    from tests import vqfr_cpu as ov
    from tests.golden.make_golden import codeformer_input, toy_model
    model, sd = hip_model
    x_T = codeformer_input(batch=1, seed=34) * 0.8
    g = torch.Generator().manual_seed(6)
    tape = [torch.randn(1, 3, 512, 512, generator=g) for _ in range(2)]
    tab = odiff.Spaced(odiff.spaced_steps(1000, "50"), odiff.named_betas("face_blur", 1000))
    codes = []

    def ora_aux(x0, t, xt):
        r = ov.vqfr_forward(sd, x0, ov.RELEASE)
        codes.append(r["idx"])
        return r["main_dec"]

    ref_trace = []
    ref = odiff.sample_loop(tab, toy_model, x_T, model_kwargs=dict(num_frames=1), aux_model=ora_aux, w=0.5, tau=0,
                            rho=0.35, t_start=1, step_noise=tape, trace=ref_trace)
    calls = iter(codes)

    class M:
        def parameters(self):
            return iter([x_T.to(dev)])

        def __call__(self, x, t, **kw):
            return toy_model(x, t, **kw)

    class Forced:                                   # vqfr_aux around the network with the oracle's codes injected
        def __call__(self, x0, fidelity_ratio):
            return model(x0, fidelity_ratio, code_idx=next(calls))

    got_trace = []
    got = wl.diffusion_for(50).p_sample_loop(
        M(), x_T.shape, noise=x_T.to(dev), model_kwargs=dict(num_frames=1), device=dev, restore_fn=None,
        aux_model=wl.vqfr_aux(Forced()),
        post_fn=lambda o: got_trace.append((int(o["t"][0]), o["pred_xstart"].cpu(), o["sample"].cpu())),
        w=0.5, tau=0, aligned=True, rho=0.35, noise_level=None, zeta=-1, prev_recon=None, t_start=1,
        noise_fn=lambda it, like: tape[it].to(dev))
    assert len(got_trace) == len(ref_trace) == 2
    for (ti, x0r, sr), (tg, x0g, sg) in zip(ref_trace, got_trace):
        assert ti == tg
        assert (x0r - x0g).abs().max().item() <= 5e-4, (ti, (x0r - x0g).abs().max().item())
        assert (sr - sg).abs().max().item() <= 1e-3 * max(1.0, sr.abs().max().item()), ti
    assert (ref - got.cpu()).abs().max().item() <= 1e-3


# ------------------------------------------------------------------------------------------- command line, unaligned
@pytest.mark.gpu
def test_cli_unaligned_vqfr_matches_in_process_pipeline(dev, tmp_path, hip_model):
    """python -m flair_amd restore ... --prior vqfrv2 (fresh process, time limit) on one unaligned 512 x 512 window
    (3 frames) with synthetic checkpoints, VQFR_v2.pth in BasicSR's params_ema form with the release configuration's
    shapes and no CodeFormer or RestoreFormer file == build_pipeline(..., prior="vqfrv2").restore_video_files(...) in this
    process, PNG for PNG."""
    import scipy.io
    from PIL import Image
    from flair_amd import pipeline as pl
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion.parsenet import ParseNet
    from flair_amd.guided_diffusion.unet_new import UNetModel
    from flair_amd.guided_diffusion.vqfr import VQFRv2
    from tests.test_gpu_restoreformer import _face_detector_state
    S, s, N = 512, 128, 3
    kw = dict(num_res_blocks=1, attention_resolutions=[16], channel_mult=[0.5, 1, 2, 4, 4], use_checkpoint=False)
    wdir = tmp_path / "weights"
    wdir.mkdir()
    torch.manual_seed(0)
    cfg = pl.model_config("gaussian", S)
    cfg.update({k: tuple(v) if isinstance(v, list) else v for k, v in kw.items()})
    m = UNetModel(**cfg)
    wl.randomize_zero_modules(m)
    torch.save(m.state_dict(), wdir / "flair_gaussian.pt")
    torch.save(_face_detector_state(), wdir / "detection_mobilenet0.25_Final.pth")
    torch.save(ParseNet(in_size=512, out_size=512, parsing_ch=19).state_dict(), wdir / "parsing_parsenet.pth")
    _, sd = hip_model
    torch.save({"params_ema": sd}, wdir / "VQFR_v2.pth")
    kernels = np.empty((1, 12), dtype=object)
    for i in range(12):
        kernels[0, i] = wl.synthetic_blur_kernel(25, 1.0 + 0.25 * i)
    scipy.io.savemat(tmp_path / "kernels_12.mat", {"kernels": kernels})
    frames = tmp_path / "frames"
    frames.mkdir()
    rng = np.random.default_rng(3)
    for i in range(N):
        Image.fromarray(rng.integers(0, 256, size=(s, s, 3), dtype=np.uint8), mode="RGB").save(frames / f"{i}.png")
    common = ["--prior", "vqfrv2", "--size", str(S), "--steps", "2", "--weights", str(wdir), "--kernels",
              str(tmp_path / "kernels_12.mat"), "--det-model", "retinaface_mobile0.25", "--model-kwargs", json.dumps(kw),
              "--seed", "12", "--tau", "0"]                  # tau 0: the prior runs on both steps
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, "-m", "flair_amd", "restore", "gaussian",
                        str(frames), str(tmp_path / "cli"), *common], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"restored 1 videos, {N} frames" in r.stdout
    p = pl.build_pipeline("gaussian", wdir, device=dev, size=S, steps=2, kernels_path=str(tmp_path / "kernels_12.mat"),
                          prior="vqfrv2", det_model="retinaface_mobile0.25", model_kwargs=kw)
    assert any(isinstance(c.cell_contents, VQFRv2) for c in p.aux_model.__closure__)
    calls, aux = [], p.aux_model

    def counted(face, t, xt):
        calls.append(face.shape)
        return aux(face, t, xt)
    p.aux_model = counted
    d = pl.MAIN_DEFAULTS
    n = p.restore_video_files(frames, tmp_path / "lib", aligned=False, t_start=d["t_start"], jpeg_qf=d["jpeg_qf"], w=d["w"],
                              tau=0, rho=d["rho"], noise_level=d["noise_level"], zeta=d["zeta"], seed=12)
    assert n == N
    assert calls == [(N, 3, S, S)] * 2                  # the prior restored the window's aligned crops on both steps
    assert sorted(os.listdir(tmp_path / "cli")) == sorted(os.listdir(tmp_path / "lib")) == [f"{i:04d}.png" for i in range(N)]
    for i in range(N):
        assert (tmp_path / "cli" / f"{i:04d}.png").read_bytes() == (tmp_path / "lib" / f"{i:04d}.png").read_bytes(), i
