"""BiSeNet face parser on the GPU: the three entries of parse.hip against torch closed forms (dense and on strided channel
views with guarded neighbours), the network, its parse map, FaceRestoreHelper.inverse_faces, face_weight and two
unaligned sampler steps against the reference's own output (tests/golden/g15_bisenet.npz) and the CPU restatement
(tests/bisenet_cpu.py), and ParseNet's path bit for bit against the launches it issued before the parser protocol."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bisenet_cpu as bc
from tests.test_gpu_strides import close, run_both
from tests.util import IN_FILL, assert_untouched, from_clip, guarded, rb

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "g15_bisenet.npz")
BF, FP = torch.bfloat16, torch.float32
SUB = {"small": (1, 1, 1), "big": (2, 4, 2)}
HEADS = ("conv_out", "conv_out16", "conv_out32")
OUTS = ("out", "out16", "out32", "feat", "feat16", "feat32")
# f32 HIP network against the fixture, relative to max|ref|, measured on one MI355X: 1/8-resolution logits of the three
# heads 4.8e-7 / 7.4e-7 / 7.7e-7 (136 x 168) and 1.31e-6 / 1.21e-6 / 1.43e-6 (512 x 512); full-size logits and return_feat
# maps at the sampled pixels 3.7e-7 .. 7.5e-7 and 8.7e-7 .. 1.45e-6.  The f32 CPU restatement against the fixture on the
# fixture's host: 0 (the same ATen calls in the same order, tests/test_bisenet_cpu.py).  Bound: 8 x the larger of the two,
# inside the 1e-6 .. 3e-4 the other f32 convolution stacks here keep.
NET_BOUND = 1.2e-5


def _ops():
    from flair_amd import ops
    return ops


def _net(dev=None, **kw):
    from flair_amd.guided_diffusion.bisenet import BiSeNet
    g = np.load(GOLD)
    net = BiSeNet(num_class=19).eval()
    sd = bc.seeded_state_dict(net, head=g["head"], **kw)
    net.load_state_dict(sd)
    return (net.to(dev) if dev is not None else net), sd, g


def _g(dtype):
    return 16 // torch.tensor([], dtype=dtype).element_size()


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("dtype", [FP, BF])
@pytest.mark.parametrize("shape", [(2, 16, 16, 512), (2, 5, 6, 128), (3, 9, 11, 128), (2, 64, 64, 256), (1, 7, 3, 40)])
def test_global_avgpool(dev, dtype, shape):
    ops = _ops()
    T, H, W, C = shape
    gv = _g(dtype)
    gen = torch.Generator().manual_seed(C + H)
    x = rb(torch.randn(T, H, W, C, generator=gen) + 0.3, dtype)
    out = run_both(dev, {"x": (x, dtype, 2 * gv, C + 3 * gv)}, {"y": ((T, 1, 1, C), FP, 4, C + 8)},
                   lambda x, y: ops.global_avgpool(x, out=y[:, 0, 0, :]), f"avgpool {shape}")
    ref = x.double().mean((1, 2))
    err = (out["y"][:, 0, 0, :] - ref).abs().max().item()
    assert err <= 2e-6 * max(1.0, ref.abs().max().item()), err           # f32 sums of <= 4096 terms, exact inputs


GATE_USES = {"arm32": dict(logit=True, bias=True), "arm16": dict(logit=True, add=True), "ffm": dict(logit=True, add_x=True),
             "plain": dict(logit=False, bias=True, add=True, add_x=True)}


@pytest.mark.parametrize("dtype", [FP, BF])
@pytest.mark.parametrize("use", list(GATE_USES))
@pytest.mark.parametrize("shape", [(2, 9, 11, 128), (2, 16, 16, 256), (1, 5, 3, 40)])
def test_channel_gate(dev, dtype, use, shape):
    ops = _ops()
    kw = GATE_USES[use]
    T, H, W, C = shape
    gv = _g(dtype)
    gen = torch.Generator().manual_seed(C + len(use))
    x = rb(torch.randn(T, H, W, C, generator=gen), dtype)
    a = rb(torch.randn(T, H, W, C, generator=gen), dtype)
    gate = torch.randn(T, C, generator=gen) * 2
    bias = torch.randn(T, C, generator=gen)
    gd, bd = gate.to(dev), bias.to(dev)
    ins = {"x": (x, dtype, gv, C + 2 * gv)}
    if kw.get("add"):
        ins["a"] = (a, dtype, 2 * gv, C + 2 * gv)

    def call(x, y, a=None):
        ops.channel_gate(x, gd, logit=kw["logit"], add_x=kw.get("add_x", False), bias=bd if kw.get("bias") else None, add=a, out=y)
    out = run_both(dev, ins, {"y": ((T, H, W, C), dtype, gv, C + 3 * gv)}, call, f"gate {use} {shape}")
    g64 = (torch.sigmoid(gate.double()) if kw["logit"] else gate.double()).view(T, 1, 1, C)
    ref = x.double() * g64
    if kw.get("add_x"):
        ref = ref + x.double()
    if kw.get("bias"):
        ref = ref + bias.double().view(T, 1, 1, C)
    if kw.get("add"):
        ref = ref + a.double()
    close(out["y"], ref, dtype, f"gate {use}")
    # in place, as the model calls it
    xd = x.to(dev, dtype).contiguous()
    ops.channel_gate(xd, gd, logit=kw["logit"], add_x=kw.get("add_x", False), bias=bd if kw.get("bias") else None,
                     add=a.to(dev, dtype) if kw.get("add") else None, out=xd)
    close(xd.double().cpu(), ref, dtype, f"gate {use} in place")


def _cpu_argmax(logits_nhwc, n, size):
    """F.interpolate(..., align_corners=True).argmax(1) on the CPU, and the top-2 margin of the enlarged logits."""
    big = F.interpolate(logits_nhwc[..., :n].permute(0, 3, 1, 2).float(), size, mode="bilinear", align_corners=True)
    top2 = big.topk(2, dim=1)[0] if n > 1 else torch.stack([big[:, 0], big[:, 0] - 1], 1)
    return big.argmax(1), top2[:, 0] - top2[:, 1], big.abs().max().item()


UA_CASES = [  # (T, h, w, N, ld, coff, H, W)
    (2, 17, 21, 19, 20, 0, 136, 168),         # the conv output of the f32 model: 19 classes padded to 20, 16-byte loads
    (2, 17, 21, 19, 28, 4, 136, 168),         # a channel slice at a 16-byte offset
    (2, 17, 21, 19, 23, 1, 136, 168),         # odd offset and stride: element loads
    (1, 64, 64, 19, 24, 0, 512, 512),
    (2, 9, 11, 19, 20, 0, 9, 11),             # H == h: the plain arg-max
    (1, 13, 7, 5, 8, 0, 40, 51),
    (1, 6, 5, 32, 32, 0, 31, 17),
    (1, 4, 4, 1, 4, 0, 9, 9),
]


@pytest.mark.parametrize("dtype", [FP, BF])
@pytest.mark.parametrize("case", UA_CASES, ids=lambda c: "x".join(map(str, c)))
def test_upsample_argmax(dev, dtype, case):
    ops = _ops()
    T, h, w, N, ld, coff, H, W = case
    gen = torch.Generator().manual_seed(h * w + N)
    logits = rb(torch.randn(T, h, w, N, generator=gen), dtype)
    table = torch.randn(N, 3, generator=gen)
    ref, margin, scale = _cpu_argmax(logits, N, (H, W))
    dense = torch.zeros(T, h, w, max(ld - coff, N), dtype=dtype)
    dense[..., :N] = logits
    idx_d, y_d = ops.upsample_argmax(dense.to(dev), N, (H, W), table.to(dev))
    buf, view = guarded(T, h, w, N, dtype, dev, coff=coff, ld=ld, fill=IN_FILL)
    view.copy_(logits.to(dev, dtype))
    before = buf.clone()
    idx_s, y_s = ops.upsample_argmax(view, N, (H, W), table.to(dev))
    torch.cuda.synchronize()
    assert_untouched(buf, before, None, "upsample_argmax input")
    assert idx_d.shape == (T, H, W) and idx_d.dtype == torch.int32
    assert torch.equal(idx_d, idx_s) and torch.equal(y_d, y_s)            # a stride must not change the result
    got = idx_d.cpu().long()
    assert torch.equal(y_d.cpu(), table[got])
    if (H, W) == (h, w):
        assert torch.equal(got, logits[..., :N].argmax(3))                # exact
        return
    clear = margin > 4e-6 * scale                                         # a few ulp of the blend: FMA contraction may differ
    assert clear.float().mean().item() > 0.995
    assert torch.equal(got[clear], ref[clear])


def test_upsample_argmax_ties_go_to_the_first_index(dev):
    ops = _ops()
    gen = torch.Generator().manual_seed(3)
    logits = torch.randn(2, 8, 9, 20, generator=gen)
    logits[..., 11] = logits[..., 4] = logits[..., :19].max(3)[0] + 1.0   # classes 4 and 11 tie for the maximum everywhere
    logits[..., 19] = 100.0                                               # the pad channel must not take part
    for size in ((8, 9), (64, 72), (61, 70)):
        ref = F.interpolate(logits[..., :19].permute(0, 3, 1, 2), size, mode="bilinear", align_corners=True).argmax(1)
        assert (ref == 4).all()
        got = ops.upsample_argmax(logits.to(dev), 19, size)[0]
        assert (got == 4).all(), size


def test_upsample_argmax_on_the_fixture_logits(dev):
    """The 136 x 168 case stores its 1/8-resolution logits in full: the fused kernel on the reference's logits gives the
    reference's map wherever the stored margin is clear of the blend's rounding."""
    ops = _ops()
    g = np.load(GOLD)
    low = torch.from_numpy(g["small_low_conv_out"]).permute(0, 2, 3, 1).contiguous()
    x = torch.zeros(*low.shape[:3], 20)
    x[..., :19] = low
    got = ops.upsample_argmax(x.to(dev), 19, bc.SIZES["small"])[0].cpu()
    ref = torch.from_numpy(g["small_argmax"]).int()
    clear = torch.from_numpy(g["small_margin_q"]).float() > 160 + 4 * np.log2(4e-6)
    assert clear.float().mean().item() > 0.995
    assert torch.equal(got[clear], ref[clear])


# ------------------------------------------------------------------------------------------------ 2. / 3. the network
def _low_logits(net, x):
    clip = net._to_clip(x)
    f8, cp8, cp16 = net.cp.run(clip)
    return [net.conv_out.run(net.ffm.run(f8, cp8)), net.conv_out16.run(cp8), net.conv_out32.run(cp16)]


@pytest.mark.parametrize("case", ["small", "big"])
def test_network_matches_reference_fixture(dev, case):
    net, _, g = _net(dev)
    x = bc.bisenet_input(g[f"{case}_u8"], case).to(dev)
    worst = 0.0
    for (low, _), name, s in zip(_low_logits(net, x), HEADS, SUB[case]):
        ref = torch.from_numpy(g[f"{case}_low_{name}"])
        err = (from_clip(low, 19)[:, :, ::s, ::s] - ref).abs().max().item() / ref.abs().max().item()
        print(f"bisenet {case} 1/8 logits {name}: {err:.2e} of max|ref|")
        worst = max(worst, err)
    outs = net(x, return_feat=True)
    assert len(outs) == 6 and all(tuple(o.shape[2:]) == bc.SIZES[case] for o in outs)
    pix = torch.from_numpy(g[f"{case}_pix"]).long()
    for t, name in zip(outs, OUTS):
        ref = torch.from_numpy(g[f"{case}_pix_{name}"])
        assert t.shape[1] == ref.shape[1]
        err = (bc.gather_pixels(t.cpu(), pix) - ref).abs().max().item() / ref.abs().max().item()
        print(f"bisenet {case} full-size {name} at {pix.shape[1]} pixels: {err:.2e} of max|ref|")
        worst = max(worst, err)
    three = net(x)
    assert len(three) == 3 and torch.equal(three[0], outs[0])
    assert worst <= NET_BOUND, worst


@pytest.mark.parametrize("case", ["small", "big"])
def test_parse_map_matches_reference_fixture(dev, case):
    """parse_indices (the fused tail) equals the reference's arg-max wherever its top-2 margin exceeds 4 x the logit
    error measured here; at most 10 % of the pixels may be left out that way."""
    net, _, g = _net(dev)
    x = bc.bisenet_input(g[f"{case}_u8"], case).to(dev)
    ref_low = torch.from_numpy(g[f"{case}_low_conv_out"])
    s = SUB[case][0]
    err = (from_clip(net._main_logits(x), 19)[:, :, ::s, ::s] - ref_low).abs().max().item()
    idx = net.parse_indices(x)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (2, *bc.SIZES[case])
    margin = float(g[f"{case}_logit_max"]) * torch.exp2((torch.from_numpy(g[f"{case}_margin_q"]).float() - 160) / 4)
    clear = margin > 4 * err
    excluded = 1 - clear.float().mean().item()
    print(f"bisenet {case} parse map: logit error {err:.2e}, excluded share {excluded:.4f}")
    assert excluded <= 0.10, excluded
    ref = torch.from_numpy(g[f"{case}_argmax"]).int()
    assert torch.equal(idx.cpu()[clear], ref[clear])
    assert (idx.cpu() == ref).float().mean().item() > 0.99


def test_bf16_runs_and_reports_agreement(dev):
    """convert_to_bf16(): compared by agreement of the parse with the f32 run; reported, not gated."""
    net, _, g = _net(dev)
    x = bc.bisenet_input(g["big_u8"], "big").to(dev)
    f32 = net.parse_indices(x)
    b16 = net.convert_to_bf16().parse_indices(x)
    assert b16.shape == f32.shape and b16.dtype == torch.int32
    print(f"bisenet bf16 parse map equals the f32 run on {(b16 == f32).float().mean().item():.4f} of the pixels")
    assert torch.equal(net.convert_to_fp32().parse_indices(x), f32)


# ------------------------------------------------------------------------------------------------ 4. / 5. / 6. the consumers
def test_inverse_faces_with_bisenet_vs_oracle(dev):
    """inverse_faces on the 512 x 512 fixture frames against oracle/facewarp.py driven by the reference's parse map; where
    the map's margin is not clear of the logit error (ties), the oracle is given the HIP index, so the comparison of the
    masks stays at the helper's own precision (test_face_warp.py's bounds).  The clear pixels are checked to be equal."""
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    from oracle import facewarp as fw
    from tests.test_face_warp import _matrices
    net, _, g = _net(dev)
    x = bc.bisenet_input(g["big_u8"], "big")
    mats = _matrices(2, 512)
    helper = FaceRestoreHelper(face_size=512, device=dev, face_parse=net)
    inv_faces, inv_masks = helper.inverse_faces(x.to(dev), mats)
    idx = net.parse_indices(x.to(dev)).cpu()
    ref_idx = torch.from_numpy(g["big_argmax"]).int()
    margin = float(g["big_logit_max"]) * torch.exp2((torch.from_numpy(g["big_margin_q"]).float() - 160) / 4)
    clear = margin > 4 * NET_BOUND * float(g["big_logit_max"])
    assert clear.float().mean().item() >= 0.90
    assert torch.equal(idx[clear], ref_idx[clear])
    parse = torch.where(clear, ref_idx, idx)
    ref_faces, ref_masks = fw.inverse_faces(x, mats, parse.numpy())
    assert 0.02 < ref_masks.mean().item() < 0.98                          # a real mask, not a constant
    assert (inv_masks.cpu() - ref_masks).abs().max().item() <= 1e-6
    assert (inv_faces.cpu() - ref_faces).abs().max().item() <= 2e-6
    # mask_colormap: the argument reaches the paste mask
    only0 = FaceRestoreHelper(face_size=512, device=dev, face_parse=net, mask_colormap=[0] * 19)
    assert only0.inverse_faces(x.to(dev), mats)[1].abs().max().item() == 0.0


@pytest.mark.parametrize("case", ["small", "big"])
def test_face_weight_with_rows_swapped(dev, case):
    """vsrpp_weights of the bicubic tasks (video_sample.py:427-444).  Class 0 never wins with the fixture's head, so rows
    0 and 2 of it are exchanged: that permutes the logits exactly, and the reference's map with labels 0 and 2 exchanged
    is the reference for the swapped network."""
    from flair_amd import workload as wl
    net, _, g = _net(dev, swap=(0, 2))
    x = bc.bisenet_input(g[f"{case}_u8"], case)
    am = torch.from_numpy(g[f"{case}_argmax"]).long()
    swapped = torch.where(am == 0, 2, torch.where(am == 2, 0, am))
    mask = (swapped == 0).float().unsqueeze(1)
    share = mask.mean().item()
    assert 0.02 < share < 0.98, share
    ref = mask * 0.93 + (1 - mask) * 1.0
    got = net.face_weight(x.to(dev), 0.93).cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32
    margin = float(g[f"{case}_logit_max"]) * torch.exp2((torch.from_numpy(g[f"{case}_margin_q"]).float() - 160) / 4)
    clear = (margin > 4 * NET_BOUND * float(g[f"{case}_logit_max"])).unsqueeze(1)
    assert clear.float().mean().item() >= 0.90
    assert torch.equal(got[clear], ref[clear])
    assert set(got.unique().tolist()) <= {1.0, float(np.float32(0.93))}
    if case == "big":
        fn = wl.parsenet_weights_fn(net, "x8_bicubic")                    # accepts either parser
        assert torch.equal(fn(x[None].to(dev)).cpu(), got[None])


def test_unaligned_sampler_steps_with_bisenet_vs_oracle(dev):
    """Two sampler steps with aligned=False and face_parse=BiSeNet against the oracle loop on oracle/facewarp.py + the CPU
    restatement (tests/test_face_warp.py::test_unaligned_sampler_steps_vs_oracle with the other parser; same bound: a
    parse flipped on a near-tie is spread by the two 101-tap blurs to < 1e-4 of mask)."""
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    from oracle import diffusion as odiff
    from oracle import facewarp as fw
    from tests.test_face_warp import _matrices
    from tests.test_gpu_sampler import toy_model
    T, S, STEPS = 2, 512, 10
    net, sd, _ = _net(dev)
    mats = _matrices(T, S)[:T]
    g = torch.Generator().manual_seed(11)
    x_T = torch.randn(T, 3, S, S, generator=g)
    tape = [torch.randn(T, 3, S, S, generator=g) for _ in range(2)]
    aux = lambda face, t, xt: 0.85 * face + 0.05 * xt         # noqa: E731  (stand-in prior on the CROPS)

    class OracleHelper:
        def get_crop_face_from_affine_matrices(self, imgs, ms):
            return fw.get_crop_face_from_affine_matrices(imgs, ms)

        def inverse_faces(self, restored, ms):
            return fw.inverse_faces(restored, ms, bc.parse_map(sd, restored.float())[0].numpy())
    tab = odiff.Spaced(odiff.spaced_steps(1000, str(STEPS)), odiff.named_betas("face_blur", 1000))
    ref_trace, calls = [], []

    class Stop(Exception):
        pass

    def omodel(x, t, **kw):
        if len(calls) == 2:
            raise Stop()
        calls.append(1)
        return toy_model(x, t, **kw)
    try:
        odiff.sample_loop(tab, omodel, x_T, model_kwargs=dict(num_frames=T), aux_model=aux, w=0.5, tau=2, rho=0.25,
                          step_noise=tape + tape, trace=ref_trace, aligned=False, face_restore_helper=OracleHelper(),
                          affine_matrices=mats)
    except Stop:
        pass
    assert len(ref_trace) == 2

    class M:
        def parameters(self):
            return iter([x_T.to(dev)])

        def __call__(self, x, t, **kw):
            return toy_model(x, t, **kw)
    diffusion = wl.diffusion_for(STEPS)
    gen = diffusion.p_sample_loop_progressive(
        M(), x_T.shape, noise=x_T.to(dev), model_kwargs=dict(num_frames=T), device=dev, aux_model=aux, w=0.5, tau=2,
        aligned=False, rho=0.25, face_restore_helper=FaceRestoreHelper(device=dev, face_parse=net), affine_matrices=mats,
        noise_fn=lambda it, like: tape[it].to(dev))
    for (ti, x0r, sr) in ref_trace:
        out = next(gen)
        assert int(out["t"][0]) == ti
        assert (out["pred_xstart"].cpu() - x0r).abs().max().item() <= 2e-3
        assert (out["sample"].cpu() - sr).abs().max().item() <= 2e-3 * max(1.0, sr.abs().max().item())


# ------------------------------------------------------------------------------------------------ 7. ParseNet unchanged
def test_parsenet_path_is_bit_identical_to_its_launch_sequence(dev):
    """parse_indices / inverse_faces with ParseNet against the launches inverse_faces issued before the parser protocol,
    restated with ops calls."""
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    from flair_amd.guided_diffusion.parsenet import ParseNet
    from tests.golden.weights import name_seeded_weights
    from tests.test_face_warp import _frames, _matrices
    ops = _ops()
    net = name_seeded_weights(ParseNet(in_size=512, out_size=512, parsing_ch=19)).eval().to(dev)
    B, S = 2, 512
    x = _frames(B, S, 5).to(dev).float().contiguous()
    mats = _matrices(B, S)
    helper = FaceRestoreHelper(device=dev, face_parse=net)
    lut, kern = helper._consts(x.device)
    logits = net.out_mask_conv.run(net._features(x))
    _, idx = ops.argmax_codebook(logits, net.parsing_ch, torch.zeros((net.parsing_ch, 1), dtype=torch.float32, device=x.device))
    mask = ops.face_mask_blur(idx, B, S, S, lut, kern, repeats=2, edge=10, div=255.0)
    minv = helper._minv(mats, x.device, twice=True)
    want_faces = ops.warp_affine_cubic(x, minv, (S, S), pre=True, post=True)
    want_masks = ops.warp_affine_cubic(mask, minv, (S, S))
    got_idx = net.parse_indices(x)
    assert got_idx.dtype == torch.int32 and tuple(got_idx.shape) == (B, S, S)
    assert torch.equal(got_idx.reshape(-1), idx)
    got_faces, got_masks = helper.inverse_faces(x, mats)
    assert torch.equal(got_faces, want_faces) and torch.equal(got_masks, want_masks)
    assert len(idx.unique()) > 1


def test_pipeline_builds_either_parser(dev, tmp_path):
    """build_pipeline from a weights directory: ParseNet without the argument, BiSeNet with parser='bisenet'."""
    import scipy.io
    from flair_amd import pipeline as pl
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion.bisenet import BiSeNet
    from flair_amd.guided_diffusion.parsenet import ParseNet
    from flair_amd.guided_diffusion.retinaface import RetinaFace
    from flair_amd.guided_diffusion.unet_new import UNetModel
    S = 64
    kw = dict(num_res_blocks=1, attention_resolutions=[2, 4], channel_mult=[0.5, 1, 4], use_checkpoint=False)
    torch.manual_seed(0)
    cfg = pl.model_config("gaussian", S)
    cfg.update({k: tuple(v) if isinstance(v, list) else v for k, v in kw.items()})
    torch.save(UNetModel(**cfg).state_dict(), tmp_path / "flair_gaussian.pt")
    torch.save(RetinaFace("mobile0.25", device="cpu").state_dict(), tmp_path / "detection_mobilenet0.25_Final.pth")
    torch.save(ParseNet(in_size=512, out_size=512, parsing_ch=19).state_dict(), tmp_path / "parsing_parsenet.pth")
    bsd = BiSeNet(num_class=19).state_dict()
    torch.save(bsd, tmp_path / "parsing_bisenet.pth")
    kernels = np.empty((1, 12), dtype=object)
    for i in range(12):
        kernels[0, i] = wl.synthetic_blur_kernel(25, 1.0 + 0.25 * i)
    scipy.io.savemat(tmp_path / "kernels_12.mat", {"kernels": kernels})
    common = dict(device=dev, size=S, steps=2, kernels_path=str(tmp_path / "kernels_12.mat"), prior=False,
                  det_model="retinaface_mobile0.25", model_kwargs=kw, graph=False)
    p = pl.build_pipeline("gaussian", tmp_path, **common)
    assert isinstance(p.face_helper.face_parse, ParseNet)
    p = pl.build_pipeline("gaussian", tmp_path, parser="bisenet", **common)
    parser = p.face_helper.face_parse
    assert isinstance(parser, BiSeNet)
    assert all(torch.equal(v.cpu(), bsd[k]) for k, v in parser.state_dict().items())
    x = torch.rand(1, 3, 72, 56, generator=torch.Generator().manual_seed(1)).to(dev) * 2 - 1
    assert tuple(parser.parse_indices(x).shape) == (1, 72, 56)
