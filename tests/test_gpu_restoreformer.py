"""RestoreFormer prior on the MI355X: the codebook-search entry (flair_vq_nearest_nhwc) against numpy, the HIP network
against the reference's own output (tests/golden/g13_restoreformer.npz) and the CPU restatement (tests/restoreformer_cpu.py),
the sampler with the prior, and the command line with ``--prior restoreformer`` on an unaligned window.

The code indices are an arg-min over 1024 distances per token: two correct f32 implementations can differ on near-ties, so
indices are compared where the fixture's top-2 margin exceeds the error bound, and the decoder is compared with the
fixture's indices injected (``code_idx``)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.golden.weights import name_seeded_weights
from tests.util import parity_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g13_restoreformer.npz")


# ------------------------------------------------------------------------------------------- the codebook search entry
def _np_nearest(z, e):
    """f32 distances |z|^2 + |e|^2 - 2 z.e in float64 (exact enough to rank), -> (idx, sorted top-2 margin)."""
    z64, e64 = z.astype(np.float64), e.astype(np.float64)
    d = (z64 ** 2).sum(1, keepdims=True) + (e64 ** 2).sum(1)[None] - 2 * z64 @ e64.T
    top2 = np.sort(d, axis=1)[:, :2]
    return d.argmin(1), top2[:, 1] - top2[:, 0], d


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,N,D,ld", [(2 * 256, 1024, 256, 256), (37, 300, 12, 20), (9, 5, 1024, 1032)])
def test_vq_nearest_random(dev, dtype, rows, N, D, ld):
    """Random codebooks, z a channel slice of a wider tensor: the nearest row wherever the float64 margin is clear of
    f32 rounding, otherwise a row within that rounding of the minimum; the gathered row in z's dtype."""
    from flair_amd import ops
    g = torch.Generator().manual_seed(rows * 7 + N + D)
    e = torch.randn(N, D, generator=g) / D ** 0.5
    buf = torch.randn(1, rows, 1, ld, generator=g).to(dtype)
    z = buf[..., ld - D:]
    codes, idx = ops.vq_nearest(z.to(dev), e.to(dev))
    torch.cuda.synchronize()
    zf = z.float().reshape(rows, D).numpy()
    want, margin, d = _np_nearest(zf, e.numpy())
    got = idx.cpu().numpy()
    tol = 1e-5 * (np.abs(d).max() + 1.0)
    clear = margin > tol
    assert clear.mean() > 0.9
    assert np.array_equal(got[clear], want[clear])
    assert (d[np.arange(rows), got] - d.min(1) <= tol).all()
    assert torch.equal(codes.cpu().reshape(rows, D), e[torch.from_numpy(got).long()].to(dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_vq_nearest_exact_ties_and_forced(dev, dtype):
    """Duplicated codebook rows and z equidistant from +e / -e: the first index wins (torch.min); ``forced_idx`` replaces
    the search, out-of-range indices clamped."""
    from flair_amd import ops
    g = torch.Generator().manual_seed(3)
    N, D, rows = 1024, 256, 64
    e = torch.randn(N, D, generator=g) / 16
    e[700] = e[5]                                  # rows 5 and 700 equal
    e[900] = e[300]
    z = torch.randn(1, 8, 8, D, generator=g)
    z[0, 0] = e[700].to(dtype).float()             # pixels 0-7: nearest rows 5 and 700 (equal) -> 5
    z[0, 1] = e[900].to(dtype).float()             # pixels 8-15: rows 300 and 900 -> 300
    z = z.to(dtype)
    codes, idx = ops.vq_nearest(z.to(dev), e.to(dev))
    torch.cuda.synchronize()
    got = idx.cpu()
    assert got[:8].tolist() == [5] * 8 and got[8:16].tolist() == [300] * 8
    zf = z.float().reshape(rows, D)
    d = zf.pow(2).sum(1, keepdim=True) + e.pow(2).sum(1) - 2 * zf @ e.t()
    _, margin, _ = _np_nearest(zf.numpy(), e.numpy())
    clear = torch.from_numpy(margin > 1e-3)
    assert torch.equal(got[clear], d.argmin(1)[clear].int())
    # z = 0 against rows e, -e, e (the same |e|^2, so the same distance bit for bit) behind a longer row: index 1
    e1 = torch.randn(1, D, generator=g)
    e3 = torch.cat([2 * e1, e1, -e1, e1])
    zero = torch.zeros(1, 2, 2, D, dtype=dtype)
    _, idx3 = ops.vq_nearest(zero.to(dev), e3.to(dev))
    assert idx3.cpu().tolist() == [1] * 4
    forced = torch.tensor([3, 1023, -5, 5000] * 16, dtype=torch.int32)
    codes_f, idx_f = ops.vq_nearest(z.to(dev), e.to(dev), forced_idx=forced.to(dev))
    torch.cuda.synchronize()
    want = forced.clamp(0, N - 1)
    assert torch.equal(idx_f.cpu(), want)
    assert torch.equal(codes_f.cpu().reshape(rows, D), e[want.long()].to(dtype))


# ------------------------------------------------------------------------------------------- the whole prior
def _state_dict():
    from flair_amd.guided_diffusion.restoreformer import VQVAEGANMultiHeadTransformer
    model = name_seeded_weights(VQVAEGANMultiHeadTransformer())
    return model, {k: v.detach().clone() for k, v in model.state_dict().items()}


@pytest.fixture(scope="module")
def hip_model(dev):
    model, sd = _state_dict()
    return model.to(dev).eval(), sd


def _at(dec, pix):
    return torch.stack([dec[b].reshape(dec.shape[1], -1)[:, pix[b]] for b in range(dec.shape[0])])


def _idx_bound(z_err, sd):
    """How far an error of max|dz| per element can move the top-2 distance margin: 4 |dz|_2 max|e|_2, plus f32 rounding
    of the distances."""
    e = sd["quantize.embedding.weight"]
    return 4 * z_err * e.shape[1] ** 0.5 * e.norm(dim=1).max().item() + 1e-4


@pytest.mark.gpu
def test_hip_restoreformer_matches_reference_fixture_f32(dev, hip_model):
    from tests.golden.make_golden_restoreformer import restoreformer_input
    g = np.load(GOLD)
    model, sd = hip_model
    x = restoreformer_input(g["x_u8"]).to(dev)
    z = model.quant_input(x).cpu()
    z_ref = torch.from_numpy(g["z"])
    z_err = (z - z_ref).abs().max().item()
    assert z_err <= 2e-4 * z_ref.abs().max().item(), z_err
    dec, emb_loss, info, hs = model(x)
    torch.cuda.synchronize()
    assert emb_loss is None and info[0] is None and info[1] is None and info[3] is None
    idx = info[2].cpu().reshape(2, 256)
    ref_idx = torch.from_numpy(g["idx"]).long()
    bound = _idx_bound(z_err, sd)
    clear = torch.from_numpy(g["margin"]) > bound
    assert clear.float().mean() > 0.9
    assert torch.equal(idx[clear], ref_idx[clear])
    mid = torch.from_numpy(g["mid_atten_c4"])
    mid_err = (hs["mid_atten"].cpu()[:, ::4] - mid).abs().max().item()
    assert mid_err <= 2e-4 * mid.abs().max().item()
    assert set(hs) == {"in", "block_0", "block_1", "block_2", "block_3", "block_4", "block_5_atten", "mid_atten", "out"}
    pix = torch.from_numpy(g["dec_pix"]).long()
    dec_ref = torch.from_numpy(g["dec_sub"])
    dec_f = model(x, code_idx=ref_idx)[0].cpu()
    dec_err = (_at(dec_f, pix) - dec_ref).abs().max().item()
    assert dec_err <= 3e-4 * dec_ref.abs().max().item(), dec_err
    agree = (idx == ref_idx).float().mean().item()
    if agree == 1.0:
        assert (_at(dec.cpu(), pix) - dec_ref).abs().max().item() <= 3e-4 * dec_ref.abs().max().item()
    parity_log(f"restoreformer f32 vs g13: z {z_err / z_ref.abs().max().item():.2e} rel-max, index bound {bound:.2e} "
               f"({clear.float().mean().item():.3f} clear), codes agree {agree:.4f}, mid_atten "
               f"{mid_err / mid.abs().max().item():.2e}, dec (fixture codes) {dec_err / dec_ref.abs().max().item():.2e}")


@pytest.mark.gpu
def test_hip_restoreformer_batch_and_bf16(dev, hip_model):
    """Two faces at once against two single-face calls and the CPU restatement; then bf16: code agreement reported,
    ``dec`` bounded (fixture codes injected)."""
    from tests import restoreformer_cpu as orf
    from tests.golden.make_golden_restoreformer import restoreformer_input
    g = np.load(GOLD)
    model, sd = hip_model
    x = restoreformer_input(g["x_u8"])
    ref_idx = torch.from_numpy(g["idx"]).long()
    ref = orf.restoreformer_forward(sd, x, code_idx=ref_idx)["dec"]
    dec = model(x.to(dev), code_idx=ref_idx)[0].cpu()
    assert (dec - ref).abs().max().item() <= 3e-4 * ref.abs().max().item()
    for b in range(2):
        solo = model(x[b:b + 1].to(dev), code_idx=ref_idx[b:b + 1])[0].cpu()
        assert (solo[0] - dec[b]).abs().max().item() <= 1e-4 * dec.abs().max().item()
    idx32 = model(x.to(dev))[2][2].cpu().reshape(2, 256)
    try:
        model.convert_to_bf16()
        dec16, _, info16, _ = model(x.to(dev))
        torch.cuda.synchronize()
        assert torch.isfinite(dec16).all()
        agree = (info16[2].cpu().reshape(2, 256) == idx32).float().mean().item()
        dec16f = model(x.to(dev), code_idx=ref_idx)[0].cpu()
        err = (dec16f - ref).abs().max().item() / ref.abs().max().item()
        parity_log(f"restoreformer bf16 vs f32: code agreement {agree:.3f}, dec (fixture codes) {err:.2e} rel-max")
        assert agree > 0.5
        assert err <= 8e-2
    finally:
        model.dtype = torch.float32
        model._packed_key = None


@pytest.mark.gpu
def test_sampler_steps_with_hip_restoreformer(dev, hip_model):
    """gaussian_diffusion.py:471-496 with aligned=True, two steps on one 512x512 face (toy eps-model): the HIP sampler with
    the HIP prior against the oracle loop with the CPU restatement as prior; the restatement's code indices are injected
    so a near-tie cannot fork the trajectories."""
    from flair_amd import workload as wl
    from oracle import diffusion as odiff
    from tests import restoreformer_cpu as orf
    from tests.golden.make_golden import codeformer_input, toy_model
    model, sd = hip_model
    x_T = codeformer_input(batch=1, seed=34) * 0.8
    g = torch.Generator().manual_seed(6)
    tape = [torch.randn(1, 3, 512, 512, generator=g) for _ in range(2)]
    tab = odiff.Spaced(odiff.spaced_steps(1000, "50"), odiff.named_betas("face_blur", 1000))
    codes = []

    def ora_aux(x0, t, xt):
        r = orf.restoreformer_forward(sd, x0)
        codes.append(r["idx"])
        return r["dec"]

    ref_trace = []
    ref = odiff.sample_loop(tab, toy_model, x_T, model_kwargs=dict(num_frames=1), aux_model=ora_aux, w=0.5, tau=0,
                            rho=0.35, t_start=1, step_noise=tape, trace=ref_trace)
    calls = iter(codes)

    class M:
        def parameters(self):
            return iter([x_T.to(dev)])

        def __call__(self, x, t, **kw):
            return toy_model(x, t, **kw)

    hip_aux = wl.restoreformer_aux(model)
    got_trace = []
    got = wl.diffusion_for(50).p_sample_loop(
        M(), x_T.shape, noise=x_T.to(dev), model_kwargs=dict(num_frames=1), device=dev, restore_fn=None,
        aux_model=lambda x0, t, xt: model(x0, code_idx=next(calls))[0],
        post_fn=lambda o: got_trace.append((int(o["t"][0]), o["pred_xstart"].cpu(), o["sample"].cpu())),
        w=0.5, tau=0, aligned=True, rho=0.35, noise_level=None, zeta=-1, prev_recon=None, t_start=1,
        noise_fn=lambda it, like: tape[it].to(dev))
    assert len(got_trace) == len(ref_trace) == 2
    for (ti, x0r, sr), (tg, x0g, sg) in zip(ref_trace, got_trace):
        assert ti == tg
        assert (x0r - x0g).abs().max().item() <= 5e-4, (ti, (x0r - x0g).abs().max().item())
        assert (sr - sg).abs().max().item() <= 1e-3 * max(1.0, sr.abs().max().item()), ti
    assert (ref - got.cpu()).abs().max().item() <= 1e-3
    x0 = x_T.to(dev)
    a, b = hip_aux(x0, None, x0), model(x0)[0]
    assert (a - b).abs().max().item() <= 1e-6 * b.abs().max().item()


# ------------------------------------------------------------------------------------------- command line, unaligned
_TPL = np.array([[192.98138, 239.94708], [318.90277, 240.1936], [256.63416, 314.01935], [201.26117, 371.41043],
                 [313.08905, 371.15118]]) / 512.0 - 0.5


def _face_detector_state():
    """A RetinaFace MobileNet-0.25 whose heads ignore the image: every 512-pixel anchor of the stride-32 level is a face
    (score 0.993, box = the anchor) with the 512 template's landmarks scaled to it; every other anchor is background."""
    from flair_amd.guided_diffusion.retinaface import RetinaFace
    net = RetinaFace("mobile0.25", device="cpu")
    sd = net.state_dict()
    for k in sd:
        if k.startswith(("ClassHead", "BboxHead", "LandmarkHead")):
            sd[k] = torch.zeros_like(sd[k])
    for lvl in range(3):
        sd[f"ClassHead.{lvl}.conv1x1.bias"] = torch.tensor([5.0, 0.0, 0.0, 5.0] if lvl == 2 else [5.0, 0.0, 5.0, 0.0])
        sd[f"LandmarkHead.{lvl}.conv1x1.bias"] = torch.from_numpy(np.tile(_TPL.reshape(-1) / 0.1, 2)).float()
    return sd


@pytest.mark.gpu
def test_cli_unaligned_restoreformer_matches_in_process_pipeline(dev, tmp_path):
    """python -m flair_amd restore ... --prior restoreformer (fresh process, time limit) on one unaligned 512 x 512 window
    (3 frames, detection + alignment + the prior on the crops + paste) with synthetic checkpoints == build_pipeline(...,
    prior="restoreformer").restore_video_files(...) in this process, PNG for PNG."""
    import scipy.io
    from PIL import Image
    from flair_amd import pipeline as pl
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion.parsenet import ParseNet
    from flair_amd.guided_diffusion.restoreformer import VQVAEGANMultiHeadTransformer
    from flair_amd.guided_diffusion.unet_new import UNetModel
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
    _, sd = _state_dict()
    torch.save({"state_dict": {"vqvae." + k: v for k, v in sd.items()}}, wdir / "RestoreFormer.ckpt")
    kernels = np.empty((1, 12), dtype=object)
    for i in range(12):
        kernels[0, i] = wl.synthetic_blur_kernel(25, 1.0 + 0.25 * i)
    scipy.io.savemat(tmp_path / "kernels_12.mat", {"kernels": kernels})
    frames = tmp_path / "frames"
    frames.mkdir()
    rng = np.random.default_rng(3)
    for i in range(N):
        Image.fromarray(rng.integers(0, 256, size=(s, s, 3), dtype=np.uint8), mode="RGB").save(frames / f"{i}.png")
    common = ["--prior", "restoreformer", "--size", str(S), "--steps", "2", "--weights", str(wdir), "--kernels",
              str(tmp_path / "kernels_12.mat"), "--det-model", "retinaface_mobile0.25", "--model-kwargs", json.dumps(kw),
              "--seed", "12", "--tau", "0"]                  # tau 0: the prior runs on both steps
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, "-m", "flair_amd", "restore", "gaussian",
                        str(frames), str(tmp_path / "cli"), *common], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"restored 1 videos, {N} frames" in r.stdout
    p = pl.build_pipeline("gaussian", wdir, device=dev, size=S, steps=2, kernels_path=str(tmp_path / "kernels_12.mat"),
                          prior="restoreformer", det_model="retinaface_mobile0.25", model_kwargs=kw)
    assert isinstance(p.aux_model.__closure__[0].cell_contents, VQVAEGANMultiHeadTransformer)
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
    assert np.asarray(Image.open(tmp_path / "lib" / "0000.png")).shape == (S, S, 3)
