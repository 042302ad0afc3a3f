"""Unaligned face videos end to end: the window loop with aligned=False (flair_amd/video.py, scripts/video_sample.py:446-479)
against the same loop assembled from the CPU oracles, the no-face rule, the unchanged aligned loop, and the command line
(python -m flair_amd) against the in-process pipeline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TPL = np.array([[192.98138, 239.94708], [318.90277, 240.1936], [256.63416, 314.01935], [201.26117, 371.41043],
                 [313.08905, 371.15118]]) / 512.0 - 0.5


def _face(cx, cy, size, score):
    """Box + score + five landmarks of a face of ``size`` pixels centred at (cx, cy) (the 512 template scaled)."""
    lm = _TPL * size + np.array([cx, cy])
    return np.concatenate([[cx - size / 2, cy - size / 2, cx + size / 2, cy + size / 2, score], lm.reshape(-1)]).astype(np.float32)


def _detections(k):
    """Fixed detections of the k-th frame of a batch: a small face listed first and the largest one, which is kept."""
    return np.stack([_face(30.0 + k, 34.0, 24.0, 0.99), _face(70.0 + 3 * k, 62.0 - 2 * k, 72.0 - 4 * k, 0.9)])


class StubDetector:
    """batched_detect_faces with fixed per-frame detections; frames that are black after the [-1, 1] -> [0, 255] mapping
    have none and are skipped, as the reference's detector skips them (retinaface.py:393-395)."""

    def __init__(self):
        self.calls = 0

    def batched_detect_faces(self, frames, conf_threshold=0.8, nms_threshold=0.4, use_origin_size=True, pre=None):
        assert conf_threshold == 0.5 and pre == (127.5, 127.5, 0.0, 255.0)
        self.calls += 1
        return [_detections(k) for k in range(frames.shape[0]) if frames[k].max().item() > -0.99]


def _toy_model(x, t, **kw):
    lr = kw["low_res_input"][0]
    eps = 0.3 * x - 0.2 * lr + 0.05 * torch.roll(x, 1, 0) + 0.01 * t.view(-1, 1, 1, 1).float() / 50.0
    return torch.cat([eps, 0.1 * x], 1)


class _M:
    """Toy network with the two attributes the sampler reads; counts its calls."""

    def __init__(self, like):
        self.like, self.calls = like, 0

    def parameters(self):
        return iter([self.like])

    def __call__(self, x, t, **kw):
        self.calls += 1
        return _toy_model(x, t, **kw)


def _aux(face, t, xt):                  # stand-in prior on the crops (as tests/test_face_warp.py)
    return 0.85 * face + 0.05 * xt


def _setup(dev, N, s, S, L, OV, steps, seed):
    from flair_amd import video
    g = torch.Generator().manual_seed(seed)
    degraded = torch.rand(1, N, 3, s, s, generator=g)
    wins = video.window_indices(N, L, OV)
    tapes = [[torch.randn(len(w), 3, S, S, generator=g) for _ in range(steps)] for w in wins]
    qnoise = [torch.randn(len(w), 3, S, S, generator=g) for w in wins]
    return degraded, wins, tapes, qnoise


def _blur_op(dev):
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion import pseudoSR as psr
    A = psr.pseudoSR(psr.Get_pseudoSR_Conf(4), upscale_kernel=wl.synthetic_blur_kernel(),
                     kernel_indx=10).WrapArchitecture_PyTorch().to(dev)
    return lambda d_n: (lambda x0: A.A_pinv(d_n[0].contiguous(), x0))


@pytest.mark.gpu
def test_unaligned_video_vs_oracle_loop(dev):
    """Two windows (4 frames, windows of 3 sharing 1) at 128 x 128 with aligned=False: detection by a stub detector, then
    alignment (largest face, LMEDS fit), crops, the HIP ParseNet mask and the paste for real, against the same two windows
    assembled from oracle.diffusion with aligned=False and an oracle helper on oracle/facewarp.py + oracle/parsenet.py,
    with the same noise tapes and matrices.  Bounds of test_unaligned_sampler_steps_vs_oracle."""
    from flair_amd import video
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    from flair_amd.guided_diffusion.parsenet import ParseNet
    from flair_amd.guided_diffusion.retinaface_utils import estimate_affine_partial
    from oracle import degrade as odeg
    from oracle import diffusion as odiff
    from oracle import facewarp as fw
    from oracle import parsenet as opn
    from tests.golden.weights import name_seeded_weights
    N, s, S, L, OV, steps, tau = 4, 32, 128, 3, 1, 2, 0
    degraded, wins, tapes, qnoise = _setup(dev, N, s, S, L, OV, steps, 31)
    assert wins == [[0, 1, 2], [2, 3]]
    hp = wl.TASKS["gaussian"]
    net = name_seeded_weights(ParseNet(in_size=512, out_size=512, parsing_ch=19)).eval()
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.to(dev)
    tpl = np.array([[192.98138, 239.94708], [318.90277, 240.1936], [256.63416, 314.01935], [201.26117, 371.41043],
                    [313.08905, 371.15118]]) * (S / 512.0)
    mats_of = [[estimate_affine_partial(_detections(k)[1][5:15].reshape(5, 2), tpl) for k in range(len(w))] for w in wins]

    # ---- the oracle loop (scripts/video_sample.py:371-485 with aligned=False)
    class OracleHelper:
        def get_crop_face_from_affine_matrices(self, imgs, ms):
            return fw.get_crop_face_from_affine_matrices(imgs, ms, face_size=(S, S))

        def inverse_faces(self, restored, ms):
            with torch.no_grad():
                parse = opn.parsenet_forward(sd, restored)[0].argmax(1)
            return fw.inverse_faces(restored, ms, parse.numpy())
    tab = odiff.Spaced(odiff.spaced_steps(1000, str(steps)), odiff.named_betas("face_blur", 1000))
    oblur = odeg.BlurOperator(wl.synthetic_blur_kernel(), 4)
    prev, ref = None, []
    for wi, idx in enumerate(wins):
        d = degraded[:, idx[0]:idx[-1] + 1]
        init = F.interpolate(d[0], (S, S), mode="area").clamp(0, 1)[None]
        d_n, init_n = (d - 0.5) / 0.5, (init - 0.5) / 0.5
        a = torch.from_numpy(tab.sqrt_alphas_cumprod).float()[tab.num_timesteps - 1]
        b = torch.from_numpy(tab.sqrt_one_minus_alphas_cumprod).float()[tab.num_timesteps - 1]
        rnn = F.interpolate(d_n[0], (S, S), mode="bicubic", align_corners=False).clamp(-1, 1)[None]
        sample = odiff.sample_loop(tab, _toy_model, a * init_n[0] + b * qnoise[wi],
                                   model_kwargs=dict(low_res_input=init_n, num_frames=len(idx), rnn_input=rnn),
                                   restore_fn=lambda x0, _d=d_n: oblur.a_pinv(_d[0], x0), aux_model=_aux, w=hp["w"],
                                   tau=tau, rho=hp["rho"], noise_level=hp["noise_level"], zeta=hp["zeta"], prev_recon=prev,
                                   step_noise=tapes[wi], aligned=False, face_restore_helper=OracleHelper(),
                                   affine_matrices=mats_of[wi])[None]
        if prev is not None:
            sample = sample[:, OV:]
        prev = sample[:, -OV:].clone()
        ref.append((sample.clamp(-1, 1) + 1) / 2)
    ref = torch.cat(ref, 1)[0]

    # ---- the HIP loop
    det = StubDetector()
    helper = FaceRestoreHelper(face_size=S, device=dev, face_det=det, face_parse=net)
    used = []
    crop = helper.get_crop_face

    def spy(*a, **k):
        out = crop(*a, **k)
        assert k == dict(only_keep_largest=True, eye_dist_threshold=0.1)
        used.append(out[1])
        return out
    helper.get_crop_face = spy
    m = _M(degraded.to(dev))
    got = video.restore_video("gaussian", degraded.to(dev), m, wl.diffusion_for(steps), _blur_op(dev), size=S,
                              aux_model=_aux, tau=tau, length=L, overlap=OV, aligned=False, face_helper=helper,
                              noise_fn=lambda wi, it, like: tapes[wi][it].to(dev),
                              q_noise_fn=lambda wi, like: qnoise[wi].to(dev))
    torch.cuda.synchronize()
    assert det.calls == len(wins) and len(used) == len(wins) and m.calls == steps * len(wins)
    for mats, want in zip(used, mats_of):
        assert len(mats) == len(want) and all(np.array_equal(a, b) for a, b in zip(mats, want))
    assert got.shape == ref.shape == (N, 3, S, S)
    # the frame shared by the two windows comes from window 0 (prev_recon), every frame exactly once
    for i in range(N):
        err = (got[i].cpu() - ref[i]).abs().max().item()
        assert err <= 2e-3, (i, err)
    # the prior changed the frames: an aligned run of the same tapes differs
    aligned = video.restore_video("gaussian", degraded.to(dev), _M(degraded.to(dev)), wl.diffusion_for(steps),
                                  _blur_op(dev), size=S, aux_model=_aux, tau=tau, length=L, overlap=OV,
                                  noise_fn=lambda wi, it, like: tapes[wi][it].to(dev),
                                  q_noise_fn=lambda wi, like: qnoise[wi].to(dev))
    assert (aligned.cpu() - got.cpu()).abs().max().item() > 1e-2


@pytest.mark.gpu
def test_window_without_a_face_is_refused_before_sampling(dev):
    from flair_amd import video
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    from flair_amd.guided_diffusion.parsenet import ParseNet
    N, s, S, L, OV, steps = 4, 16, 64, 3, 1, 2
    degraded, wins, tapes, qnoise = _setup(dev, N, s, S, L, OV, steps, 5)
    helper = FaceRestoreHelper(face_size=S, device=dev, face_det=StubDetector(),
                               face_parse=ParseNet(in_size=512, out_size=512, parsing_ch=19).to(dev).eval())
    common = dict(size=S, aux_model=_aux, tau=0, length=L, overlap=OV, aligned=False, face_helper=helper,
                  noise_fn=lambda wi, it, like: tapes[wi][it].to(dev), q_noise_fn=lambda wi, like: qnoise[wi].to(dev))
    for black, window in ((1, 0), (3, 1)):
        d = degraded.clone()
        d[0, black] = 0.0                                   # -> -1 after normalisation: no detection
        m = _M(d.to(dev))
        with pytest.raises(ValueError, match=rf"window {window} \(frames {wins[window][0]}\.\.{wins[window][-1]}\) "
                                             rf"has no face in frame\(s\) \[{black}\]"):
            video.restore_video("gaussian", d.to(dev), m, wl.diffusion_for(steps), _blur_op(dev), **common)
        assert m.calls == steps * window                    # nothing of the faceless window was sampled
    with pytest.raises(ValueError, match="face_helper"):
        video.restore_video("gaussian", degraded.to(dev), _M(degraded.to(dev)), wl.diffusion_for(steps), _blur_op(dev),
                            **dict(common, face_helper=None))
    with pytest.raises(ValueError, match="face size"):     # frames must be face_size square
        video.restore_video("gaussian", degraded.to(dev), _M(degraded.to(dev)), wl.diffusion_for(steps), _blur_op(dev),
                            **dict(common, size=128))


@pytest.mark.gpu
def test_aligned_default_is_the_previous_loop(dev):
    """restore_video with its default arguments == the window loop as it was before the unaligned mode, restated here
    (diffusion.sample with aligned=True, no helper, no matrices), bit for bit."""
    from flair_amd import video
    from flair_amd import workload as wl
    N, s, S, L, OV, steps = 5, 8, 32, 4, 1, 3
    degraded, wins, tapes, qnoise = _setup(dev, N, s, S, L, OV, steps, 9)
    degraded = degraded.to(dev)
    diffusion = wl.diffusion_for(steps)
    rf = _blur_op(dev)
    hp = wl.TASKS["gaussian"]
    got = video.restore_video("gaussian", degraded, _M(degraded), diffusion, rf, size=S, tau=1, length=L, overlap=OV,
                              noise_fn=lambda wi, it, like: tapes[wi][it].to(dev),
                              q_noise_fn=lambda wi, like: qnoise[wi].to(dev))
    prev, out = None, []
    for wi, idx in enumerate(wins):
        deg = degraded[0, idx[0]:idx[-1] + 1].float().contiguous()
        T = deg.shape[0]
        init_n = video.init_frames("gaussian", deg, S)[None]
        deg_n, deg_n_clip = video.normalise(deg)
        tt = torch.full((T,), diffusion.num_timesteps - 1, device=dev, dtype=torch.long)
        noise = diffusion.q_sample(init_n[0].contiguous(), tt, noise=qnoise[wi].to(dev))
        kwargs = dict(low_res_input=init_n, num_frames=T, enable_cross_frames=True, vsrpp_weights=1.0,
                      rnn_input=video.rnn_input(deg_n_clip, S)[None])
        sample = diffusion.sample(
            _M(degraded), noise, model_kwargs=kwargs, device=dev, progress=False, clip_denoised=True,
            restore_fn=rf(deg_n[None]), post_fn=None, face_restore_helper=None, aux_model=wl.identity_aux, w=hp["w"],
            tau=1, affine_matrices=None, aligned=True, sample_mode="ddpm", rho=hp["rho"], noise_level=hp["noise_level"],
            prev_recon=prev, zeta=hp["zeta"], t_start=-1, noise_fn=lambda it, like, _wi=wi: tapes[_wi][it].to(dev))
        keep = sample if prev is None else sample[OV:]
        prev = keep[-OV:].clone()[None]
        out.append(video._affine(video._to_clip(keep.contiguous()), 0.5, 0.5, 0.0, 1.0))
    torch.cuda.synchronize()
    assert torch.equal(got, torch.cat(out))


@pytest.mark.gpu
def test_cli_matches_in_process_pipeline(dev, tmp_path):
    """python -m flair_amd restore (fresh process, time limit) on 13 synthetic frames with a small gaussian-task UNetModel
    (--model-kwargs), random detector / parser checkpoints and a savemat kernel file == build_pipeline(...)
    .restore_video_files(...) in this process, PNG for PNG."""
    import scipy.io
    from PIL import Image
    from flair_amd import pipeline as pl
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion.parsenet import ParseNet
    from flair_amd.guided_diffusion.retinaface import RetinaFace
    from flair_amd.guided_diffusion.unet_new import UNetModel
    S, s, N = 64, 16, 13
    kw = dict(num_res_blocks=1, attention_resolutions=[2, 4], channel_mult=[0.5, 1, 4], use_checkpoint=False)
    wdir = tmp_path / "weights"
    wdir.mkdir()
    torch.manual_seed(0)
    cfg = pl.model_config("gaussian", S)
    cfg.update({k: tuple(v) if isinstance(v, list) else v for k, v in kw.items()})
    m = UNetModel(**cfg)
    wl.randomize_zero_modules(m)
    torch.save(m.state_dict(), wdir / "flair_gaussian.pt")
    torch.save(RetinaFace("mobile0.25", device="cpu").state_dict(), wdir / "detection_mobilenet0.25_Final.pth")
    torch.save(ParseNet(in_size=512, out_size=512, parsing_ch=19).state_dict(), wdir / "parsing_parsenet.pth")
    kernels = np.empty((1, 12), dtype=object)
    for i in range(12):
        kernels[0, i] = wl.synthetic_blur_kernel(25, 1.0 + 0.25 * i)
    scipy.io.savemat(tmp_path / "kernels_12.mat", {"kernels": kernels})
    frames = tmp_path / "frames"
    frames.mkdir()
    rng = np.random.default_rng(2)
    for i in range(N):
        Image.fromarray(rng.integers(0, 256, size=(s, s, 3), dtype=np.uint8), mode="RGB").save(frames / f"{i}.png")
    common = ["--aligned", "--no-prior", "--size", str(S), "--steps", "2", "--weights", str(wdir), "--kernels",
              str(tmp_path / "kernels_12.mat"), "--det-model", "retinaface_mobile0.25", "--model-kwargs", json.dumps(kw),
              "--seed", "11"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "flair_amd", "restore", "gaussian",
                        str(frames), str(tmp_path / "cli"), *common], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "restored 1 videos, 13 frames" in r.stdout
    p = pl.build_pipeline("gaussian", wdir, device=dev, size=S, steps=2, kernels_path=str(tmp_path / "kernels_12.mat"),
                          prior=False, det_model="retinaface_mobile0.25", model_kwargs=kw)
    d = pl.MAIN_DEFAULTS
    n = p.restore_video_files(frames, tmp_path / "lib", aligned=True, t_start=d["t_start"], jpeg_qf=d["jpeg_qf"], w=d["w"],
                              tau=d["tau"], rho=d["rho"], noise_level=d["noise_level"], zeta=d["zeta"], seed=11)
    assert n == N
    assert sorted(os.listdir(tmp_path / "cli")) == sorted(os.listdir(tmp_path / "lib")) == [f"{i:04d}.png" for i in range(N)]
    for i in range(N):
        a = (tmp_path / "cli" / f"{i:04d}.png").read_bytes()
        b = (tmp_path / "lib" / f"{i:04d}.png").read_bytes()
        assert a == b, i
    assert np.asarray(Image.open(tmp_path / "lib" / "0000.png")).shape == (S, S, 3)
