"""FLAIR's sampler on MI355X: same Python surface as the reference's
``guided_diffusion/gaussian_diffusion.py`` (``GaussianDiffusion``, ``get_named_beta_schedule``,
the three enums, ``_extract_into_tensor``), restructured around the hardware:

  * the coefficient tables are host float64 arrays (as in the reference, :112-173); the
    sampling loop runs every image of a call at the same step, so each step's coefficients
    are plain scalars handed to two fused HIP kernels (``flair_predict_xstart`` and
    ``flair_sampler_update``) instead of ~15 broadcast elementwise passes and ~10 tiny
    host-to-device table uploads per step (gaussian_diffusion.py:692-705);
  * the model, ``restore_fn`` and ``aux_model`` callables see the same tensors as in the
    reference ((N,C,H,W) f32 on the GPU).

Only the paths ``scripts/video_sample.py`` reaches are implemented: EPSILON mean type,
LEARNED_RANGE / FIXED_SMALL / FIXED_LARGE variance, ``sample_mode="ddpm"`` (FLAIR's
generalised DDIM step with stochasticity ``rho``).  There is no CPU path.
"""
import enum
import math

import numpy as np
import torch as th

from .. import ops


def get_named_beta_schedule(schedule_name, num_diffusion_timesteps):
    """gaussian_diffusion.py:15-36."""
    if schedule_name == "face_blur":
        scale = 1000 / num_diffusion_timesteps
        return np.linspace(scale * 0.0001, scale * 0.02, num_diffusion_timesteps, dtype=np.float64)
    if schedule_name == "face_bicubic":
        return np.linspace(1e-6, 1e-2, 2000, dtype=np.float64)
    raise NotImplementedError(f"unknown beta schedule: {schedule_name}")


def betas_for_alpha_bar(num_diffusion_timesteps, alpha_bar, max_beta=0.999):
    """gaussian_diffusion.py:39-56: betas that discretise a cumulative-product function alpha_bar(t), t in [0, 1]
    (host helper; neither named schedule of the reference uses it)."""
    steps = np.arange(num_diffusion_timesteps + 1) / num_diffusion_timesteps
    bar = np.array([alpha_bar(t) for t in steps], dtype=np.float64)
    return np.minimum(1 - bar[1:] / bar[:-1], max_beta)


class ModelMeanType(enum.Enum):
    PREVIOUS_X = enum.auto()
    START_X = enum.auto()
    EPSILON = enum.auto()


class ModelVarType(enum.Enum):
    LEARNED = enum.auto()
    FIXED_SMALL = enum.auto()
    FIXED_LARGE = enum.auto()
    LEARNED_RANGE = enum.auto()


class LossType(enum.Enum):
    MSE = enum.auto()
    RESCALED_MSE = enum.auto()
    KL = enum.auto()
    RESCALED_KL = enum.auto()

    def is_vb(self):
        return self in (LossType.KL, LossType.RESCALED_KL)


def _uniform_step(t):
    """The sampling loop advances every image at the same step; recover it as an int."""
    v = int(t.reshape(-1)[0].item())
    return v


class GaussianDiffusion:
    """Sampling utilities (gaussian_diffusion.py:95-689)."""

    def __init__(self, *, betas, model_mean_type, model_var_type, loss_type, rescale_timesteps=False):
        if model_mean_type not in (ModelMeanType.EPSILON, ModelMeanType.START_X, ModelMeanType.PREVIOUS_X):
            raise NotImplementedError(model_mean_type)
        self.model_mean_type = model_mean_type
        self.model_var_type = model_var_type
        self.loss_type = loss_type
        self.rescale_timesteps = rescale_timesteps

        betas = np.array(betas, dtype=np.float64)
        self.betas = betas
        assert betas.ndim == 1, "betas must be 1-D"
        assert (betas > 0).all() and (betas <= 1).all()
        self.num_timesteps = int(betas.shape[0])
        alphas = 1.0 - betas
        self.alphas_cumprod = np.cumprod(alphas, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.alphas_cumprod_next = np.append(self.alphas_cumprod[1:], 0.0)
        self.sqrt_alphas_cumprod_prev = np.sqrt(np.append(1.0, self.alphas_cumprod))   # T+1 entries
        self.sqrt_alphas_cumprod = np.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod_prev = np.append(0.0, np.sqrt(1.0 - self.alphas_cumprod[:-1]))
        self.log_one_minus_alphas_cumprod = np.log(1.0 - self.alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = np.log(
            np.append(self.posterior_variance[1], self.posterior_variance[1:]))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = ((1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas)
                                     / (1.0 - self.alphas_cumprod))
        self.posterior_mean_coef3 = self.posterior_mean_coef1 + (
            self.posterior_mean_coef2 * np.sqrt(self.alphas_cumprod))
        self.posterior_mean_coef4 = self.posterior_mean_coef2 * np.sqrt(1 - self.alphas_cumprod)

    # ------------------------------------------------------------------ forward process
    def q_mean_variance(self, x_start, t):
        """Mean / variance / log-variance of q(x_t | x_0) (gaussian_diffusion.py:189-204); uniform t."""
        i = _uniform_step(t)
        f32 = lambda v: float(np.float32(v))  # noqa: E731
        x = x_start.float().contiguous()
        mean = ops.axpby(x, x, f32(self.sqrt_alphas_cumprod[i]), 0.0)
        return (mean, th.full_like(mean, f32(1.0 - self.alphas_cumprod[i])),
                th.full_like(mean, f32(self.log_one_minus_alphas_cumprod[i])))

    def q_sample(self, x_start, t, noise=None):
        """sqrt(acp_t) x0 + sqrt(1-acp_t) eps (gaussian_diffusion.py:206-224); uniform t."""
        if noise is None:
            noise = th.randn_like(x_start)
        assert noise.shape == x_start.shape
        i = _uniform_step(t)
        return ops.axpby(x_start.float().contiguous(), noise.float().contiguous(),
                         float(np.float32(self.sqrt_alphas_cumprod[i])),
                         float(np.float32(self.sqrt_one_minus_alphas_cumprod[i])))

    def q_posterior_mean_variance(self, x_start, x_t, t):
        """Mean / variance / clipped log-variance of q(x_{t-1} | x_t, x_0)
        (gaussian_diffusion.py:226-248); uniform t."""
        assert x_start.shape == x_t.shape
        i = _uniform_step(t)
        f32 = lambda v: float(np.float32(v))  # noqa: E731
        mean = ops.axpby(x_start.float().contiguous(), x_t.float().contiguous(),
                         f32(self.posterior_mean_coef1[i]), f32(self.posterior_mean_coef2[i]))
        var = th.full_like(mean, f32(self.posterior_variance[i]))
        logvar = th.full_like(mean, f32(self.posterior_log_variance_clipped[i]))
        return mean, var, logvar

    def _scale_timesteps(self, t):
        if self.rescale_timesteps:
            return t.float() * (1000.0 / self.num_timesteps)
        return t

    # ------------------------------------------------------------------ reverse process
    def p_mean_variance(self, model, x, t, clip_denoised=True, model_kwargs=None, _step=None,
                        _moments=True):
        """gaussian_diffusion.py:250-342.  Returns the reference's dict; ``_moments=False``
        (used by the sampling loop, which only consumes ``pred_xstart``) skips the
        posterior mean / variance tensors."""
        if model_kwargs is None:
            model_kwargs = {}
        model_kwargs["sqrt_recip_alphas_cumprod"] = self.sqrt_recip_alphas_cumprod
        model_kwargs["sqrt_recipm1_alphas_cumprod"] = self.sqrt_recipm1_alphas_cumprod
        B, C = x.shape[:2]
        assert t.shape == (B,)
        i = _uniform_step(t) if _step is None else _step
        model_output = model(x, self._scale_timesteps(t), **model_kwargs).float().contiguous()
        learned = self.model_var_type in (ModelVarType.LEARNED_RANGE, ModelVarType.LEARNED)
        if learned:
            assert model_output.shape == (B, C * 2, *x.shape[2:])
        x = x.float().contiguous()
        f32 = lambda v: float(np.float32(v))  # noqa: E731  (the reference casts table entries to f32)
        # pred_xstart = clamp(a * x - b * model_output[:, :C]) for all three mean parametrisations (gaussian_diffusion.py:316-333):
        #   EPSILON     a = sqrt(1/acp), b = sqrt(1/acp - 1);   START_X  a = 0, b = -1;
        #   PREVIOUS_X  (xprev - coef2 x) / coef1:  a = -coef2 / coef1, b = -1 / coef1
        if self.model_mean_type == ModelMeanType.EPSILON:
            ca, cb = f32(self.sqrt_recip_alphas_cumprod[i]), f32(self.sqrt_recipm1_alphas_cumprod[i])
        elif self.model_mean_type == ModelMeanType.START_X:
            ca, cb = 0.0, -1.0
        else:
            ca = -f32(self.posterior_mean_coef2[i] / self.posterior_mean_coef1[i])
            cb = -f32(1.0 / self.posterior_mean_coef1[i])
        pred_xstart = ops.predict_xstart(x, model_output, ca, cb, clip_denoised)
        out = {"pred_xstart": pred_xstart}
        if _moments:
            if self.model_mean_type == ModelMeanType.PREVIOUS_X:
                out["mean"] = model_output[:, :C].contiguous()
            else:
                out["mean"] = ops.axpby(pred_xstart, x, f32(self.posterior_mean_coef1[i]),
                                        f32(self.posterior_mean_coef2[i]))
            if self.model_var_type == ModelVarType.LEARNED:
                # log-variance = the raw second half of the output: frac * max + (1 - frac) * min with min = -1, max = 1
                var, logvar = ops.learned_range_variance(model_output, C, -1.0, 1.0)
            elif learned:
                var, logvar = ops.learned_range_variance(
                    model_output, C, f32(self.posterior_log_variance_clipped[i]), f32(np.log(self.betas[i])))
            else:
                if self.model_var_type == ModelVarType.FIXED_LARGE:
                    v = np.append(self.posterior_variance[1], self.betas[1:])[i]
                    lv = np.log(v)
                else:
                    v, lv = self.posterior_variance[i], self.posterior_log_variance_clipped[i]
                var = th.full_like(x, f32(v))
                logvar = th.full_like(x, f32(lv))
            out["variance"], out["log_variance"] = var, logvar
        return out

    def _predict_xstart_from_eps(self, x_t, t, eps):
        """sqrt(1/acp_t) x_t - sqrt(1/acp_t - 1) eps (gaussian_diffusion.py:344-349); uniform t."""
        assert x_t.shape == eps.shape
        i = _uniform_step(t)
        return ops.axpby(x_t.float().contiguous(), eps.float().contiguous(),
                         float(np.float32(self.sqrt_recip_alphas_cumprod[i])),
                         -float(np.float32(self.sqrt_recipm1_alphas_cumprod[i])))

    def _predict_xstart_from_xprev(self, x_t, t, xprev):
        """(xprev - coef2 x_t) / coef1 (gaussian_diffusion.py:351-360); uniform t."""
        assert x_t.shape == xprev.shape
        i = _uniform_step(t)
        return ops.axpby(xprev.float().contiguous(), x_t.float().contiguous(),
                         float(np.float32(1.0 / self.posterior_mean_coef1[i])),
                         -float(np.float32(self.posterior_mean_coef2[i] / self.posterior_mean_coef1[i])))

    def _predict_eps_from_xstart(self, x_t, t, pred_xstart):
        """gaussian_diffusion.py:362-366; uniform t."""
        i = _uniform_step(t)
        a = float(np.float32(self.sqrt_recip_alphas_cumprod[i]))
        b = float(np.float32(self.sqrt_recipm1_alphas_cumprod[i]))
        return ops.axpby(x_t.float().contiguous(), pred_xstart.float().contiguous(), a / b, -1.0 / b)

    def p_sample(self, model, x, t, clip_denoised=True, model_kwargs=None, restore_fn=None,
                 affine_matrices=None, face_restore_helper=None, aux_model=None, w=0.5,
                 start_timestep=None, tau=None, aligned=False, rho=0.35, prev_recon=None, gamma=None,
                 noise=None, _step=None, face_frames=None):
        """One generalised-DDIM step (gaussian_diffusion.py:423-517).  ``w`` / ``gamma`` may be
        python floats or the broadcast tensors the reference passes (their first element is
        used: the loop's values are uniform).  ``face_frames`` (extension, aligned=False only): the frame of every
        affine matrix, sorted -- a frame may then have no face or several; an empty list is the step with the prior off."""
        i = _uniform_step(t) if _step is None else _step
        out = self.p_mean_variance(model, x, t, clip_denoised=clip_denoised, model_kwargs=model_kwargs,
                                   _step=i, _moments=False)
        x = x.float().contiguous()
        x0 = out["pred_xstart"]
        restored = None
        if restore_fn is not None:
            restored = restore_fn(x0).float().contiguous()
        aux = None
        # the reference compares against whatever the loop passed (gaussian_diffusion.py:473-474) and
        # fails on its own default None; a direct call without it means "the prior is on from the start"
        if start_timestep is None:
            start_timestep = self.num_timesteps - 1
        if tau is None:
            tau = 0
        if face_frames is not None:
            if aligned:
                raise ValueError("face_frames belongs to aligned=False (the aligned prior sees whole frames)")
            if affine_matrices is None or len(face_frames) != len(affine_matrices):
                raise ValueError("face_frames needs one entry per affine matrix")
            if any(not 0 <= int(f) < x.shape[0] for f in face_frames):
                raise ValueError(f"face_frames entries must be in [0, {x.shape[0]})")
        no_faces = face_frames is not None and len(face_frames) == 0   # a window without any face: the prior is off
        if aux_model is not None and i <= start_timestep and i >= tau and not no_faces:
            # NB: the reference evaluates the aux prior on the data-consistent x0; the fused
            # kernel applies consistency + blend in one pass, so materialise that x0 first.
            if restored is not None:
                g = _scalar(gamma, 1.0)
                if clip_denoised:
                    x0c = ops.axpby(x0, restored, 1.0, -g, lo=-1.0, hi=1.0)
                else:
                    x0c = ops.axpby(x0, restored, 1.0, -g)
                x0, restored = x0c, None
            if not aligned and face_frames is not None:
                # the branch below for K faces in T frames: crops read through a frame index, the prior on the K crops,
                # one paste launch that leaves frames without a face as x0
                if face_restore_helper is None:
                    raise ValueError("aligned=False needs face_restore_helper and affine_matrices "
                                     "(gaussian_diffusion.py:476-483)")
                aux_face = face_restore_helper.get_crop_face_from_affine_matrices(x0, affine_matrices, face_frames)
                aux_xt = face_restore_helper.get_crop_face_from_affine_matrices(x, affine_matrices, face_frames)
                K = len(face_frames)                            # t is uniform: one entry per crop, without an index upload
                tk = t if K == t.shape[0] else th.full((K,), i, device=t.device, dtype=t.dtype)
                aux_face = aux_model(aux_face, tk, aux_xt)
                aux = face_restore_helper.paste_faces(x0, aux_face, affine_matrices, face_frames)
            elif not aligned:
                # gaussian_diffusion.py:476-493: crop the faces out of x0 and x_t with the window's affine matrices, run
                # the prior on the crops, warp its output back and paste it through the blurred parsing mask -- all on
                # the GPU (flair_amd.guided_diffusion.face_restoration_helper; the reference goes through numpy / cv2)
                if face_restore_helper is None or affine_matrices is None:
                    raise ValueError("aligned=False needs face_restore_helper and affine_matrices "
                                     "(gaussian_diffusion.py:476-483)")
                aux_face = face_restore_helper.get_crop_face_from_affine_matrices(x0, affine_matrices)
                aux_xt = face_restore_helper.get_crop_face_from_affine_matrices(x, affine_matrices)
                if aux_face is None or aux_xt is None:
                    # (the reference hands None on to aux_model here, gaussian_diffusion.py:484-486, and fails inside it)
                    raise ValueError("aligned=False: no face crop (affine_matrices is empty): one affine matrix per frame is needed")
                aux_face = aux_model(aux_face, t, aux_xt)
                inv_face, inv_mask = face_restore_helper.inverse_faces(aux_face, affine_matrices)
                if tuple(inv_face.shape) != tuple(x0.shape):
                    raise ValueError(f"inverse_faces returned {tuple(inv_face.shape)} for frames of {tuple(x0.shape)}: the "
                                     "reference pastes at the face size (face_restoration_helper.py:318-323), so frames "
                                     "must be face_size x face_size")
                aux = ops.face_blend(x0, inv_face.float().contiguous(), inv_mask.float().contiguous())
            else:
                aux = aux_model(x0, t, x).float().contiguous()
        c = ops.SamplerCoefs()
        c.gamma = _scalar(gamma, 1.0)
        c.w_aux = _scalar(w, 0.5)
        f32 = lambda v: float(np.float32(v))  # noqa: E731
        c.sqrt_recip_alphas_cumprod = f32(self.sqrt_recip_alphas_cumprod[i])
        c.sqrt_recipm1_alphas_cumprod = f32(self.sqrt_recipm1_alphas_cumprod[i])
        c.sqrt_alphas_cumprod_prev = f32(self.sqrt_alphas_cumprod_prev[i])
        c.sqrt_one_minus_alphas_cumprod_prev = f32(self.sqrt_one_minus_alphas_cumprod_prev[i])
        c.sqrt_one_minus_rho = float(np.sqrt(1 - rho))
        c.sqrt_rho = float(np.sqrt(rho))
        c.clip_denoised = int(bool(clip_denoised))
        c.nonzero = int(i != 0)
        prev = None
        if prev_recon is not None:
            prev = prev_recon.float().contiguous()
            c.frame_elems = int(x[0].numel())
            c.frames = int(model_kwargs["num_frames"])
            c.prev_frames = int(prev_recon.shape[1])
        if noise is None and i != 0:
            noise = th.randn_like(x)
        sample = ops.sampler_update(c, x, x0, restored, aux, noise, prev)
        return {"sample": sample, "pred_xstart": x0}

    def sample(self, model, noise, model_kwargs, restore_fn, face_restore_helper, aux_model, post_fn,
               clip_denoised=True, sample_mode="ddpm", device=None, progress=False, w=0.5, tau=None,
               aligned=False, affine_matrices=None, rho=0.35, noise_level=None, prev_recon=None,
               zeta=-1, t_start=-1, noise_fn=None, face_frames=None):
        """gaussian_diffusion.py:372-421."""
        if tau is None:
            tau = 0
        if sample_mode != "ddpm":
            raise NotImplementedError("flair_amd: sample_mode must be 'ddpm' (the reference's only mode)")
        return self.p_sample_loop(
            model=model, shape=noise.shape, noise=noise, clip_denoised=clip_denoised,
            model_kwargs=model_kwargs, progress=progress, device=device, restore_fn=restore_fn,
            face_restore_helper=face_restore_helper, aux_model=aux_model, post_fn=post_fn, w=w, tau=tau,
            aligned=aligned, affine_matrices=affine_matrices, rho=rho, noise_level=noise_level,
            prev_recon=prev_recon, zeta=zeta, t_start=t_start, noise_fn=noise_fn, face_frames=face_frames)

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, model_kwargs=None, device=None,
                      progress=False, affine_matrices=None, restore_fn=None, face_restore_helper=None,
                      aux_model=None, post_fn=None, w=0.5, tau=None, aligned=False, rho=0.35,
                      noise_level=None, prev_recon=None, zeta=-1, t_start=-1, noise_fn=None, face_frames=None):
        """gaussian_diffusion.py:519-587.  ``noise_fn(step_index, like)`` (extension) supplies the
        per-step gaussian draw instead of ``th.randn_like`` so runs can share a noise tape."""
        final = None
        for sample in self.p_sample_loop_progressive(
                model, shape, noise=noise, clip_denoised=clip_denoised, model_kwargs=model_kwargs,
                device=device, progress=progress, restore_fn=restore_fn, affine_matrices=affine_matrices,
                face_restore_helper=face_restore_helper, aux_model=aux_model, w=w, tau=tau,
                aligned=aligned, rho=rho, noise_level=noise_level, prev_recon=prev_recon, zeta=zeta,
                t_start=t_start, noise_fn=noise_fn, face_frames=face_frames):
            if post_fn is not None:
                post_fn(sample)
            final = sample
        return final["sample"]

    ddim_sample_loop = p_sample_loop  # FLAIR's p_sample *is* the DDIM step (rho=0 -> eta=0)

    def schedules(self, start_timestep, tau, w, zeta, noise_level, have_aux=True):
        """The ``ws`` ramp and ``gammas`` of gaussian_diffusion.py:632-657 (host float64)."""
        T = self.num_timesteps
        if have_aux:
            if start_timestep - tau > 0:
                ws = np.linspace(0, 1, start_timestep - tau + 1)
                ws = 1.0 * np.exp(-ws * 1)
                ws = (ws - ws.min()) / (ws.max() - ws.min()) * (1 - w)
                ws = 1 - ws
                ws = np.append(ws, np.ones(T - start_timestep - 1))
                ws = np.concatenate([np.ones(tau), ws])
            else:
                ws = np.ones(T) * w
        else:
            ws = np.ones(T)
        if zeta == -1:
            gammas = np.ones_like(self.betas)
        else:
            gammas = zeta * (noise_level ** 2
                             / (self.sqrt_one_minus_alphas_cumprod / self.sqrt_alphas_cumprod) ** 2)
            gammas[gammas >= 1] = 0.991
            gammas[gammas <= 1e-1] = 1e-6
            gammas = 1 - gammas
        return ws, gammas

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, model_kwargs=None,
                                  device=None, progress=False, affine_matrices=None,
                                  face_restore_helper=None, aux_model=None, restore_fn=None, w=0.5,
                                  tau=None, aligned=False, rho=0.35, noise_level=None, prev_recon=None,
                                  zeta=-1, t_start=-1, noise_fn=None, face_frames=None):
        """gaussian_diffusion.py:589-689."""
        if device is None:
            device = next(model.parameters()).device
        assert isinstance(shape, (tuple, list, th.Size))
        img = noise if noise is not None else th.randn(*shape, device=device)
        if tau is None:
            tau = 0
        indices = list(range(self.num_timesteps))
        if t_start != -1:
            if t_start < 0 or t_start >= self.num_timesteps:
                raise ValueError("t_start must be in [0, num_timesteps)")
            indices = indices[: t_start + 1]
        indices = indices[::-1]
        if aux_model is None:
            raise ValueError("p_sample_loop needs an aux_model (the reference leaves "
                             "start_timestep unbound without one, gaussian_diffusion.py:632-680)")
        start_timestep = indices[0]
        ws, gammas = self.schedules(start_timestep, tau, w, zeta, noise_level)
        # optical flow is cached per conditioning clip for the length of ONE chain: a caller may refill the
        # same rnn_input storage through kernels that do not bump torch's version counter
        inner = getattr(model, "model", model)
        if hasattr(inner, "reset_flow_cache"):
            inner.reset_flow_cache()
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        for it, i in enumerate(indices):
            t = th.full((shape[0],), i, device=device, dtype=th.long)
            z = None
            if noise_fn is not None and i != 0:
                z = noise_fn(it, img)
            with th.no_grad():
                out = self.p_sample(model, img, t, clip_denoised=clip_denoised, model_kwargs=model_kwargs,
                                    restore_fn=restore_fn, affine_matrices=affine_matrices,
                                    face_restore_helper=face_restore_helper, aux_model=aux_model,
                                    w=float(np.float32(ws[i])), start_timestep=start_timestep, tau=tau,
                                    aligned=aligned, rho=rho, prev_recon=prev_recon,
                                    gamma=float(np.float32(gammas[i])), noise=z, _step=i, face_frames=face_frames)
                img = out["sample"]
                out["t"] = t
                yield out


def _scalar(v, default):
    if v is None:
        return float(default)
    if isinstance(v, th.Tensor):
        return float(v.reshape(-1)[0].item())
    return float(v)


def _extract_into_tensor(arr, timesteps, broadcast_shape, dtype=th.float32):
    """gaussian_diffusion.py:692-705 (kept for API compatibility; the hot loop uses scalars)."""
    res = th.from_numpy(np.asarray(arr)).to(device=timesteps.device)[timesteps].float()
    while len(res.shape) < len(broadcast_shape):
        res = res[..., None]
    return res.expand(broadcast_shape)
