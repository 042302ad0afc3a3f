"""Several faces per frame and frames without a face in the un-aligned prior branch: the indexed crop
(flair_warp_affine_cubic_indexed), the fused paste (flair_face_paste), the sampler's face_frames argument and the window
loop's faces="all" mode, against the launches the project already had (bit for bit) and against oracle/facewarp.py +
oracle/diffusion.py composed per face (the reference itself never pastes two faces into one frame)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, H, W, FS = 3, 40, 56, 32                     # three 40 x 56 frames, five 32 x 32 faces
SRC_INDEX = [0, 0, 2, 2, 2]
FRAME_START = [0, 2, 2, 5]
POISON = -7777.0


def _similarity(scale, theta, tx, ty):
    c, s = scale * np.cos(theta), scale * np.sin(theta)
    return np.array([[c, -s, tx], [s, c, ty]], dtype=np.float64)


def _smooth(n, c, h, w, seed, amp=0.6, noise=0.15):
    g = torch.Generator().manual_seed(seed)
    base = torch.nn.functional.interpolate(torch.randn(n, c, 5, 7, generator=g), size=(h, w), mode="bicubic", align_corners=False)
    return (base * amp + noise * torch.randn(n, c, h, w, generator=g)).clamp(-1.3, 1.3)      # some values beyond [-1, 1]


def _face_at(scale, theta, cx, cy):
    """Frame -> face matrix (what estimateAffinePartial2D returns) of a face centred at (cx, cy) of the frame."""
    M = _similarity(scale, theta, 0.0, 0.0)
    M[:, 2] = (FS - 1) / 2.0 - M[:, :2] @ np.array([cx, cy])
    return M


# two overlapping faces in frame 0 (one tilted); in frame 2 a small tilted one, one cut by the frame's right edge (its crop
# reaches the border fill) and a large one that overlaps both and hangs over the bottom edge
MATS = [_face_at(1.6, 0.0, 13.5, 11.5), _face_at(1.25, 0.31, 24.0, 18.0), _face_at(2.1, -0.21, 8.0, 24.0),
        _face_at(1.1, 0.12, 50.0, 10.0), _face_at(0.8, -0.4, 28.0, 22.0)]

_case = {}


def case():
    """Inputs and CPU references shared by the tests below (computed once, never modified)."""
    if not _case:
        from oracle import facewarp as fw
        x = _smooth(T, 3, H, W, 3)
        faces = _smooth(5, 3, FS, FS, 5)
        g = torch.Generator().manual_seed(7)
        masks = torch.nn.functional.interpolate(torch.rand(5, 1, 4, 4, generator=g, dtype=torch.float64), size=(FS, FS),
                                                mode="bilinear", align_corners=True).clamp(0, 1)
        crops = fw.get_crop_face_from_affine_matrices(x[SRC_INDEX], MATS, face_size=(FS, FS))
        f255 = (((faces + 1.0) / 2.0).clamp(0, 1) * 255).permute(0, 2, 3, 1).contiguous().numpy()
        inv_f, inv_m = [], []
        for k in range(5):
            inv = fw.invert_affine(MATS[k])
            inv_f.append(fw.warp_affine_cubic(f255[k], inv, (W, H)).astype(np.float32))
            inv_m.append(fw.warp_affine_cubic(masks[k, 0].numpy(), inv, (W, H)).astype(np.float32))
        f = torch.from_numpy(np.stack(inv_f)).permute(0, 3, 1, 2) / 255.0
        f = ((f - 0.5) / 0.5).clamp(-1, 1)
        m = torch.from_numpy(np.stack(inv_m)).unsqueeze(1)
        pasted = x.clone()
        for t in range(T):
            for k in range(FRAME_START[t], FRAME_START[t + 1]):
                pasted[t] = fw.blend(pasted[t], f[k], m[k])
        _case.update(x=x, faces=faces, masks=masks, crops=crops, inv_masks=m, pasted=pasted)
    return _case


def _helper(dev, size=FS, **kw):
    from flair_amd.guided_diffusion.face_restoration_helper import FaceRestoreHelper
    return FaceRestoreHelper(face_size=size, device=dev, **kw)


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _three_launches(x0, faces, masks, minv, frame_start):
    """The paste as the launches that predate flair_face_paste, face by face onto the running frame."""
    from flair_amd import ops
    Hh, Ww = x0.shape[-2:]
    run = x0.clone()
    for t in range(x0.shape[0]):
        for k in range(frame_start[t], frame_start[t + 1]):
            f = ops.warp_affine_cubic(faces[k:k + 1].contiguous(), minv[k:k + 1].contiguous(), (Hh, Ww), pre=True, post=True)
            m = ops.warp_affine_cubic(masks[k:k + 1].contiguous(), minv[k:k + 1].contiguous(), (Hh, Ww))
            run[t:t + 1] = ops.face_blend(run[t:t + 1].contiguous(), f, m)
    return run


def test_the_case_has_overlapping_faces_and_a_cut_one():
    """CPU-side properties of the shared case that the GPU tests rely on."""
    m = case()["inv_masks"]
    assert ((m[3, 0] > 0.1) & (m[4, 0] > 0.1)).any() and ((m[2, 0] > 0.1) & (m[4, 0] > 0.1)).any()     # frame 2: overlaps
    assert ((m[0, 0] > 0.1) & (m[1, 0] > 0.1)).any()                                                    # frame 0 too
    assert (case()["crops"][3, :, :, -1] == torch.tensor([135.0, 133.0, 132.0]).div(255).sub(0.5).div(0.5)[:, None]).all()
    assert T * H * W % 256 != 0


def test_indexed_crop_vs_oracle_and_old_entry(dev):
    from flair_amd import ops
    c = case()
    x = c["x"].to(dev)
    helper = _helper(dev)
    got = helper.get_crop_face_from_affine_matrices(x, MATS, SRC_INDEX)
    torch.cuda.synchronize()
    assert got.shape == (5, 3, FS, FS)
    err = (got.cpu() - c["crops"]).abs().max().item()
    print(f"indexed crop vs oracle: max|err| = {err:.3e}")
    assert err <= 2e-6, err                                   # the bound of test_crop_faces_vs_oracle
    # the same crops from a gathered copy of the frames through the old entry, and src_index = arange on that copy
    minv = helper._minv(MATS, dev)
    gathered = x[SRC_INDEX].contiguous()
    kw = dict(border=(135.0, 133.0, 132.0), pre=True, post=True)
    old = ops.warp_affine_cubic(gathered, minv, (FS, FS), **kw)
    ident = ops.warp_affine_cubic(gathered, minv, (FS, FS), src_index=_i32(list(range(5)), dev), src_index_host=list(range(5)), **kw)
    assert torch.equal(ident, old) and torch.equal(got, old)
    # the f64 form (masks) reads through the index too
    m = c["masks"].to(dev)
    mi = helper._minv(MATS[:3], dev)
    a = ops.warp_affine_cubic(m, mi, (H, W), src_index=_i32([4, 0, 4], dev), src_index_host=[4, 0, 4])
    b = ops.warp_affine_cubic(m[[4, 0, 4]].contiguous(), mi, (H, W))
    assert torch.equal(a, b)


def test_paste_equals_the_three_launch_sequence(dev):
    from flair_amd import ops
    c = case()
    x0, faces, masks = c["x"].to(dev), c["faces"].to(dev), c["masks"].to(dev)
    minv = _helper(dev)._minv(MATS, dev, twice=True)
    want = _three_launches(x0, faces, masks, minv, FRAME_START)
    got = ops.face_paste(x0, faces, masks, minv, _i32(FRAME_START, dev), FRAME_START)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(got[1], x0[1])                         # the frame without a face
    assert not torch.equal(got[0], x0[0]) and not torch.equal(got[2], x0[2])
    # order matters where faces overlap: the last face of frame 2 pasted first gives another frame
    swapped = [0, 1, 4, 2, 3]
    other = ops.face_paste(x0, faces[swapped].contiguous(), masks[swapped].contiguous(), minv[swapped].contiguous(),
                           _i32(FRAME_START, dev), FRAME_START)
    assert torch.equal(other[:2], got[:2]) and not torch.equal(other[2], got[2])
    # guarded neighbours: x0 and out in the middle of larger poisoned buffers
    n, G = x0.numel(), 1000
    src = torch.full((n + 2 * G,), POISON, device=dev)
    dst = torch.full((n + 2 * G,), POISON, device=dev)
    src[G:G + n] = x0.reshape(-1)
    out = ops.face_paste(src[G:G + n].view_as(x0), faces, masks, minv, _i32(FRAME_START, dev), FRAME_START,
                         out=dst[G:G + n].view_as(x0))
    torch.cuda.synchronize()
    assert torch.equal(out, want) and out.data_ptr() == dst[G:].data_ptr()
    for buf in (src, dst):
        assert (buf[:G] == POISON).all() and (buf[G + n:] == POISON).all()
    assert torch.equal(src[G:G + n], x0.reshape(-1))


def test_paste_vs_oracle(dev):
    """Bound 1.5e-5: per layer |d(v(1-m)+fm)| <= |dv| + |df| + |dm| |f - v| <= 2e-6 + 1e-6 * 2.3 (the warps' bounds of
    test_mask_blur_and_inverse_warp_vs_oracle, |v| <= 1.3, |f| <= 1), three layers in frame 2."""
    from flair_amd import ops
    c = case()
    minv = _helper(dev)._minv(MATS, dev, twice=True)
    got = ops.face_paste(c["x"].to(dev), c["faces"].to(dev), c["masks"].to(dev), minv, _i32(FRAME_START, dev), FRAME_START)
    torch.cuda.synchronize()
    err = (got.cpu() - c["pasted"]).abs().max().item()
    print(f"paste vs oracle: max|err| = {err:.3e}")
    assert err <= 1.5e-5, err
    assert (c["pasted"] - c["x"]).abs().max().item() > 0.1    # the paste did something


def test_paste_without_faces_is_a_copy(dev):
    from flair_amd import ops
    x0 = case()["x"].to(dev)
    zeros = [0] * (T + 1)
    out = ops.face_paste(x0, None, None, None, _i32(zeros, dev), zeros)
    torch.cuda.synchronize()
    assert torch.equal(out, x0) and out.data_ptr() != x0.data_ptr()
    empty = ops.face_paste(x0, torch.empty(0, 3, FS, FS, device=dev), torch.empty(0, 1, FS, FS, dtype=torch.float64, device=dev),
                           torch.empty(0, 6, dtype=torch.float64, device=dev), _i32(zeros, dev), zeros)
    assert torch.equal(empty, x0)
    assert torch.equal(_helper(dev, face_parse=object()).paste_faces(x0, None, [], []), x0)


# --------------------------------------------------------------------------------------------------------- sampler
class StubParser:
    """parse_indices returns a fixed blobby label map per face and ignores its input: no arg-max near-ties."""

    def __init__(self, n, size, dev, seed=6):
        g = torch.Generator().manual_seed(seed)
        blob = torch.nn.functional.interpolate(torch.rand(n, 1, 6, 6, generator=g), size=(size, size), mode="bilinear")
        self.maps = (blob[:, 0] * 19).long().clamp(0, 18)
        self.dev_maps = self.maps.to(torch.int32).to(dev)

    def parse_indices(self, x):
        return self.dev_maps[:x.shape[0]].contiguous()


S = 64
SMATS = [_similarity(1.45, 0.08, -12.0, -9.0), _similarity(2.1, -0.21, -41.3, -32.5), _similarity(0.93, 0.3, 7.6, -2.6)]


def _aux(face, t, xt):
    return 0.85 * face + 0.05 * xt


class _M:
    def __init__(self, like):
        self.like = like

    def parameters(self):
        return iter([self.like])

    def __call__(self, x, t, **kw):
        from tests.test_gpu_sampler import toy_model
        return toy_model(x, t, **kw)


def _steps(dev, x_T, tape, **kw):
    """Two p_sample steps (9, 8 of a 10-step chain) from x_T with the noise tape; returns [(pred_xstart, sample)]."""
    from flair_amd import workload as wl
    diffusion = wl.diffusion_for(10)
    x, out = x_T.to(dev), []
    for it, i in enumerate((9, 8)):
        t = torch.full((x.shape[0],), i, device=dev, dtype=torch.long)
        with torch.no_grad():
            o = diffusion.p_sample(_M(x), x, t, model_kwargs=dict(num_frames=x.shape[0]), w=0.5, tau=2, rho=0.25,
                                   noise=tape[it].to(dev), **kw)
        out.append((o["pred_xstart"], o["sample"]))
        x = o["sample"]
    torch.cuda.synchronize()
    return out


def _tape(n=3):
    g = torch.Generator().manual_seed(11)
    return torch.randn(n, 3, S, S, generator=g), [torch.randn(n, 3, S, S, generator=g) for _ in range(2)]


def test_sampler_steps_with_two_faces_in_a_frame_vs_oracle(dev):
    """Two steps at T = 3, 64 x 64, face_frames = [0, 0, 2] against oracle.diffusion with the prior restated per face on
    oracle.facewarp (crop by frame index, prior on the crops, inverse_faces, sequential blend).  Bounds: those of a sampler
    step without any parsing (tests/test_gpu_sampler.py: 2e-4 on x0, 5e-4 relative on the sample -- what remains of
    test_unaligned_sampler_steps_vs_oracle's 2e-3 once arg-max flips cannot occur, the parser here being a fixed map) plus
    the paste's 1.5e-5 (test_paste_vs_oracle), which enters x0 with weight 1 - w <= 1: 2.2e-4 / 5.2e-4."""
    from oracle import diffusion as odiff
    from oracle import facewarp as fw
    from tests.test_gpu_sampler import toy_model
    ff = [0, 0, 2]
    parser = StubParser(3, S, dev)
    x_T, tape = _tape()

    def oracle_prior(x0, t, img):                              # -> x_with_face, as the aligned branch's aux_model
        crops = fw.get_crop_face_from_affine_matrices(x0[ff], SMATS, face_size=(S, S))
        crops_t = fw.get_crop_face_from_affine_matrices(img[ff], SMATS, face_size=(S, S))
        inv_f, inv_m = fw.inverse_faces(_aux(crops, t, crops_t), SMATS, parser.maps.numpy())
        v = x0.clone()
        for k, fr in enumerate(ff):
            v[fr] = fw.blend(v[fr], inv_f[k], inv_m[k])
        assert torch.equal(v[1], x0[1])
        return v
    tab = odiff.Spaced(odiff.spaced_steps(1000, "10"), odiff.named_betas("face_blur", 1000))
    ref, calls = [], []

    class Stop(Exception):
        pass

    def omodel(x, t, **kw):
        if len(calls) == 2:
            raise Stop()
        calls.append(1)
        return toy_model(x, t, **kw)
    try:
        odiff.sample_loop(tab, omodel, x_T, model_kwargs=dict(num_frames=3), aux_model=oracle_prior, w=0.5, tau=2, rho=0.25,
                          step_noise=tape + tape, trace=ref)
    except Stop:
        pass
    assert len(ref) == 2
    # the oracle loop ramps w over [tau, start]; p_sample is called directly here, so take the loop (same ramp) on the GPU
    from flair_amd import workload as wl
    helper = _helper(dev, S, face_parse=parser)
    gen = wl.diffusion_for(10).p_sample_loop_progressive(
        _M(x_T.to(dev)), x_T.shape, noise=x_T.to(dev), model_kwargs=dict(num_frames=3), device=dev, aux_model=_aux, w=0.5,
        tau=2, aligned=False, rho=0.25, face_restore_helper=helper, affine_matrices=SMATS, face_frames=ff,
        noise_fn=lambda it, like: tape[it].to(dev))
    for (ti, x0r, sr) in ref:
        out = next(gen)
        assert int(out["t"][0]) == ti
        e0 = (out["pred_xstart"].cpu() - x0r).abs().max().item()
        e1 = (out["sample"].cpu() - sr).abs().max().item()
        print(f"step {ti}: x0 max|err| = {e0:.3e}, sample max|err| = {e1:.3e} (|sample| <= {sr.abs().max().item():.2f})")
        assert e0 <= 2.2e-4, (ti, e0)
        assert e1 <= 5.2e-4 * max(1.0, sr.abs().max().item()), (ti, e1)


def test_sampler_no_faces_is_the_prior_off_and_one_per_frame_is_the_old_branch(dev):
    parser = StubParser(3, S, dev)
    helper = _helper(dev, S, face_parse=parser)
    x_T, tape = _tape()
    off = _steps(dev, x_T, tape, aux_model=None)
    none = _steps(dev, x_T, tape, aux_model=_aux, aligned=False, face_restore_helper=helper, affine_matrices=[], face_frames=[])
    for (a0, a1), (b0, b1) in zip(off, none):
        assert torch.equal(a0, b0) and torch.equal(a1, b1)
    old = _steps(dev, x_T, tape, aux_model=_aux, aligned=False, face_restore_helper=helper, affine_matrices=SMATS)
    new = _steps(dev, x_T, tape, aux_model=_aux, aligned=False, face_restore_helper=helper, affine_matrices=SMATS,
                 face_frames=[0, 1, 2])
    for (a0, a1), (b0, b1) in zip(old, new):
        assert torch.equal(a0, b0) and torch.equal(a1, b1)
    assert not torch.equal(old[1][1], off[1][1])              # the prior did something
    with pytest.raises(ValueError, match="one entry per affine matrix"):
        _steps(dev, x_T, tape, aux_model=_aux, aligned=False, face_restore_helper=helper, affine_matrices=SMATS, face_frames=[0, 1])
    with pytest.raises(ValueError, match=r"in \[0, 3\)"):
        _steps(dev, x_T, tape, aux_model=_aux, aligned=False, face_restore_helper=helper, affine_matrices=SMATS, face_frames=[0, 1, 3])


# ------------------------------------------------------------------------------------------------------ window loop
_TPL = np.array([[192.98138, 239.94708], [318.90277, 240.1936], [256.63416, 314.01935], [201.26117, 371.41043],
                 [313.08905, 371.15118]])


def _face(cx, cy, size, score):
    lm = (_TPL / 512.0 - 0.5) * size + np.array([cx, cy])
    return np.concatenate([[cx - size / 2, cy - size / 2, cx + size / 2, cy + size / 2, score], lm.reshape(-1)]).astype(np.float32)


SMALL, BIG, MID = _face(16.0, 18.0, 14.0, 0.99), _face(36.0, 32.0, 36.0, 0.9), _face(30.0, 34.0, 26.0, 0.8)


class StubDetector:
    """batched_detect_faces with a fixed list of detections per frame of the window; frames with none are skipped unless
    keep_empty.  A call on other batches (window_faces probes single frames to name the faceless ones) finds its frames by
    their content."""

    def __init__(self, per_frame):
        self.per_frame, self.calls, self.by_content = per_frame, [], {}

    def batched_detect_faces(self, frames, conf_threshold=0.8, nms_threshold=0.4, use_origin_size=True, pre=None,
                             keep_empty=False):
        assert conf_threshold == 0.5 and pre == (127.5, 127.5, 0.0, 255.0)
        keys = [round(frames[k].double().sum().item(), 4) for k in range(frames.shape[0])]
        if len(keys) == len(self.per_frame):
            self.calls.append(keep_empty)
            self.by_content = dict(zip(keys, self.per_frame))
        out = [np.stack(self.by_content[k]) if self.by_content[k] else np.zeros((0, 15), dtype=np.float32) for k in keys]
        return out if keep_empty else [d for d in out if len(d)]


def _frame_model(x, t, **kw):                                  # no coupling between the frames of a window
    lr = kw["low_res_input"][0]
    eps = 0.3 * x - 0.2 * lr + 0.01 * t.view(-1, 1, 1, 1).float() / 50.0
    return torch.cat([eps, 0.1 * x], 1)


class _W:
    def __init__(self, like):
        self.like = like

    def parameters(self):
        return iter([self.like])

    def __call__(self, x, t, **kw):
        return _frame_model(x, t, **kw)


def _window(dev, helper, **kw):
    from flair_amd import video
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion import pseudoSR as psr
    g = torch.Generator().manual_seed(5)
    degraded = torch.rand(1, 3, 3, 16, 16, generator=g).to(dev)
    tape = [torch.randn(3, 3, S, S, generator=g).to(dev) for _ in range(2)]
    qn = torch.randn(3, 3, S, S, generator=g).to(dev)
    A = psr.pseudoSR(psr.Get_pseudoSR_Conf(4), upscale_kernel=wl.synthetic_blur_kernel(), kernel_indx=10).WrapArchitecture_PyTorch().to(dev)
    out = video.restore_video("gaussian", degraded, _W(degraded), wl.diffusion_for(2),
                              lambda d_n: (lambda x0: A.A_pinv(d_n[0].contiguous(), x0)), size=S, tau=0, length=3, overlap=1,
                              noise_fn=lambda wi, it, like: tape[it], q_noise_fn=lambda wi, like: qn, face_helper=helper, **kw)
    torch.cuda.synchronize()
    return out


def test_window_with_two_none_and_one_face(dev):
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion.retinaface_utils import estimate_affine_partial
    det = StubDetector([[SMALL, BIG], [], [MID]])
    helper = _helper(dev, S, face_det=det, face_parse=StubParser(3, S, dev))
    seen = []
    paste = helper.paste_faces

    def spy(x0, restored, mats, frames):
        seen.append((restored.shape[0], [np.array(m) for m in mats], list(frames)))
        return paste(x0, restored, mats, frames)
    helper.paste_faces = spy
    got = _window(dev, helper, aux_model=_aux, aligned=False, faces="all")
    assert det.calls == [True] and len(seen) == 2             # one detection pass, the paste in both steps
    tpl = _TPL * (S / 512.0)
    want = [estimate_affine_partial(d[5:15].reshape(5, 2), tpl) for d in (BIG, SMALL, MID)]      # largest first
    for n, mats, frames in seen:
        assert n == 3 and frames == [0, 0, 2] and all(np.array_equal(a, b) for a, b in zip(mats, want))
    # frames are independent in this window (model and restore_fn act per frame), so the frame without a face is the frame
    # of a run whose prior returns x0 itself, bit for bit, and the two frames with faces are not
    plain = _window(dev, helper, aux_model=wl.identity_aux, aligned=True)
    assert got.shape == plain.shape == (3, 3, S, S)
    assert torch.equal(got[1], plain[1])
    assert (got[0] - plain[0]).abs().max().item() > 1e-3 and (got[2] - plain[2]).abs().max().item() > 1e-3
    # the cap: one face per frame leaves the small face of frame 0 out
    seen.clear()
    _window(dev, helper, aux_model=_aux, aligned=False, faces="all", max_faces=1)
    assert [s[2] for s in seen] == [[0, 2]] * 2
    # the default mode still refuses this window
    with pytest.raises(ValueError, match=r"window 0 \(frames 0\.\.2\) has no face in frame\(s\) \[1\]"):
        _window(dev, helper, aux_model=_aux, aligned=False)
    # a window without any face runs with the prior off
    det.per_frame = [[], [], []]
    seen.clear()
    empty = _window(dev, helper, aux_model=_aux, aligned=False, faces="all")
    assert not seen and empty.shape == (3, 3, S, S) and torch.isfinite(empty).all()


def test_all_with_one_face_per_frame_is_largest(dev):
    det = StubDetector([[SMALL, BIG], [MID], [BIG, MID, SMALL]])
    helper = _helper(dev, S, face_det=det, face_parse=StubParser(6, S, dev))
    largest = _window(dev, helper, aux_model=_aux, aligned=False)
    capped = _window(dev, helper, aux_model=_aux, aligned=False, faces="all", max_faces=1)
    assert det.calls == [False, True]
    assert torch.equal(largest, capped)
    every = _window(dev, helper, aux_model=_aux, aligned=False, faces="all")
    assert not torch.equal(every[0], largest[0])             # the second face of frame 0 is pasted too
