"""Tiled denoising on the GPU: the gather against torch slicing byte for byte, the blend per element against the float64
definition of tests/tile_ref.py at the bound its operation count gives, TiledModel on the small UNet against the same model run
eagerly on every torch-sliced crop, and the tiled window loop against the oracle loop around a model tiled by tests/tile_ref.py."""
import numpy as np
import pytest
import torch

from tests import tile_ref as R

pytestmark = pytest.mark.gpu

GUARD = 1024.0                     # a value no input holds


def _plan(H, W, th, tw, p, g):
    return R.plan_axis(H, th, p, g), R.plan_axis(W, tw, p, g)


def _guarded(dev, shape, offset, fill=None):
    """A dense view of ``shape`` that starts ``offset`` floats into a buffer of GUARD values (offset 1: a 4-byte aligned base
    that is not 16-byte aligned), and the buffer."""
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), GUARD, device=dev)
    view = buf[offset:offset + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return view, buf


def _guards_intact(buf, offset, n):
    return bool((buf[:offset] == GUARD).all()) and bool((buf[offset + n:] == GUARD).all())


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("C", [1, 3, 6])
@pytest.mark.parametrize("H,W,th,tw,p", [(44, 60, 32, 32, 8), (40, 116, 32, 64, 16)])
def test_gather_is_torch_slicing_byte_for_byte(dev, H, W, th, tw, p, C):
    from flair_amd import ops
    oy, ox = _plan(H, W, th, tw, p, 4)
    frame = torch.randn(2, C, H, W, generator=torch.Generator().manual_seed(H + C))
    want = torch.from_numpy(R.gather(frame.numpy(), oy, ox, th, tw))
    got = ops.tile_gather(frame.to(dev), oy, ox, (th, tw))
    assert got.shape == want.shape == (len(oy) * len(ox) * 2, C, th, tw)
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    # a frame view with a misaligned base between guards, into a misaligned output between guards
    view, _ = _guarded(dev, frame.shape, 1, frame.to(dev))
    out, obuf = _guarded(dev, want.shape, 3)
    ops.tile_gather(view, oy, ox, (th, tw), out=out)
    assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32)) and _guards_intact(obuf, 3, want.numel())


def test_gather_odd_sizes_take_the_scalar_path(dev):
    """W, tw and the origins no multiple of 4: no row is 16-byte aligned."""
    from flair_amd import ops
    frame = torch.randn(3, 2, 45, 61, generator=torch.Generator().manual_seed(2))
    oy, ox = [0, 13], [0, 11, 28]
    got = ops.tile_gather(frame.to(dev), oy, ox, (32, 33))
    assert torch.equal(got.cpu(), torch.from_numpy(R.gather(frame.numpy(), oy, ox, 32, 33)))


# ------------------------------------------------------------------------------------------------ blend
# (H, W, th, tw, ramp, g): 2 x 3 tiles with triple cover in W; 3 x 3 with triple cover on both axes (nine tiles on a pixel); a second
# tile inside the frame border's first pixels (where a ramped border would show); odd everything (scalar path); 16-aligned all
BLENDS = [(44, 60, 32, 32, 8, 4), (116, 116, 64, 64, 16, 4), (36, 60, 32, 32, 8, 4), (45, 61, 32, 33, 7, 1), (64, 96, 32, 64, 16, 16)]
_blend_cases = {}


def _blend_case(case):
    """Random tiles of one plan, the float64 reference, its magnitude and cover: computed once, shared, never changed."""
    if case not in _blend_cases:
        H, W, th, tw, p, g = case
        oy, ox = _plan(H, W, th, tw, p, g)
        N, C = 2, 3
        tiles = torch.randn(len(oy) * len(ox) * N, C, th, tw, generator=torch.Generator().manual_seed(H * W))
        ref, mag, cover = R.blend(tiles.numpy(), H, W, oy, ox, p)
        _blend_cases[case] = (oy, ox, tiles, ref, mag, cover)
    return _blend_cases[case]


def _worst_ratio(got, ref, mag, cover):
    err, bound = np.abs(got.double().cpu().numpy() - ref), R.bound(mag, cover)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max())


@pytest.mark.parametrize("case", BLENDS, ids=lambda c: "x".join(map(str, c)))
def test_blend_per_element_against_the_float64_definition(dev, case):
    """|error| <= (k + 2) 2^-24 sum w^ |v| for k covering tiles, bit exact under one tile, the same bits in two runs and on a
    misaligned base between guards."""
    from flair_amd import ops
    H, W, th, tw, p, g = case
    oy, ox, tiles, ref, mag, cover = _blend_case(case)
    got = ops.tile_blend(tiles.to(dev), oy, ox, (H, W), p)
    ratio = _worst_ratio(got, ref, mag, cover)
    print(f"blend {case}: up to {cover.max()} tiles on a pixel, worst |error| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    single = torch.from_numpy(cover == 1).expand(2, 3, H, W)
    assert single.any() and torch.equal(got.cpu()[single].view(torch.int32), torch.from_numpy(ref).float()[single].view(torch.int32))
    again = ops.tile_blend(tiles.to(dev), oy, ox, (H, W), p)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    view, _ = _guarded(dev, tiles.shape, 1, tiles.to(dev))
    out, obuf = _guarded(dev, got.shape, 2)
    ops.tile_blend(view, oy, ox, (H, W), p, out=out)
    assert torch.equal(out.view(torch.int32), got.view(torch.int32)) and _guards_intact(obuf, 2, got.numel())


def test_blend_is_exact_on_integers_with_dyadic_weights(dev):
    """56 = 32 + 24 with ramp 8: the two tiles of an axis overlap in exactly the ramp, their weights (p + 0.5) / 8 are
    sixteenths that sum to one, and integers up to 100 times 1/256 are exact in f32: the blend must equal the float64 one."""
    from flair_amd import ops
    H = W = 56
    oy, ox = _plan(H, W, 32, 32, 8, 4)
    assert oy == ox == [0, 24]
    tiles = torch.randint(-100, 101, (4 * 2, 3, 32, 32), generator=torch.Generator().manual_seed(9)).float()
    ref, _, cover = R.blend(tiles.numpy(), H, W, oy, ox, 8)
    w, _ = R.weights(H, W, 32, 32, oy, ox, 8)
    assert cover.max() == 4 and np.array_equal(w.sum(0), np.ones((H, W))) and np.array_equal(ref, ref.astype(np.float32))
    got = ops.tile_blend(tiles.to(dev), oy, ox, (H, W), 8)
    assert torch.equal(got.cpu(), torch.from_numpy(ref).float())


@pytest.mark.parametrize("C", [1, 6, 11])
def test_blend_of_one_tile_is_a_copy_and_gather_then_blend_is_the_frame(dev, C):
    """A 1 x 1 grid (the tile is the frame) is a pure copy, signed zeros included; gather followed by blend (an identity model)
    gives the frame back within the bound, for channel counts on both sides of the kernel's register chunk of 8."""
    from flair_amd import ops
    frame = torch.randn(2, C, 32, 48, generator=torch.Generator().manual_seed(C))
    frame[0, 0, 0, :4] = torch.tensor([0.0, -0.0, 1.0, -1.0])
    one = ops.tile_blend(frame.to(dev), [0], [0], (32, 48), 8)
    assert torch.equal(one.cpu().view(torch.int32), frame.view(torch.int32))
    assert torch.equal(ops.tile_gather(frame.to(dev), [0], [0], (32, 48)).cpu().view(torch.int32), frame.view(torch.int32))
    H, W, th, tw, p = 40, 116, 32, 64, 16
    oy, ox = _plan(H, W, th, tw, p, 4)
    frame = torch.randn(2, C, H, W, generator=torch.Generator().manual_seed(C + 1))
    tiles = ops.tile_gather(frame.to(dev), oy, ox, (th, tw))
    ref, mag, cover = R.blend(tiles.cpu().numpy(), H, W, oy, ox, p)
    assert np.abs(ref - frame.double().numpy()).max() <= 1e-14
    ratio = _worst_ratio(ops.tile_blend(tiles, oy, ox, (H, W), p), frame.double().numpy(), mag, cover)
    print(f"gather -> blend, C = {C}: worst |error| / bound = {ratio:.3f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ TiledModel
T, FH, FW, TILE, OVERLAP = 2, 44, 60, 32, 8
_unet = {}


def _small_unet(dev, width=32):
    if width not in _unet:
        from tests.test_gpu_rect import hip_unet, rect_oracle
        from tests.test_gpu_unet import SMALL
        cfg = dict(SMALL, image_size=width)
        _unet[width] = hip_unet(cfg, rect_oracle(cfg).state_dict()).to(dev)
    return _unet[width]


def _unet_inputs(H, W, seed):
    from tests.test_gpu_rect import unet_inputs
    x, lr, _ = unet_inputs(T, H, W, seed=seed)
    _, rnn, _ = unet_inputs(T, H, W, seed=seed + 100)
    return x, lr, rnn, torch.tensor([371, 12], dtype=torch.long)          # a timestep per frame: a wrong repeat would show


def test_tiled_model_is_the_model_on_every_crop_blended(dev):
    """f32, T = 2, 44 x 60 with 32 x 32 tiles and overlap 8: 2 x 3 tiles, triple cover in W.  The reference runs the same
    model eagerly on every torch-sliced crop of x, low_res_input and rnn_input and blends in float64; then one hipGraph per
    tile, and two steps of replay bit-identical to eager."""
    from flair_amd import tiling
    m = _small_unet(dev)
    plan = tiling.make_plan((FH, FW), (TILE, TILE), OVERLAP, 4)
    assert (plan.oy, plan.ox) == ([0, 12], [0, 12, 28])
    tm = tiling.TiledModel(m, plan)
    assert tm.model is m and tm.dtype == m.dtype and next(tm.parameters()) is next(m.parameters())
    steps, eager = [_unet_inputs(FH, FW, 3), _unet_inputs(FH, FW, 4)], []
    lr, rnn = steps[0][1].to(dev), steps[0][2].to(dev)                     # one conditioning clip for both steps
    for x, _, _, t in steps:
        crops = []
        for a, b in plan.origins():
            cut = lambda v: v[..., a:a + TILE, b:b + TILE].contiguous()    # noqa: E731
            crops.append(m(cut(x.to(dev)), t.to(dev), low_res_input=cut(lr), rnn_input=cut(rnn), num_frames=T, vsrpp_weights=1.0).cpu())
        ref, mag, cover = R.blend(torch.cat(crops).numpy(), FH, FW, plan.oy, plan.ox, OVERLAP)
        got = tm(x.to(dev), t.to(dev), low_res_input=lr, rnn_input=rnn, num_frames=T, vsrpp_weights=1.0)
        torch.cuda.synchronize()
        ratio = _worst_ratio(got, ref, mag, cover)
        print(f"TiledModel {FH}x{FW}: worst |error| / blend bound = {ratio:.3f}")
        assert got.shape == (T, 6, FH, FW) and ratio <= 1.0
        eager.append(got.clone())
    assert m._flow_cache_limit == 16                                       # six tiles: the bound of before
    assert not torch.equal(eager[0], eager[1])
    tm.enable_hip_graph()
    graphs = []
    for (x, _, _, t), want in zip(steps, eager):
        got = tm(x.to(dev), t.to(dev), low_res_input=lr, rnn_input=rnn, num_frames=T, vsrpp_weights=1.0)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert len(m._graphs) == plan.n_tiles == 6 and sorted(k[-1] for k in m._graphs) == list(range(6))
        graphs.append([m._graphs[k]["graph"] for k in sorted(m._graphs, key=lambda k: k[-1])])
    assert all(a is b for a, b in zip(*graphs))                            # the second step replayed: nothing was captured again
    # more tile clips than graph_tiles: the first four replay graphs, the other two are launched eagerly, said once, same bits
    few = tiling.TiledModel(m, plan, graph_tiles=4).enable_hip_graph()
    (x, _, _, t), want = steps[0], eager[0]
    with pytest.warns(UserWarning, match="6 tile clips; the first 4 replay captured hipGraphs"):
        got = few(x.to(dev), t.to(dev), low_res_input=lr, rnn_input=rnn, num_frames=T, vsrpp_weights=1.0)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and sorted(k[-1] for k in m._graphs) == [0, 1, 2, 3]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        again = few(x.to(dev), t.to(dev), low_res_input=lr, rnn_input=rnn, num_frames=T, vsrpp_weights=1.0)
    torch.cuda.synchronize()
    assert torch.equal(again.view(torch.int32), want.view(torch.int32)) and m._graph_clip_limit is None
    tm.enable_hip_graph(False)


def test_tiled_model_with_one_tile_is_the_model(dev):
    from flair_amd import tiling
    m = _small_unet(dev, 48)
    x, lr, rnn, t = (v.to(dev) for v in _unet_inputs(32, 48, 5))
    want = m(x, t, low_res_input=lr, rnn_input=rnn, num_frames=T, vsrpp_weights=1.0).clone()
    tm = tiling.TiledModel(m, tiling.make_plan((32, 48), (32, 48), OVERLAP, 4))
    got = tm(x, t, low_res_input=lr, rnn_input=rnn, num_frames=T, vsrpp_weights=1.0)
    torch.cuda.synchronize()
    assert tm.plan.n_tiles == 1 and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_tiled_model_raises_the_flow_cache_bound_and_cuts_weight_maps(dev):
    """More tiles than the flow cache's 16 entries: the wrapper raises the bound for the inner call and puts it back; a per-pixel weight map
    on the low-resolution grid is cut into the tiles' crops; vsrpp_weights_fn sees every tile's init frames."""
    from flair_amd import tiling

    class Inner:
        _flow_cache_limit, dtype = 16, torch.float32

        def __call__(self, x, t, **kw):
            self.seen = dict(kw, x=x, t=t, bound=self._flow_cache_limit)
            return x * 2.0

    inner = Inner()
    plan = tiling.make_plan((64, 64), (16, 16), 4, 4)
    assert plan.n_tiles == 25
    tm = tiling.TiledModel(inner, plan)
    x = torch.randn(T, 3, 64, 64, device=dev)
    lr = torch.randn(1, T, 3, 64, 64, device=dev)
    vw = torch.rand(1, T, 1, 16, 16, device=dev)
    out = tm(x, torch.tensor([5, 7], device=dev), low_res_input=lr, num_frames=T, vsrpp_weights=vw)
    assert inner.seen["bound"] == 25 and inner._flow_cache_limit == 16 and inner.seen["rnn_input"] is None     # raised for the call only
    assert torch.equal(inner.seen["t"].cpu(), torch.tensor([5, 7] * 25))
    k = 7                                                                  # tile (1, 2)
    a, b = plan.origins()[k]
    assert torch.equal(inner.seen["x"][k * T:(k + 1) * T], x[..., a:a + 16, b:b + 16])
    assert torch.equal(inner.seen["low_res_input"][k], lr[0, ..., a:a + 16, b:b + 16])
    assert torch.equal(inner.seen["vsrpp_weights"][k], vw[0, ..., a // 4:a // 4 + 4, b // 4:b // 4 + 4])
    ref, mag, cover = R.blend((inner.seen["x"] * 2.0).cpu().numpy(), 64, 64, plan.oy, plan.ox, 4)
    assert _worst_ratio(out, ref, mag, cover) <= 1.0
    calls = []
    tm = tiling.TiledModel(inner, plan, vsrpp_weights_fn=lambda init: calls.append(init) or init[:, :, :1] * 0.5)
    tm(x, torch.tensor([5, 7], device=dev), low_res_input=lr, num_frames=T, vsrpp_weights=None)
    assert len(calls) == 25 and torch.equal(calls[k][0], lr[0, ..., a:a + 16, b:b + 16])
    assert torch.equal(inner.seen["vsrpp_weights"][k], lr[0, :, :1, a:a + 16, b:b + 16] * 0.5)


# ------------------------------------------------------------------------------------------------ the window loop
class _Clips:
    """The stub network of tests/test_gpu_unaligned_video.py for a batch of clips: ``fn`` on every clip of ``num_frames`` frames
    with that clip's conditioning.  Counts its calls."""

    def __init__(self, like, fn):
        self.like, self.fn, self.calls = like, fn, 0

    def parameters(self):
        return iter([self.like])

    def __call__(self, x, t, **kw):
        self.calls += 1
        n = int(kw["num_frames"])
        outs = []
        for b in range(x.shape[0] // n):
            k = dict(kw, low_res_input=kw["low_res_input"][b:b + 1])
            if kw.get("rnn_input") is not None:
                k["rnn_input"] = kw["rnn_input"][b:b + 1]
            outs.append(self.fn(x[b * n:(b + 1) * n], t[b * n:(b + 1) * n], **k))
        return torch.cat(outs)


def _positional(x, t, **kw):
    """The toy model plus a pattern fixed to the TILE's own pixel grid: a wrong origin or weight moves it."""
    from tests.test_gpu_unaligned_video import _toy_model
    h, w = x.shape[-2:]
    ramp = 0.01 * torch.arange(h, device=x.device, dtype=x.dtype)[:, None] + 0.003 * torch.arange(w, device=x.device, dtype=x.dtype)[None, :]
    return _toy_model(x, t, **kw) + ramp


@pytest.mark.parametrize("positional", [False, True], ids=["toy", "tile_local"])
def test_tiled_window_loop_vs_oracle_loop_around_a_tiled_model(dev, positional):
    """restore_video(size=(44, 60), tile=(32, 32), tile_overlap=8) with the tapes and the stub model of
    test_window_loop_rect_aligned_vs_oracle_loop, against the oracle loop whose model is that stub tiled by tests/tile_ref.py, at
    that test's 2e-3.  44 x 60 is refused whole (check_frame_size), with and without the feature."""
    from flair_amd import pipeline as pl
    from flair_amd import video
    from flair_amd import workload as wl
    from tests.test_gpu_rect import _oracle_windows, _tapes
    from tests.test_gpu_unaligned_video import _blur_op, _toy_model
    N, H, W, L, OV, steps, tau = 4, FH, FW, 3, 1, 2, 0
    fn = _positional if positional else _toy_model
    degraded, wins, tapes, qnoise = _tapes(N, H // 4, W // 4, H, W, L, OV, steps, 31)
    oy, ox = _plan(H, W, TILE, TILE, OVERLAP, 4)
    ref = _oracle_windows(degraded, wins, tapes, qnoise, H, W, OV, steps, tau, R.tiled(fn, H, W, TILE, TILE, oy, ox, OVERLAP), None)
    m = _Clips(degraded.to(dev), fn)
    common = dict(tau=tau, length=L, overlap=OV, noise_fn=lambda wi, it, like: tapes[wi][it].to(dev),
                  q_noise_fn=lambda wi, like: qnoise[wi].to(dev))
    got = video.restore_video("gaussian", degraded.to(dev), m, wl.diffusion_for(steps), _blur_op(dev), size=(H, W), tile=(TILE, TILE),
                              tile_overlap=OVERLAP, **common)
    torch.cuda.synchronize()
    assert got.shape == ref.shape == (N, 3, H, W) and m.calls == steps * len(wins)
    for i in range(N):
        err = (got[i].cpu() - ref[i]).abs().max().item()
        print(f"tiled window loop {H}x{W}, frame {i}: max|err| = {err:.3e}")
        assert err <= 2e-3, (i, err)
    if positional:                                                         # the pattern is there: the untiled stub differs
        plain = video.restore_video("gaussian", degraded.to(dev), _Clips(degraded.to(dev), _toy_model), wl.diffusion_for(steps), _blur_op(dev),
                                    size=(H, W), tile=(TILE, TILE), tile_overlap=OVERLAP, **common)
        assert (plain - got).abs().max().item() > 1e-2
    with pytest.raises(ValueError, match=r"gaussian: frame size 44x60 is not valid: H and W must be multiples of 64"):
        pl.check_frame_size("gaussian", (H, W))
    with pytest.raises(ValueError, match=r"frame size 44x60 is not valid"):
        pl.build_pipeline("gaussian", "/nonexistent", device=dev, size=(H, W), tile=None)
    m = _Clips(degraded.to(dev), fn)
    with pytest.raises(ValueError, match="smaller than one tile of 64x64"):
        video.restore_video("gaussian", degraded.to(dev), m, wl.diffusion_for(steps), _blur_op(dev), size=(H, W), tile=(64, 64), **common)
    assert m.calls == 0
