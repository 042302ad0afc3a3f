"""Whole-UNet parity: flair_amd UNetModel (HIP, through the C ABI) vs the CPU oracle."""
import pytest
import torch

from tests.util import from_clip

SMALL = dict(image_size=32, in_channels=6, model_channels=128, out_channels=6, num_res_blocks=1,
             attention_resolutions=(2, 4), rnn_resolutions=(1, 2), channel_mult=(0.5, 1, 4),
             use_fp16=False, num_head_channels=64, resblock_updown=True, use_scale_shift_norm=True,
             temporal_block=True, use_checkpoint=False)


def build_pair(cfg, seed=0):
    from oracle.unet import UNetModel as Oracle
    from flair_amd.guided_diffusion.unet_new import UNetModel
    torch.manual_seed(seed)
    o = Oracle(**cfg)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in o.parameters():            # zero-initialised modules would hide whole branches
            if p.abs().sum() == 0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    m = UNetModel(**cfg)
    missing = m.load_state_dict(o.state_dict(), strict=True)
    return o.eval(), m.eval()


def test_state_dict_names_match_oracle():
    """CPU: the HIP model exposes exactly the reference's parameter names/shapes
    (the oracle's names are pinned against the reference in tests/golden)."""
    o, m = build_pair(SMALL)
    so, sm = o.state_dict(), m.state_dict()
    assert list(so.keys()) == list(sm.keys())
    assert all(so[k].shape == sm[k].shape for k in so)


def test_cpu_tensors_are_refused():
    from flair_amd.guided_diffusion.unet_new import UNetModel
    m = UNetModel(**SMALL)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.long), low_res_input=torch.zeros(1, 2, 3, 32, 32),
          num_frames=2)


def _inputs(T, S, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, 3, S, S, generator=g)
    base = torch.rand(1, 1, 3, S, S, generator=g) * 2 - 1
    # frames = slowly shifting copies + noise, so that SPyNet sees real motion
    lr = torch.stack([torch.roll(base[0, 0], shifts=(i, 2 * i), dims=(1, 2)) for i in range(T)])[None]
    lr = (lr + 0.05 * torch.randn(1, T, 3, S, S, generator=g)).clamp(-1, 1)
    t = torch.full((T,), 371, dtype=torch.long)
    return x, lr, t


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unet_small_vs_oracle(dev, dtype):
    o, m = build_pair(SMALL)
    T, S = 4, 32
    x, lr, t = _inputs(T, S)
    stages = []

    def hook(name):
        def f(mod, inp, out):
            stages.append((name, out.detach()))
        return f
    for i, b in enumerate(o.input_blocks):
        b.register_forward_hook(hook(f"input_blocks.{i}"))
    o.middle_block.register_forward_hook(hook("middle_block"))
    for i, b in enumerate(o.output_blocks):
        b.register_forward_hook(hook(f"output_blocks.{i}"))
    with torch.no_grad():
        ref = o(x, t, low_res_input=lr, num_frames=T, vsrpp_weights=1.0)
    m = m.to(dev)
    if dtype == torch.bfloat16:
        m.convert_to_fp16()
    m._trace = []
    y = m(x.to(dev), t.to(dev), low_res_input=lr.to(dev), num_frames=T, vsrpp_weights=1.0)
    torch.cuda.synchronize()
    # stated tolerance: f32 kernels 2e-4 of the stage's max magnitude (deep net, accumulation
    # order + fp16-emulating temporal attention); bf16 5e-2 (end-to-end drift of bf16 storage).
    rel = 2e-4 if dtype == torch.float32 else 5e-2
    report = []
    for (n1, a), (n2, b) in zip(stages, m._trace):
        assert n1 == n2
        a4 = a[0].float()                         # (T,C,H,W)
        e = (from_clip(b) - a4).abs().max().item() / (a4.abs().max().item() + 1e-12)
        report.append((n1, e))
    bad = [r for r in report if r[1] > rel]
    assert not bad, f"stages beyond {rel}: {bad[:4]} (all: {report})"
    err = (y.cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err <= rel, (err, report)


@pytest.mark.gpu
def test_unet_flows_vs_oracle(dev):
    """SPyNet + bicubic flow-input resize (once-per-clip part) against the oracle, f32."""
    o, m = build_pair(SMALL)
    T, S = 3, 64
    _, lr, _ = _inputs(T, S, seed=8)
    with torch.no_grad():
        ff, fb = o.compute_flow(lr)
    m = m.to(dev)
    m._ensure_packed(dev)
    gf, gb = m.compute_flow(lr[0].to(dev))
    torch.cuda.synchronize()
    for got, ref in ((gf, ff), (gb, fb)):
        ref = ref[0].permute(0, 2, 3, 1)
        err = (got.cpu() - ref).abs().max().item()
        assert err <= 2e-4 * max(1.0, ref.abs().max().item()), err


@pytest.mark.gpu
def test_spynet_pair_flows(dev):
    """SPyNet.pair_flows: a single frame has no neighbour (two empty stacks); on three frames it is what
    compute_flow returns, bit for bit."""
    _, m = build_pair(SMALL)
    m = m.to(dev)
    m._ensure_packed(dev)
    S = 32
    for T in (1, 3):
        lr = _inputs(T, S, seed=8)[1][0].to(dev)
        raw = torch.zeros((T, S, S, 4), dtype=torch.float32, device=dev)
        raw[..., :3] = lr.permute(0, 2, 3, 1)
        got = m.spynet.pair_flows(raw)
        want = m.compute_flow(lr)
        torch.cuda.synchronize()
        for g, w in zip(got, want):
            assert g.shape == (T - 1, S, S, 2) and g.dtype == torch.float32
            assert torch.equal(g, w)


@pytest.mark.gpu
@pytest.mark.parametrize("tensor_weights", [False, True])
def test_hip_graph_replay_matches_eager(dev, tensor_weights):
    """enable_hip_graph(): the captured forward replays bit-identically to eager launches, for new
    latents / timesteps, after the conditioning clip changes (flows recomputed into the same buffers), and with a
    per-pixel propagation-weight map (a static input of the graph: a new map tensor re-captures)."""
    _, m = build_pair(SMALL)
    m = m.to(dev)
    m.convert_to_fp16()
    T, S = 4, 32
    g = torch.Generator().manual_seed(2)
    wmap = (0.9 + 0.1 * torch.rand(1, T, 1, S, S, generator=g)).to(dev) if tensor_weights else 1.0
    wmap2 = (0.9 + 0.1 * torch.rand(1, T, 1, S, S, generator=g)).to(dev) if tensor_weights else 1.0
    cases, clips = [], {}
    for seed, tval, w in [(3, 371, wmap), (3, 12, wmap), (3, 655, wmap), (8, 940, wmap), (8, 207, wmap2)]:
        # the same clip three times, then a new clip, then a new weight map of the same shape
        x, lr, t = _inputs(T, S, seed=seed)
        x = x + 0.01 * tval                                    # a different latent every time
        if seed not in clips:
            clips[seed] = lr.to(dev)                           # ONE device tensor per clip: later calls are pure replays
        cases.append((x.to(dev), clips[seed], torch.full((T,), tval, dtype=torch.long, device=dev), w))
    eager = [m(x, t, low_res_input=lr, num_frames=T, vsrpp_weights=w).clone() for x, lr, t, w in cases]
    m.enable_hip_graph()
    graphs = []
    for (x, lr, t, w), ref in zip(cases, eager):
        y = m(x, t, low_res_input=lr, num_frames=T, vsrpp_weights=w)
        torch.cuda.synchronize()
        assert torch.equal(y, ref)
        assert len(m._graphs) == 1
        graphs.append(next(iter(m._graphs.values()))["graph"])
    # calls 2 and 3 replayed the graph captured by call 1 with new x / t (nothing baked in at capture time);
    # the new clip re-captured; a new map tensor re-captures, the same number replays
    assert graphs[0] is graphs[1] is graphs[2] and graphs[3] is not graphs[0]
    assert (graphs[4] is not graphs[3]) if tensor_weights else (graphs[4] is graphs[3])
    m.enable_hip_graph(False)


@pytest.mark.gpu
def test_two_clips_in_one_call_replay_two_graphs_bit_identically(dev):
    """B = 2 with enable_hip_graph(): each clip of the batch gets its own captured graph (the key carries the clip index; one shared
    entry would be evicted and re-captured by the other clip on every forward), and the batched output equals the two single-clip
    eager forwards bit for bit -- on the capturing call and on pure replays with new latents."""
    _, m = build_pair(SMALL)
    m = m.to(dev)
    m.convert_to_fp16()
    T, S, B = 4, 32, 2
    lrs = [_inputs(T, S, seed=11 + b)[1].to(dev) for b in range(B)]
    lr2 = torch.cat(lrs)                                            # (B, T, 3, S, S): ONE device tensor for the batched calls
    rounds = []
    for r, tval in enumerate((371, 64, 903)):
        xs = [(_inputs(T, S, seed=11 + b)[0] + 0.02 * (r + 1) * (b + 1)).to(dev) for b in range(B)]
        t = torch.full((T,), tval, dtype=torch.long, device=dev)
        single = [m(xs[b], t, low_res_input=lrs[b], num_frames=T, vsrpp_weights=1.0).clone() for b in range(B)]
        rounds.append((torch.cat(xs), torch.cat([t, t]), torch.cat(single)))
    m.enable_hip_graph()
    graphs = []
    for x2, t2, ref in rounds:
        y = m(x2, t2, low_res_input=lr2, num_frames=T, vsrpp_weights=1.0)
        torch.cuda.synchronize()
        assert torch.equal(y, ref)
        assert len(m._graphs) == B
        graphs.append([ent["graph"] for ent in m._graphs.values()])
    assert all(g0 is g1 for g0, g1 in zip(graphs[0], graphs[1])) and all(g0 is g2 for g0, g2 in zip(graphs[0], graphs[2]))
    m.enable_hip_graph(False)


def test_reference_checkpoint_ingest(tmp_path):
    """CPU: a reference-format checkpoint file (fp32 state dict with the reference's keys) loads through the
    safe loader; wrong files are refused."""
    from flair_amd.checkpoint import load_reference_checkpoint
    o, m = build_pair(SMALL, seed=5)
    path = tmp_path / "flair_gaussian.pt"
    torch.save(o.state_dict(), path)
    with torch.no_grad():
        for p in m.parameters():
            p.zero_()
    rep = load_reference_checkpoint(m, str(path))
    assert not rep.missing_keys and not rep.unexpected_keys
    so, sm = o.state_dict(), m.state_dict()
    assert all(torch.equal(so[k], sm[k]) for k in so)
    wrapped = tmp_path / "wrapped.pt"
    torch.save({"params_ema": o.state_dict()}, wrapped)
    load_reference_checkpoint(m, str(wrapped))
    bad = tmp_path / "bad.pt"
    torch.save({"a": 1}, bad)
    with pytest.raises(ValueError):
        load_reference_checkpoint(m, str(bad))


@pytest.mark.gpu
@pytest.mark.parametrize("T,S", [(1, 32), (2, 32), (3, 48), (2, 40)])
def test_unet_edge_shapes_vs_oracle(dev, T, S):
    """Single-frame clip (no propagation), two frames (first-order only), sides that are not a multiple
    of 32 (3x3 convs fall back to the im2col kernel, SPyNet resizes to a multiple of 32): f32 kernels."""
    cfg = dict(SMALL, image_size=S)
    o, m = build_pair(cfg, seed=2)
    x, lr, t = _inputs(T, S, seed=11)
    with torch.no_grad():
        ref = o(x, t, low_res_input=lr, num_frames=T, vsrpp_weights=1.0)
    m = m.to(dev)
    y = m(x.to(dev), t.to(dev), low_res_input=lr.to(dev), num_frames=T, vsrpp_weights=1.0)
    torch.cuda.synchronize()
    err = (y.cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err <= 2e-4, err


@pytest.mark.gpu
def test_unet_call_variants_vs_oracle(dev):
    """Two clips in one call (B=2), per-pixel vsrpp weights, rnn_input different from low_res_input, and
    enable_cross_frames=False: the argument handling of unet_new.py:1311-1362, f32 kernels."""
    o, m = build_pair(SMALL, seed=4)
    m = m.to(dev)
    T, S, B = 3, 32, 2
    xs, lrs, rnns = [], [], []
    for b in range(B):
        x, lr, t = _inputs(T, S, seed=20 + b)
        _, rnn, _ = _inputs(T, S, seed=40 + b)
        xs.append(x); lrs.append(lr); rnns.append(rnn)
    x, lr, rnn = torch.cat(xs), torch.cat(lrs), torch.cat(rnns)
    t = torch.tensor([371] * T + [48] * T)
    g = torch.Generator().manual_seed(1)
    vw = 0.8 + 0.2 * torch.rand(B, T, 1, S, S, generator=g)
    for kw in (dict(vsrpp_weights=vw, rnn_input=rnn), dict(vsrpp_weights=1.0, enable_cross_frames=False)):
        with torch.no_grad():
            ref = o(x, t, low_res_input=lr, num_frames=T, **kw)
        kd = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        y = m(x.to(dev), t.to(dev), low_res_input=lr.to(dev), num_frames=T, **kd)
        torch.cuda.synchronize()
        err = (y.cpu() - ref).abs().max().item() / ref.abs().max().item()
        assert err <= 2e-4, (list(kw), err)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["unet_new", "sr3"])
def test_packed_weight_blob_gives_identical_forward(dev, family):
    """flair_amd.checkpoint.export_packed / import_packed: a model with DIFFERENT fp32 parameters that is handed
    the source model's kernel-native blob (what broadcast_packed_weights ships) computes bit-identical outputs
    without repacking (f3 / section 8e)."""
    from flair_amd import checkpoint
    if family == "unet_new":
        from flair_amd.guided_diffusion.unet_new import UNetModel as Net
        cfg = SMALL
        T, S = 3, 32
        x, lr, t = _inputs(T, S)
        call = lambda m: m(x.to(dev), t.to(dev), low_res_input=lr.to(dev), num_frames=T, vsrpp_weights=1.0)   # noqa: E731
    else:
        from flair_amd.guided_diffusion.sr3 import UNet as Net
        from tests.test_gpu_sr3 import SR3_SMALL as cfg, inputs
        x, lr, level = inputs(T=3, S=64)
        call = lambda m: m(x.to(dev), level.to(dev), low_res_input=lr.to(dev), num_frames=3, vsrpp_weights=0.93)   # noqa: E731
    torch.manual_seed(0)
    a = Net(**cfg).to(dev).eval()
    torch.manual_seed(1)
    b = Net(**cfg).to(dev).eval()
    for m in (a, b):
        with torch.no_grad():
            for p in m.parameters():
                if p.abs().sum() == 0:
                    p.normal_(0, 0.02)
        m.convert_to_fp16()
    ya = call(a)
    assert not torch.equal(ya, call(b))
    meta, blob = checkpoint.export_packed(a)
    checkpoint.import_packed(b, meta, blob.clone())
    yb = call(b)
    torch.cuda.synchronize()
    assert torch.equal(ya, yb)
    masters = sum(p.numel() * 4 for p in a.parameters())
    assert blob.numel() < 0.75 * masters
