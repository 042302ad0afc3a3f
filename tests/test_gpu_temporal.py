"""GPU: the flow-warping error kernels (csrc/temporal.hip, include/flair_temporal.h) and flair_amd.temporal against
tests/temporal_ref.py.

Known answers and dyadic data are compared bit for bit: there every sum is exact in double in any order.  On arbitrary f32
flows the mask is compared on every pixel whose two sides of a test differ by more than 1e-9 relative in the reference (the
kernels do the reference's operations in its order, so it is equal on the others too, but only that is promised), N exactly and
S within 1e-12 relative of the reference's exact sum: S adds non-negative terms in a fixed tree at most 30
additions deep here (8 rows, 6 lane steps, 3 waves, up to 9 tiles), each within 2^-53 relative of its result, so within
30 * 2^-53 < 4e-15.

SPyNet's flows come from flair_conv_nhwc, which picks its K split by launch size: a pair's FLOW may differ in the last bits
between batch sizes, as the ArcFace trunk's embeddings do (tests/test_gpu_ident.py).  Only the two new kernels promise equal
bits, so the end-to-end test evaluates the reference on the GPU's own flows."""
import functools
import json
import re

import numpy as np
import pytest
import torch

from tests import temporal_ref as R

pytestmark = pytest.mark.gpu


def on(dev, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def run(dev, frames, f, g, frames2=None):
    """Both entries on numpy inputs -> (mask (P, H, W) uint8, out (sets, P, 2) float64) as numpy."""
    from flair_amd import ops
    tf = on(dev, f)
    mask = ops.flow_occlusion(tf, on(dev, g))
    out = ops.warp_error(on(dev, frames), tf, mask, a2=on(dev, frames2))
    return mask.cpu().numpy(), out.cpu().numpy()


def assert_close_to_reference(got_mask, got_out, frames, f, g, frames2=None):
    """The comparison on arbitrary flows: the reference alone must leave at most 0.1 % of the pixels undecided; then the mask on
    the decided pixels, N exactly and S within 1e-12 relative."""
    P = f.shape[0]
    occ = [R.occlusion(f[i], g[i]) for i in range(P)]
    decided = np.stack([o["margin"] > 1e-9 for o in occ])
    assert (~decided).mean() <= 1e-3                 # on the reference alone, before the GPU's result is looked at
    want_mask, want = R.batch(frames, f, g, frames2)
    assert np.array_equal(got_mask[decided], want_mask[decided])
    assert got_out.shape == want.shape and np.array_equal(got_out[..., 1], want[..., 1])
    rel = np.abs(got_out[..., 0] - want[..., 0]) / want[..., 0]
    print(f"S within {rel.max():.3e} relative of fsum; kept {want[0, :, 1] / (f.shape[1] * f.shape[2])}")
    assert (want[..., 0] > 0).all() and rel.max() <= 1e-12


# ------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("index", range(5))
def test_known_answers_bit_for_bit(dev, index):
    """Integer shifts at 37 x 70, 1 x 40 and 40 x 1 (mask = inside, S = 0, one changed byte of the second set gives 49), the
    half-pixel flow that is not occluded, the flow step whose boundary is one column."""
    case = R.known_answers()[index]
    mask, out = run(dev, case["frames"], case["f"], case["g"], case["frames2"])
    assert R.check_known_answer(case, mask, out) == []
    if case["frames2"] is not None:
        assert out[0, 0, 0] == 0.0 and out[1, 0, 0] == 49.0 and out[0, 0, 1] == out[1, 0, 1] == case["N"]


# ------------------------------------------------------------------------------------------- dyadic data
@pytest.mark.parametrize("with_a2", [False, True])
@pytest.mark.parametrize("P", [1, 3])
def test_dyadic_data_bit_for_bit(dev, P, with_a2):
    d = R.dyadic_case(P)
    frames2 = d["frames2"] if with_a2 else None
    want_mask, want = R.batch(d["frames"], d["f"], d["g"], frames2)
    mask, out = run(dev, d["frames"], d["f"], d["g"], frames2)
    assert np.array_equal(mask, want_mask)           # everywhere
    assert out.shape == (2 if with_a2 else 1, P, 2) and np.array_equal(out, want)
    assert (want[..., 0] * 256 == np.round(want[..., 0] * 256)).all() and (want[..., 1] > 700).all()


# ------------------------------------------------------------------------------------------- arbitrary flows
def test_random_flows_against_the_reference(dev):
    d = R.random_case()
    mask, out = run(dev, d["frames"], d["f"], d["g"], d["frames2"])
    assert_close_to_reference(mask, out, d["frames"], d["f"], d["g"], d["frames2"])


@functools.lru_cache(maxsize=None)
def wide_case():
    """70 x 140: three rows and three columns of 32 x 64 tiles, the last of each partial; two pairs."""
    return R.random_case(P=2, H=70, W=140, seed=R.RANDOM_SEED + 1)


def test_a_launch_beyond_one_row_and_column_of_tiles_and_odd_addresses(dev):
    from flair_amd import ops
    d = wide_case()
    mask, out = run(dev, d["frames"], d["f"], d["g"], d["frames2"])
    assert_close_to_reference(mask, out, d["frames"], d["f"], d["g"], d["frames2"])
    # the frames at odd byte addresses: the same bits
    f, m = on(dev, d["f"]), on(dev, mask)
    n = d["frames"].size
    for off, off2 in ((1, 3), (2, 1)):
        hold, hold2 = (torch.full((n + 8,), 0x5A, dtype=torch.uint8, device=dev) for _ in range(2))
        a, a2 = hold[off:off + n].view(d["frames"].shape), hold2[off2:off2 + n].view(d["frames"].shape)
        assert a.data_ptr() % 4 == off and a2.data_ptr() % 4 == off2
        a.copy_(on(dev, d["frames"]))
        a2.copy_(on(dev, d["frames2"]))
        assert np.array_equal(ops.warp_error(a, f, m, a2=a2).cpu().numpy(), out)
        assert int(hold[:off].sum()) == 0x5A * off and int(hold[off + n:].sum()) == 0x5A * (8 - off)


def test_equal_bits_in_every_run_and_at_every_batch_position(dev):
    d = wide_case()
    first = run(dev, d["frames"], d["f"], d["g"], d["frames2"])
    again = run(dev, d["frames"], d["f"], d["g"], d["frames2"])
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    # pair 0 alone (P = 1) and the same pair as pair 2 of P = 3
    r = R.random_case()
    alone = run(dev, r["frames"][:2], r["f"][:1], r["g"][:1], r["frames2"][:2])
    other = R.random_case(seed=R.RANDOM_SEED + 2)
    pad = lambda k: np.concatenate([other[k][:2], r[k][:2]])              # noqa: E731  frames 2 and 3 are the pair's
    flow = lambda k: np.concatenate([other[k][:1], other[k][1:2], r[k][:1]])    # noqa: E731  (pair 1 joins two unrelated frames)
    third = run(dev, pad("frames"), flow("f"), flow("g"), pad("frames2"))
    assert np.array_equal(third[0][2], alone[0][0]) and np.array_equal(third[1][:, 2], alone[1][:, 0])
    assert alone[1][0, 0, 0] != alone[1][1, 0, 0]    # the two sets differ, so the comparison says something


def test_a_mask_that_does_not_fit_the_flow_reads_nothing_outside(dev):
    """A pixel whose mask is set but whose q is outside is left out like a masked one (the header's wording)."""
    from flair_amd import ops
    case = R.known_answers()[0]
    ones = torch.ones(case["mask"].shape, dtype=torch.uint8, device=dev)
    out = ops.warp_error(on(dev, case["frames"]), on(dev, case["f"]), ones).cpu().numpy()
    assert out[0, 0, 0] == 0.0 and out[0, 0, 1] == case["N"]
    nan = case["f"].copy()
    nan[0, 3, 4, 0] = np.nan
    nan[0, 5, 6, 1] = np.inf
    mask = ops.flow_occlusion(on(dev, nan), on(dev, case["g"])).cpu().numpy()
    assert mask[0, 3, 4] == 0 and mask[0, 5, 6] == 0 and set(np.unique(mask)) == {0, 1}


# ------------------------------------------------------------------------------------------- refusals
def test_every_refusal_of_the_header_comes_before_any_launch(dev):
    from flair_amd import _lib, ops
    lib = _lib.lib()
    for name, args, what in R.entry_refusals():
        R.assert_refused(lib, name, args, what)
    torch.cuda.synchronize()                       # nothing was enqueued: the device is as it was
    f = torch.zeros(9, 8, 2, device=dev).view(-1)[1:1 + 2 * 8 * 8].view(1, 8, 8, 2)          # 4 bytes off an 8-byte boundary
    assert f.data_ptr() % 8 == 4
    ok = torch.zeros(1, 8, 8, 2, device=dev)
    with pytest.raises(_lib.FlairHipError, match="flair_flow_occlusion: f = .* and g = .* must be 8-byte aligned"):
        ops.flow_occlusion(f, ok)
    with pytest.raises(_lib.FlairHipError, match="flair_flow_occlusion: f = .* and g = .* must be 8-byte aligned"):
        ops.flow_occlusion(ok, f)
    a, mask = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=dev), torch.ones(1, 8, 8, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.FlairHipError, match="flair_warp_error: f = .* must be 8-byte aligned"):
        ops.warp_error(a, f, mask)
    out = torch.full((1, 1, 2), 7.0, dtype=torch.float64, device=dev)
    ws = torch.zeros(64, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.FlairHipError, match=r"flair_warp_error: ws_bytes = 15, sets \* P \* ceil\(H / FLAIR_WARP_TILE_H\) \* ceil\(W / FLAIR_WARP_TILE_W\) \* 16 = 16"):
        _lib.call.flair_warp_error(a, None, ok, mask, 1, 8, 8, out, ws, 15)
    with pytest.raises(_lib.FlairHipError, match="flair_warp_error: ws = .* must be 8-byte aligned"):
        _lib.call.flair_warp_error(a, None, ok, mask, 1, 8, 8, out, ws[4:], 32)
    with pytest.raises(_lib.FlairHipError, match="flair_warp_error: f must be float32, got float64"):
        _lib.call.flair_warp_error(a, None, ok.double(), mask, 1, 8, 8, out, ws, 64)
    with pytest.raises(ValueError, match="warp_error: f is a dense .* float32 tensor"):
        ops.warp_error(a, ok.double(), mask)
    torch.cuda.synchronize()
    assert out.tolist() == [[[7.0, 7.0]]]            # the refused calls wrote nothing


# ------------------------------------------------------------------------------------------- end to end
def moving_frames(T=4, S=64, seed=3):
    """T frames of S x S: one smooth picture sliding by (2, 1) pixels per frame, + a little noise, so that SPyNet sees motion."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(1, 3, 10, 10, generator=g)
    big = torch.nn.functional.interpolate(coarse, size=(S + 16, S + 16), mode="bicubic", align_corners=False)[0]
    frames = torch.stack([big[:, 8 - i:8 - i + S, 8 - 2 * i:8 - 2 * i + S] for i in range(T)])
    frames = frames * 200 + 28 + 3 * torch.randn(frames.shape, generator=g)
    return frames.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def seeded_unet_state():
    from flair_amd.guided_diffusion.unet_new import UNetModel
    from tests.golden.weights import name_seeded_weights
    from tests.test_gpu_unet import SMALL
    return name_seeded_weights(UNetModel(**SMALL)).state_dict()


CALM = 1.0 / 8.0


@functools.lru_cache(maxsize=None)
def spynet_state(kind):
    """The seeded UNetModel's SPyNet as a bare mmedit state dict.  "seeded": as it is.  Its two directions are unrelated (the
    weights are random), so f + g~ is several pixels everywhere and the mask is EMPTY: N = 0 on every pair (seen with the
    oracle on the CPU).  "calmed": the last convolution of every level times 1/8, which keeps the flows a function of the
    frames but under a pixel: 650 .. 850 of 4096 pixels stay, the rest falls to both rules."""
    sd = {k[len("spynet."):]: v for k, v in seeded_unet_state().items() if k.startswith("spynet.")}
    if kind == "calmed":
        sd = {k: v * CALM if re.search(r"basic_module\.4\.conv\.", k) else v for k, v in sd.items()}
    return sd


@pytest.fixture(scope="module")
def flow_files(tmp_path_factory):
    """seeded: a task checkpoint as a user has it, the whole seeded UNetModel's state dict; calmed: a bare SPyNet file."""
    d = tmp_path_factory.mktemp("flow")
    torch.save(seeded_unet_state(), d / "flair_task.pt")
    torch.save(spynet_state("calmed"), d / "spynet_calmed.pth")
    return dict(seeded=str(d / "flair_task.pt"), calmed=str(d / "spynet_calmed.pth"))


@functools.lru_cache(maxsize=None)
def oracle_unet():
    from oracle.unet import UNetModel as Oracle
    from tests.test_gpu_unet import SMALL
    o = Oracle(**SMALL)
    o.load_state_dict(seeded_unet_state(), strict=True)
    return o.eval()


@pytest.mark.parametrize("kind", ["seeded", "calmed"])
def test_pairs_equal_the_reference_on_the_gpus_own_flows(dev, flow_files, kind):
    from flair_amd import ops
    from flair_amd import temporal as ftm
    model = ftm.WarpError(ftm.load_flow(flow_files[kind], dev))
    frames = moving_frames()
    g2 = torch.Generator().manual_seed(9)
    restored = (frames.int() + torch.randint(-6, 7, frames.shape, generator=g2)).clamp(0, 255).to(torch.uint8)
    f, g = model.flows(frames.to(dev))
    assert f.shape == g.shape == (3, 64, 64, 2) and f.dtype == torch.float32
    # the flows against the oracle's compute_flow, within the bound test_unet_flows_vs_oracle uses
    o = oracle_unet()
    o.spynet.load_state_dict(spynet_state(kind), strict=True)
    lqs = (frames.permute(0, 3, 1, 2).float() * (2.0 / 255.0) - 1.0)[None]
    with torch.no_grad():
        ff, fb = o.compute_flow(lqs)
    for got, ref in ((g, ff), (f, fb)):              # flows_backward is a -> b, this module's f
        ref = ref[0].permute(0, 2, 3, 1)
        err = (got.cpu() - ref).abs().max().item()
        print(f"{kind} flow: max |gpu - oracle| = {err:.3e}, |ref|max = {ref.abs().max().item():.3f}")
        assert err <= 2e-4 * max(1.0, ref.abs().max().item()), err
    assert fb.abs().max().item() > 0.05              # the network does give a flow

    def check(got, sets, flows_f, flows_g):
        """The reference on the SAME flows: the mask on the decided pixels, and S, N of the reference under the GPU's mask."""
        mask = ops.flow_occlusion(on(dev, flows_f), on(dev, flows_g)).cpu().numpy()
        for i in range(3):
            occ = R.occlusion(flows_f[i], flows_g[i])
            decided = occ["margin"] > 1e-9
            assert (~decided).mean() <= 1e-3 and np.array_equal(mask[i][decided], occ["mask"][decided])
            for s, frames_s in enumerate(sets):
                S, N = R.sums(frames_s[i], frames_s[i + 1], flows_f[i], mask[i])
                assert got[s, i, 1] == N and abs(got[s, i, 0] - S) <= 1e-12 * S, (s, i, got[s, i], S, N)
        print(f"{kind}: kept {got[0, :, 1] / 4096}, warp_err x 1e3 {[None if p[1] == 0 else 1e3 * R.warp_err(*p) for p in got[0]]}")

    # without truth: the frames' own flows and mask
    own = model.pairs(restored.to(dev))
    fr, gr = (t.cpu().numpy() for t in model.flows(restored.to(dev)))
    assert own.shape == (1, 3, 2) and own.dtype == np.float64
    check(own, [restored.numpy()], fr, gr)
    # with truth: the truth's flows and ONE mask judge both sets
    both = model.pairs(restored.to(dev), frames.to(dev))
    assert both.shape == (2, 3, 2) and np.array_equal(both[0, :, 1], both[1, :, 1])
    check(both, [restored.numpy(), frames.numpy()], f.cpu().numpy(), g.cpu().numpy())
    same = model.pairs(frames.to(dev), frames.to(dev))
    assert np.array_equal(same[0], same[1]) and np.array_equal(same[1], both[1])
    assert model.pairs(restored[:1].to(dev)).shape == (1, 0, 2)
    with pytest.raises(ValueError, match="warp-error: a frame is 16x64"):
        model.pairs(restored[:, :16].contiguous().to(dev))
    if kind == "seeded":
        return
    assert (both[..., 1] > 400).all() and (both[..., 1] < 1200).all()
    assert (both[0, :, 0] > both[1, :, 0]).all()     # the noisy set is the less consistent one
    # sub-batches that overlap by one frame: the same pairs (the flows may differ in their last bits between batch sizes)
    split = model.pairs(restored.to(dev), frames.to(dev), max_pairs=2)
    assert split.shape == (2, 3, 2) and np.abs(split[..., 1] - both[..., 1]).max() <= 0.02 * 4096
    assert np.allclose(split[..., 0] / split[..., 1], both[..., 0] / both[..., 1], rtol=0.05)


def test_evaluate_and_warp_error_commands_with_a_declared_cut(dev, flow_files, tmp_path, capsys):
    flow_file = flow_files["calmed"]
    from PIL import Image
    from flair_amd import temporal as ftm
    from flair_amd.__main__ import main
    truth = torch.cat([moving_frames(3, seed=3), moving_frames(2, seed=4)])          # frame 3 starts another shot
    g2 = torch.Generator().manual_seed(10)
    restored = (truth.int() + torch.randint(-6, 7, truth.shape, generator=g2)).clamp(0, 255).to(torch.uint8)
    for d, t in (("out", restored), ("truth", truth)):
        (tmp_path / d).mkdir()
        for n in range(5):
            Image.fromarray(t[n].numpy(), mode="RGB").save(tmp_path / d / f"{n:04d}.png", format="PNG")
    with open(tmp_path / "cuts.json", "w") as fh:
        json.dump(dict(cuts=[3], distances=[0.0] * 4, frames=5), fh)
    model = ftm.WarpError(ftm.load_flow(flow_file, dev))
    want = model.pairs(restored.to(dev), truth.to(dev))                                 # the same launch sizes as the command's
    value = lambda s, i: float(want[s, i, 0]) / (255.0 ** 2 * float(want[s, i, 1]))   # noqa: E731
    rc = main(["evaluate", str(tmp_path / "out"), str(tmp_path / "truth"), "--warp-error", flow_file, "--scene-cuts", str(tmp_path / "cuts.json"),
               "--json", str(tmp_path / "m.json"), "--device", "cuda:0"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert rc == 0 and len(lines) == 6
    per_frame = [None, value(0, 0), value(0, 1), None, value(0, 3)]
    for n, v in enumerate(per_frame):
        tail = "n/a" if v is None else f"{v * 1e3:.4f}"
        assert re.fullmatch(rf"{n:04d}\.png  psnr \S+  ssim \S+  warp-err {re.escape(tail)}", lines[n]), (lines[n], v)
    got = json.load(open(tmp_path / "m.json"))
    assert [f["warp_err"] for f in got["frames"]] == per_frame                          # unscaled, null where there is none
    mean = got["mean"]
    assert set(mean) == {"psnr", "ssim", "warp_err", "warp_err_truth", "warp_err_pairs", "masked"} and mean["warp_err_pairs"] == 3
    assert mean["warp_err"] == (value(0, 0) + value(0, 1) + value(0, 3)) / 3 and mean["warp_err_truth"] == (value(1, 0) + value(1, 1) + value(1, 3)) / 3
    assert mean["masked"] == sum(1.0 - float(want[0, i, 1]) / 4096 for i in (0, 1, 3)) / 3 and mean["warp_err"] > mean["warp_err_truth"]
    assert lines[5].endswith(f"  warp-err {mean['warp_err'] * 1e3:.4f} (truth {mean['warp_err_truth'] * 1e3:.4f})  masked {mean['masked']:.4f}"), lines[5]
    # without the cut the pair across it counts, and it is the worst one
    main(["evaluate", str(tmp_path / "out"), str(tmp_path / "truth"), "--warp-error", flow_file, "--json", str(tmp_path / "nocut.json"), "--device", "cuda:0"])
    capsys.readouterr()
    nocut = json.load(open(tmp_path / "nocut.json"))
    assert nocut["mean"]["warp_err_pairs"] == 4 and nocut["frames"][3]["warp_err"] == value(0, 2) > max(v for v in per_frame if v is not None)
    # without the option: the lines and the keys of before
    main(["evaluate", str(tmp_path / "out"), str(tmp_path / "truth"), "--json", str(tmp_path / "plain.json"), "--device", "cuda:0"])
    plain = capsys.readouterr().out.strip().splitlines()
    assert plain == [re.sub(r"  warp-err .*", "", line) for line in lines]
    assert set(json.load(open(tmp_path / "plain.json"))["mean"]) == {"psnr", "ssim"}

    # the command for footage without truth: the frames' own flows
    alone = model.pairs(restored.to(dev))
    rc = main(["warp-error", str(tmp_path / "out"), "--flow-weights", flow_file, "--scene-cuts", str(tmp_path / "cuts.json"),
               "--json", str(tmp_path / "w.json"), "--device", "cuda:0"])
    lines = capsys.readouterr().out.strip().splitlines()
    own = lambda i: float(alone[0, i, 0]) / (255.0 ** 2 * float(alone[0, i, 1]))       # noqa: E731
    per_frame = [None, own(0), own(1), None, own(3)]
    assert rc == 0 and lines[:5] == [f"{n:04d}.png  warp-err " + ("n/a" if v is None else f"{v * 1e3:.4f}") for n, v in enumerate(per_frame)]
    got = json.load(open(tmp_path / "w.json"))
    assert [f["warp_err"] for f in got["frames"]] == per_frame and got["count"] == 5
    assert list(got["mean"]) == ["warp_err", "warp_err_pairs", "masked"] and got["mean"]["warp_err"] == (own(0) + own(1) + own(3)) / 3
    assert lines[5] == f"mean of 3 pairs of 5 frames  warp-err {got['mean']['warp_err'] * 1e3:.4f}  masked {got['mean']['masked']:.4f}"
