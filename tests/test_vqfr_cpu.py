"""VQFR v2 prior without a GPU: the CPU restatement (tests/vqfr_cpu.py) pinned to the reference's own output
(tests/golden/g14_vqfr.npz, tests/golden/make_golden_vqfr.py), the module's state-dict names, checkpoint formats,
construction refusals, and the prior selection of build_pipeline and the command line."""
import json
import os

import numpy as np
import pytest
import torch

from tests.util import fixture_threads  # noqa: F401  (pytest fixture)

GOLD = os.path.join(os.path.dirname(__file__), "golden", "g14_vqfr.npz")


def build(cfg=None):
    """VQFRv2 (the HIP module, a parameter container on the CPU) with the fixture's weights, and its state dict."""
    from flair_amd.guided_diffusion.vqfr import VQFRv2
    from tests import vqfr_cpu as ov
    net = VQFRv2(**(cfg or ov.RELEASE))
    return net, ov.seeded_state_dict(net)


def test_restatement_matches_reference_fixture(fixture_threads):
    from tests import vqfr_cpu as ov
    g = np.load(GOLD)
    _, sd = build()
    trace = {}
    r = ov.vqfr_forward(sd, ov.vqfr_input(torch.from_numpy(g["x_u8"])), ov.RELEASE, trace=trace)
    clear = torch.from_numpy(g["margin"]) > 1e-3
    assert clear.float().mean() > 0.9
    assert torch.equal(r["idx"][clear], torch.from_numpy(g["idx"]).long()[clear])
    warp, offset = trace["Level_1"]
    tpix = torch.from_numpy(g["twm1_pix"])
    for got, name in ((warp, "twm1_out"), (offset, "twm1_offset")):
        ref = torch.from_numpy(g[name])
        assert (ov.take(got, tpix) - ref).abs().max().item() <= 5e-4 * ref.abs().max().item(), name
    r = ov.vqfr_forward(sd, ov.vqfr_input(torch.from_numpy(g["x_u8"])), ov.RELEASE, code_idx=torch.from_numpy(g["idx"]))
    ref = torch.from_numpy(g["dec_sub"])
    assert (ov.take(r["main_dec"], torch.from_numpy(g["dec_pix"])) - ref).abs().max().item() <= 5e-4 * ref.abs().max().item()


def test_restatement_matches_reference_fixture_nearest(fixture_threads):
    from tests import vqfr_cpu as ov
    g = np.load(GOLD)
    _, sd = build(ov.SMALL_NEAREST)
    x = ov.vqfr_input(torch.from_numpy(g["n_x_u8"]))
    r = ov.vqfr_forward(sd, x, ov.SMALL_NEAREST)
    clear = torch.from_numpy(g["n_margin"]) > 1e-3
    assert clear.float().mean() > 0.9
    assert torch.equal(r["idx"][clear], torch.from_numpy(g["n_idx"]).long()[clear])
    r = ov.vqfr_forward(sd, x, ov.SMALL_NEAREST, code_idx=torch.from_numpy(g["n_idx"]))
    ref = torch.from_numpy(g["n_dec_sub"])
    assert (ov.take(r["main_dec"], torch.from_numpy(g["n_dec_pix"])) - ref).abs().max().item() <= 5e-4 * ref.abs().max().item()


def test_offsets_leave_the_frame(fixture_threads):
    """The fixture's level-1 offsets are several pixels long: some border samples fall outside the 512^2 frame."""
    g = np.load(GOLD)
    assert np.abs(g["twm1_offset"]).max() > 0.5


def test_state_dict_names_match_reference():
    from tests import vqfr_cpu as ov
    g = np.load(GOLD)
    _, sd = build()
    assert list(sd.keys()) == [str(n) for n in g["param_names"]]
    assert [";".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g["param_shapes"]]
    assert len(sd) == 503 and sum(v.numel() for v in sd.values()) == 83_486_539
    _, sds = build(ov.SMALL_NEAREST)
    assert list(sds.keys()) == [str(n) for n in g["n_param_names"]]


def test_checkpoint_formats(tmp_path):
    """A bare state dict, BasicSR's {"params_ema": ...} (preferred over "params") and {"params": ...} load strictly; a
    missing tensor is an error."""
    from flair_amd import checkpoint
    from tests import vqfr_cpu as ov
    _, sd = build()
    bad = {k: torch.zeros_like(v) for k, v in sd.items()}
    torch.save(sd, tmp_path / "plain.pth")
    torch.save({"params_ema": sd, "params": bad}, tmp_path / "ema.pth")
    torch.save({"params": sd}, tmp_path / "params.pth")
    for f in ("plain.pth", "ema.pth", "params.pth"):
        net, _ = build()
        for p in net.parameters():
            p.data.zero_()
        checkpoint.load_reference_checkpoint(net, str(tmp_path / f), strict=True)
        got = net.state_dict()
        assert all(torch.equal(got[k], v) for k, v in sd.items()), f
    short = dict(sd)
    short.pop("main_branch.align_func_dict.Level_1.dcn.conv_offset.weight")
    torch.save(short, tmp_path / "short.pth")
    with pytest.raises(RuntimeError, match="conv_offset"):
        checkpoint.load_reference_checkpoint(build(ov.RELEASE)[0], str(tmp_path / "short.pth"), strict=True)


@pytest.mark.parametrize("change,err,match", [
    (dict(code_dim=128), ValueError, "code_dim=128"),
    (dict(channel_multipliers=(1, 2, 2, 4, 8)), ValueError, "16 x 16"),
    (dict(base_channels=48), ValueError, "multiples of 32"),
    (dict(base_channels=32), ValueError, "at least 64"),
    (dict(align_opt=dict(cond_channels=32, deformable_groups=2)), NotImplementedError, "deformable_groups=2"),
    (dict(align_opt=dict(cond_channels=32, deformable_groups=16)), NotImplementedError, "group width"),
    (dict(align_opt=dict(cond_channels=16, deformable_groups=4)), ValueError, "cond_channels"),
    (dict(base_channels=96, channel_multipliers=(1, 2, 2, 4, 4, 8)), NotImplementedError, "deformable_groups=4"),
    (dict(code_selection_mode="Random"), ValueError, "code_selection_mode"),
])
def test_unsupported_configurations_refused(change, err, match):
    from flair_amd.guided_diffusion.vqfr import VQFRv2
    from tests import vqfr_cpu as ov
    with pytest.raises(err, match=match):
        VQFRv2(**dict(ov.RELEASE, **change))


def test_attention_width_refused():
    """The single-head AttnBlock is as wide as its channels; widths the attention kernels cannot run are refused."""
    from flair_amd.guided_diffusion import vqfr
    vqfr.AttnBlock(512)
    with pytest.raises(NotImplementedError):
        vqfr.AttnBlock(4)


def _names(task, det):
    det_file = {"retinaface_resnet50": "detection_Resnet50_Final.pth",
                "retinaface_mobile0.25": "detection_mobilenet0.25_Final.pth"}[det]
    return [f"flair_{task}.pt", det_file, "parsing_parsenet.pth"]


def test_vqfr_selects_its_checkpoint(tmp_path):
    """``prior="vqfrv2"`` names VQFR_v2.pth when it is missing and never requires another prior's file."""
    from flair_amd import pipeline as pl
    task, det = "gaussian", "retinaface_mobile0.25"
    names = _names(task, det) + ["VQFR_v2.pth"]
    for missing in names:
        d = tmp_path / missing.replace(".", "_")
        d.mkdir()
        for n in names:
            if n != missing:
                (d / n).write_bytes(b"")
        with pytest.raises(FileNotFoundError, match=missing.replace(".", r"\.")):
            pl.build_pipeline(task, d, device="cpu", size=512, prior="vqfrv2", det_model=det,
                              kernels_path=str(tmp_path / "none.mat"))
    files = [os.path.basename(f) for f in pl._required_files(task, tmp_path, det, "vqfrv2")]
    assert sorted(files) == sorted(names)
    assert not {"codeformer.pth", "RestoreFormer.ckpt"} & set(files)


def test_vqfr_prior_argument_rules(tmp_path):
    from flair_amd import pipeline as pl
    assert pl.prior_name("vqfrv2") == "vqfrv2" and pl.PRIOR_FILES["vqfrv2"] == "VQFR_v2.pth"
    for bad in ("vqfr", "VQFRv2", "vqfr_v2"):
        with pytest.raises(ValueError, match="prior="):
            pl.prior_name(bad)
    with pytest.raises(ValueError, match="VQFR prior restores 512 x 512"):
        pl.build_pipeline("gaussian", tmp_path, device="cpu", size=256, prior="vqfrv2")


def test_release_configuration_defaults():
    """build_pipeline's constructor arguments are the v2 release configuration; the network builds from them."""
    from flair_amd import pipeline as pl
    from tests import vqfr_cpu as ov
    assert pl.VQFR_CONFIG == ov.RELEASE
    build(pl.VQFR_CONFIG)


def test_cli_vqfr_options(tmp_path):
    from flair_amd import __main__ as cli
    ap = cli.make_parser()
    base = ["restore", "gaussian", str(tmp_path), str(tmp_path / "o")]
    assert cli.prior_of(ap.parse_args(base + ["--prior", "vqfrv2"])) == "vqfrv2"
    a = ap.parse_args(base + ["--prior", "vqfrv2", "--prior-kwargs", json.dumps({"fidelity_ratio": 0.5})])
    assert json.loads(a.prior_kwargs) == {"fidelity_ratio": 0.5}
    with pytest.raises(SystemExit):
        cli.prior_of(ap.parse_args(base + ["--no-prior", "--prior", "vqfrv2"]))


def test_cli_vqfr_needs_its_checkpoint(tmp_path):
    """``--prior vqfrv2`` fails on a missing VQFR_v2.pth by name, with or without the other priors' files present."""
    from flair_amd import __main__ as cli
    frames = tmp_path / "frames"
    frames.mkdir()
    w = tmp_path / "w"
    w.mkdir()
    for n in _names("gaussian", "retinaface_mobile0.25"):
        (w / n).write_bytes(b"")
    argv = ["restore", "gaussian", str(frames), str(tmp_path / "o"), "--prior", "vqfrv2", "--weights", str(w),
            "--det-model", "retinaface_mobile0.25", "--device", "cpu", "--kernels", str(tmp_path / "k.mat")]
    with torch.enable_grad():                     # main() turns autograd off for the process; keep it to this test
        with pytest.raises(FileNotFoundError, match=r"VQFR_v2\.pth"):
            cli.main(argv)
        (w / "codeformer.pth").write_bytes(b"")
        (w / "RestoreFormer.ckpt").write_bytes(b"")
        with pytest.raises(FileNotFoundError, match=r"VQFR_v2\.pth"):
            cli.main(argv)
    assert torch.is_grad_enabled()


def test_vqfr_aux_closure_passes_fidelity_ratio():
    from flair_amd import workload as wl
    calls = []

    def net(x, fidelity_ratio):
        calls.append(fidelity_ratio)
        return {"main_dec": x * fidelity_ratio, "texture_dec": None}
    x = torch.ones(1, 3, 4, 4)
    assert torch.equal(wl.vqfr_aux(net)(x, torch.zeros(1), x), x) and calls == [1.0]
    assert torch.equal(wl.vqfr_aux(net, 0.25)(x, torch.zeros(1), x), x * 0.25) and calls == [1.0, 0.25]
