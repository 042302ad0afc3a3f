"""RestoreFormer prior without a GPU: the CPU restatement (tests/restoreformer_cpu.py) pinned to the reference's own output
(tests/golden/g13_restoreformer.npz, tests/golden/make_golden_restoreformer.py), the module's state-dict names, checkpoint
formats, and the prior selection of build_pipeline and the command line."""
import json
import os

import numpy as np
import pytest
import torch

from tests.golden.weights import name_seeded_weights
from tests.util import fixture_threads  # noqa: F401  (pytest fixture)

GOLD = os.path.join(os.path.dirname(__file__), "golden", "g13_restoreformer.npz")


def state_dict():
    """Name-seeded weights under the reference's parameter names (the HIP module keeps those names)."""
    from flair_amd.guided_diffusion.restoreformer import VQVAEGANMultiHeadTransformer
    model = name_seeded_weights(VQVAEGANMultiHeadTransformer())
    return model, {k: v.detach().clone() for k, v in model.state_dict().items()}


def test_restatement_matches_reference_fixture(fixture_threads):
    from tests import restoreformer_cpu as orf
    from tests.golden.make_golden_restoreformer import restoreformer_input
    g = np.load(GOLD)
    _, sd = state_dict()
    r = orf.restoreformer_forward(sd, restoreformer_input(g["x_u8"]))
    z_ref = torch.from_numpy(g["z"])
    assert torch.allclose(r["z"], z_ref, atol=2e-4, rtol=1e-4)
    clear = torch.from_numpy(g["margin"]) > 1e-3
    assert clear.float().mean() > 0.9
    assert torch.equal(r["idx"][clear], torch.from_numpy(g["idx"]).long()[clear])
    mid = torch.from_numpy(g["mid_atten_c4"])
    assert torch.allclose(r["hs"]["mid_atten"][:, ::4], mid, atol=5e-4 * mid.abs().max().item(), rtol=1e-4)
    pix = torch.from_numpy(g["dec_pix"]).long()
    dec_ref = torch.from_numpy(g["dec_sub"])
    r = orf.restoreformer_forward(sd, restoreformer_input(g["x_u8"]), code_idx=torch.from_numpy(g["idx"]))
    dec = torch.stack([r["dec"][b].reshape(3, -1)[:, pix[b]] for b in range(2)])
    assert (dec - dec_ref).abs().max().item() <= 5e-4 * dec_ref.abs().max().item()


def test_state_dict_names_match_reference():
    g = np.load(GOLD)
    model, sd = state_dict()
    assert list(sd.keys()) == [str(n) for n in g["param_names"]]
    assert [";".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g["param_shapes"]]
    assert len(sd) == 441 and sum(v.numel() for v in sd.values()) == 73_472_579


def test_checkpoint_formats(tmp_path):
    """A plain state dict and a training checkpoint ({'state_dict': {'vqvae.<name>': ..., 'loss.<x>': ...}}) load
    strictly; a missing tensor is an error."""
    from flair_amd import checkpoint
    from flair_amd.guided_diffusion.restoreformer import VQVAEGANMultiHeadTransformer
    _, sd = state_dict()
    torch.save(sd, tmp_path / "plain.ckpt")
    wrapped = {"vqvae." + k: v for k, v in sd.items()}
    wrapped.update({"loss.discriminator.main.0.weight": torch.zeros(4, 3, 4, 4), "loss.logvar": torch.zeros(())})
    torch.save({"state_dict": wrapped}, tmp_path / "train.ckpt")
    for name in ("plain.ckpt", "train.ckpt"):
        dst = VQVAEGANMultiHeadTransformer()
        report = checkpoint.load_reference_checkpoint(dst, str(tmp_path / name))
        assert not report.missing_keys and not report.unexpected_keys
        assert all(torch.equal(a, b) for a, b in zip(dst.state_dict().values(), sd.values()))
    dst = VQVAEGANMultiHeadTransformer()
    assert dst.load_state_dict({"state_dict": wrapped}) is not None
    missing = dict(sd)
    missing.pop("decoder.up.4.attn.2.norm2.weight")
    with pytest.raises(RuntimeError, match="decoder.up.4.attn.2.norm2.weight"):
        VQVAEGANMultiHeadTransformer().load_state_dict(missing)
    torch.save({"state_dict": {k: v for k, v in wrapped.items() if not k.endswith("quant_conv.bias")}},
               tmp_path / "short.ckpt")
    with pytest.raises(RuntimeError, match="quant_conv.bias"):
        checkpoint.load_reference_checkpoint(VQVAEGANMultiHeadTransformer(), str(tmp_path / "short.ckpt"))


def test_head_widths_refused_at_construction():
    from flair_amd.guided_diffusion.restoreformer import VQVAEGANMultiHeadTransformer
    from flair_amd.guided_diffusion.unet_new import qkv_head_width
    for hs in (1, 2, 8):                                      # widths 512 / 256 / 64 at 16x16, 256 / 128 / 32 at 32x32
        VQVAEGANMultiHeadTransformer(head_size=hs)
    with pytest.raises(NotImplementedError):
        qkv_head_width(256, 3)
    with pytest.raises((NotImplementedError, AssertionError)):
        VQVAEGANMultiHeadTransformer(head_size=3)
    with pytest.raises(NotImplementedError):
        VQVAEGANMultiHeadTransformer(head_size=128)            # width 2 at 32x32 (256 channels)


def _names(task, det):
    det_file = {"retinaface_resnet50": "detection_Resnet50_Final.pth",
                "retinaface_mobile0.25": "detection_mobilenet0.25_Final.pth"}[det]
    return [f"flair_{task}.pt", det_file, "parsing_parsenet.pth"]


@pytest.mark.parametrize("prior,prior_file", [("restoreformer", "RestoreFormer.ckpt"), ("codeformer", "codeformer.pth"),
                                              (True, "codeformer.pth"), (False, None), (None, None)])
def test_prior_selects_its_checkpoint(tmp_path, prior, prior_file):
    """Each prior names exactly its own file when it is missing; the other prior's file is never required."""
    from flair_amd import pipeline as pl
    task, det = "gaussian", "retinaface_mobile0.25"
    names = _names(task, det) + ([prior_file] if prior_file else [])
    for missing in names:
        d = tmp_path / missing.replace(".", "_")
        d.mkdir()
        for n in names:
            if n != missing:
                (d / n).write_bytes(b"")
        with pytest.raises(FileNotFoundError, match=missing.replace(".", r"\.")):
            pl.build_pipeline(task, d, device="cpu", size=512, prior=prior, det_model=det,
                              kernels_path=str(tmp_path / "none.mat"))
    files = [os.path.basename(f) for f in pl._required_files(task, tmp_path, det, prior)]
    assert sorted(files) == sorted(names)
    other = {"codeformer.pth", "RestoreFormer.ckpt"} - {prior_file}
    assert not other & set(files)


def test_prior_argument_rules(tmp_path):
    from flair_amd import pipeline as pl
    assert [pl.prior_name(p) for p in (True, False, None, "codeformer", "restoreformer")] == \
        ["codeformer", None, None, "codeformer", "restoreformer"]
    with pytest.raises(ValueError, match="prior="):
        pl.prior_name("vqfr")
    with pytest.raises(ValueError, match="RestoreFormer prior restores 512 x 512"):
        pl.build_pipeline("gaussian", tmp_path, device="cpu", size=256, prior="restoreformer")
    with pytest.raises(ValueError, match="CodeFormer prior restores 512 x 512"):
        pl.build_pipeline("gaussian", tmp_path, device="cpu", size=256)


def test_cli_prior_options(tmp_path):
    from flair_amd import __main__ as cli
    ap = cli.make_parser()
    base = ["restore", "gaussian", str(tmp_path), str(tmp_path / "o")]
    a = ap.parse_args(base)
    assert a.prior is None and not a.no_prior and a.prior_kwargs is None and cli.prior_of(a) == "codeformer"
    assert cli.prior_of(ap.parse_args(base + ["--no-prior"])) is False
    assert cli.prior_of(ap.parse_args(base + ["--prior", "restoreformer"])) == "restoreformer"
    assert cli.prior_of(ap.parse_args(base + ["--prior", "codeformer"])) == "codeformer"
    a = ap.parse_args(base + ["--prior", "restoreformer", "--prior-kwargs", json.dumps({"head_size": 8})])
    assert json.loads(a.prior_kwargs) == {"head_size": 8}
    with pytest.raises(SystemExit):
        cli.prior_of(ap.parse_args(base + ["--no-prior", "--prior", "restoreformer"]))
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--prior", "vqfr"])
    d = ap.parse_args(["gaussian-demo"])
    assert cli.prior_of(d) == "codeformer"


def test_cli_restoreformer_needs_its_checkpoint(tmp_path):
    """``--prior restoreformer`` fails on a missing RestoreFormer.ckpt by name and does not ask for codeformer.pth."""
    from flair_amd import __main__ as cli
    frames = tmp_path / "frames"
    frames.mkdir()
    w = tmp_path / "w"
    w.mkdir()
    for n in _names("gaussian", "retinaface_mobile0.25"):
        (w / n).write_bytes(b"")
    argv = ["restore", "gaussian", str(frames), str(tmp_path / "o"), "--prior", "restoreformer", "--weights", str(w),
            "--det-model", "retinaface_mobile0.25", "--device", "cpu", "--kernels", str(tmp_path / "k.mat")]
    with torch.enable_grad():                     # main() turns autograd off for the process; keep it to this test
        with pytest.raises(FileNotFoundError, match=r"RestoreFormer\.ckpt"):
            cli.main(argv)
        (w / "codeformer.pth").write_bytes(b"")
        with pytest.raises(FileNotFoundError, match=r"RestoreFormer\.ckpt"):
            cli.main(argv)
    assert torch.is_grad_enabled()


def test_restoreformer_aux_closure():
    from flair_amd import workload as wl
    calls = []

    def net(x):
        calls.append(x)
        return x * 2, None, None, {}
    aux = wl.restoreformer_aux(net)
    x = torch.ones(1, 3, 4, 4)
    assert torch.equal(aux(x, torch.zeros(1), x), x * 2) and len(calls) == 1
