"""The weight-packing protocol of every network (flair_amd/guided_diffusion/packing.py), on the CPU: whatever makes the
kernel-native copies stale invalidates them, a repack follows the fp32 masters, and ``checkpoint.export_packed`` /
``import_packed`` carry ALL of a network's packed state (each module's ``_pk``) and nothing else is needed to run."""
import pytest
import torch

CPU = torch.device("cpu")


def _builders():
    from flair_amd.guided_diffusion.bisenet import BiSeNet
    from flair_amd.guided_diffusion.codeformer import CodeFormer
    from flair_amd.guided_diffusion.parsenet import ParseNet
    from flair_amd.guided_diffusion.restoreformer import VQVAEGANMultiHeadTransformer
    from flair_amd.guided_diffusion.retinaface import RetinaFace
    from flair_amd.guided_diffusion.sr3 import UNet
    from flair_amd.guided_diffusion.unet_new import UNetModel
    from flair_amd.guided_diffusion.vqfr import VQFRv2
    from flair_amd.guided_diffusion.yolov5face import Model
    from tests.test_gpu_sr3 import SR3_SMALL
    from tests.test_gpu_unet import SMALL
    from tests.vqfr_cpu import RELEASE
    return {"codeformer": CodeFormer, "restoreformer": VQVAEGANMultiHeadTransformer, "vqfr": lambda: VQFRv2(**RELEASE),
            "parsenet": lambda: ParseNet(in_size=512, out_size=512), "bisenet": lambda: BiSeNet(19),
            "retinaface_resnet50": lambda: RetinaFace("resnet50", device="cpu"),
            "retinaface_mobile": lambda: RetinaFace("mobile0.25", device="cpu"), "yolov5n": lambda: Model("yolov5n"),
            "unet_new": lambda: UNetModel(**SMALL), "sr3": lambda: UNet(**SR3_SMALL)}


# network -> (state-dict key of one convolution weight, the module whose _pk holds its packed copy, the key in that _pk)
CONV = {"codeformer": ("encoder.blocks.0.weight", "encoder.blocks.0", "w"),
        "restoreformer": ("encoder.conv_in.weight", "encoder.conv_in", "w"),
        "vqfr": ("encoder.conv_in.weight", "encoder.conv_in", "w"),
        "parsenet": ("encoder.0.conv2d.weight", "encoder.0", "w"),
        "bisenet": ("cp.resnet.conv1.weight", "cp.resnet", "w"),
        "retinaface_resnet50": ("body.conv1.weight", "body", "w"),
        "retinaface_mobile": ("body.stage1.0.0.weight", "body.stage1.0", "w"),
        "yolov5n": ("model.0.stem_1.conv.weight", "model.0.stem_1", "w"),
        "unet_new": ("input_blocks.1.0.in_layers.2.wrapped_module.weight", "input_blocks.1.0", "w1"),
        "sr3": ("downs.1.res_block.block1.block.3.wrapped_module.weight", "downs.1.res_block", "w1")}
NAMES = sorted(CONV)
F32_ONLY = ("retinaface_mobile", "yolov5n")             # their depthwise path asserts float32
UNETS = ("unet_new", "sr3")


def build(name, seed):
    """The network with seeded random parameters and BatchNorm statistics (so that no fold is the identity)."""
    torch.manual_seed(seed)
    net = _builders()[name]()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        for n, b in net.named_buffers():
            if n.endswith("running_var"):
                b.copy_(torch.rand(b.shape, generator=g) + 0.5)
            elif n.endswith("running_mean"):
                b.copy_(torch.randn(b.shape, generator=g) * 0.1)
    return net


CASES = [(n, dt) for n in NAMES for dt in (torch.float32, torch.bfloat16) if dt == torch.float32 or n not in F32_ONLY]


def packed(name, dtype):
    """Network ``name`` packed on the CPU in ``dtype``."""
    net = build(name, 0)
    if dtype == torch.bfloat16:
        net.convert_to_bf16()
    net._ensure_packed(CPU)
    return net


def _stale(net, name):
    net._packed_key = "stale"
    if name in UNETS:
        net._graphs = {"stale": None}


def _fresh(net, name):
    return net._packed_key is None and (name not in UNETS or net._graphs == {})


@pytest.mark.parametrize("name", NAMES)
def test_every_change_of_the_weights_invalidates(name, tmp_path):
    from flair_amd import checkpoint
    net = _builders()[name]()
    sd = net.state_dict()
    _stale(net, name)
    net.load_state_dict(sd)
    assert _fresh(net, name)
    _stale(net, name)
    net.convert_to_bf16()
    assert _fresh(net, name) and net.dtype == torch.bfloat16
    _stale(net, name)
    net.convert_to_fp32()
    assert _fresh(net, name) and net.dtype == torch.float32
    torch.save(sd, tmp_path / "net.pth")
    _stale(net, name)
    report = checkpoint.load_reference_checkpoint(net, str(tmp_path / "net.pth"))
    assert _fresh(net, name) and not report.missing_keys and not report.unexpected_keys


@pytest.mark.parametrize("name", UNETS)
def test_unets_keep_the_reference_name_for_reduced_precision(name):
    net = _builders()[name]()
    _stale(net, name)
    net.convert_to_fp16()
    assert _fresh(net, name) and net.dtype == torch.bfloat16


def _same(a, b):
    """Leaf for leaf: tensors bitwise (dtype and shape included), containers by type and length, plain values by ==."""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and \
            torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def _tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _tensors(v)


@pytest.mark.parametrize("name,dtype", CASES, ids=[f"{n}-{str(dt)[6:]}" for n, dt in CASES])
def test_export_import_carries_all_packed_state_and_a_repack_follows_the_masters(name, dtype):
    from flair_amd import checkpoint
    a = packed(name, dtype)
    b = build(name, 1)                                   # different weights, never packed
    before = {n: set(vars(m)) for n, m in b.named_modules()}
    for n, m in a.named_modules():
        # pack() itself sets nothing but _pk: no other state that a blob would miss
        assert set(vars(m)) - before[n] <= {"_pk"}, (n, set(vars(m)) - before[n])
    meta, blob = checkpoint.export_packed(a, CPU)
    checkpoint.import_packed(b, meta, blob)
    assert b._packed_key == (a.dtype, CPU) == a._packed_key
    base = blob.untyped_storage().data_ptr()
    mods_a = dict(a.named_modules())
    n_tensors = 0
    for n, m in b.named_modules():
        # nothing but _pk (and the blob on the model) appears on the importing side either
        assert set(vars(m)) - before[n] <= {"_pk", "_packed_blob"}, (n, set(vars(m)) - before[n])
        assert ("_pk" in vars(m)) == ("_pk" in vars(mods_a[n])), n
        if "_pk" in vars(m):
            assert _same(mods_a[n]._pk, m._pk), n
            for t in _tensors(m._pk):
                assert t.untyped_storage().data_ptr() == base, n
                n_tensors += 1
    assert n_tensors == len(meta["layout"]) > 0
    b._ensure_packed(CPU)                                # packed already: the views stay
    assert next(_tensors(dict(b.named_modules())[CONV[name][1]]._pk)).untyped_storage().data_ptr() == base
    # a convolution weight scaled by 2 and loaded doubles its packed copy on the next _ensure_packed
    net = a
    key, mod, k = CONV[name]
    holder = dict(net.named_modules())[mod]
    w0 = holder._pk[k].clone()
    assert w0.abs().max() > 0
    sd = {n: (v * 2 if n == key else v) for n, v in net.state_dict().items()}
    net.load_state_dict(sd)
    assert net._packed_key is None
    net._ensure_packed(CPU)
    assert net._packed_key == (net.dtype, CPU)
    assert torch.equal(holder._pk[k].float(), 2 * w0.float())
