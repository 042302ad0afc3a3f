"""CPU restatement of the BiSeNet face parser in plain PyTorch (test infrastructure only).

Follows the reference's guided_diffusion/facelib/parsing/bisenet.py (``BiSeNet.forward``, :111-140) and resnet.py, written
as functions over a STATE DICT with the reference's parameter names, so the same weights drive the reference
(tests/golden/make_golden_bisenet.py), this restatement and the HIP module.  Pinned to g15_bisenet.npz by
tests/test_bisenet_cpu.py; the GPU tests use it as their oracle where the fixture stores no value.  Also holds what the
fixture generator and the tests share: the inputs, the weights and the sampled pixel positions.
"""
import torch
import torch.nn.functional as F

from tests.golden.weights import name_seeded_weights

SIZES = {"small": (136, 168), "big": (512, 512)}        # 136 x 168: odd feature sizes at every level (17 x 21, 9 x 11, 5 x 6)
SEEDS = {"small": 151, "big": 152}
HEAD = "conv_out.conv_out.weight"                        # the main head's bias-free 1x1: refitted, stored in the fixture
PIXELS = 24                                              # sampled full-size positions per frame


def input_u8(case):
    """Two frames of seeded uint8 blocks, one per 8 x 8 pixels of the frame."""
    H, W = SIZES[case]
    g = torch.Generator().manual_seed(SEEDS[case])
    return torch.randint(0, 256, (2, 3, -(-H // 8), -(-W // 8)), generator=g, dtype=torch.uint8)


def bisenet_input(u8, case):
    """(2, 3, h, w) uint8 blocks -> (2, 3, H, W) f32 in [-1, 1): (u8 - 128) / 128 enlarged bilinearly."""
    x = (torch.as_tensor(u8).float() - 128.0) / 128.0
    return F.interpolate(x, size=SIZES[case], mode="bilinear", align_corners=False).contiguous()


def sample_pixels(case):
    """PIXELS seeded flat positions into the H x W grid per frame, sorted: (2, PIXELS) int64."""
    H, W = SIZES[case]
    g = torch.Generator().manual_seed(SEEDS[case] + 1000)
    return torch.stack([torch.randperm(H * W, generator=g)[:PIXELS].sort()[0] for _ in range(2)])


def seeded_state_dict(net, head=None, swap=None):
    """Name-seeded weights of ``net`` as a state dict (CPU f32); ``head`` replaces the main head's 1x1 weight (19, 256)
    and ``swap = (i, j)`` exchanges two of its rows afterwards (that permutes the class logits exactly)."""
    sd = {k: v.detach().float().cpu().clone() for k, v in name_seeded_weights(net).state_dict().items()}
    if head is not None:
        sd[HEAD] = torch.as_tensor(head).float().reshape(sd[HEAD].shape).clone()
    if swap is not None:
        i, j = swap
        w = sd[HEAD].clone()
        w[[i, j]] = w[[j, i]]
        sd[HEAD] = w
    return sd


def _bn(sd, name, x):
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"],
                        False, 0.0, 1e-5)


def conv_bn_relu(sd, name, x, stride=1):
    """ConvBNReLU.forward (:16-19)."""
    w = sd[name + ".conv.weight"]
    return F.relu(_bn(sd, name + ".bn", F.conv2d(x, w, None, stride=stride, padding=w.shape[2] // 2)))


def basic_block(sd, name, x, stride):
    """BasicBlock.forward (resnet.py:27-40)."""
    r = F.relu(_bn(sd, name + ".bn1", F.conv2d(x, sd[name + ".conv1.weight"], None, stride=stride, padding=1)))
    r = _bn(sd, name + ".bn2", F.conv2d(r, sd[name + ".conv2.weight"], None, padding=1))
    s = x
    if name + ".downsample.0.weight" in sd:
        s = _bn(sd, name + ".downsample.1", F.conv2d(x, sd[name + ".downsample.0.weight"], None, stride=stride))
    return F.relu(s + r)


def resnet18(sd, name, x):
    """ResNet18.forward (resnet.py:63-72) -> feat8, feat16, feat32."""
    x = F.relu(_bn(sd, name + ".bn1", F.conv2d(x, sd[name + ".conv1.weight"], None, stride=2, padding=3)))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    feats = []
    for i, stride in ((1, 1), (2, 2), (3, 2), (4, 2)):
        for j in range(2):
            x = basic_block(sd, f"{name}.layer{i}.{j}", x, stride if j == 0 else 1)
        feats.append(x)
    return feats[1], feats[2], feats[3]


def arm(sd, name, x):
    """AttentionRefinementModule.forward (:43-52)."""
    feat = conv_bn_relu(sd, name + ".conv", x)
    atten = F.avg_pool2d(feat, feat.size()[2:])
    atten = torch.sigmoid(_bn(sd, name + ".bn_atten", F.conv2d(atten, sd[name + ".conv_atten.weight"])))
    return torch.mul(feat, atten)


def context_path(sd, x):
    """ContextPath.forward (:66-85)."""
    feat8, feat16, feat32 = resnet18(sd, "cp.resnet", x)
    avg = conv_bn_relu(sd, "cp.conv_avg", F.avg_pool2d(feat32, feat32.size()[2:]))
    avg_up = F.interpolate(avg, feat32.size()[2:], mode="nearest")
    feat32_sum = arm(sd, "cp.arm32", feat32) + avg_up
    feat32_up = conv_bn_relu(sd, "cp.conv_head32", F.interpolate(feat32_sum, feat16.size()[2:], mode="nearest"))
    feat16_sum = arm(sd, "cp.arm16", feat16) + feat32_up
    feat16_up = conv_bn_relu(sd, "cp.conv_head16", F.interpolate(feat16_sum, feat8.size()[2:], mode="nearest"))
    return feat8, feat16_up, feat32_up


def ffm(sd, fsp, fcp):
    """FeatureFusionModule.forward (:98-108)."""
    feat = conv_bn_relu(sd, "ffm.convblk", torch.cat([fsp, fcp], dim=1))
    atten = F.avg_pool2d(feat, feat.size()[2:])
    atten = torch.sigmoid(F.conv2d(F.relu(F.conv2d(atten, sd["ffm.conv1.weight"])), sd["ffm.conv2.weight"]))
    return torch.mul(feat, atten) + feat


def heads(sd, x):
    """The three BiSeNetOutput heads before the enlargement: [(logits, feat)] for conv_out, conv_out16, conv_out32."""
    feat_res8, feat_cp8, feat_cp16 = context_path(sd, x)
    out = []
    for name, t in (("conv_out", ffm(sd, feat_res8, feat_cp8)), ("conv_out16", feat_cp8), ("conv_out32", feat_cp16)):
        feat = conv_bn_relu(sd, name + ".conv", t)
        out.append((F.conv2d(feat, sd[name + ".conv_out.weight"]), feat))
    return out


def enlarge(t, size):
    return F.interpolate(t, size, mode="bilinear", align_corners=True)


@torch.no_grad()
def bisenet_forward(sd, x, return_feat=False):
    """BiSeNet.forward (:120-140)."""
    hs = heads(sd, x)
    size = tuple(x.shape[2:])
    outs = tuple(enlarge(o, size) for o, _ in hs)
    if return_feat:
        outs += tuple(enlarge(f, size) for _, f in hs)
    return outs


@torch.no_grad()
def parse_map(sd, x):
    """face_parse(x)[0].argmax(dim=1) -> (B, H, W) int64, and the main head's 1/8-resolution logits."""
    low = heads(sd, x)[0][0]
    return enlarge(low, tuple(x.shape[2:])).argmax(1), low


def gather_pixels(t, pix):
    """(B, C, H, W), (B, K) flat positions -> (B, C, K)."""
    return torch.stack([t[b].reshape(t.shape[1], -1)[:, pix[b]] for b in range(t.shape[0])])
