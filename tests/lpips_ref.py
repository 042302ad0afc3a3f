"""The LPIPS definition of include/flair_eval.h in plain torch on the CPU (``lpips`` 0.1, spatial=False, eval mode), in float64
and, by a dtype switch, float32 -- the restatement whose own deviation from float64 sets the GPU tests' bounds (4 x, the
project's convention).  Trunk weights are seeded by their names and He-scaled; the lin weights are non-negative with some
exact zeros, as the published ones are.  No pretrained file is read anywhere in the tests."""
import functools
import zlib

import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10

VGG_CONVS = {0: (3, 64), 2: (64, 64), 5: (64, 128), 7: (128, 128), 10: (128, 256), 12: (256, 256), 14: (256, 256),
             17: (256, 512), 19: (512, 512), 21: (512, 512), 24: (512, 512), 26: (512, 512), 28: (512, 512)}
VGG_TAPS = (2, 7, 14, 21, 28)               # the convolution whose ReLU (features index + 1) is tapped
VGG_POOL_AFTER = (2, 7, 14, 21)             # MaxPool2d(2, 2), floor mode
ALEX_CONVS = {0: (3, 64, 11, 4, 2), 3: (64, 192, 5, 1, 2), 6: (192, 384, 3, 1, 1), 8: (384, 256, 3, 1, 1), 10: (256, 256, 3, 1, 1)}
ALEX_POOL_AFTER = (0, 3)                    # MaxPool2d(3, 2), no padding, floor mode
TAP_WIDTHS = {"vgg": (64, 128, 256, 512, 512), "alex": (64, 192, 384, 256, 256)}
MIN_SIDE = {"vgg": 16, "alex": 31}


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


@functools.lru_cache(maxsize=None)
def state_dicts(net):
    """-> (trunk, lin): float32 state dicts under torchvision's and the package's key names."""
    trunk, lin = {}, {}
    convs = {i: (ci, co, 3) for i, (ci, co) in VGG_CONVS.items()} if net == "vgg" else {i: v[:3] for i, v in ALEX_CONVS.items()}
    for i, (cin, cout, k) in convs.items():
        name = f"features.{i}"
        trunk[name + ".weight"] = torch.randn(cout, cin, k, k, generator=_gen(net + name + "w")) * (2.0 / (cin * k * k)) ** 0.5
        trunk[name + ".bias"] = torch.randn(cout, generator=_gen(net + name + "b")) * 0.05
    for k, c in enumerate(TAP_WIDTHS[net]):
        g = _gen(net + f"lin{k}")
        w = torch.rand(c, generator=g) * 2.0 / c
        w[torch.rand(c, generator=g) < 0.2] = 0.0
        lin[f"lin{k}.model.1.weight"] = w.view(1, c, 1, 1)
    return trunk, lin


def prepare(u8, dtype, minus_one=True):
    """(N, H, W, 3) uint8 -> (N, 3, H, W): steps 1 and 2."""
    x = 2.0 * u8.to(dtype) / 255.0 - (1.0 if minus_one else 0.0)
    x = (x - torch.tensor(SHIFT, dtype=dtype)) / torch.tensor(SCALE, dtype=dtype)
    return x.permute(0, 3, 1, 2).contiguous()


def features(net, x, trunk):
    """The five taps of the trunk on x (N, 3, H, W), in x's dtype."""
    dt = x.dtype
    taps = []
    if net == "vgg":
        for i in VGG_CONVS:
            x = F.relu(F.conv2d(x, trunk[f"features.{i}.weight"].to(dt), trunk[f"features.{i}.bias"].to(dt), padding=1))
            if i in VGG_TAPS:
                taps.append(x)
            if i in VGG_POOL_AFTER:
                x = F.max_pool2d(x, 2, 2)
        return taps
    for i, (_, _, k, s, p) in ALEX_CONVS.items():
        x = F.relu(F.conv2d(x, trunk[f"features.{i}.weight"].to(dt), trunk[f"features.{i}.bias"].to(dt), stride=s, padding=p))
        taps.append(x)
        if i in ALEX_POOL_AFTER:
            x = F.max_pool2d(x, 3, 2)
    return taps


def tap_distance(fa, fb, w, *, eps_inside=False, no_weights=False, mean_first=False):
    """fa, fb: (F, P, C) features, w: (C,) -> (F,): the mean over the P pixels of d = sum_c w_c (a^_c - b^_c)^2.  The three
    switches are the misreadings tests/test_lpips_cpu.py shows to matter; all off is the definition."""
    def unit(t):
        s = t.pow(2).sum(-1, keepdim=True)
        return t / (torch.sqrt(s + EPS) if eps_inside else torch.sqrt(s) + EPS)
    sq = (unit(fa) - unit(fb)).pow(2)
    w = w.to(fa.dtype)
    if no_weights:
        d = sq.sum(-1)
    elif mean_first:
        d = sq.mean(-1) * w.sum()
    else:
        d = (sq * w).sum(-1)
    return d.mean(-1)


def lpips(net, a_u8, b_u8, dtype=torch.float64, minus_one=True):
    """(N, H, W, 3) uint8 x 2 -> (N,) in ``dtype``, with the seeded weights of state_dicts(net)."""
    trunk, lin = state_dicts(net)
    N = a_u8.shape[0]
    with torch.no_grad():
        taps = features(net, prepare(torch.cat([a_u8, b_u8]), dtype, minus_one), trunk)
        total = torch.zeros(N, dtype=dtype)
        for k, t in enumerate(taps):
            t = t.permute(0, 2, 3, 1).reshape(2 * N, -1, t.shape[1])
            total = total + tap_distance(t[:N], t[N:], lin[f"lin{k}.model.1.weight"].reshape(-1))
    return total


def random_tap_case(C, P, Fr, seed=0):
    """Random post-ReLU features (half of them zero) of two similar frames and lin-like weights: fa, fb (Fr, P, C), w (C,) f32."""
    g = torch.Generator().manual_seed(1000 * C + 10 * P + Fr + seed)
    fa = torch.randn(Fr, P, C, generator=g).clamp_min(0.0)
    fb = (fa + 0.3 * torch.randn(Fr, P, C, generator=g)).clamp_min(0.0)
    w = torch.rand(C, generator=g) * 2.0 / C
    w[torch.rand(C, generator=g) < 0.2] = 0.0
    return fa, fb, w


def bound_4x(ref64, f32):
    """The bound of a GPU result against ref64: 4 x the largest deviation of the float32 CPU restatement on the same inputs."""
    return 4.0 * (f32.double() - ref64).abs().max().item()
