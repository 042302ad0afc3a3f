"""The ArcFace identity definition of include/flair_ident.h in plain torch on the CPU, in float64 and, by a dtype switch,
float32 -- the restatement whose own deviation from float64 sets the GPU tests' bounds (4 x, the project's convention).

The network is written out from a state dict with torch.nn.functional, independently of flair_amd/identity.py: every BatchNorm
is applied where the definition has it, nothing is folded.  Weights are seeded by their names (He-scaled convolutions, BatchNorm
variances in 0.5 .. 1.5, PReLU slopes in 0.1 .. 0.4).  With such weights alone every cosine of two frames lies in 0.75 .. 1: the
embeddings share one large mean, and a test on them would be blind.  So a case CALIBRATES bn5: its running mean and variance
become the mean and the biased variance of fc5's float64 outputs over the case's own frames, which spreads the cosines over
-0.3 .. 1.  No pretrained file is read anywhere in the tests."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

SIDE = 128
WIDTH = 512
PLANES = (64, 128, 256, 512)
BN_EPS = 1e-5
PARAMETERS = 25627081
ENTRIES = 181                                   # of the state dict, num_batches_tracked included


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def blocks():
    """(prefix, cin, planes, stride, has_downsample) of the eight IRBlocks."""
    out, cin = [], 64
    for i, planes in enumerate(PLANES):
        stride = 1 if i == 0 else 2
        out.append((f"layer{i + 1}.0", cin, planes, stride, stride != 1 or cin != planes))
        out.append((f"layer{i + 1}.1", planes, planes, 1, False))
        cin = planes
    return out


def shapes():
    """{key: shape} of the whole state dict in the module's order."""
    s = {}

    def bn(name, c):
        s.update({f"{name}.weight": (c,), f"{name}.bias": (c,), f"{name}.running_mean": (c,), f"{name}.running_var": (c,),
                  f"{name}.num_batches_tracked": ()})
    s["conv1.weight"] = (64, 1, 3, 3)
    bn("bn1", 64)
    s["prelu.weight"] = (1,)
    for p, cin, planes, stride, ds in blocks():
        bn(f"{p}.bn0", cin)
        s[f"{p}.conv1.weight"] = (cin, cin, 3, 3)
        bn(f"{p}.bn1", cin)
        s[f"{p}.prelu.weight"] = (1,)
        s[f"{p}.conv2.weight"] = (planes, cin, 3, 3)
        bn(f"{p}.bn2", planes)
        if ds:
            s[f"{p}.downsample.0.weight"] = (planes, cin, 1, 1)
            bn(f"{p}.downsample.1", planes)
    bn("bn4", 512)
    s["fc5.weight"] = (WIDTH, 512 * 8 * 8)
    s["fc5.bias"] = (WIDTH,)
    bn("bn5", WIDTH)
    return s


@functools.lru_cache(maxsize=None)
def state_dict():
    """The seeded float32 state dict (bn5 as seeded: a case calibrates its own copy)."""
    sd = {}
    for k, shape in shapes().items():
        g = _gen(k)
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(1000, dtype=torch.int64)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shape, generator=g)
        elif k.endswith("running_mean"):
            sd[k] = 0.1 * torch.randn(shape, generator=g)
        elif k.endswith("prelu.weight"):
            sd[k] = 0.1 + 0.3 * torch.rand(shape, generator=g)
        elif len(shape) == 1 and k.endswith(".weight"):                   # a BatchNorm's scale
            sd[k] = 0.8 + 0.4 * torch.rand(shape, generator=g)
        elif k.endswith(".bias"):
            sd[k] = 0.1 * torch.randn(shape, generator=g)
        else:                                                             # convolutions and fc5: He-scaled
            fan_in = int(np.prod(shape[1:]))
            sd[k] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
    return sd


# ------------------------------------------------------------------------------------------- the definition
def prepare(u8, dtype=torch.float64):
    """(N, H, W, 3) uint8 -> (N, 1, 128, 128): steps 1 and 2."""
    x = 2.0 * u8.to(dtype) / 255.0 - 1.0
    gray = 0.2989 * x[..., 0] + 0.5870 * x[..., 1] + 0.1140 * x[..., 2]
    return F.interpolate(gray[:, None], size=(SIDE, SIDE), mode="bilinear", align_corners=False)


def _bn(x, sd, name):
    dt = x.dtype
    shape = (1, -1) + (1,) * (x.dim() - 2)
    p = {k: sd[f"{name}.{k}"].to(dt).view(shape) for k in ("weight", "bias", "running_mean", "running_var")}
    return (x - p["running_mean"]) / torch.sqrt(p["running_var"] + BN_EPS) * p["weight"] + p["bias"]


def _prelu(x, sd, name):
    return torch.where(x >= 0, x, sd[name].to(x.dtype) * x)


def features(x, sd):
    """(F, 1, 128, 128) -> the (F, 512, 8, 8) output of layer4, in x's dtype."""
    dt = x.dtype
    x = _prelu(_bn(F.conv2d(x, sd["conv1.weight"].to(dt), padding=1), sd, "bn1"), sd, "prelu.weight")
    x = F.max_pool2d(x, 2, 2)
    for p, cin, planes, stride, ds in blocks():
        out = _bn(x, sd, f"{p}.bn0")
        out = _prelu(_bn(F.conv2d(out, sd[f"{p}.conv1.weight"].to(dt), padding=1), sd, f"{p}.bn1"), sd, f"{p}.prelu.weight")
        out = _bn(F.conv2d(out, sd[f"{p}.conv2.weight"].to(dt), stride=stride, padding=1), sd, f"{p}.bn2")
        res = _bn(F.conv2d(x, sd[f"{p}.downsample.0.weight"].to(dt), stride=stride), sd, f"{p}.downsample.1") if ds else x
        x = _prelu(out + res, sd, f"{p}.prelu.weight")
    return x


def fc_outputs(feat, sd):
    """fc5(flatten(bn4(feat))) in (C, H, W) order, before bn5."""
    z = _bn(feat, sd, "bn4").flatten(1)
    return z @ sd["fc5.weight"].to(z.dtype).t() + sd["fc5.bias"].to(z.dtype)


def embed(u8, sd, dtype=torch.float64):
    """(F, H, W, 3) uint8 -> (F, 512) embeddings in ``dtype``."""
    with torch.no_grad():
        return _bn(fc_outputs(features(prepare(u8, dtype), sd), sd), sd, "bn5")


def cosines(ea, eb):
    """Row-wise cosines of two (N, 512) float64 arrays."""
    ea, eb = np.asarray(ea, dtype=np.float64), np.asarray(eb, dtype=np.float64)
    return (ea * eb).sum(1) / np.sqrt((ea * ea).sum(1) * (eb * eb).sum(1))


def drift(e):
    e = np.asarray(e, dtype=np.float64)
    return float(np.mean(1.0 - cosines(e[1:], e[:-1])))


# ------------------------------------------------------------------------------------------- the calibrated case
def smooth_frame(seed, side=64):
    """A face-sized blob picture: a coarse random grid enlarged, plus a little texture."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(1, 3, 8, 8, generator=g)
    img = F.interpolate(coarse, size=(side, side), mode="bicubic", align_corners=False)[0].permute(1, 2, 0)
    img = img * 200 + 28 + 6 * torch.randn(side, side, 3, generator=g)
    return img.round().clamp(0, 255).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def case_frames(side=64):
    """Six pairs (a, b), (6, side, side, 3) uint8 each: identical, + noise, another frame, its negative, half brightness,
    uniform noise."""
    g = torch.Generator().manual_seed(11)
    a = torch.stack([smooth_frame(s, side) for s in range(6)])
    b = a.clone()
    b[1] = (a[1].int() + torch.randint(-8, 9, a[1].shape, generator=g)).clamp(0, 255).to(torch.uint8)
    b[2] = smooth_frame(100, side)
    b[3] = 255 - a[3]
    b[4] = a[4] // 2
    b[5] = torch.randint(0, 256, a[5].shape, generator=g).to(torch.uint8)
    return a, b


@functools.lru_cache(maxsize=None)
def case():
    """The calibrated case: dict(a, b, sd (float32, bn5 calibrated on these 12 frames), feat64 the (12, 512, 8, 8) float64
    output of layer4, e64 (12, 512) float64 numpy, e32 the float32 restatement's as float64 numpy).  Computed once and shared; treat it as read-only."""
    a, b = case_frames()
    sd = dict(state_dict())
    both = torch.cat([a, b])
    with torch.no_grad():
        feat = features(prepare(both, torch.float64), sd)
        y = fc_outputs(feat, sd)
        sd["bn5.running_mean"] = y.mean(0).float()
        sd["bn5.running_var"] = y.var(0, unbiased=False).float()
        e64 = _bn(y, sd, "bn5").numpy()
    e32 = embed(both, sd, torch.float32).double().numpy()
    return dict(a=a, b=b, sd=sd, feat64=feat, e64=e64, e32=e32)


# ------------------------------------------------------------------------------------------- the entries' refusals
def entry_refusals():
    """[(entry, argument tuple without the stream, text the message must hold)]: every refusal include/flair_ident.h lists,
    on pointers that are never dereferenced (a refusal comes before any launch)."""
    import ctypes
    P, odd4, odd8 = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4), ctypes.c_void_p((1 << 20) + 8)
    Z = ctypes.c_size_t
    out = []
    prep = lambda **k: tuple({**dict(a=P, b=P, N=1, H=64, W=64, y=P, y_ld=16), **k}.values())  # noqa: E731
    for k, what in [(dict(a=None), "null pointer"), (dict(y=None), "null pointer"), (dict(N=0), "N = 0"), (dict(H=0), "H = 0"),
                    (dict(W=-2), "W = -2"), (dict(y_ld=12), "y_ld = 12 must be >= C = 16"), (dict(y_ld=18), "multiple of 4"),
                    (dict(y=odd4), "16-byte aligned"), (dict(y=odd8), "16-byte aligned"), (dict(N=1 << 30), "exceed one launch")]:
        out.append(("flair_ident_prepare", prep(**k), what))
    emb = lambda **k: tuple({**dict(x=P, x_ld=1024, F=2, K=1024, w=P, bias=P, O=8, out=P, out_ld=8, ws=P, ws_bytes=Z(128)), **k}.values())  # noqa: E731
    for k, what in [(dict(x=None), "null pointer"), (dict(w=None), "null pointer"), (dict(bias=None), "null pointer"),
                    (dict(out=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(F=0), "F = 0"), (dict(K=0, x_ld=0), "K = 0"),
                    (dict(O=0), "O = 0"), (dict(K=1022), "K = 1022 is not a multiple of 4"), (dict(K=(1 << 30) + 4, x_ld=(1 << 30) + 4), "up to 2^30"),
                    (dict(x_ld=1020), "x_ld = 1020 must be >= C = 1024"), (dict(x_ld=1026), "multiple of 4"), (dict(x=odd4), "x = "),
                    (dict(w=odd8), "w = "), (dict(out_ld=7), "out_ld = 7 must be >= O = 8"), (dict(ws=odd4), "8-byte aligned"),
                    (dict(ws_bytes=Z(127)), "ws_bytes = 127, ceil(K / FLAIR_IDENT_EMBED_KCHUNK) * F * O * 8 = 128"),
                    (dict(K=1028, x_ld=1028, ws_bytes=Z(128)), "= 256"), (dict(F=65535 * 16 + 1, ws_bytes=Z(1 << 40)), "exceed one launch")]:
        out.append(("flair_ident_embed", emb(**k), what))
    return out


def assert_refused(lib, name, args, what):
    rc = getattr(lib, name)(*args, None)
    msg = lib.flair_last_error().decode()
    assert rc == -1 and msg.startswith(name + ":") and what in msg, (name, what, rc, msg)
