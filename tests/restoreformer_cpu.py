"""CPU restatement of the RestoreFormer prior in plain PyTorch (test infrastructure only).

Follows the reference's guided_diffusion/restoreformer.py: ``VQVAEGANMultiHeadTransformer.forward`` (:857-861) with its
default configuration (ch 64, ch_mult (1, 2, 2, 4, 4, 8), two res blocks per level, attention at 16 in the encoder and at
16 / 32 in the decoder -- ex_multi_scale_num=1 --, 1024 x 256 codebook).  Written as functions over a STATE DICT with
the reference's parameter names, so the same name-seeded weights drive the reference (tests/golden/
make_golden_restoreformer.py), this restatement and the HIP module.  Pinned to g13_restoreformer.npz by
tests/test_restoreformer_cpu.py; the GPU tests use it as their oracle.
"""
import torch
import torch.nn.functional as F

CH, CH_MULT, NUM_RES_BLOCKS = 64, (1, 2, 2, 4, 4, 8), 2
ENC_ATTN, DEC_ATTN = (16,), (16, 32)


def _gn(sd, name, x):
    return F.group_norm(x, 32, sd[name + ".weight"], sd[name + ".bias"], 1e-6)


def _conv(sd, name, x, padding=1, stride=1):
    return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], stride=stride, padding=padding)


def _swish(x):
    return x * torch.sigmoid(x)                                   # nonlinearity(), :111-113


def resnet_block(sd, name, x):
    """ResnetBlock.forward without timestep embedding (:195-215)."""
    h = _conv(sd, name + ".conv1", _swish(_gn(sd, name + ".norm1", x)))
    h = _conv(sd, name + ".conv2", _swish(_gn(sd, name + ".norm2", h)))
    if name + ".nin_shortcut.weight" in sd:
        x = _conv(sd, name + ".nin_shortcut", x, padding=0)
    return x + h


def attn_block(sd, name, x, y=None, head_size=4):
    """MultiHeadAttnBlock.forward (:245-285): q from norm1(x) (self) or norm2(y) (cross), k and v from norm1(x)."""
    h_ = _gn(sd, name + ".norm1", x)
    y = h_ if y is None else _gn(sd, name + ".norm2", y)
    q = _conv(sd, name + ".q", y, padding=0)
    k = _conv(sd, name + ".k", h_, padding=0)
    v = _conv(sd, name + ".v", h_, padding=0)
    b, c, hh, ww = q.shape
    att = c // head_size
    q, k, v = (t.reshape(b, head_size, att, hh * ww).transpose(2, 3) for t in (q, k, v))   # b, head, hw, att
    w_ = F.softmax(torch.matmul(q * att ** -0.5, k.transpose(2, 3)), dim=3)
    o = torch.matmul(w_, v).transpose(2, 3).reshape(b, c, hh, ww)
    return x + _conv(sd, name + ".proj_out", o, padding=0)


def encoder(sd, x, head_size=4):
    """MultiHeadEncoder.forward (:375-412) -> hs."""
    hs = {}
    h = _conv(sd, "encoder.conv_in", x)
    hs["in"] = h
    res, n = x.shape[2], len(CH_MULT)
    for i in range(n):
        for j in range(NUM_RES_BLOCKS):
            h = resnet_block(sd, f"encoder.down.{i}.block.{j}", h)
            if res in ENC_ATTN:
                h = attn_block(sd, f"encoder.down.{i}.attn.{j}", h, head_size=head_size)
        if i != n - 1:
            hs[f"block_{i}"] = h
            h = _conv(sd, f"encoder.down.{i}.downsample.conv", F.pad(h, (0, 1, 0, 1)), padding=0, stride=2)
            res //= 2
    h = resnet_block(sd, "encoder.mid.block_1", h)
    hs[f"block_{n - 1}_atten"] = h
    h = attn_block(sd, "encoder.mid.attn_1", h, head_size=head_size)
    h = resnet_block(sd, "encoder.mid.block_2", h)
    hs["mid_atten"] = h
    hs["out"] = _conv(sd, "encoder.conv_out", _swish(_gn(sd, "encoder.norm_out", h)))
    return hs


def quantize(sd, z):
    """VectorQuantizer.forward's search and lookup (:28-62): f32 squared distances, first index on ties."""
    b, c, hh, ww = z.shape
    zf = z.permute(0, 2, 3, 1).reshape(-1, c)
    e = sd["quantize.embedding.weight"]
    d = torch.sum(zf ** 2, dim=1, keepdim=True) + torch.sum(e ** 2, dim=1) - 2 * torch.matmul(zf, e.t())
    idx = torch.min(d, dim=1)[1]
    return idx, d


def decoder(sd, z, hs, head_size=4):
    """MultiHeadDecoderTransformer.forward (:636-675)."""
    h = _conv(sd, "decoder.conv_in", z)
    h = resnet_block(sd, "decoder.mid.block_1", h)
    h = attn_block(sd, "decoder.mid.attn_1", h, hs["mid_atten"], head_size)
    h = resnet_block(sd, "decoder.mid.block_2", h)
    res = h.shape[2]
    for i in reversed(range(len(CH_MULT))):
        for j in range(NUM_RES_BLOCKS + 1):
            h = resnet_block(sd, f"decoder.up.{i}.block.{j}", h)
            if res in DEC_ATTN:
                key = f"block_{i}_atten" if f"block_{i}_atten" in hs else f"block_{i}"
                h = attn_block(sd, f"decoder.up.{i}.attn.{j}", h, hs[key], head_size)
        if i != 0:
            h = _conv(sd, f"decoder.up.{i}.upsample.conv", F.interpolate(h, scale_factor=2.0, mode="nearest"))
            res *= 2
    return _conv(sd, "decoder.conv_out", _swish(_gn(sd, "decoder.norm_out", h)))


@torch.no_grad()
def restoreformer_forward(sd, x, head_size=4, code_idx=None):
    """x (B, 3, 512, 512) -> dict(dec, z, idx (B, 256), d (B*256, n_e), hs).  ``code_idx`` replaces the search."""
    hs = encoder(sd, x, head_size)
    z = _conv(sd, "quant_conv", hs["out"], padding=0)
    idx, d = quantize(sd, z)
    b, c, hh, ww = z.shape
    if code_idx is not None:
        idx = code_idx.reshape(-1).long()
    zq = sd["quantize.embedding.weight"][idx].reshape(b, hh, ww, c).permute(0, 3, 1, 2)
    dec = decoder(sd, _conv(sd, "post_quant_conv", zq, padding=0), hs, head_size)
    return dict(dec=dec, z=z, idx=idx.reshape(b, hh * ww), d=d, hs=hs)
