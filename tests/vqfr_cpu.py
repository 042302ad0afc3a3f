"""CPU restatement of the VQFR v2 prior in plain PyTorch (test infrastructure only).

Follows the reference's guided_diffusion/vqfr.py: ``VQFRv2.forward`` (:565-586) and the modules it is built from, written
as functions over a STATE DICT with the reference's parameter names, so the same weights drive the reference
(tests/golden/make_golden_vqfr.py), this restatement and the HIP module.  ``DCNv2Pack`` runs on
oracle.thirdparty.deform_conv2d (torchvision.ops.deform_conv2d semantics, the branch vqfr.py:358-369 takes).  Pinned to
g14_vqfr.npz by tests/test_vqfr_cpu.py; the GPU tests use it as their oracle where the fixture stores no value.
"""
import torch
import torch.nn.functional as F

from oracle.thirdparty import deform_conv2d
from tests.golden.weights import name_seeded_weights

# the VQFR project's v2 release configuration (pipeline.VQFR_CONFIG) and the small "Nearest" configuration of g14
RELEASE = dict(base_channels=64, channel_multipliers=(1, 2, 2, 4, 4, 8), num_enc_blocks=2, use_enc_attention=True,
               num_dec_blocks=2, use_dec_attention=True, code_dim=256, inpfeat_dim=32, code_selection_mode="Predict",
               align_opt=dict(cond_channels=32, deformable_groups=4))
SMALL_NEAREST = dict(base_channels=64, channel_multipliers=(1, 1, 1, 1, 1, 1), num_enc_blocks=1, use_enc_attention=False,
                     num_dec_blocks=1, use_dec_attention=False, code_dim=256, inpfeat_dim=32,
                     code_selection_mode="Nearest", align_opt=dict(cond_channels=32, deformable_groups=8))
OFFSET_GAIN = 4.0        # conv_offset weights x 4: offsets of several pixels, so that samples leave the frame


def vqfr_seeded_weights(model):
    """Name-seeded weights (tests/golden/weights.py) with every ``dcn.conv_offset`` scaled by OFFSET_GAIN."""
    name_seeded_weights(model)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if ".dcn.conv_offset." in name:
                p.mul_(OFFSET_GAIN)
    return model


def seeded_state_dict(net):
    """The same weights as a plain state dict (CPU f32)."""
    return {k: v.detach().float().cpu() for k, v in vqfr_seeded_weights(net).state_dict().items()}


def _gn(sd, name, x):
    return F.group_norm(x, 32, sd[name + ".weight"], sd[name + ".bias"], 1e-6)


def _conv(sd, name, x, padding=1, stride=1, groups=1):
    return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], stride=stride, padding=padding, groups=groups)


def resnet_block(sd, name, x):
    """ResnetBlock.forward (:130-144)."""
    h = _conv(sd, name + ".conv1", F.silu(_gn(sd, name + ".norm1", x)))
    h = _conv(sd, name + ".conv2", F.silu(_gn(sd, name + ".norm2", h)))
    if name + ".residual_func.weight" in sd:
        x = _conv(sd, name + ".residual_func", x, padding=0)
    return h + x


def attn_block(sd, name, x):
    """AttnBlock.forward (:168-194)."""
    h_ = _gn(sd, name + ".norm", x)
    q, k, v = (_conv(sd, f"{name}.{t}", h_, padding=0) for t in "qkv")
    b, c, hh, ww = q.shape
    q, k, v = (t.reshape(b, c, hh * ww) for t in (q, k, v))
    w_ = F.softmax(torch.bmm(q.permute(0, 2, 1), k) * int(c) ** (-0.5), dim=2)
    h_ = torch.bmm(v, w_.permute(0, 2, 1)).reshape(b, c, hh, ww)
    return x + _conv(sd, name + ".proj_out", h_, padding=0)


def _kinds(cfg, encoder):
    """The block kinds of each level's nn.Sequential, in the reference's construction order (:216-235, :301-320)."""
    n = len(cfg["channel_multipliers"])
    nb = cfg["num_enc_blocks" if encoder else "num_dec_blocks"]
    att = cfg["use_enc_attention" if encoder else "use_dec_attention"]
    out = []
    for i in (range(n) if encoder else reversed(range(n))):
        first = 0 if encoder else n - 1
        ks = [] if i == first else ["down" if encoder else "up"]
        for _ in range(nb):
            ks.append("res")
            if i == n - 1 and att:
                ks.append("attn")
        out.append(ks)
    return out


def _run_level(sd, name, kinds, x):
    for j, k in enumerate(kinds):
        nm = f"{name}.{j}"
        if k == "down":
            x = _conv(sd, nm + ".conv", F.pad(x, (0, 1, 0, 1)), padding=0, stride=2)
        elif k == "up":
            x = _conv(sd, nm + ".conv", F.interpolate(x, scale_factor=2.0, mode="nearest"))
        elif k == "res":
            x = resnet_block(sd, nm, x)
        else:
            x = attn_block(sd, nm, x)
    return x


def _mid(sd, name, x, att):
    x = resnet_block(sd, name + ".0", x)
    if att:
        x = attn_block(sd, name + ".1", x)
    return resnet_block(sd, name + (".2" if att else ".1"), x)


def encoder(sd, x, cfg):
    """VQGANEncoder.forward (:260-266)."""
    x = _conv(sd, "encoder.conv_in", x)
    for i, ks in enumerate(_kinds(cfg, True)):
        x = _run_level(sd, f"encoder.blocks.{i}", ks, x)
    x = _mid(sd, "encoder.mid_blocks", x, cfg["use_enc_attention"])
    return _conv(sd, "encoder.conv_out.2", F.silu(_gn(sd, "encoder.conv_out.0", x)))


def decoder(sd, z, cfg):
    """VQGANDecoder.forward (:328-338) -> dec_res."""
    n = len(cfg["channel_multipliers"])
    x = _mid(sd, "decoder.mid_blocks", _conv(sd, "decoder.conv_in", z), cfg["use_dec_attention"])
    dec_res = {}
    for i, ks in enumerate(_kinds(cfg, False)):
        x = _run_level(sd, f"decoder.blocks.{i}", ks, x)
        dec_res["Level_%d" % 2 ** (n - 1 - i)] = x
    return dec_res


def decoder_conv_out(sd, x):
    return _conv(sd, "decoder.conv_out.2", F.silu(_gn(sd, "decoder.conv_out.0", x)))


def twm(sd, name, x_main, inpfeat, rate, previous_offset=None):
    """TextureWarpingModule.forward (:409-427) with DCNv2Pack.forward (:352-380)."""
    h, w = inpfeat.shape[2:]
    inpfeat = F.interpolate(inpfeat, size=(h // rate, w // rate), mode="bilinear", align_corners=False)
    c = x_main.shape[1]
    o = _conv(sd, name + ".offset_conv1.0", torch.cat([inpfeat, x_main], dim=1), padding=0)
    o = F.silu(_gn(sd, name + ".offset_conv1.1", o))
    o = _conv(sd, name + ".offset_conv1.3", o, padding=3, groups=c)
    o = F.silu(_gn(sd, name + ".offset_conv1.4", o))
    o = _conv(sd, name + ".offset_conv1.6", o, padding=0)
    if previous_offset is not None:
        o = torch.cat([o, previous_offset], dim=1)
    offset = F.silu(_gn(sd, name + ".offset_conv2.1", _conv(sd, name + ".offset_conv2.0", o)))
    out = _conv(sd, name + ".dcn.conv_offset", offset)
    o1, o2, mask = torch.chunk(out, 3, dim=1)
    warp = deform_conv2d(x_main, torch.cat((o1, o2), dim=1), sd[name + ".dcn.weight"], sd[name + ".dcn.bias"],
                         (1, 1), (1, 1), (1, 1), torch.sigmoid(mask))
    return warp, offset


def main_decoder(sd, dec_res, inpfeat, cfg, fidelity_ratio=1.0, trace=None):
    """MainDecoder.forward (:465-487)."""
    n = len(cfg["channel_multipliers"])
    top = "Level_%d" % 2 ** (n - 1)
    x, offset = twm(sd, "main_branch.align_func_dict." + top, dec_res[top], inpfeat, 2 ** (n - 1))
    if trace is not None:
        trace[top] = (x, offset)
    for scale in reversed(range(n - 1)):
        key = "Level_%d" % 2 ** scale
        x = _conv(sd, f"main_branch.pre_upsample_dict.{key}.1", F.interpolate(x, scale_factor=2, mode="nearest"))
        up = F.interpolate(offset, scale_factor=2, align_corners=False, mode="bilinear") * 2
        warp, offset = twm(sd, "main_branch.align_func_dict." + key, dec_res[key], inpfeat, 2 ** scale, up)
        if trace is not None:
            trace[key] = (warp, offset)
        x = resnet_block(sd, "main_branch.decoder_dict." + key, torch.cat([x, warp], dim=1))
    return dec_res["Level_1"] + fidelity_ratio * x


@torch.no_grad()
def vqfr_forward(sd, x, cfg, fidelity_ratio=1.0, code_idx=None, trace=None):
    """x (B, 3, 512, 512) -> dict(main_dec, enc_feat, idx (B, 256), score (B*256, 1024): the logits ("Predict") or the
    negated distances ("Nearest"), larger is better).  ``code_idx`` replaces the selection."""
    inpfeat = _conv(sd, "inpfeat_extraction", x)
    enc = encoder(sd, x, cfg)
    b, c, hh, ww = enc.shape
    tok = enc.permute(0, 2, 3, 1).reshape(-1, c)
    e = sd["quantizer.embedding.weight"]
    if cfg["code_selection_mode"] == "Predict":
        t = F.layer_norm(tok, (256,), sd["feat2index.0.weight"], sd["feat2index.0.bias"], 1e-5)
        score = F.linear(t, sd["feat2index.1.weight"], sd["feat2index.1.bias"])
    else:
        score = -(torch.sum(tok ** 2, dim=1, keepdim=True) + torch.sum(e ** 2, dim=1) - 2 * tok @ e.t())
    idx = score.argmax(dim=1)
    if code_idx is not None:
        idx = code_idx.reshape(-1).long()
    quant = e[idx].reshape(b, hh, ww, c).permute(0, 3, 1, 2)
    dec_res = decoder(sd, quant, cfg)
    main = main_decoder(sd, dec_res, inpfeat, cfg, fidelity_ratio, trace)
    return dict(main_dec=decoder_conv_out(sd, main), enc_feat=enc, idx=idx.reshape(b, hh * ww), score=score)


def vqfr_input(x_u8):
    """(B, 3, 128, 128) uint8 -> (B, 3, 512, 512) f32 in [-1, 1): each pixel a 4 x 4 block."""
    x = (torch.as_tensor(x_u8).float() - 128.0) / 128.0
    return x.repeat_interleave(4, dim=2).repeat_interleave(4, dim=3).contiguous()


def pixels(n, count, seed):
    """``count`` seeded flat pixel indices of a 512 x 512 grid per face, sorted."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(512 * 512, generator=g)[:count].sort()[0] for _ in range(n)])


def take(t, pix):
    """(B, C, 512, 512), (B, K) flat indices -> (B, C, K)."""
    return torch.stack([t[b].reshape(t.shape[1], -1)[:, pix[b].long()] for b in range(t.shape[0])])

