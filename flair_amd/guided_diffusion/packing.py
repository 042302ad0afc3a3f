"""The one place that knows how weights are packed for the kernels ("Weight packing").

Every network keeps its fp32 parameters under the reference's state-dict names and, next to them, a one-time repack in the
kernels' own format: conv weights as ``[Cout][taps][Cin]`` in the compute dtype, eval-mode BatchNorms folded in, output
channels zero-padded, f32 biases and norm parameters.  Each module's ``pack(dtype, device)`` stores all of it in ONE dict,
``self._pk`` (tensors, nested containers of tensors, plain ints), which is what ``checkpoint.export_packed`` ships.
``PackedModel`` is the "pack once, invalidate on change" protocol of the networks themselves.
"""
import torch

from .. import ops


def dev_f32(p, device):
    """p as a detached f32 contiguous tensor on ``device`` (p itself when it already is one)."""
    t = p.detach()
    if t.device != torch.device(device) or t.dtype != torch.float32 or not t.is_contiguous():
        t = t.to(device=device, dtype=torch.float32).contiguous()
    return t


def pack_w(w, dtype, device, segs=None, cout_pad=None):
    """(Cout, Cin, *k) or (Cout, Cin) f32 -> packed [Cout][taps][Cin] in ``dtype``.  segs: (real, padded) widths of the
    input segments (default: one segment padded to the K step); cout_pad: zero output channels appended up to that width."""
    w = w.detach().to(device)
    if w.dim() == 2:
        w = w[:, :, None, None]
    cin = w.shape[1]
    return ops.pack_conv_weight(w, segs or [(cin, ops.pad_channels(cin, dtype))], dtype, cout_pad)


def pad_cout(c, g=4):
    """Output width of a convolution whose real width need not be a multiple of ``g`` channels."""
    return (c + g - 1) // g * g


def pad_bias(b, cpad):
    """b zero-extended to cpad entries."""
    return torch.cat([b, b.new_zeros(cpad - b.shape[0])]).contiguous()


def fold_bn(conv, bn):
    """conv's weight / bias (f32) with an eval-mode BatchNorm after it folded in (bn may be None)."""
    w = conv.weight.detach().float()
    b = conv.bias.detach().float() if conv.bias is not None else w.new_zeros(w.shape[0])
    if bn is not None:
        g = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        w = w * g.view(-1, 1, 1, 1)
        b = (b - bn.running_mean.detach().float()) * g + bn.bias.detach().float()
    return w, b


def packed_conv(conv, bn, dtype, device, cout_pad=None):
    """dict(w=, b=, cout=) of conv followed by an eval-mode BatchNorm (bn may be None), the output channels zero-padded to
    cout_pad (default: the next multiple of 4)."""
    w, b = fold_bn(conv, bn)
    cpad = cout_pad if cout_pad is not None else pad_cout(w.shape[0])
    return dict(w=pack_w(w, dtype, device, cout_pad=cpad), b=pad_bias(b.to(device), cpad), cout=cpad)


def run_conv(x, pk, conv, act=ops.ACT_NONE, **kw):
    """ops.conv of a ``packed_conv`` dict; kernel size and stride are read from ``conv``."""
    k = conv.kernel_size[0]
    return ops.conv(x, pk["w"], pk["b"], pk["cout"], (1, k, k), stride=conv.stride[0], act=act, **kw)


def pk_int(name):
    """Class attribute for a plain int that lives in ``_pk`` (so that a blob carries it): where a block's embedding
    linear starts in its network's batched embedding matrix.  ``pack`` takes it as an argument; whoever packs one block
    on its own may also assign it afterwards (``block.film_off = off``), packed or not."""
    def fset(self, value):
        self.__dict__.setdefault("_pk", {})[name] = value
    return property(lambda self: self._pk[name], fset)


class LinearStack:
    """A network's embedding linears batched into one matrix (one launch per step evaluates them all)."""

    def __init__(self):
        self.linears, self.width = [], 0

    def add(self, lin):
        """-> the row at which ``lin`` starts in the batched matrix."""
        off = self.width
        self.linears.append(lin)
        self.width += lin.out_features
        return off

    def cat(self, device):
        """-> (W, b): the f32 weights and biases of every added linear, concatenated along the output rows."""
        return (torch.cat([dev_f32(lin.weight, device) for lin in self.linears]).contiguous(),
                torch.cat([dev_f32(lin.bias, device) for lin in self.linears]).contiguous())


def invalidate_packed(model):
    """``model.invalidate_packed()``; a foreign container that merely carries a ``_packed_key`` has it cleared."""
    if isinstance(model, PackedModel):
        model.invalidate_packed()
    elif hasattr(model, "_packed_key"):
        model._packed_key = None


class PackedModel:
    """Mixin in front of ``nn.Module``: the packed copies are built on the first forward and rebuilt after anything that makes
    them stale (a state dict, a dtype change, a weight broadcast).  ``_packed_key`` is (dtype, device) of the valid copies."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.dtype = torch.float32
        self._packed_key = None

    def invalidate_packed(self):
        """Subclasses extend this with whatever else was derived from the packed weights (captured graphs ...)."""
        self._packed_key = None

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate_packed()
        return out

    def convert_to_bf16(self):
        self.dtype = torch.bfloat16
        self.invalidate_packed()
        return self

    def convert_to_fp32(self):
        self.dtype = torch.float32
        self.invalidate_packed()
        return self

    def _ensure_packed(self, device):
        key = (self.dtype, device)
        if self._packed_key != key:
            self._pack_all(self.dtype, device)
            self._packed_key = key

    def _pack_all(self, dtype, device):
        """Default: every module that has a ``pack`` (the model itself included) packs its own parameters, once."""
        for m in self.modules():
            if hasattr(m, "pack"):
                m.pack(dtype, device)
