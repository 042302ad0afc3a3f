"""Helpers shared by the parity tests."""
import pytest
import torch


def to_clip(x, dtype, device, pad_to=None):
    """(N,C,H,W) f32 cpu -> (N,H,W,C[padded]) clip tensor on device."""
    y = x.permute(0, 2, 3, 1).contiguous()
    if pad_to is not None and pad_to > y.shape[3]:
        y = torch.cat([y, y.new_zeros(*y.shape[:3], pad_to - y.shape[3])], dim=3)
    return y.to(device=device, dtype=dtype).contiguous()


def from_clip(y, c=None):
    y = y.float().cpu()
    if c is not None:
        y = y[..., :c]
    return y.permute(0, 3, 1, 2).contiguous()


def rb(x, dtype):
    """Round an f32 cpu tensor through `dtype` (so the CPU reference sees what the GPU sees)."""
    return x.to(dtype).float()


# Tolerances (stated per dtype, relative to the reference's max magnitude):
#   f32 : accumulation-order differences only            -> 2e-5 * max|ref| + 1e-6
#   bf16: output rounding (2^-9 rel) + bf16 intermediates -> 1.6e-2 * max|ref| + 1e-3
TOL = {torch.float32: (2e-5, 1e-6), torch.bfloat16: (1.6e-2, 1e-3)}


def assert_close(got, ref, dtype, what="", scale=1.0):
    rel, ab = TOL[dtype]
    err = (got - ref).abs().max().item()
    bound = scale * rel * ref.abs().max().item() + ab
    assert err <= bound, f"{what}: max|err|={err:.3e} > {bound:.3e} (max|ref|={ref.abs().max().item():.3e})"
    return err


def parity_log(line):
    """Append one measured-error line to gpurun_out/r04_parity.txt (merged back from the GPU box; the copy under
    profiles/ is the committed record).  Never fails a test."""
    import os
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        d = os.path.join(root, "gpurun_out")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "r04_parity.txt"), "a") as f:
            f.write(line.rstrip() + "\n")
    except OSError:
        pass
    print(line)


# The fp32 fixtures under tests/golden/ were written by tests/golden/make_golden.py with torch on 8 intra-op CPU threads.
# How torch splits a CPU reduction over threads sets its summation order, and the networks amplify that last-bit
# difference about a thousandfold (a whole-network output moves by ~1e-3 relative at 1, 3 or 16 threads), so the CPU
# oracle is compared with a fixture on the fixture's own thread count.
FIXTURE_THREADS = 8


@pytest.fixture
def fixture_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(FIXTURE_THREADS)
    yield
    torch.set_num_threads(n)


# Guarded views: a clip tensor placed as a channel slice [coff, coff + C) of a wider buffer, with one guard frame before
# and one after it.  Everything outside the view holds a sentinel: NaN around inputs (a kernel that reads outside its
# input turns its result into NaN), a finite, bf16-exact value around outputs (a kernel that writes outside its output
# changes it).  The guards also keep stray accesses inside the test's own allocation.
IN_FILL = float("nan")
OUT_FILL = -1232.0          # exact in bf16 and f32
# Around the logits of an arg-max: `NaN > best` is false, so a NaN guard never shows a read past the last class; a finite
# value above every logit (exact in bf16) wins instead and changes the index.
ARGMAX_FILL = 30720.0       # 15 * 2^11


def guarded(T, H, W, C, dtype, dev, *, coff=0, ld=None, fill=OUT_FILL):
    """-> (buf, view): buf (T + 2, H, W, ld) filled with `fill`; view = buf[1:T + 1, :, :, coff:coff + C]."""
    ld = coff + C if ld is None else ld
    assert coff >= 0 and coff + C <= ld, (coff, C, ld)
    buf = torch.full((T + 2, H, W, ld), fill, dtype=dtype, device=dev)
    return buf, buf[1:T + 1, :, :, coff:coff + C]


def bits(t):
    """Integer view of a tensor's bits (NaN patterns compare as numbers)."""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def view_mask(buf, view):
    """Boolean mask over buf of the elements of `view` (a [f0:f0 + T, :, :, c0:c0 + C] slice of buf)."""
    assert view.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
    off = view.storage_offset() - buf.storage_offset()
    frame = buf.shape[1] * buf.shape[2] * buf.shape[3]
    f0, c0 = off // frame, off % frame
    assert c0 < buf.shape[3] and tuple(view.shape[1:3]) == tuple(buf.shape[1:3])
    m = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    m[f0:f0 + view.shape[0], :, :, c0:c0 + view.shape[3]] = True
    return m


def assert_untouched(buf, before, view=None, what=""):
    """buf is bitwise equal to `before` (its copy taken before the launch) outside `view`; everywhere when view is None."""
    changed = bits(buf) != bits(before)
    if view is not None:
        changed &= ~view_mask(buf, view)
    n = int(changed.sum().item())
    if n:
        idx = changed.nonzero()[0].tolist()
        where = "outside the view" if view is not None else "in a read-only buffer"
        raise AssertionError(f"{what}: {n} element(s) changed {where}, first at {idx}: "
                             f"{before[tuple(idx)].item()!r} -> {buf[tuple(idx)].item()!r}")


def flat_guarded(shape, dtype, dev, fill, src=None, pad=64):
    """A dense tensor of `shape` inside a longer 1-D allocation of `fill`, for entries that take no stride: pad elements
    before and after (a multiple of 16 bytes in every dtype here, so the slice keeps the allocation's alignment).
    -> (buf, dense view, copy of buf taken after `src` was written)."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
    v = buf[pad:pad + n].view(shape)
    if src is not None:
        v.copy_(src.to(dev, dtype).view(shape))
    return buf, v, buf.clone()


def assert_flat_untouched(buf, before, view=None, what=""):
    """The 1-D allocation is bitwise equal to `before` outside the dense slice `view` (everywhere when view is None)."""
    changed = bits(buf) != bits(before)
    if view is not None:
        o = view.storage_offset() - buf.storage_offset()
        changed[o:o + view.numel()] = False
    n = int(changed.sum().item())
    if n:
        i = int(changed.nonzero()[0].item())
        where = "outside the tensor" if view is not None else "in a read-only buffer"
        raise AssertionError(f"{what}: {n} element(s) changed {where}, first at {i}: {before[i].item()!r} -> {buf[i].item()!r}")


# Exact arithmetic (tests/test_gpu_exact.py, tests/test_exact_cpu.py): on integer-valued data every product and every
# partial sum of a convolution is an integer below 2^24, hence exact in f32 in ANY accumulation order, tile shape, split
# or matrix instruction; the one correct output is the exact value (f32) or its round-to-nearest-even (bf16).
def int_tensor(shape, lo, hi, g):
    """Uniform integers in [lo, hi] as float32 (exact in bf16 for |v| <= 256)."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def assert_exact_headroom(abs_sum):
    """abs_sum: the float64 tensor conv(|x|, |w|) + |bias| + |frame_bias| + sum |res| -- a bound on every partial sum in
    every order.  Below 2^24 all of them are integers (or multiples of the data's power-of-two step) that f32 holds exactly."""
    assert abs_sum.dtype == torch.float64
    m = abs_sum.max().item()
    assert m < 2 ** 24, f"partial sums up to {m:.0f} >= 2^24: not exact in f32"
    return m


def assert_bits_equal(got, ref, what="", tile=None):
    """got and ref (same shape and dtype, (T, H, W, C) clip layout when `tile` is given) are equal bit for bit, compared
    through bits().  The sign of a zero is left open: it is no part of the arithmetic contract, and the kernels' two
    spellings of ReLU differ in it (`v > 0 ? v : 0` gives +0, `fmaxf(v, v * 0)` gives -0 for v < 0).
    tile = (rows, cols, couts): also counts the differing elements by (h % rows, w % cols, c % couts), so that a failure
    names the lane, the row or the store group at fault."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    ne = (bits(got) != bits(ref)) & ~((got == 0) & (ref == 0))
    n = int(ne.sum().item())
    if not n:
        return
    idx = ne.nonzero()
    first = tuple(idx[0].tolist())
    d = (got.double() - ref.double()).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    msg = (f"{what}: {n} of {ne.numel()} element(s) differ in bits; first at {list(first)}: got {got[first].item()!r}, "
           f"expected {ref[first].item()!r}; largest |difference| {d[ne].max().item():.6g}")
    if tile is not None and got.dim() == 4:
        rows, cols, couts = tile
        key = (idx[:, 1] % rows) * (cols * couts) + (idx[:, 2] % cols) * couts + idx[:, 3] % couts
        cnt = torch.bincount(key, minlength=rows * cols * couts).view(rows, cols, couts)
        msg += (f"\n  by h % {rows}: {cnt.sum((1, 2)).tolist()}\n  by w % {cols}: {cnt.sum((0, 2)).tolist()}"
                f"\n  by c % {couts}: {cnt.sum((0, 1)).tolist()}")
        top = cnt.flatten().argsort(descending=True)[:8].tolist()
        msg += "\n  most hit (h % rows, w % cols, c % couts): " + ", ".join(
            f"({k // (cols * couts)}, {k // couts % cols}, {k % couts}): {int(cnt.flatten()[k])}" for k in top if cnt.flatten()[k] > 0)
    raise AssertionError(msg)
