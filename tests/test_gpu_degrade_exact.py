"""The data-consistency operators of csrc/degrade.hip, judged bit for bit where the answer is unique and per element against
float64 where the arithmetic is rounded.  tests/degrade_ref.py holds the references, the data and the bounds (n u S per
element, n counted from the kernel source); tests/test_degrade_exact_cpu.py proves them sound and sharp and shows which
comparison rejects which mutant.

  A  bit for bit   flair_depthwise_filter on integers (Down, Up at three stuffing offsets, InvHtH through the generic and
                   the tiled kernel, reflect at the smallest legal size, non-square and even filters, stride 3, more than
                   one grid of outputs) and on isolated impulses, whose response is the real inv / down / up filter itself;
                   flair_matmul_f32 and flair_gather_mac_f32 on integers; the quantised levels of both JPEG entries with a
                   selector matrix for the DCT (identity: exact ties on the chroma planes must round half to even; cyclic
                   shift: direction, transposition and table orientation)
  B  per element   flair_gather_mac_f32 with Resizer's cubic tables; the decoded JPEG image against jpeg_ycc_to_rgb in
                   float64 on the exactly known decoded planes; pseudoSR.A on the smallest frame

Every entry is called through ops on tests/util.py:flat_guarded buffers: inputs between NaNs, outputs between sentinels,
both checked after the call.  A ratio above 1 or a differing bit is a finding about the kernel, never a reason to widen."""
import numpy as np
import pytest
import torch

from tests import degrade_ref as R
from tests.util import (IN_FILL, OUT_FILL, assert_bits_equal, assert_exact_headroom, assert_flat_untouched, bits, flat_guarded,
                        parity_log)

pytestmark = pytest.mark.gpu
FP = torch.float32


def _ops():
    from flair_amd import ops
    return ops


def _in(dev, t, dtype=FP):
    """A cpu tensor as a dense device tensor between NaNs (an int32 one between zeros)."""
    return flat_guarded(tuple(t.shape), dtype, dev, IN_FILL if dtype == FP else 0, t)


def _out(dev, shape, pad=64):
    return flat_guarded(tuple(shape), FP, dev, OUT_FILL, pad=pad)


def _check_guards(ins, outs, what):
    torch.cuda.synchronize()
    for i, (buf, _, before) in enumerate(ins):
        assert_flat_untouched(buf, before, None, f"{what}: input {i}")
    for i, (buf, v, before) in enumerate(outs):
        assert_flat_untouched(buf, before, v, f"{what}: output {i}")


def log_bits(what):
    parity_log(f"degrade_exact {what}: bit for bit")


def log_ratio(what, r):
    parity_log(f"degrade_exact {what}: worst err / bound = {r:.3f}")


def _run_filter(dev, x, K, kw, unaligned=False):
    """ops.depthwise_filter between guards -> the output on the cpu.  unaligned: the output slice starts 4 bytes past a
    16-byte boundary, which sends a 39 x 39 call to the generic kernel by the entry's own rule."""
    ins = [_in(dev, x), _in(dev, K)]
    out = _out(dev, (*x.shape[:2], *kw["out_hw"]), pad=65 if unaligned else 64)
    assert (out[1].data_ptr() % 16 != 0) == unaligned
    _ops().depthwise_filter(ins[0][1], ins[1][1], out=out[1], **kw)
    _check_guards(ins, [out], f"depthwise_filter {kw}")
    return out[1].cpu()


# ================================================================================================ depthwise filter
@pytest.mark.parametrize("name", list(R.FILTER_CASES))
def test_depthwise_filter_int_bits(dev, name):
    c = R.FILTER_CASES[name]
    x, K, _, ref, S = R.filter_int_case(name)
    assert_exact_headroom(S)
    if name == "two_trips":
        assert ref.numel() > R.GRID        # 1,080,000 outputs on 4096 x 256 threads: 31,424 threads run twice
    got = _run_filter(dev, x, K, c["kw"], c.get("unaligned", False))
    assert_bits_equal(got, ref.float(), f"depthwise_filter {name}")
    log_bits(f"depthwise_filter {name} filter {tuple(K.shape)} planes {tuple(x.shape)} -> {c['kw']['out_hw']}")


@pytest.mark.parametrize("reflect", [False, True], ids=["replicate", "reflect"])
@pytest.mark.parametrize("i", range(len(R.TILED_CASES)), ids=[f"{a[0]}x{a[1]}to{b[0]}x{b[1]}off{o}" for a, b, o in R.TILED_CASES])
def test_depthwise_filter_tiled_int_bits(dev, i, reflect):
    """39 x 39 taps, stride 1, outputs of whole 32 x 32 tiles: the tiled kernel; the same call into an output 4 bytes off a
    16-byte boundary: the generic one.  Both exact, hence equal."""
    hw, out_hw, off = R.TILED_CASES[i]
    x, K, _, ref, S = R.tiled_int_case(i, reflect)
    assert_exact_headroom(S)
    kw = dict(pad=19, out_offset=off, out_hw=out_hw, reflect=reflect)
    tiled, generic = _run_filter(dev, x, K, kw), _run_filter(dev, x, K, kw, unaligned=True)
    assert_bits_equal(tiled, ref.float(), f"depthwise_filter tiled {hw} -> {out_hw} off {off} reflect {reflect}")
    assert_bits_equal(generic, ref.float(), f"depthwise_filter generic {hw} -> {out_hw} off {off} reflect {reflect}")
    assert torch.equal(bits(tiled), bits(generic))
    log_bits(f"depthwise_filter tiled and generic 39 x 39, {hw} -> {out_hw} out_offset {off} reflect {reflect}")


@pytest.mark.parametrize("name", list(R.IMPULSE_CASES))
def test_depthwise_filter_impulse_response_is_the_filter(dev, name):
    """Every output is one product of a real tap and +-2^k, plus zeros: one correct value.  inv runs through the tiled
    kernel (96 x 128 outputs) and, into an unaligned output, through the generic one."""
    x, K, kw, want = R.impulse_case(name)
    direct, seen = R.impulse_expected(name)
    assert bool(seen.all()) and torch.equal(direct, want)
    got = _run_filter(dev, x, K, kw)
    assert_bits_equal(got, want, f"depthwise_filter impulses {name}")
    if name == "inv":
        assert_bits_equal(_run_filter(dev, x, K, kw, unaligned=True), want, "depthwise_filter impulses inv, generic kernel")
    log_bits(f"depthwise_filter impulse response of the real {name} filter, {int(seen.sum())} taps shown")


def test_depthwise_filter_refuses_a_second_reflection(dev):
    """F.pad(mode='reflect') raises when the pad reaches the plane's size; pad_index would clamp.  The entry refuses, and
    writes nothing."""
    from flair_amd import _lib
    K = R.int_filter(9, 9)
    for shape, out_hw in (((1, 2, 4, 6), (4, 6)), ((1, 2, 5, 4), (5, 4)), ((1, 2, 5, 6), (6, 6))):
        ins = [_in(dev, R.int_planes(shape)), _in(dev, K)]
        out = _out(dev, (1, 2) + out_hw)
        with pytest.raises(_lib.FlairHipError, match="flair_depthwise_filter: reflect padding reaches"):
            _ops().depthwise_filter(ins[0][1], ins[1][1], pad=4, out_hw=out_hw, reflect=True, out=out[1])
        torch.cuda.synchronize()
        assert_flat_untouched(out[0], out[2], None, "refused depthwise_filter")


def test_pseudosr_forward_on_the_smallest_frame(dev):
    """The one caller of the reflect form, pseudoSR.A (9 x 9 filter, pad 4), on an 8 x 12 frame, the smallest multiple of the
    factor that the refusal above lets through: per element against the definition, n = 81 fmaf roundings."""
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion import pseudoSR as psr
    Ks, pre, f = R.real_filters()
    x = torch.rand(1, 3, 8, 12, generator=torch.Generator().manual_seed(8)) * 2 - 1
    A = psr.pseudoSR(psr.Get_pseudoSR_Conf(4), upscale_kernel=wl.synthetic_blur_kernel(sigma=1.8), kernel_indx=10).WrapArchitecture_PyTorch().to(dev)
    got = A.A(x.to(dev)).cpu()
    ref, S = R.filter_ref64(x, Ks["down"], 4, out_hw=(8, 12), reflect=True)
    r = R.within(got, ref[:, :, pre:, pre:], 81 * R.U * S[:, :, pre:, pre:], "pseudoSR.A 8 x 12")
    log_ratio("pseudoSR.A 8 x 12 (reflect, 81 taps)", r)


# ================================================================================================ matmul
@pytest.mark.parametrize("shared", R.MATMUL_SHARED)
@pytest.mark.parametrize("M,N,K", R.MATMUL_SHAPES)
def test_matmul_int_bits(dev, M, N, K, shared):
    a, b, ref, S = R.matmul_case(M, N, K, shared)
    assert_exact_headroom(S)
    ins = [_in(dev, a), _in(dev, b)]
    out = _out(dev, (3, M, N))
    _ops().matmul(ins[0][1], ins[1][1], out=out[1])
    _check_guards(ins, [out], "matmul")
    assert_bits_equal(out[1].cpu(), ref.float(), f"matmul {M}x{N}x{K} shared={shared}")
    log_bits(f"matmul {M}x{N}x{K} batch 3 shared={shared}")


def test_matmul_batch_strides_beyond_the_matrices(dev):
    """Batch strides of M K + 5 and K N + 3 with NaN in the gaps, through the C entry."""
    from flair_amd import _lib
    M, N, K = 17, 33, 50
    a, b, ref, S = R.matmul_case(M, N, K, "none")
    sa, sb = M * K + 5, K * N + 3
    A = torch.full((3, sa), float("nan"))
    B = torch.full((3, sb), float("nan"))
    A[:, :M * K], B[:, :K * N] = a.reshape(3, -1), b.reshape(3, -1)
    ins = [_in(dev, A), _in(dev, B)]
    out = _out(dev, (3, M, N))
    _lib.call.flair_matmul_f32(ins[0][1], sa, ins[1][1], sb, out[1], 3, M, N, K)
    _check_guards(ins, [out], "matmul strided")
    assert_bits_equal(out[1].cpu(), ref.float(), "matmul with batch strides")
    log_bits(f"matmul {M}x{N}x{K} batch strides {sa}, {sb}")


def test_matmul_refuses_what_the_grid_cannot_hold(dev):
    """batch and ceil(M / 16) are grid extents: 65535 passes, 65536 is refused before the launch."""
    from flair_amd import _lib
    ops = _ops()
    g = torch.Generator().manual_seed(1)
    a, b = R.signed_ints((65535, 1, 1), 1, 16, g), R.signed_ints((65535, 1, 1), 1, 16, g)
    got = ops.matmul(a.to(dev), b.to(dev))
    assert_bits_equal(got.cpu(), a * b, "matmul batch 65535")
    one = torch.ones(65536, 1, 1, device=dev)
    out = _out(dev, (65536, 1, 1))
    with pytest.raises(_lib.FlairHipError, match="flair_matmul_f32: batch = 65536"):
        ops.matmul(one, one, out=out[1])
    rows = 65535 * 16 + 1
    tall = _out(dev, (1, rows, 1))
    with pytest.raises(_lib.FlairHipError, match=r"flair_matmul_f32: batch = 1 and ceil\(M / 16\) = 65536"):
        ops.matmul(torch.ones(rows, 1, device=dev), torch.ones(1, 1, device=dev), out=tall[1])
    torch.cuda.synchronize()
    assert_flat_untouched(out[0], out[2], None, "refused matmul")
    assert_flat_untouched(tall[0], tall[2], None, "refused matmul")
    rows -= 1
    a = R.signed_ints((rows, 1), 1, 16, g)
    assert_bits_equal(ops.matmul(a.to(dev), torch.full((1, 1), 3.0, device=dev)).cpu(), (a * 3.0)[None], "matmul M = 65535 * 16")


# ================================================================================================ gather-MAC
@pytest.mark.parametrize("name", list(R.GATHER_CASES))
def test_gather_mac_int_bits(dev, name):
    outer, Lin, inner, taps, Lout = R.GATHER_CASES[name]
    x, fov, w, ref, S = R.gather_int_case(name)
    assert_exact_headroom(S)
    if name == "two_trips":
        assert ref.numel() > R.GRID
    ins = [_in(dev, x), _in(dev, fov, torch.int32), _in(dev, w)]
    out = _out(dev, (outer, Lout, inner))
    _ops().gather_mac(ins[0][1], outer, Lin, inner, ins[1][1], ins[2][1], out=out[1])
    _check_guards(ins, [out], "gather_mac")
    assert_bits_equal(out[1].cpu(), ref.float(), f"gather_mac {name}")
    log_bits(f"gather_mac {name} outer {outer} {Lin} -> {Lout} inner {inner} taps {taps}")


@pytest.mark.parametrize("Lin,Lout", [(64, 16), (16, 64)])
def test_gather_mac_resizer_tables(dev, Lin, Lout):
    """Resizer's cubic tables (16 taps antialiased down, 4 up): |got - ref64| <= (taps + 1) u sum_k |w x|."""
    x, fov, w = R.resizer_case(Lin, Lout)
    ref, S = R.gather_ref64(x, fov, w)
    ins = [_in(dev, x), _in(dev, fov, torch.int32), _in(dev, w)]
    out = _out(dev, ref.shape)
    _ops().gather_mac(ins[0][1], x.shape[0], Lin, x.shape[2], ins[1][1], ins[2][1], out=out[1])
    _check_guards(ins, [out], "gather_mac resizer")
    r = R.within(out[1].cpu(), ref, R.N_GATHER(fov.shape[0]) * R.U * S, f"gather_mac cubic {Lin} -> {Lout}")
    log_ratio(f"gather_mac cubic table {Lin} -> {Lout} taps {fov.shape[0]}", r)


# ================================================================================================ JPEG
def _run_jpeg(dev, x, mode, entry):
    D, q1, q2 = R.MODES[mode]
    N, _, H, W = x.shape
    ins = [_in(dev, x)]
    outs = [_out(dev, (N, 3, H, W)), _out(dev, (N, 1, H, W)), _out(dev, (N, 2, H // 2, W // 2))]
    ws = _out(dev, (N, 3, H, W)) if entry == "square" else None
    _ops().jpeg_roundtrip(ins[0][1], q1.reshape(-1), q2.reshape(-1), D.reshape(-1), entry=entry, out=outs[0][1],
                          levels=(outs[1][1], outs[2][1]), workspace=None if ws is None else ws[1])
    _check_guards(ins, outs + ([ws] if ws else []), f"jpeg_roundtrip {entry} {mode}")
    return tuple(o[1].cpu() for o in outs)


JPEG_RUNS = [("hw",) + s for s in R.JPEG_SIZES_HW] + [("square",) + s for s in R.JPEG_SIZES_SQUARE]


@pytest.mark.parametrize("mode", list(R.MODES))
@pytest.mark.parametrize("entry,H,W,N", JPEG_RUNS, ids=[f"{e}-{h}x{w}x{n}" for e, h, w, n in JPEG_RUNS])
def test_jpeg_levels_with_selector_matrices(dev, entry, H, W, N, mode):
    """dct8 = I: the level is rintf((plane - 128) / q) of a known value; at least a quarter of the chroma coefficients are
    exact ties (Cb - 128 = b / 2, q = 1) and must round half to even, and no luma coefficient is within 1e-3 of a tie.
    dct8 = the cyclic shift P with 64 distinct powers of two for a table: the levels are (P blk P^T) / q and nothing is
    lost, so the decoded planes are the input blocks.  The image: jpeg_ycc_to_rgb in float64 on those planes, 5 u S."""
    x, b = R.jpeg_case(H, W, N)
    e = R.jpeg_expected(b, mode)
    if mode == "identity":
        share = R.tie_share(np.concatenate([e["coefq_cb"].ravel(), e["coefq_cr"].ravel()]))
        assert share >= 0.25, share
        assert float(R._frac_tie_distance(e["coefq_l"]).min()) >= 1e-3
    img, luma, chroma = _run_jpeg(dev, x, mode, entry)
    what = f"jpeg {entry} {N}x3x{H}x{W} dct8={mode}"
    assert_bits_equal(chroma, e["chroma"], what + " chroma levels")
    assert_bits_equal(luma, e["luma"], what + " luma levels")
    r = R.within(img, e["ref64"], e["bound"], what + " image")
    log_bits(what + " levels")
    log_ratio(what + " image", r)


@pytest.mark.parametrize("mode", list(R.MODES))
@pytest.mark.parametrize("H,W,N", R.JPEG_SIZES_SQUARE)
def test_jpeg_entries_agree_with_selector_matrices(dev, H, W, N, mode):
    x, _ = R.jpeg_case(H, W, N)
    for one, two in zip(_run_jpeg(dev, x, mode, "hw"), _run_jpeg(dev, x, mode, "square")):
        assert torch.equal(bits(one), bits(two))
