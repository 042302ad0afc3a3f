"""The warp and resize kernels of csrc/warp.hip against the float64 closed forms of tests/resample_ref.py, per element.

Sources are integers in [-8, 8] (D = 16 bounds a neighbour difference), flows are quarter-pixel with a fixed set of pinned
landings, and every element must satisfy

    |got - ref64| <= out_rounding(ref64, dtype) + 4 * D * 2^-24 * m,     m = the largest extent,

the bound derived in tests/resample_ref.py; tests/test_resample_exact_cpu.py shows that the f32 reference on the CPU meets
it with 4x headroom and that no mutant of a closed form does.  With quarter-pixel flows the exact result is a bf16 number,
so in bf16 too the bound is the coordinate term, about 1e-4.  Inputs lie in NaN-guarded channel views, outputs in views
whose surroundings must keep their sentinel.  The worst err / bound per kernel and dtype goes to parity_log
(profiles/resample_parity.txt is the record).
"""
import pytest
import torch

from tests import resample_ref as R
from tests.util import IN_FILL, OUT_FILL, assert_untouched, guarded, parity_log

pytestmark = pytest.mark.gpu
BF, FP = torch.bfloat16, torch.float32
DTYPES = [FP, BF]
ids = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c).replace("torch.", "")


def _ops():
    from flair_amd import ops
    return ops


def _g(dtype):
    """Elements in 16 bytes: the granularity of the vector kernels' channel offsets and strides."""
    return 8 if dtype == BF else 4


def placed(t, dtype, dev, coff=None, ld=None):
    """t (F, H, W, C) f32 -> a channel view holding it, between NaN frames and NaN channels."""
    F_, H, W, C = t.shape
    gr = _g(dtype)
    coff = gr if coff is None else coff
    buf, v = guarded(F_, H, W, C, dtype, dev, coff=coff, ld=C + 2 * gr if ld is None else ld, fill=IN_FILL)
    v.copy_(t.to(dev))
    return v


class Out:
    """An output view between sentinel frames and channels; done() checks that only the view was written."""

    def __init__(self, shape, dtype, dev, coff=None, ld=None):
        F_, H, W, C = shape
        gr = _g(dtype)
        coff = 2 * gr if coff is None else coff
        self.buf, self.view = guarded(F_, H, W, C, dtype, dev, coff=coff, ld=C + 3 * gr if ld is None else ld, fill=OUT_FILL)
        self.before = self.buf.clone()

    def done(self, what):
        torch.cuda.synchronize()
        assert_untouched(self.buf, self.before, self.view, what)
        return self.view.float().cpu()


def log(kernel, dtype, case, ratio):
    parity_log(f"resample_exact {kernel} {str(dtype).replace('torch.', '')} {case}: worst err/bound {ratio:.3f}")


# --------------------------------------------------------------------------------------------------------------- warps
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("border", [False, True], ids=["zeros", "border"])
@pytest.mark.parametrize("case", R.WARP_CASES, ids=ids)
def test_flow_warp_exact(dev, dtype, border, case):
    ops = _ops()
    H, W, C = case
    d = R.warp_case(H, W, C)
    out = Out(d["x"].shape, dtype, dev)
    ops.flow_warp(placed(d["x"], dtype, dev), d["flow"].to(dev), border=border, out=out.view)
    what = f"flow_warp {case} border={border}"
    ratio = R.assert_within(out.done(what), R.warp_ref64(d["x"], d["flow"], border), dtype, max(H, W), what)
    log("flow_warp", dtype, f"{case} border={border}", ratio)


def run_warp2(ops, d, dtype, dev):
    prop, feat2 = placed(d["x"], dtype, dev), placed(d["x2"], dtype, dev, coff=0)
    c1, c2 = Out(d["x"].shape, dtype, dev), Out(d["x"].shape, dtype, dev, coff=_g(dtype))
    f1d, f2d = d["flow"].to(dev), d["flow2"].to(dev)
    for f in range(d["x"].shape[0]):
        s = slice(f, f + 1)
        ops.vsrpp_warp2(prop[s], feat2[s], f1d[s], f2d[s], c1.view[s], c2.view[s])
    return c1, c2


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("case", R.WARP_CASES, ids=ids)
def test_vsrpp_warp2_exact(dev, dtype, case):
    H, W, C = case
    d = R.warp_case(H, W, C)
    c1, c2 = run_warp2(_ops(), d, dtype, dev)
    what = f"vsrpp_warp2 {case}"
    r1 = R.assert_within(c1.done(what), R.warp_ref64(d["x"], d["flow"], False), dtype, max(H, W), what + " cond1")
    r2 = R.assert_within(c2.done(what), R.warp_ref64(d["x2"], d["flow2"], False), dtype, max(H, W), what + " cond2")
    log("vsrpp_warp2", dtype, case, max(r1, r2))


def run_prep(ops, d, dtype, dev, second):
    """-> cond1, cond2 (Out), flow2_out (F, H, W, 2) f32 on the device, flowpad (F, H, W, P) on the device, P."""
    F_, H, W, C = d["x"].shape
    P = 2 * _g(dtype)
    prop, feat2 = placed(d["x"], dtype, dev), placed(d["x2"], dtype, dev, coff=0)
    c1, c2 = Out(d["x"].shape, dtype, dev), Out(d["x"].shape, dtype, dev, coff=_g(dtype))
    f1d, fpd = d["flow"].to(dev), d["flow_prev"].to(dev)
    f2o = torch.full((F_, H, W, 2), OUT_FILL, dtype=FP, device=dev)
    pad = torch.full((F_, H, W, P), 7.0, dtype=dtype, device=dev)
    for f in range(F_):
        s = slice(f, f + 1)
        if second:
            ops.vsrpp_prep(prop[s], feat2[s], f1d[s], fpd[s], c1.view[s], c2.view[s], f2o[s], pad[s])
        else:
            ops.vsrpp_prep(prop[s], None, f1d[s], None, c1.view[s], None, None, pad[s])
    return c1, c2, f2o, pad, P


def check_prep(d, dtype, second, got, what):
    c1, c2, f2o, pad, P = got
    H, W = d["x"].shape[1:3]
    m = max(H, W)
    c1v, c2v = c1.done(what), c2.done(what)
    f2 = f2o.cpu()
    ref = R.prep_ref64(d["x"], d["x2"], d["flow"], d["flow_prev"] if second else None, dtype, flow2=f2 if second else None)
    r = R.assert_within(c1v, ref["cond1"], dtype, m, what + " cond1")
    if second:
        # flow2_out samples flow_prev, whose neighbours differ by at most DP: the bound with DP in the place of D
        r = max(r, R.assert_within(f2, ref["flow2"], FP, m * R.DP / R.D, what + " flow2_out"))
        r = max(r, R.assert_within(c2v, ref["cond2"], dtype, m, what + " cond2"))
    else:
        assert bool((c2v == OUT_FILL).all()) and bool((f2 == OUT_FILL).all()), what + ": second-order outputs written"
    padc = pad.double().cpu()
    assert torch.equal(padc[..., :4], ref["flowpad"]), what + ": flowpad"
    assert bool((padc[..., 4:] == 7.0).all()), what + ": flowpad beyond channel 3"
    return r


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("second", [False, True], ids=["first_order", "second_order"])
@pytest.mark.parametrize("case", R.WARP_CASES, ids=ids)
def test_vsrpp_prep_exact(dev, dtype, second, case):
    H, W, C = case
    d = R.warp_case(H, W, C)
    order = f"{case} {'second' if second else 'first'} order"
    log("vsrpp_prep", dtype, order, check_prep(d, dtype, second, run_prep(_ops(), d, dtype, dev, second), "vsrpp_prep " + order))


@pytest.mark.parametrize("hw", [c[:2] for c in R.WARP_CASES], ids=ids)
def test_flow_compose_exact(dev, hw):
    H, W = hw
    d = R.compose_case(H, W)
    F_ = d["f1"].shape[0]
    b1, v1 = guarded(F_, H, W, 2, FP, dev, fill=IN_FILL)        # dense by contract: guard frames only
    b2, v2 = guarded(F_, H, W, 2, FP, dev, fill=IN_FILL)
    v1.copy_(d["f1"].to(dev))
    v2.copy_(d["f2"].to(dev))
    out = Out((F_, H, W, 2), FP, dev, coff=0, ld=2)
    _ops().flow_compose(v1, v2, out=out.view)
    what = f"flow_compose {hw}"
    log("flow_compose", FP, hw, R.assert_within(out.done(what), R.compose_ref64(d["f1"], d["f2"]), FP, max(H, W), what))


# ---- more than one grid: grid_for caps a launch at 4096 * 256 threads, beyond which the grid-stride loops (and the 32-bit
# index arithmetic of vsrpp_warp2_kernel) take a second trip
@pytest.mark.parametrize("kernel", ["flow_warp", "vsrpp_warp2", "vsrpp_prep"])
def test_warp_kernels_beyond_one_grid(dev, kernel):
    ops = _ops()
    H, W, C = R.BIG_WARP
    assert H * W * (C // 8) > 4096 * 256
    d = R.warp_case(H, W, C)
    what = f"{kernel} {R.BIG_WARP}"
    if kernel == "flow_warp":
        out = Out(d["x"].shape, BF, dev)
        ops.flow_warp(placed(d["x"], BF, dev), d["flow"].to(dev), out=out.view)
        r = R.assert_within(out.done(what), R.warp_ref64(d["x"], d["flow"], False), BF, max(H, W), what)
    elif kernel == "vsrpp_warp2":
        c1, c2 = run_warp2(ops, d, BF, dev)
        r = max(R.assert_within(c1.done(what), R.warp_ref64(d["x"], d["flow"], False), BF, max(H, W), what + " cond1"),
                R.assert_within(c2.done(what), R.warp_ref64(d["x2"], d["flow2"], False), BF, max(H, W), what + " cond2"))
    else:
        r = check_prep(d, BF, True, run_prep(ops, d, BF, dev, True), what)
    log(kernel, BF, f"{R.BIG_WARP} (beyond one grid)", r)


def test_flow_compose_beyond_one_grid(dev):
    H, W = R.BIG_COMPOSE
    assert H * W > 4096 * 256
    d = R.compose_case(H, W)
    got = _ops().flow_compose(d["f1"].to(dev), d["f2"].to(dev))
    torch.cuda.synchronize()
    what = f"flow_compose {R.BIG_COMPOSE}"
    ratio = R.assert_within(got.cpu(), R.compose_ref64(d["f1"], d["f2"]), FP, max(H, W), what)
    log("flow_compose", FP, f"{R.BIG_COMPOSE} (beyond one grid)", ratio)


# -------------------------------------------------------------------------------------------------------------- resize
def run_resize(ops, x, size, mode, dtype, dev, off_vector=True, **scales):
    """x (F, Hi, Wi, C) f32 -> the result (F, Ho, Wo, C) f32 on the CPU.  off_vector: channel views at offset 1 with a
    stride of C + 3 elements (the scalar kernel); otherwise dense 16-byte-aligned tensors."""
    F_, Hi, Wi, C = x.shape
    if off_vector:
        xin = placed(x, dtype, dev, coff=1, ld=C + 3)
        out = Out((F_, *size, C), dtype, dev, coff=2, ld=C + 5)
        ops.resize(xin, size, mode, channels=C, out=out.view, **scales)
        return out.done(f"resize mode {mode} {(Hi, Wi)}->{size}")
    xin = x.to(dev, dtype).contiguous()
    y = torch.full((F_, *size, C), OUT_FILL, dtype=dtype, device=dev)
    if C >= 16:         # what the dispatch to the vector kernels asks for
        assert xin.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0 and C % _g(dtype) == 0
    ops.resize(xin, size, mode, channels=C, out=y, **scales)
    torch.cuda.synchronize()
    return y.float().cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["bilinear", "bilinear_ac", "bicubic"])
@pytest.mark.parametrize("C", [2, 3])
def test_resize_exact(dev, dtype, mode, C):
    ops = _ops()
    worst = 0.0
    for hi in R.RESIZE_IN:
        for ho in R.RESIZE_OUT:
            x = R.resize_source(R.RESIZE_FRAMES, *hi, C)
            what = f"resize mode {mode} C={C} {hi}->{ho}"
            worst = max(worst, R.assert_within(run_resize(ops, x, ho, mode, dtype, dev), R.resize_ref64(x, ho, mode), dtype,
                                               R.resize_extent(hi, ho), what))
    log(f"resize_kernel mode {mode}", dtype, f"C={C}, 36 size pairs", worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["bilinear", "bilinear_ac", "bicubic"])
def test_resize_channel_scales(dev, dtype, mode):
    """scale_c0 multiplies channel 0, scale_c1 channel 1, nothing channel 2 (SPyNet's flow resize passes w0 / w and h0 / h)."""
    ops = _ops()
    for hi, ho in R.SCALED_CASES:
        x = R.resize_source(R.RESIZE_FRAMES, *hi, 3)
        ref = R.resize_ref64(x, ho, mode, 1.5, 0.75)
        assert torch.equal(ref[..., 2], R.resize_ref64(x, ho, mode)[..., 2])
        got = run_resize(ops, x, ho, mode, dtype, dev, scale_c0=1.5, scale_c1=0.75)
        what = f"resize mode {mode} scales (1.5, 0.75) {hi}->{ho}"
        log(f"resize_kernel mode {mode}", dtype, f"scales (1.5, 0.75) {hi}->{ho}", R.assert_within(got, ref, dtype, R.resize_extent(hi, ho), what))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("C", [16, 32])
def test_resize_bilinear_vector_and_scalar_kernels(dev, dtype, C):
    """Mode 0 on dense aligned clips of 16 / 32 channels takes bilinear_vec_kernel; the same clip in a view whose stride is
    off the vector width takes resize_kernel.  One bound for both."""
    ops = _ops()
    worst = [0.0, 0.0]
    for hi, ho in R.VEC_CASES:
        x = R.resize_source(R.RESIZE_FRAMES, *hi, 32)[..., :C].contiguous()
        ref = R.resize_ref64(x, ho, 0)
        for k, off in enumerate((False, True)):
            what = f"resize mode 0 C={C} {hi}->{ho} {'scalar' if off else 'vector'}"
            worst[k] = max(worst[k], R.assert_within(run_resize(ops, x, ho, 0, dtype, dev, off_vector=off), ref, dtype,
                                                     R.resize_extent(hi, ho), what))
    log("bilinear_vec_kernel", dtype, f"C={C}", worst[0])
    log("resize_kernel mode 0", dtype, f"C={C} off the vector width", worst[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_resize_avgpool_exact(dev, dtype):
    """The mean of four integers below 16 is a multiple of 1/4 that both formats hold, and its f32 sum is exact."""
    ops = _ops()
    for ho in R.RESIZE_OUT:
        x = R.resize_source(R.RESIZE_FRAMES, 2 * ho[0], 2 * ho[1], 3)
        got = run_resize(ops, x, ho, 3, dtype, dev)
        assert torch.equal(got.double(), R.resize_ref64(x, ho, 3)), f"resize mode 3 -> {ho}"


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_resize_nearest_bit_for_bit(dev, dtype):
    """Mode 4 against F.interpolate(mode="nearest") on the CPU in f32 (whose f32 index is not the exact rational one at
    (2 -> 82) and (4 -> 82)): 2x at 16 channels on dense clips (nearest2x_kernel), 2x at 3 channels, a non-integer ratio,
    a down-scale."""
    import torch.nn.functional as F
    ops = _ops()
    for hi, ho, C in R.NEAREST_CASES:
        x = R.resize_source(R.RESIZE_FRAMES, *hi, C)
        ref = F.interpolate(x.permute(0, 3, 1, 2), size=ho, mode="nearest").permute(0, 2, 3, 1)
        assert torch.equal(ref, R.nearest_ref(x, ho))
        for off in ((False, True) if C % 8 == 0 else (True,)):
            got = run_resize(ops, x, ho, 4, dtype, dev, off_vector=off)
            assert torch.equal(got, ref), f"resize mode 4 C={C} {hi}->{ho} {'view' if off else 'dense'}"


@pytest.mark.parametrize("which", ["scalar", "vector"])
def test_resize_beyond_one_grid(dev, which):
    hi, ho, C = R.BIG_RESIZE if which == "scalar" else R.BIG_RESIZE_VEC
    dtype = FP if which == "scalar" else BF
    assert ho[0] * ho[1] * (C if which == "scalar" else C // 8) > 4096 * 256
    x = R.resize_source(1, *hi, C, big=True)
    got = run_resize(_ops(), x, ho, 0, dtype, dev, off_vector=False)
    what = f"resize mode 0 {hi}->{ho} C={C}"
    log("resize_kernel mode 0" if which == "scalar" else "bilinear_vec_kernel", dtype, f"{hi}->{ho} C={C} (beyond one grid)",
        R.assert_within(got, R.resize_ref64(x, ho, 0), dtype, R.resize_extent(hi, ho), what))
