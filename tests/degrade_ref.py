"""References, data, bounds, f32 emulations and mutants for the data-consistency operators of csrc/degrade.hip:
flair_depthwise_filter (both kernels), flair_jpeg_roundtrip / flair_jpeg_roundtrip_hw, flair_matmul_f32 and
flair_gather_mac_f32.  Plain torch / numpy on the CPU; used by tests/test_degrade_exact_cpu.py (which proves what is claimed
here) and tests/test_gpu_degrade_exact.py (which runs the entries).

Two criteria, as in tests/ew_ref.py.
  A, bit for bit: integer data whose every partial sum stays below 2^24 (assert_exact_headroom on sum |K| |x|), single
     products (one tap times one impulse, 0.114f b) and copies have exactly one correct f32 value in any fma order.
  B, per element: |got - ref64| <= n u S, u = 2^-24, S = sum |term| of that element in float64, n = the f32 roundings on the
     longest chain of the kernel's unfused form, counted from the source beside each N_* below.
No bound comes from a kernel's output, and none is relative to max |ref|.
"""
import functools

import numpy as np
import torch

from tests.ew_ref import assert_same_bits, beyond, f32, fma32, same_bits, t32, within      # noqa: F401 (re-exported)
from tests.util import U24, int_tensor

FP = torch.float32
U = U24
GRID = 4096 * 256           # threads of a capped launch: grid_for(n, 256, 4096), the looping kernels of degrade.hip
NAN = float("nan")


def signed_ints(shape, lo, hi, g):
    """Integers with lo <= |v| <= hi and a random sign: none is zero, so every term of every output counts."""
    return int_tensor(shape, lo, hi, g) * (torch.randint(0, 2, tuple(shape), generator=g).float() * 2 - 1)


# ================================================================================================ depthwise filter
def pad_index(a, n, reflect, fault=None):
    """pad_index of degrade.hip:26.  fault: 'clamp_for_reflect', 'symmetric' (-1 -> 0, n -> n - 1 in place of -1 -> 1, n -> n - 2)."""
    if reflect and fault != "clamp_for_reflect":
        if fault == "symmetric":
            a = torch.where(a < 0, -a - 1, a)
            a = torch.where(a > n - 1, 2 * n - 1 - a, a)
        else:
            a = a.abs()
            a = torch.where(a > n - 1, 2 * (n - 1) - a, a)
        return a.clamp(min=0)
    return a.clamp(0, n - 1)


FILTER_FAULTS = ("corner_tap", "cut19", "khkw", "clamp_for_reflect", "symmetric", "stuff_clamp_zero", "out_offset")


def _filter_loop(x, K, pad, stride, off, stuff, stuff_off, Ho, Wo, reflect, fault, step):
    """The index definition of include/flair_hip.h, tap by tap in the order of depthwise_filter_kernel (u outer, v inner):
      out[i][j] = sum_{u,v} K[u][v] IN(i stride + off + u - pad, j stride + off + v - pad),
    IN pads its coordinates by index on the virtual (H stuff, W stuff) image, which is zero except at coordinates
    == stuff_off (mod stuff).  step(k, xv, acc) -> acc adds one tap.  fault (the mutants of the emulation):
      corner_tap        the last tap (kh - 1, kw - 1) is dropped
      cut19             only the central 19 x 19 taps are used
      khkw              the filter is indexed ks[u * kh + v] (beyond its end: NaN)
      clamp_for_reflect, symmetric   see pad_index
      stuff_clamp_zero  a coordinate that the pad moved counts as a stuffed zero, stuff_offset is not asked: right only
                        where the clamp lands between the samples (stuff_offset 1 or 2 of 4)
      out_offset        out_offset taken for 0"""
    N, C, H, W = x.shape
    kh, kw = K.shape
    Hv, Wv = H * stuff, W * stuff
    Kf = K.reshape(-1)
    if fault == "out_offset":
        off = 0
    acc = torch.zeros(N, C, Ho, Wo, dtype=x.dtype)
    cols = []
    for v in range(kw):
        raw = torch.arange(Wo) * stride + off + v - pad
        b = pad_index(raw, Wv, reflect, fault)
        ok = (b % stuff == stuff_off) if stuff > 1 else torch.ones(Wo, dtype=torch.bool)
        if fault == "stuff_clamp_zero" and stuff > 1:
            ok = ok & (raw == b)
        cols.append((b // stuff, ok))
    for u in range(kh):
        raw = torch.arange(Ho) * stride + off + u - pad
        a = pad_index(raw, Hv, reflect, fault)
        rok = (a % stuff == stuff_off) if stuff > 1 else torch.ones(Ho, dtype=torch.bool)
        if fault == "stuff_clamp_zero" and stuff > 1:
            rok = rok & (raw == a)
        if not bool(rok.any()):
            continue
        rows = x[:, :, a // stuff]
        for v in range(kw):
            if fault == "corner_tap" and u == kh - 1 and v == kw - 1:
                continue
            if fault == "cut19" and (abs(u - kh // 2) > 9 or abs(v - kw // 2) > 9):
                continue
            b, cok = cols[v]
            kidx = u * kh + v if fault == "khkw" else u * kw + v
            k = Kf[kidx] if kidx < Kf.numel() else torch.tensor(NAN, dtype=K.dtype)
            xv = torch.where(rok[:, None] & cok[None, :], rows[:, :, :, b], torch.zeros((), dtype=x.dtype))
            acc = step(k, xv, acc)
    return acc


def filter_ref64(x, K, pad, stride=1, off=0, stuff=1, stuff_off=0, out_hw=None, reflect=False):
    """-> (ref64, S = sum |K| |x| per output), float64."""
    Ho, Wo = out_hw
    args = (pad, stride, off, stuff, stuff_off, Ho, Wo, reflect, None, lambda k, xv, acc: acc + k * xv)
    return _filter_loop(x.double(), K.double(), *args), _filter_loop(x.double().abs(), K.double().abs(), *args)


def filter_emul(x, K, pad, stride=1, off=0, stuff=1, stuff_off=0, out_hw=None, reflect=False, fault=None):
    """depthwise_filter_kernel in f32: one fmaf per tap, u outer, v inner (degrade.hip:49-58)."""
    Ho, Wo = out_hw
    return _filter_loop(x.float(), K.float(), pad, stride, off, stuff, stuff_off, Ho, Wo, reflect, fault, fma32)


def filter_tiled_emul(x, K, pad, off, out_hw, reflect, fault=None):
    """depthwise_filter_tiled_kernel<39> (degrade.hip:68-104): a workgroup per 32 x 32 output tile, its padded input patch
    staged first, then the same fmaf chain per output.  fault: 'tiles_swapped' (tilesW and tilesH exchanged in the
    decomposition of blockIdx.x), 'out_offset', 'clamp_for_reflect', 'symmetric', 'corner_tap', 'cut19'."""
    N, C, H, W = x.shape
    KS = K.shape[0]
    Ho, Wo = out_hw
    assert K.shape == (KS, KS) and Ho % 32 == 0 and Wo % 32 == 0
    if fault == "out_offset":
        off = 0
    tilesW, tilesH = Wo // 32, Ho // 32
    xp = x.float().reshape(N * C, H, W)
    y = torch.full((N * C, Ho, Wo), NAN)
    PW = 32 + KS - 1
    for blk in range(N * C * tilesW * tilesH):
        pl, t = blk // (tilesW * tilesH), blk % (tilesW * tilesH)
        tw = tilesH if fault == "tiles_swapped" else tilesW
        i0, j0 = (t // tw) * 32, (t % tw) * 32
        if i0 + 32 > Ho or j0 + 32 > Wo:
            continue                    # the faulty kernel writes beyond the plane; here the tile stays NaN
        r = pad_index(i0 + off + torch.arange(PW) - pad, H, reflect, fault)
        c = pad_index(j0 + off + torch.arange(PW) - pad, W, reflect, fault)
        patch = xp[pl][r][:, c]
        acc = torch.zeros(32, 32)
        for u in range(KS):
            for v in range(KS):
                if fault == "corner_tap" and u == KS - 1 and v == KS - 1:
                    continue
                if fault == "cut19" and (abs(u - KS // 2) > 9 or abs(v - KS // 2) > 9):
                    continue
                acc = fma32(K[u, v].float(), patch[u:u + 32, v:v + 32], acc)
        y[pl, i0:i0 + 32, j0:j0 + 32] = acc
    return y.view(N, C, Ho, Wo)


def old_rule_accepts(got, ref64):
    """The v0 rule of tests/test_gpu_image_ops.py:_close_filter -> (accepted, max |err|, bound)."""
    err = (got.double() - ref64).abs().max().item()
    bound = 2e-5 * max(1.0, ref64.abs().max().item())
    return err <= bound, err, bound


# name -> filter (kh, kw), planes (N, C, H, W), keywords of ops.depthwise_filter.  Each at the smallest size that still
# has all four borders and an interior.  unaligned: the output slice starts 4 bytes off a 16-byte boundary.
FILTER_CASES = {
    "down":        dict(k=(9, 9), x=(1, 2, 20, 28), kw=dict(pad=4, out_stride=4, out_offset=1, out_hw=(5, 7))),
    "up0":         dict(k=(9, 9), x=(1, 2, 5, 7), kw=dict(pad=4, stuff=4, stuff_offset=0, out_hw=(20, 28))),
    "up1":         dict(k=(9, 9), x=(1, 2, 5, 7), kw=dict(pad=4, stuff=4, stuff_offset=1, out_hw=(20, 28))),
    "up3":         dict(k=(9, 9), x=(1, 2, 5, 7), kw=dict(pad=4, stuff=4, stuff_offset=3, out_hw=(20, 28))),
    "inv":         dict(k=(39, 39), x=(1, 2, 21, 23), kw=dict(pad=19, out_hw=(21, 23))),
    "inv_unaligned": dict(k=(39, 39), x=(1, 2, 32, 32), kw=dict(pad=19, out_hw=(32, 32)), unaligned=True),
    "reflect":     dict(k=(9, 9), x=(1, 2, 5, 6), kw=dict(pad=4, out_hw=(5, 6), reflect=True)),
    "k5x3":        dict(k=(5, 3), x=(1, 2, 7, 9), kw=dict(pad=1, out_hw=(7, 9))),
    "k4x7_pad2":   dict(k=(4, 7), x=(1, 2, 6, 8), kw=dict(pad=2, out_hw=(6, 8))),
    "stride3_off2": dict(k=(5, 5), x=(1, 2, 13, 17), kw=dict(pad=2, out_stride=3, out_offset=2, out_hw=(4, 5))),
    "two_trips":   dict(k=(3, 3), x=(1, 3, 600, 600), kw=dict(pad=1, out_hw=(600, 600))),
}
# tiled kernel: (input H, W), out_hw, out_offset; each with replicate and reflect, two planes
TILED_CASES = [((32, 32), (32, 32), 0), ((32, 32), (32, 32), 1), ((32, 64), (32, 64), 0), ((32, 64), (32, 64), 1),
               ((64, 32), (64, 32), 0), ((64, 32), (64, 32), 1), ((40, 70), (32, 64), 0)]


def ref_kwargs(kw):
    """ops.depthwise_filter's keywords -> those of filter_ref64 / filter_emul."""
    return dict(pad=kw["pad"], stride=kw.get("out_stride", 1), off=kw.get("out_offset", 0), stuff=kw.get("stuff", 1),
                stuff_off=kw.get("stuff_offset", 0), out_hw=kw["out_hw"], reflect=kw.get("reflect", False))


@functools.lru_cache(maxsize=None)
def int_filter(kh, kw):
    """Taps in +-{1, 2, 3}, none zero."""
    return signed_ints((kh, kw), 1, 3, torch.Generator().manual_seed(100 * kh + kw))


@functools.lru_cache(maxsize=None)
def int_planes(shape):
    """Integers with 1 <= |x| <= 255 and a random sign."""
    return signed_ints(shape, 1, 255, torch.Generator().manual_seed(sum(shape)))


@functools.lru_cache(maxsize=None)
def filter_int_case(name):
    """-> x, K, keywords of the reference, ref64, S."""
    c = FILTER_CASES[name]
    x, K = int_planes(c["x"]), int_filter(*c["k"])
    kw = ref_kwargs(c["kw"])
    return (x, K, kw) + filter_ref64(x, K, **kw)


@functools.lru_cache(maxsize=None)
def tiled_int_case(i, reflect):
    hw, out_hw, off = TILED_CASES[i]
    x, K = int_planes((1, 2) + hw), int_filter(39, 39)
    kw = dict(pad=19, stride=1, off=off, stuff=1, stuff_off=0, out_hw=out_hw, reflect=reflect)
    return (x, K, kw) + filter_ref64(x, K, **kw)


@functools.lru_cache(maxsize=1)
def real_filters():
    """The filters of the operator in use: pseudoSR(Get_pseudoSR_Conf(4), synthetic_blur_kernel(sigma=1.8), kernel_indx=10)
    -> dict(inv 39 x 39, down 9 x 9, up 9 x 9) of f32 tensors, the pre-stride offset, the factor."""
    from flair_amd import workload as wl
    from flair_amd.guided_diffusion import pseudoSR as psr
    A = psr.pseudoSR(psr.Get_pseudoSR_Conf(4), upscale_kernel=wl.synthetic_blur_kernel(sigma=1.8),
                     kernel_indx=10).WrapArchitecture_PyTorch()
    return {k: torch.from_numpy(v) for k, v in A._host.items()}, int(A.pre_stride[0]), A.ds_factor


def old_inputs():
    """The planes of test_depthwise_filter_parameter_sets -> lr (2, 3, 40, 56), hr (2, 3, 160, 224)."""
    g = torch.Generator().manual_seed(3)
    return torch.rand(2, 3, 40, 56, generator=g) * 2 - 1, torch.rand(2, 3, 160, 224, generator=g) * 2 - 1


def _impulses(shape, at):
    """Zero planes with +-2^k at the listed (plane, row, column): amplitudes 2^-2 .. 2^3, alternating sign."""
    x = torch.zeros(shape)
    for n, (pl, r, c) in enumerate(at):
        x[0, pl, r, c] = (-1.0) ** n * 2.0 ** (n % 6 - 2)
    return x


# name -> which real filter, planes, impulse positions (plane, row, column), keywords.  The impulses are at least one
# filter width (on the grid the filter runs on) from each other in one axis and from every border, so every output holds
# one product at most.  down: sixteen impulses 13 apart, one for each phase (row % 4, column % 4) of the stride-4 sampling.
IMPULSE_CASES = {
    "inv":  dict(filt="inv", x=(1, 2, 96, 128), at=[(0, 40, 41), (0, 55, 86), (1, 45, 39), (1, 56, 88)],
                 kw=dict(pad=19, out_hw=(96, 128)), width=39),
    "down": dict(filt="down", x=(1, 2, 60, 60), at=[(a % 2, 9 + 13 * a, 9 + 13 * b) for a in range(4) for b in range(4)],
                 kw=dict(pad=4, out_stride=4, out_offset="pre", out_hw=(15, 15)), width=9),
    "up":   dict(filt="up", x=(1, 2, 10, 12), at=[(0, 3, 3), (0, 3, 7), (0, 6, 5), (1, 4, 4), (1, 6, 8)],
                 kw=dict(pad=4, stuff=4, stuff_offset="pre", out_hw=(40, 48)), width=9),
}


@functools.lru_cache(maxsize=None)
def impulse_case(name):
    """-> x, K (the real filter), ops keywords, the one correct f32 response (ref64 holds single products, exact in f32)."""
    c = IMPULSE_CASES[name]
    Ks, pre, f = real_filters()
    kw = {k: (pre if v == "pre" else v) for k, v in c["kw"].items()}
    x, K = _impulses(c["x"], c["at"]), Ks[c["filt"]]
    ref, _ = filter_ref64(x, K, **ref_kwargs(kw))
    assert bool((ref.float().double() == ref).all()), "an impulse response is not a single product"
    return x, K, kw, ref.float()


def impulse_expected(name):
    """The same response written down from the filter itself, without a sum: the output at (i, j) sees the impulse at
    (P, Q) of the grid the filter runs on through tap (P - (i stride + off - pad), Q - (j stride + off - pad)), if that is
    one -> (expected f32 response, bool (kh, kw): the taps that some output shows)."""
    c = IMPULSE_CASES[name]
    Ks, pre, f = real_filters()
    kw = ref_kwargs({k: (pre if v == "pre" else v) for k, v in c["kw"].items()})
    x, K = _impulses(c["x"], c["at"]), Ks[c["filt"]]
    kh, kwid = K.shape
    Ho, Wo = kw["out_hw"]
    want = torch.zeros(c["x"][:2] + (Ho, Wo))
    seen = torch.zeros(kh, kwid, dtype=torch.bool)
    i, j = torch.arange(Ho)[:, None], torch.arange(Wo)[None, :]
    for pl, r, col in c["at"]:
        P, Q = r * kw["stuff"] + (kw["stuff_off"] if kw["stuff"] > 1 else 0), col * kw["stuff"] + (kw["stuff_off"] if kw["stuff"] > 1 else 0)
        u, v = P - (i * kw["stride"] + kw["off"] - kw["pad"]), Q - (j * kw["stride"] + kw["off"] - kw["pad"])
        ok = (u >= 0) & (u < kh) & (v >= 0) & (v < kwid)
        u, v = u.clamp(0, kh - 1).expand(Ho, Wo), v.clamp(0, kwid - 1).expand(Ho, Wo)
        assert not bool((want[0, pl][ok] != 0).any()), "two impulses reach one output"
        want[0, pl] = torch.where(ok, K[u, v] * x[0, pl, r, col], want[0, pl])
        seen[u[ok], v[ok]] = True
    return want, seen


# ================================================================================================ matmul
MATMUL_SHAPES = ((1, 1, 1), (16, 16, 16), (15, 31, 17), (17, 33, 50), (64, 48, 256))
MATMUL_SHARED = ("none", "A", "B")


@functools.lru_cache(maxsize=None)
def matmul_case(M, N, K, shared):
    """Batch 3, integers in [-16, 16] without the zero -> a, b, ref64, S = |a| |b|."""
    g = torch.Generator().manual_seed(M + N + K)
    a = signed_ints((() if shared == "A" else (3,)) + (M, K), 1, 16, g)
    b = signed_ints((() if shared == "B" else (3,)) + (K, N), 1, 16, g)
    return a, b, a.double() @ b.double(), a.double().abs() @ b.double().abs()


def matmul_emul(a, b, fault=None):
    """matmul_kernel (degrade.hip:304): 16-wide k tiles, zero beyond K, one fmaf per k.  fault: 'k_tail' (the loop runs
    over the full tiles only: k0 + 16 <= K)."""
    K = a.shape[-1]
    Ke = K // 16 * 16 if fault == "k_tail" else K
    acc = torch.zeros(torch.broadcast_shapes(a.shape[:-2], b.shape[:-2]) + (a.shape[-2], b.shape[-1]))
    for k in range(Ke):
        acc = fma32(a[..., :, k:k + 1].float(), b[..., k:k + 1, :].float(), acc)
    return acc.expand(3, -1, -1) if acc.dim() == 2 else acc


# ================================================================================================ gather-MAC
# name -> outer, Lin, inner, taps, Lout
GATHER_CASES = {f"{'shrink' if Lin > Lout else 'grow'}_taps{taps}_inner{inner}": (6, Lin, inner, taps, Lout)
                for Lin, Lout in ((24, 7), (9, 31)) for taps in (1, 8) for inner in (1, 5)}
GATHER_CASES["two_trips"] = (6, 300, 256, 2, 700)       # 6 x 700 x 256 = 1,075,200 outputs > GRID


@functools.lru_cache(maxsize=None)
def gather_int_case(name):
    """x integers 1 <= |x| <= 255, w in +-{1, 2, 3}; index 0 and Lin - 1 present, and with more than one tap a column of fov
    that repeats an index -> x, fov, w, ref64, S."""
    outer, Lin, inner, taps, Lout = GATHER_CASES[name]
    g = torch.Generator().manual_seed(taps * 100 + Lin + inner)
    x = signed_ints((outer, Lin, inner), 1, 255, g)
    fov = torch.randint(0, Lin, (taps, Lout), generator=g).int()
    fov[0, 0], fov[-1, -1] = 0, Lin - 1
    if taps > 1:
        fov[1, 2] = fov[0, 2]
    w = signed_ints((taps, Lout), 1, 3, g)
    return (x, fov, w) + gather_ref64(x, fov, w)


def gather_ref64(x, fov, w):
    """y[o][i][n] = sum_k w[k][i] x[o][fov[k][i]][n] -> (ref64, S = sum_k |w x|)."""
    xs = x.double()[:, fov.long()]                          # outer, taps, Lout, inner
    return (torch.einsum("ki,okin->oin", w.double(), xs), torch.einsum("ki,okin->oin", w.double().abs(), xs.abs()))


def N_GATHER(taps):
    """gather_mac_kernel (degrade.hip:333): `acc += x * w` per tap, uncontracted: the first product is rounded once and then
    passes through one sum per tap (the first of them, 0 + p, rounds nothing but is counted) -> n = taps + 1."""
    return taps + 1


def gather_emul(x, fov, w, fused=False, fault=None):
    """fault: 'fov_stride_lin' (fov read at k * Lin + i: beyond the table, NaN)."""
    outer, Lin, inner = x.shape
    taps, Lout = fov.shape
    ff = fov.reshape(-1).long()
    acc = torch.zeros(outer, Lout, inner)
    for k in range(taps):
        at = k * (Lin if fault == "fov_stride_lin" else Lout) + torch.arange(Lout)
        ok = at < ff.numel()
        idx = ff[at.clamp_max(ff.numel() - 1)]
        xv = torch.where(ok[None, :, None], x.float()[:, idx], torch.tensor(NAN))
        wk = w[k].float()[None, :, None]
        acc = fma32(xv, wk, acc) if fused else acc + xv * wk
    return acc


@functools.lru_cache(maxsize=None)
def resizer_case(Lin, Lout):
    """The cubic table of Resizer for Lin -> Lout along one axis (antialiased when shrinking), x = randn (6, Lin, 5)."""
    from flair_amd.guided_diffusion.resizer import Resizer
    fov, w = Resizer((1, 1, Lin, Lin), scale_factor=Lout / Lin, kernel="cubic")._tables[0]
    assert fov.shape[1] == Lout and int(fov.max()) < Lin and int(fov.min()) >= 0
    x = torch.randn(6, Lin, 5, generator=torch.Generator().manual_seed(Lin))
    return x, fov.contiguous(), w.contiguous()


# ================================================================================================ JPEG
JPEG_SIZES_HW = ((16, 16, 1), (16, 48, 2), (48, 32, 3), (32, 176, 1))       # H, W, N: 1, 6, 18 and 22 MCUs in groups of ten
JPEG_SIZES_SQUARE = ((16, 16, 1), (48, 48, 2))
C_Y, C_CR = np.float32(0.114), np.float32(-0.0813)      # the blue column of jpeg_rgb_to_ycc (degrade.hip:151-153)
# jpeg_ycc_to_rgb (degrade.hip:158-160): rows of (cr, cb) coefficients
YCC = ((1.40198758, -3.68199903e-05), (-7.14103821e-01, -3.44113281e-01), (-1.34583413e-04, 1.77197812))
N_YCC2RGB = 5   # degrade.hip:157-160: Cb - 128, the inner fmaf, the outer fmaf, the division by 255, the last fmaf

IDENTITY = np.eye(8, dtype=np.float32)
SHIFT = np.roll(np.eye(8, dtype=np.float32), 1, axis=1)         # P[k][n] = 1 where n = k + 1 (mod 8): order 8, P P != I
_I, _J = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
Q1_SEL = (2.0 ** ((_I + 2 * _J) % 4 - 1)).astype(np.float32)    # 0.5, 1, 2, 4; Q1_SEL != Q1_SEL^T
Q2_SEL = np.ones((8, 8), dtype=np.float32)                      # with it every odd blue is a tie of Cb
Q_POW2 = (2.0 ** -(17 + 8 * _I + _J)).astype(np.float32)        # 64 distinct powers of two, 2^-17 .. 2^-80: below the unit
#                                                                 in the last place of every plane value, so nothing is lost
MODES = {"identity": (IDENTITY, Q1_SEL, Q2_SEL), "shift": (SHIFT, Q_POW2, Q_POW2)}


def _frac_tie_distance(v):
    v = np.asarray(v, dtype=np.float64)
    return np.abs((v - np.floor(v)) - 0.5)


def blue_input(k):
    """2 k / 255 - 1 in numpy float32 operations."""
    return np.float32(2) * np.asarray(k).astype(np.float32) / np.float32(255) - np.float32(1)


@functools.lru_cache(maxsize=1)
def blue_pool():
    """The blue levels k in [0, 255] whose input x = blue_input(k) comes back as exactly k from the kernel's
    (x + 1) / 2 * 255 in single f32 operations (193 of the 256, 96 of them odd) -> (all of them, those kept for the images).
    Kept: those whose luma coefficient (f32(0.114f k) - 128) / q stays 1e-3 clear of a tie for every q of Q1_SEL."""
    k = np.arange(256)
    x = blue_input(k)
    back = (x + np.float32(1)) / np.float32(2) * np.float32(255)
    exact = k[back == k.astype(np.float32)]
    yb = (C_Y * exact.astype(np.float32)) - np.float32(128)
    clear = np.all([_frac_tie_distance(yb.astype(np.float64) / q) >= 1e-3 for q in (0.5, 1.0, 2.0, 4.0)], axis=0)
    return exact, exact[clear]


@functools.lru_cache(maxsize=None)
def jpeg_case(H, W, N):
    """r = g = 0 and a blue level of blue_pool() per pixel, odd with probability 0.7 -> x (N, 3, H, W) f32 in [-1, 1],
    b (N, H, W) f32 integers."""
    pool = blue_pool()[1]
    odd, even = pool[pool % 2 == 1], pool[pool % 2 == 0]
    rng = np.random.default_rng(H * 1000 + W + N)
    pick_odd = rng.random((N, H, W)) < 0.7
    b = np.where(pick_odd, odd[rng.integers(0, odd.size, (N, H, W))], even[rng.integers(0, even.size, (N, H, W))])
    x = np.full((N, 3, H, W), -1.0, dtype=np.float32)
    x[:, 2] = blue_input(b)
    return torch.from_numpy(x), b.astype(np.float32)


def _blocks(p):
    """(N, H, W) -> (N, H / 8, W / 8, 8, 8)."""
    N, H, W = p.shape
    return p.reshape(N, H // 8, 8, W // 8, 8).transpose(0, 1, 3, 2, 4)


def _unblocks(b):
    N, hb, wb = b.shape[:3]
    return b.transpose(0, 1, 3, 2, 4).reshape(N, hb * 8, wb * 8)


def jpeg_expected(b, mode):
    """What both entries must return for an image of jpeg_case, from single numpy f32 operations (each correctly rounded,
    as the kernel's are): the block values Y - 128 = f32(f32(0.114f b) - 128), Cb - 128 = 0.5 b, Cr - 128 =
    f32(f32(f32(-0.0813f b) + 128) - 128) at the even pixels; a selector matrix moves them without arithmetic
    (identity: coef = blk, shift: coef = P blk P^T, coef[k][c] = blk[k + 1][c + 1]); level = rint(coef / q), half to even.
    -> dict(luma (N, 1, H, W), chroma (N, 2, H / 2, W / 2) f32 levels, coefq_l, coefq_c = coef / q before the rounding,
    ref64 and bound (N, 3, H, W): jpeg_ycc_to_rgb in float64 on the exactly known decoded planes, N_YCC2RGB u S)."""
    D, q1, q2 = MODES[mode]
    N, H, W = b.shape
    one28 = np.float32(128)
    yb = (C_Y * b) - one28
    cbb = (np.float32(0.5) * b)[:, ::2, ::2]
    assert np.array_equal((cbb + one28) - one28, cbb)
    crb = (((C_CR * b) + one28) - one28)[:, ::2, ::2]
    out = {}
    planes = []
    for name, blk, q in (("l", yb, q1), ("cb", cbb, q2), ("cr", crb, q2)):
        B = _blocks(blk)
        coef = B if mode == "identity" else np.roll(B, (-1, -1), axis=(3, 4))
        cq = coef / q
        level = np.rint(cq)
        dec = level * q
        assert dec.dtype == np.float32 and np.array_equal(dec.astype(np.float64), level.astype(np.float64) * q.astype(np.float64))
        back = dec if mode == "identity" else np.roll(dec, (1, 1), axis=(3, 4))
        plane = _unblocks(back) + one28
        assert np.array_equal(plane.astype(np.float64), _unblocks(back).astype(np.float64) + 128.0), "decoded plane not exact"
        out["level_" + name], out["coefq_" + name], out["blk_" + name] = _unblocks(level), _unblocks(cq), blk
        planes.append(plane.astype(np.float64))
    Y, Cb, Cr = planes[0], planes[1].repeat(2, 1).repeat(2, 2), planes[2].repeat(2, 1).repeat(2, 2)
    cb, cr = Cb - 128.0, Cr - 128.0
    ref, S = [], []
    for c_cr, c_cb in YCC:
        c_cr, c_cb = f32(c_cr), f32(c_cb)
        ref.append((c_cr * cr + c_cb * cb + Y) / 255.0 * 2.0 - 1.0)
        S.append((np.abs(c_cr * cr) + np.abs(c_cb * cb) + np.abs(Y)) / 255.0 * 2.0 + 1.0)
    out["luma"] = torch.from_numpy(out["level_l"][:, None].copy())
    out["chroma"] = torch.from_numpy(np.stack([out["level_cb"], out["level_cr"]], 1))
    out["ref64"] = torch.from_numpy(np.stack(ref, 1))
    out["bound"] = N_YCC2RGB * U * torch.from_numpy(np.stack(S, 1))
    return out


def tie_share(cq):
    """The share of the coefficients coef / q that are exact ties."""
    return float(np.mean(_frac_tie_distance(cq) == 0.0))


def _dct_emul(D, blk, inverse, transposed_second=False):
    """dct8x8 (degrade.hip:113): M[k][n] = D[k][n] forward, D[n][k] inverse; tmp[r][k] = sum_n in[r][n] M[k][n], then
    out[k][c] = sum_n tmp[n][c] M[k][n]; one fmaf per n, n ascending."""
    M1 = D.t() if inverse else D
    M2 = D.t() if inverse != transposed_second else D
    tmp = torch.zeros_like(blk)
    for n in range(8):
        tmp = fma32(blk[..., :, n:n + 1], M1[:, n].expand(8, 8), tmp)           # [r][k] += in[r][n] M[k][n]
    out = torch.zeros_like(blk)
    for n in range(8):
        out = fma32(tmp[..., n:n + 1, :], M2[:, n:n + 1].expand(8, 8), out)     # [k][c] += tmp[n][c] M[k][n]
    return out


JPEG_FAULTS = ("roundf", "q_transposed", "d_swapped", "d_pass_transposed", "inverse_forward")


def jpeg_emul(x, q1, q2, D, fault=None):
    """Both JPEG entries, literally, in f32 (they share jpeg_rgb_to_ycc, codec8x8 and jpeg_ycc_to_rgb) -> (image, luma
    levels, chroma levels).  fault: 'roundf' (half away from zero for rintf), 'q_transposed' (q[j * 8 + i]), 'd_swapped'
    (D^T forward, D inverse), 'd_pass_transposed' (the second pass of each transform reads D the other way),
    'inverse_forward' (the inverse transform applies D like the forward one)."""
    N, _, H, W = x.shape
    D = torch.from_numpy(np.ascontiguousarray(D, dtype=np.float32).reshape(8, 8))
    rgb = [(x[:, c] + 1.0) / 2.0 * 255.0 for c in range(3)]
    r, g, bl = rgb
    Y = fma32(0.114, bl, fma32(0.299, r, t32(0.587) * g))
    Cb = fma32(0.5, bl, fma32(-0.1687, r, t32(-0.3313) * g)) + 128.0
    Cr = fma32(-0.0813, bl, fma32(0.5, r, t32(-0.4187) * g)) + 128.0
    dec, levels = [], []
    for plane, q in ((Y, q1), (Cb[:, ::2, ::2], q2), (Cr[:, ::2, ::2], q2)):
        q = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32).reshape(8, 8))
        if fault == "q_transposed":
            q = q.t()
        blk = torch.from_numpy(_blocks((plane - 128.0).numpy()).copy())
        swap = fault == "d_swapped"
        tr = fault == "d_pass_transposed"
        c = _dct_emul(D, blk, swap, tr) / q
        if fault == "roundf":
            level = (torch.sign(c).double() * torch.floor(c.double().abs() + 0.5)).float()
        else:
            level = torch.from_numpy(np.rint(c.numpy()))
        back = _dct_emul(D, level * q, swap if fault == "inverse_forward" else not swap, tr)
        levels.append(torch.from_numpy(_unblocks(level.numpy()).copy()))
        dec.append(torch.from_numpy(_unblocks(back.numpy()).copy()) + 128.0)
    Yd = dec[0]
    cb = dec[1].repeat_interleave(2, 1).repeat_interleave(2, 2) - 128.0
    cr = dec[2].repeat_interleave(2, 1).repeat_interleave(2, 2) - 128.0
    out = [fma32(fma32(c_cr, cr, fma32(c_cb, cb, Yd)) / 255.0, 2.0, -1.0) for c_cr, c_cb in YCC]
    return torch.stack(out, 1), levels[0][:, None], torch.stack(levels[1:], 1)
