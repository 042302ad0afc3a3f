"""Reference and data for the deformable alignment at FRACTIONAL sampling positions (tests/test_dcn_frac_cpu.py checks
them without a GPU, tests/test_gpu_dcn_frac.py runs flair_dcn_align against them).  CPU only.

dcn_corner_ref is a float64 modulated deformable 3x3 convolution (stride 1, padding 1) written as a four-corner gather:
a corner outside the frame contributes 0 (the DCNv2 / torchvision rule), no grid_sample.  The sampling positions are
computed in float32 in the kernel's own order (dcn.hip: sy = ((ph - 1) + ikh) + flow.y, then + residue, floor,
ay = sy - floor) and widened afterwards, so the reference and the kernel blend with the same fractions; the weights, the
blend, the sum over K and the bias are float64.

Two families of data:
  dyadic  x, w, bias integers, masks in {0, 0.5, 1}, flows and residues multiples of 1/4: every weight is a multiple of
          1/32 (exact in bf16), every blended sample a multiple of 1/32 of magnitude <= 8 (exact in bf16), every partial sum
          a multiple of 1/32 below 2^24 / 32 -- the whole operator is exact in f32 and in bf16, in any order, so the kernel's
          output has to equal the reference bit for bit (tests/test_gpu_exact.py's method, carried to fractional positions);
  generic randn data for the one-hot test: a weight matrix with ONE nonzero per output channel turns each output into
          bias + w * (one blended sample), checked per element against a bound that follows from the kernel's arithmetic.

Edge bands.  Nine (group, tap) pairs spread over both input halves are pinned, at every pixel they cover, to one absolute
target: a row in (-1, 0), a row in (H - 1, H), a column in (-1, 0), a column in (W - 1, W), a corner of the frame, exactly
-1 (a row beyond -1 on generic data), exactly H (a row beyond H), a fractional position well inside, and far outside
(residue -+1000, which has to give exactly 0 through the kernel's v_med3 clamp).  A pixel is covered where the residue
target - (pixel + tap + flow) can be stored: always in f32; in bf16 where it is representable (dyadic data: 8 significant
bits, so every pixel within 64 of the target and about half of the others) or below 64 in magnitude (generic data: the
rounding moves the position by at most 1/8, the targets keep 0.29 from the next integer).  Elsewhere the random offsets
stay.  Mode 0 has no bands: its residues are max_mag * tanh = -2, 0 or 2, and its edges come from the wider flows.
"""
import functools
import types

import torch
import torch.nn.functional as F

from tests.util import int_tensor, rb

BF, FP = torch.bfloat16, torch.float32
MAX_MAG = 2.0               # mode 0: raw residues {-60, 0, 60} -> 2 tanh = {-2, 0, 2} (__expf overflows to inf, underflows to 0)
# raw_activated = 2 (ops.dcn_pack): F, H, W, C, G
PACK_SHAPES = [(2, 9, 13, 64, 4),          # G = 4: the 24-byte raw slab (bf16), fetched as two 16-byte pieces
               (1, 16, 16, 256, 4),        # two cout slices of 128
               (2, 20, 24, 64, 8),
               (1, 128, 128, 128, 4)]      # the large-P tiles


def strided_cases():
    """Every entry of tests/test_gpu_strides.DCN_CASES as (mode, dtype, F, H, W, half, cout, G): mode 1 = activated, 0 not."""
    from tests.test_gpu_strides import DCN_CASES
    return [(1 if c[7] else 0,) + tuple(c[:7]) for c in DCN_CASES]


def pack_cases():
    return [(2, dt, Fr, H, W, C // 2, C, G) for (Fr, H, W, C, G) in PACK_SHAPES for dt in (BF, FP)]


def exact_cases():
    """Family A: all 21 DCN_CASES and the mode-2 shapes in both dtypes."""
    return strided_cases() + pack_cases()


def onehot_cases():
    """Family B: one case per instantiation of modes 1 and 2."""
    return [c for c in strided_cases() if c[0] == 1] + pack_cases()


def case_id(c):
    mode, dtype, Fr, H, W, half, cout, G = c
    return f"m{mode}-{'bf16' if dtype == BF else 'f32'}-{Fr}x{H}x{W}-h{half}-o{cout}-G{G}"


def pixel_tile(case):
    """Pixels per workgroup of the instantiation flair_dcn_align picks for a mode 0 / 1 case (dcn.hip, flair_dcn_align)."""
    mode, dtype, Fr, H, W, half, cout, G = case
    P = Fr * H * W
    if dtype != BF:
        return 64 if cout <= 64 else 32
    if cout > 64:
        return 64 if P >= 64 * 256 else 32
    return 128 if P >= 128 * 512 else 64


def is_dot2(case):
    """The bf16 per-frame activated forms (ACTIVATED && ONEFRAME) blend on v_dot2c with the weights rounded to bf16."""
    mode, dtype, Fr, H, W = case[:5]
    return dtype == BF and mode == 1 and (H * W) % pixel_tile(case) == 0


def corner_weights(ay, ax, m):
    """(1 - ay)(1 - ax) m, (1 - ay) ax m, ay (1 - ax) m, ay ax m: the corners (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)."""
    return torch.stack([(1 - ay) * (1 - ax) * m, (1 - ay) * ax * m, ay * (1 - ax) * m, ay * ax * m])


def blend64(k, ay, ax, m, v, cpg):
    """The four-corner blend of tap k in float64.  ay, ax (G, P) float32, m (G, P) float64, v (4, C, P) float32 corner values
    (0 outside the frame) -> (C, P) float64.  dcn_corner_ref's `blend` argument replaces it (emulations, mutations)."""
    wt = corner_weights(ay.double(), ax.double(), m)
    return (wt.repeat_interleave(cpg, dim=1) * v.double()).sum(0)


def group_flows(flows, n, G, H, W):
    """-> (fy, fx) float32 (G, H, W) of frame n: groups below G / 2 take flow1, the others flow2; flow channel 0 is x."""
    if flows is None or flows[0] is None:
        z = torch.zeros(G, H, W)
        return z, z
    f = torch.stack([flows[0][n]] * (G // 2) + [flows[1][n]] * (G - G // 2))           # G, H, W, 2
    return f[..., 1].contiguous(), f[..., 0].contiguous()


def tap_positions(k, H, W, fy, fx, ry, rx):
    """float32 sampling positions of tap k in the kernel's order: ((ph - 1) + ikh) + flow, then + residue."""
    i, j = divmod(k, 3)
    hh = torch.arange(H, dtype=FP).view(1, H, 1)
    ww = torch.arange(W, dtype=FP).view(1, 1, W)
    sy = ((hh - 1.0) + float(i)) + fy
    sx = ((ww - 1.0) + float(j)) + fx
    return sy + ry, sx + rx


def dcn_corner_ref(x, residues, flows, mask, w, b, G, blend=None, keep_cols=False):
    """x (N, C, H, W); residues (N, 18 G, H, W) float32, finished, channel 2 (g 9 + k) the row and + 1 the column
    displacement; flows None or (flow1, flow2), each (N, H, W, 2) float32; mask (N, 9 G, H, W), finished; w (Cout, C, 3, 3);
    b (Cout,) or None.  -> namespace of
      out     (N, Cout, H, W) float64
      mag     the same operator on |x|, |w|, |b|
      inside  (N, G, 9, H, W) int8: corners of the sample inside the frame, 0 .. 4
      cols    with keep_cols: (N, 9, C, H W) float64, the blended samples (the im2col columns); else None
      cols_bf16_exact   every blended sample is representable in bf16
      frac    share of the sampling coordinates that are no integers"""
    N, C, H, W = x.shape
    cpg, P = C // G, H * W
    assert residues.dtype == FP and residues.shape == (N, 18 * G, H, W) and mask.shape == (N, 9 * G, H, W)
    blend = blend or blend64
    res = residues.view(N, G, 9, 2, H, W)
    msk = mask.double().view(N, G, 9, P)
    wd = w.double()
    out = torch.zeros(N, w.shape[0], P, dtype=torch.float64)
    mag = torch.zeros_like(out)
    inside = torch.empty(N, G, 9, H, W, dtype=torch.int8)
    cols = torch.empty(N, 9, C, P, dtype=torch.float64) if keep_cols else None
    exact, nfrac = True, 0
    Wp = W + 4
    for n in range(N):
        xp = F.pad(x[n].float(), (2, 2, 2, 2)).reshape(C, (H + 4) * Wp)               # the frame in a border of zeros
        fy, fx = group_flows(flows, n, G, H, W)
        for k in range(9):
            sy, sx = tap_positions(k, H, W, fy, fx, res[n, :, k, 0], res[n, :, k, 1])
            y0, x0 = torch.floor(sy), torch.floor(sx)
            ay, ax = (sy - y0).reshape(G, P), (sx - x0).reshape(G, P)
            nfrac += int((ay != 0).sum()) + int((ax != 0).sum())
            yin = torch.stack([(y0 >= 0) & (y0 <= H - 1), (y0 + 1 >= 0) & (y0 + 1 <= H - 1)])     # 2, G, H, W
            xin = torch.stack([(x0 >= 0) & (x0 <= W - 1), (x0 + 1 >= 0) & (x0 + 1 <= W - 1)])
            inside[n, :, k] = (yin.sum(0) * xin.sum(0)).to(torch.int8)
            yc, xc = y0.clamp(-2, H).long() + 2, x0.clamp(-2, W).long() + 2           # clamped corners lie in the border
            v = []
            for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                idx = ((yc + dy) * Wp + xc + dx).reshape(G, P).repeat_interleave(cpg, dim=0)
                v.append(torch.gather(xp, 1, idx))
            v = torch.stack(v)                                                        # 4, C, P
            col = blend(k, ay, ax, msk[n, :, k], v, cpg)
            mcol = blend64(k, ay, ax, msk[n, :, k], v.abs(), cpg)
            exact = exact and bool(torch.equal(col.to(BF).double(), col))
            if keep_cols:
                cols[n, k] = col
            i, j = divmod(k, 3)
            out[n] += wd[:, :, i, j] @ col
            mag[n] += wd[:, :, i, j].abs() @ mcol
    if b is not None:
        out += b.double().view(1, -1, 1)
        mag += b.double().abs().view(1, -1, 1)
    return types.SimpleNamespace(out=out.view(N, -1, H, W), mag=mag.view(N, -1, H, W), inside=inside, cols=cols,
                                 cols_bf16_exact=exact, frac=nfrac / (2.0 * N * G * 9 * P))


# ------------------------------------------------------------------------------------------------ edge bands
def band_pairs(G):
    """Nine (group, tap) pairs, tap j with group j (G - 1) // 8: 0 .. G - 1, both input halves."""
    return [((j * (G - 1)) // 8, j) for j in range(9)]


def edge_targets(H, W, dyadic):
    """(name, row, column, corners outside the frame); None: the residue itself is -+1000."""
    if dyadic:
        return [("row in (-1, 0)", -0.5, 2.25, 2), ("row in (H-1, H)", H - 0.75, 1.5, 2), ("column in (-1, 0)", 3.25, -0.25, 2),
                ("column in (W-1, W)", 2.5, W - 0.5, 2), ("frame corner", -0.75, W - 0.25, 3), ("row -1", -1.0, 2.0, 2),
                ("row H", float(H), 1.0, 4), ("inside", 2.75, 3.25, 0), ("far outside", None, None, 4)]
    return [("row in (-1, 0)", -0.37, 2.61, 2), ("row in (H-1, H)", H - 0.63, 1.37, 2), ("column in (-1, 0)", 3.29, -0.61, 2),
            ("column in (W-1, W)", 2.43, W - 0.37, 2), ("frame corner", -0.63, W - 0.29, 3), ("row beyond -1", -1.37, 2.61, 4),
            ("row beyond H", H + 0.37, 1.29, 4), ("inside", 2.71, 3.37, 0), ("far outside", None, None, 4)]


def pin_bands(res, flows, dtype, G, dyadic):
    """Overwrites the residues res (N, 18 G, H, W; float32 values of `dtype`) of the nine band pairs in place.
    -> [(group, tap, name, corners outside, covered (N, H, W) bool)]."""
    N, _, H, W = res.shape
    r = res.view(N, G, 9, 2, H, W)
    zero = torch.zeros(N, H, W)
    bands = []
    for (g, k), (name, ty, tx, outside) in zip(band_pairs(G), edge_targets(H, W, dyadic)):
        if ty is None:
            r[:, g, k, 0], r[:, g, k, 1] = -1000.0, 1000.0                           # 125 * 8: exact in bf16
            bands.append((g, k, name, outside, torch.ones(N, H, W, dtype=torch.bool)))
            continue
        fl = None if flows is None else flows[0 if g < G // 2 else 1]
        by, bx = tap_positions(k, H, W, zero if fl is None else fl[..., 1], zero if fl is None else fl[..., 0], 0.0, 0.0)
        dy, dx = ty - by, tx - bx                                                     # float32
        if dtype == FP:
            ok = torch.ones(N, H, W, dtype=torch.bool)
        elif dyadic:
            ok = (rb(dy, dtype) == dy) & (rb(dx, dtype) == dx)
        else:
            ok = (dy.abs() < 64) & (dx.abs() < 64)
        r[:, g, k, 0] = torch.where(ok, rb(dy, dtype), r[:, g, k, 0])
        r[:, g, k, 1] = torch.where(ok, rb(dx, dtype), r[:, g, k, 1])
        bands.append((g, k, name, outside, ok))
    return bands


def _seed(case, salt):
    mode, dtype, Fr, H, W, half, cout, G = case
    return salt + 7 * mode + 1000 * Fr + 31 * H + 17 * W + half + 3 * cout + G + (0 if dtype == BF else 5)


@functools.lru_cache(maxsize=1)
def dyadic_data(case, offs_mode):
    """-> namespace: x (F, 2 half, H, W), w, b; raw (F, 27 G, H, W) as the kernel reads it, in the reference's channel order
    (o1 | o2 | mask); residues (float32) and mask (float64) as the kernel has them after its activation; f1, f2 (None in
    mode 2); bands.  Read only: shared between the tests of a case."""
    mode, dtype, Fr, H, W, half, cout, G = case
    assert mode == offs_mode
    g = torch.Generator().manual_seed(_seed(case, 101))
    x = int_tensor((Fr, 2 * half, H, W), -8, 8, g)
    w = int_tensor((cout, 2 * half, 3, 3), -3, 3, g)
    b = int_tensor((cout,), -8, 8, g)
    lvl = int_tensor((Fr, 9 * G, H, W), 0, 2, g)                                      # masks 0, 0.5, 1
    f1 = f2 = None
    if mode == 0:
        sgn = int_tensor((Fr, 18 * G, H, W), -1, 1, g)
        raw_res, res = sgn * 60.0, sgn * MAX_MAG
        f1, f2 = (int_tensor((Fr, H, W, 2), -20, 20, g) / 4 for _ in range(2))        # the fractions come from the flows
        bands = []
    else:
        res = int_tensor((Fr, 18 * G, H, W), -19, 19, g) / 4
        if mode == 1:
            f1, f2 = (int_tensor((Fr, H, W, 2), -12, 12, g) / 4 for _ in range(2))
        bands = pin_bands(res, None if mode == 2 else (f1, f2), dtype, G, True)
        for gb, k, _, _, ok in bands:                                                 # a band sample is never masked out
            lvl[:, gb * 9 + k] = torch.where(ok, torch.tensor(2.0), lvl[:, gb * 9 + k])
        raw_res = res
    mask = lvl * 0.5
    raw_mask = mask if mode == 1 else (lvl - 1) * 100.0                               # sigmoid(-100, 0, 100) = 0, 0.5, 1
    raw = torch.cat([raw_res, raw_mask], dim=1)
    assert torch.equal(rb(raw, dtype), raw) and torch.equal(rb(x, BF), x) and torch.equal(rb(w, BF), w)
    return types.SimpleNamespace(x=x, w=w, b=b, raw=raw, residues=res.contiguous(), mask=mask.double(), f1=f1, f2=f2,
                                 flows=None if f1 is None else (f1, f2), bands=bands)


def onehot_weight(cout, cin, G):
    """One nonzero per output channel: w[co, ci(co), k(co)] = +-1 or +-2, k(co) = co % 9; the first nine couts aim at the
    band pairs, the others walk all G groups of both halves (group co % G, channel (co // G) % cpg of it)."""
    cpg = cin // G
    w = torch.zeros(cout, cin, 9)
    pairs = band_pairs(G)
    for co in range(cout):
        k = co % 9
        grp = pairs[co][0] if co < 9 else co % G
        w[co, grp * cpg + (co // G) % cpg, k] = (1.0, -1.0, 2.0, -2.0)[(co // 3) % 4]
    return w.view(cout, cin, 3, 3)


@functools.lru_cache(maxsize=1)
def generic_data(case):
    """The ordinary random inputs of test_dcn_strided (mode 1: residues 10 tanh(randn), masks sigmoid(randn), flows
    2 randn) or of test_dcn_raw_offsets_match_oracle (mode 2: offsets 2.5 randn, raw masks randn), each rounded to the
    element type where the kernel reads it in that type; the bands on non-dyadic targets; one-hot weights; bias 0.1 randn."""
    mode, dtype, Fr, H, W, half, cout, G = case
    assert mode in (1, 2)
    g = torch.Generator().manual_seed(_seed(case, 202))
    x = rb(torch.randn(Fr, 2 * half, H, W, generator=g), dtype)
    b = torch.randn(cout, generator=g) * 0.1
    f1 = f2 = None
    if mode == 1:
        res = rb(10 * torch.tanh(torch.randn(Fr, 18 * G, H, W, generator=g)), dtype)
        raw_mask = rb(torch.sigmoid(torch.randn(Fr, 9 * G, H, W, generator=g)), dtype)
        f1, f2 = (torch.randn(Fr, H, W, 2, generator=g) * 2 for _ in range(2))
    else:
        res = rb(2.5 * torch.randn(Fr, 18 * G, H, W, generator=g), dtype)
        raw_mask = rb(torch.randn(Fr, 9 * G, H, W, generator=g), dtype)
    bands = pin_bands(res, None if mode == 2 else (f1, f2), dtype, G, False)
    mask = raw_mask.double() if mode == 1 else torch.sigmoid(raw_mask.double())
    return types.SimpleNamespace(x=x, w=onehot_weight(cout, 2 * half, G), b=b, raw=torch.cat([res, raw_mask], dim=1),
                                 residues=res.contiguous(), mask=mask, f1=f1, f2=f2,
                                 flows=None if f1 is None else (f1, f2), bands=bands)


# ------------------------------------------------------------------------------------------------ shares and bounds
def partly_outside_share(inside):
    """Share of the (pixel, tap, group) samples with one to three corners inside the frame."""
    return ((inside > 0) & (inside < 4)).float().mean().item()


def partly_outside_floor(H, W):
    return 0.05 if H * W <= 512 else 0.01


def band_report(inside, bands):
    """Per band: (name, covered pixels, pixels, covered pixels whose corner count is not the intended one)."""
    rows = []
    for g, k, name, outside, ok in bands:
        cnt = inside[:, g, k]
        rows.append((name, int(ok.sum()), ok.numel(), int(((cnt != 4 - outside) & ok).sum())))
    return rows


U8, U9, U24 = 2.0 ** -8, 2.0 ** -9, 2.0 ** -24


def n16(case):
    """bf16 roundings that the form applies to the blended sample: 0 in f32, 1 in bf16 (the sample is staged in bf16 for
    the MFMA), 2 in the DOT2 forms (the weights are rounded as well)."""
    return 0 if case[1] == FP else 2 if is_dot2(case) else 1


def onehot_bound(case, ref, S, as_issued=False):
    """Per element bound on |y - ref| for one-hot weights, y = bias + w * (one blended sample); S = the magnitude run.
      before the output rounding   pre = ((1 + 2^-8)^n16 - 1 + 8 2^-24 [+ 16 2^-24 in mode 2, the fast sigmoid]) S
      the output rounding          half a unit in the last place at |ref| + pre (bf16), 2^-24 (|ref| + pre) (f32)
    8 2^-24 covers the f32 weight products and the four-term blend.  One round-to-nearest to bf16 moves a value by up to
    half a unit in the last place, which is 2^-8 of the value at the bottom of a binade and 2^-9 only at its top.
    as_issued: the bound with 2^-9 per bf16 rounding, (n16 2^-9 + 8 2^-24) S + 2^-9 |ref|, as dcn.hip's comment on the dot2
    blend first had it -- the correctly rounded emulations of tests/test_dcn_frac_cpu.py leave it by a factor of 1.5 to 1.75,
    which that file keeps on record."""
    from tests.util import out_rounding
    mode, dtype = case[:2]
    f32 = 8 * U24 + (16 * U24 if mode == 2 else 0.0)
    if as_issued:
        return (n16(case) * U9 + f32) * S + (U9 if dtype == BF else U24) * ref.abs()
    pre = ((1 + U8) ** n16(case) - 1 + f32) * S
    top = ref.abs() + pre
    return pre + (out_rounding(top, BF) if dtype == BF else U24 * top)
