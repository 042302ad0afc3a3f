"""The known-statistics harness of tests/test_gpu_norm_exact.py, checked without a GPU: the preconditions of its input
builders for every GPU case, its float64 references against torch in double, and the written record of the gap it closes.

The record: a GroupNorm whose statistics lose one element of every (statistic, group), count it twice, or take one frame
from the neighbouring statistic, and one whose variance is off by 1 %, are modelled on the CPU (faulty statistics in
float64, then the kernels' f32 fold, gn_fold_f32).  On the randn data of test_gpu_kernels.test_group_norm they pass that
test's assert_close -- in bf16 in every case, in f32 for the larger tensors -- while the balanced and the spike checks
of the new file fail on each of them in both dtypes."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_norm_exact import (ADAIN_SHAPES, BF, BOTH, EXACT, FP, LN_SHAPES, MAX_COUNT, MUS, NAME, OFFSET, SPIKE,
                                       TAIL, VEC, adain_ints, balanced_case, gn_bound, gn_chain, gn_path, layernorm_balanced_case,
                                       offset_case, spike_case)
from tests.test_gpu_norm_exact import test_cases_reach_every_groupnorm_path as _cases_reach_every_path
from tests.util import (ACT_GELU, ACT_LRELU01, ACT_LRELU02, ACT_NONE, ACT_RELU, ACT_SILU, act64, adain_ref64,
                        assert_bits_equal, assert_close, assert_elem_close, gn_fold_f32, gn_from_sets, gn_ref64, gn_sets,
                        layernorm_ref64, pool2, rb, resample_ref, up2)

# the two largest tensors of the table take seconds to build on the CPU; their preconditions follow from the builder's
# construction, which the smaller cases check (count is checked for all)
SMALL = [c for c in EXACT if c.T * c.H * c.W * c.C <= 1 << 22]


def _exact_in(t, dtype):
    return torch.equal(t.float().to(dtype).double(), t.double())


def test_case_table_reaches_every_groupnorm_path():
    _cases_reach_every_path()


# ------------------------------------------------------------------------------------------------ preconditions
@pytest.mark.parametrize("c", EXACT, ids=str)
def test_balanced_counts(c):
    cnt = c.frames * c.H * c.W * (c.C // c.groups)
    assert cnt % 2 == 0 and cnt <= MAX_COUNT, (c, cnt)
    assert c.C % 8 == 0 and c.c0 % 8 == 0 and c.T % c.frames == 0


@pytest.mark.parametrize("c", SMALL, ids=str)
def test_balanced_preconditions(c):
    """Every (statistic, group) sums to 0 over count elements of +-1, no contiguous half of it does in general, and the
    expected output and its resampled forms are small integers (quarters after pooling): exact in bf16."""
    x, gamma, beta, film, pre = balanced_case(c)
    s = gn_sets(x, c.frames, c.groups)
    assert bool((s.abs() == 1).all()) and bool((s.sum((1, 3)) == 0).all())
    if s.shape[1] >= 64:
        half = s[:, :s.shape[1] // 2].sum((1, 3))
        assert bool((half != 0).any()), "every half range is balanced: a lost range would go unnoticed"
    assert bool((gamma.abs().log2() == gamma.abs().log2().round()).all()) and gamma.abs().max().item() <= 4
    assert torch.equal(beta[0::2], -gamma[0::2]) and torch.equal(beta[1::2], gamma[1::2])
    for act in (ACT_NONE, ACT_RELU):
        want = resample_ref(act64(pre, act), c.resample)
        assert _exact_in(want, BF) and _exact_in(want, FP) and want.abs().max().item() <= 64
    zeros = (pre == 0).double().mean().item()
    assert zeros >= (0.05 if film is not None else 0.45), zeros
    if c.resample:
        assert _exact_in(resample_ref(x.double(), c.resample), BF)
    # the reference of part 2 agrees: mean 0, variance 1, so A = gamma and B = beta
    r = gn_ref64(x, gamma, beta, c.frames, c.groups, 0.0, film)
    assert bool((r["mean"] == 0).all()) and bool((r["var"] == 1).all()) and torch.equal(r["pre"], pre)


def test_one_element_changes_the_f32_fold_up_to_2_21():
    """One element too few at count = 2^21: mean = -+2^-21 and var = 1 - 2^-21 - 2^-42, so the f32 rstd is 1 + 2^-22 and
    B = beta - mean * A moves by 2^-21 |gamma|: both representable next to 1, and gamma * 2^-22 stays where 0 belongs (it
    survives a bf16 output, which rounds relative to the value itself)."""
    cnt = float(MAX_COUNT)
    x = torch.tensor([1.0, -1.0]).view(1, 1, 1, 2)
    gamma, beta = torch.tensor([2.0, 2.0]), torch.tensor([-2.0, -2.0])
    for lost in (1.0, -1.0):
        for w in (-1.0, 1.0):                 # dropped or counted twice
            mean = torch.tensor(w * lost / cnt, dtype=torch.float64)
            var = (cnt + w) / cnt - mean * mean
            y = gn_fold_f32(x, mean, var, gamma, beta, 0.0)
            assert y[0, 0, 0, 0].item() != 0.0 and abs(y[0, 0, 0, 0].item()) >= 2.0 ** -23
            assert y.to(BF)[0, 0, 0, 0].item() != 0.0
    assert gn_fold_f32(x, torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64), gamma, beta, 0.0)[0, 0, 0, 0].item() == 0.0


@pytest.mark.parametrize("c", SPIKE + TAIL[1:], ids=str)
def test_spike_preconditions(c):
    """One 64 per (statistic, group), the rest integers in [-3, 3]; the first four groups hold it at the first / last pixel
    of the statistic and of a frame; sums of |x| and x^2 stay below 2^24."""
    from tests.util import spiked_ints
    g = torch.Generator().manual_seed(5)
    x, pos = spiked_ints(c.T, c.H, c.W, c.C, c.frames, c.groups, g)
    s = gn_sets(x, c.frames, c.groups)
    assert bool(((s == 64).sum((1, 3)) == 1).all()) and bool((s[s != 64].abs() <= 3).all())
    cpg, n, hw = c.C // c.groups, s.shape[1], c.H * c.W
    assert (pos[:, :4] // cpg).tolist() == [[0, n - 1, hw - 1, n - hw]] * s.shape[0]
    assert s.pow(2).sum((1, 3)).max().item() < 2 ** 24
    x, gamma, beta, film = spike_case(c)
    assert _exact_in(x, BF)
    if c.resample == 1:
        assert _exact_in(pool2(x.double()), BF)


@pytest.mark.parametrize("c,dtype,mu", [(c, dt, mu) for c in OFFSET for dt in c.dtypes for mu in MUS[dt]],
                         ids=lambda v: NAME.get(v, str(v)))
def test_offset_preconditions(c, dtype, mu):
    """Every value is exact in the dtype and the f32 sums of x are exact in any order: multiples of `step` whose absolute
    sum over everything that is added in f32 (a thread's K values in the one-launch kernel, a workgroup's pixel range of a
    group with three launches; f64 from there) stays below 2^24 * step.  K follows the launch geometry."""
    x, gamma, beta, film = offset_case(c, mu, dtype)
    assert _exact_in(x, dtype)
    step = 0.5 if dtype == BF and mu >= 64 else 1.0
    assert torch.equal((x / step).round() * step, x)
    p = gn_path(c, dtype)
    pix = c.frames * c.H * c.W
    in_f32 = gn_chain(c, dtype) if p["kernel"] == "group" else -(-pix // p["wgs"]) * (c.C // c.groups)
    assert in_f32 * x.abs().max().item() < 2 ** 24 * step
    z = x - mu
    assert z.abs().max().item() <= 2 and z.min().item() < 0 < z.max().item()
    K = gn_chain(c, dtype)
    if p["kernel"] == "group":
        assert K == pix * VEC[dtype] // (1024 // p["pp"]) == 64 // (2 if dtype == FP else 1)
    else:       # 1152 pixels: 3 workgroups of 32 rows in bf16 (384 pixels, 12 per row), 5 of 16 rows in f32 (231, 15 per row)
        assert (p["wgs"], p["rows"], K) == ((3, 32, 12 + 32 + 2) if dtype == BF else (5, 16, 15 + 16 + 2))


def test_layernorm_adain_preconditions():
    for dtype in BOTH:
        for k in range(5):
            for shape in LN_SHAPES:
                x, gamma, beta, pos = layernorm_balanced_case(dtype, k, shape)
                rows = shape[0] * shape[1] * shape[2]
                assert rows % 4 == (1 if shape == LN_SHAPES[0] else 0) and pos.shape[0] < rows
                assert bool((x.sum(-1) == 0).all()) and bool((x.abs() == 1).all())
                assert _exact_in(x.double() * gamma.double() + beta.double() + pos.double().repeat(shape[0], 1).view(*shape, -1), BF)
    for hw, C in ADAIN_SHAPES:
        content, style = adain_ints(hw, C, torch.Generator().manual_seed(1))
        assert _exact_in(content, BF) and _exact_in(style, BF) and content.abs().sum((1, 2)).max().item() < 2 ** 24


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("c", SPIKE, ids=str)
def test_gn_ref64_against_torch(c):
    x, gamma, beta, film = spike_case(c)
    r = gn_ref64(x, gamma, beta, c.frames, c.groups, 1e-5, film)
    xd = x.double().permute(0, 3, 1, 2)                                       # T, C, H, W
    ns = c.T // c.frames
    clip = xd.reshape(ns, c.frames, c.C, c.H, c.W).permute(0, 2, 1, 3, 4)     # ns, C, fps, H, W
    n = F.group_norm(clip, c.groups, gamma.double(), beta.double(), 1e-5).permute(0, 2, 1, 3, 4).reshape(c.T, c.C, c.H, c.W)
    if film is not None:
        n = n * (1 + film[:, :c.C, None, None].double()) + film[:, c.C:2 * c.C, None, None].double()
    ref = n.permute(0, 2, 3, 1)
    assert (r["pre"] - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    assert bool((r["S"] >= r["pre"].abs() * (1 - 1e-12)).all())
    for act, f in ((ACT_SILU, F.silu), (ACT_GELU, F.gelu), (ACT_RELU, F.relu), (ACT_LRELU02, lambda v: F.leaky_relu(v, 0.2)),
                   (ACT_LRELU01, lambda v: F.leaky_relu(v, 0.1))):
        assert (act64(ref, act) - f(ref)).abs().max().item() <= 1e-7 * ref.abs().max().item()
    assert torch.equal(up2(ref).permute(0, 3, 1, 2), F.interpolate(ref.permute(0, 3, 1, 2), scale_factor=2, mode="nearest"))
    assert (pool2(ref[:, :2 * (c.H // 2), :2 * (c.W // 2)]).permute(0, 3, 1, 2)
            - F.avg_pool2d(ref.permute(0, 3, 1, 2), 2)).abs().max().item() <= 1e-12 * ref.abs().max().item()


def test_layernorm_and_adain_ref64_against_torch():
    from oracle import codeformer as ocf
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 5, 72, generator=g) * 3 + 7
    s = torch.randn(2, 3, 5, 72, generator=g) * 2 - 5
    gamma, beta = torch.randn(72, generator=g), torch.randn(72, generator=g)
    y, S = layernorm_ref64(x, gamma, beta, 1e-5)
    ref = F.layer_norm(x.double(), (72,), gamma.double(), beta.double(), 1e-5)
    assert (y - ref).abs().max().item() <= 1e-12 and bool((S >= y.abs() * (1 - 1e-12)).all())
    y, S = adain_ref64(x, s, 1e-5)
    ref = ocf.adain(x.double().permute(0, 3, 1, 2), s.double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert (y - ref).abs().max().item() <= 1e-12 * ref.abs().max().item() and bool((S >= y.abs() * (1 - 1e-12)).all())


# ------------------------------------------------------------------------------------------------ the gap
FAULTS = ("dropped", "doubled", "neighbour")


def faulty_stats(x, fps, groups, fault):
    """mean and variance (float64, per element) of a GroupNorm whose sums weigh the first element of every (statistic,
    group) 0 times (dropped) or twice (doubled) while dividing by the true count, or that takes the first frame of every
    statistic from the next statistic (neighbour; the last one from the previous)."""
    T, H, W, C = x.shape
    s = gn_sets(x.double(), fps, groups).clone()
    cnt = s.shape[1] * s.shape[3]
    if fault == "neighbour":
        assert s.shape[0] > 1 and fps > 1
        other = torch.roll(s, -1, 0)
        other[-1] = s[-2]
        s[:, :H * W] = other[:, :H * W]
        sm, sq = s.sum((1, 3), keepdim=True), s.pow(2).sum((1, 3), keepdim=True)
    else:
        w = -1.0 if fault == "dropped" else 1.0
        first = s[:, :1, :, :1]
        sm = s.sum((1, 3), keepdim=True) + w * first
        sq = s.pow(2).sum((1, 3), keepdim=True) + w * first.pow(2)
    mean = sm / cnt
    var = (sq / cnt - mean * mean).clamp_min(0.0)
    full = lambda t: gn_from_sets(t.expand(s.shape), T, H, W)
    return full(mean), full(var)


def faulty_gn(x, gamma, beta, fps, groups, eps, film, act, dtype, fault, var_scale=1.0, resample=0):
    if fault is None:
        r = gn_ref64(x, gamma, beta, fps, groups, 0.0)
        mean, var = r["mean"], r["var"]
    else:
        mean, var = faulty_stats(x, fps, groups, fault)
    pre = gn_fold_f32(x, mean, var * var_scale, gamma, beta, eps, film)
    return resample_ref(act64(pre.double(), act), resample).float().to(dtype)


# test_gpu_kernels.test_group_norm: its cases (T, H, W, c0, c1, film, fps, resample) and its data
OLD_CASES = [(4, 16, 16, 64, 0, False, None), (3, 12, 20, 128, 64, True, None), (2, 16, 16, 64, 0, True, None, 1),
             (2, 8, 8, 256, 0, False, None, 2), (4, 8, 8, 96, 0, True, 1),
             (16, 4, 4, 1024, 0, True, None), (3, 4, 4, 1024, 1024, True, None), (16, 32, 32, 256, 0, True, None),
             (16, 16, 16, 256, 256, True, None), (4, 8, 8, 256, 0, True, 1), (8, 16, 16, 512, 0, False, None)]
OLD_F32_PASS = [(16, 32, 32, 256, 0, True, None), (8, 16, 16, 512, 0, False, None)]


def old_inputs(case, dtype):
    T, H, W, c0, c1, film, fps = case[:7]
    C = c0 + c1
    g = torch.Generator().manual_seed(7 + C)
    x = rb(torch.randn(T, C, H, W, generator=g) * 1.7 + 0.3, dtype)
    gamma = torch.randn(C, generator=g)
    beta = torch.randn(C, generator=g)
    emb = torch.randn(T, 2 * C + (5 if C < 512 else 8), generator=g) * 0.5 if film else None
    if fps == 1:
        n = F.group_norm(x, 32, gamma, beta, 1e-5)
    else:
        n = F.group_norm(x.permute(1, 0, 2, 3)[None], 32, gamma, beta, 1e-5)[0].permute(1, 0, 2, 3)
    if film:
        n = n * (1 + emb[:, :C, None, None]) + emb[:, C:2 * C, None, None]
    ref = resample_ref(F.silu(n).permute(0, 2, 3, 1), case[7] if len(case) > 7 else 0)
    return x.permute(0, 2, 3, 1).contiguous(), gamma, beta, emb, ref, fps or T


@pytest.mark.parametrize("fault", FAULTS[:2])
@pytest.mark.parametrize("case", OLD_CASES, ids=str)
def test_lost_element_passes_the_old_test(case, fault):
    """bf16: every case passes (error 1e-2 .. 2e-2 against a bound of about 0.3); f32: the two largest tensors pass."""
    for dtype in BOTH:
        if dtype == FP and case not in OLD_F32_PASS:
            continue
        x, gamma, beta, emb, ref, fps = old_inputs(case, dtype)
        got = faulty_gn(x, gamma, beta, fps, 32, 1e-5, emb, ACT_SILU, dtype, fault, resample=case[7] if len(case) > 7 else 0).float()
        err = assert_close(got, ref, dtype, f"{fault} {case} {NAME[dtype]}", scale=4.0)
        print(f"{fault:9s} {NAME[dtype]:4s} {case}: max|err| {err:.3e}")


@pytest.mark.parametrize("dtype", BOTH, ids=lambda d: NAME[d])
def test_neighbour_frame_and_variance_pass_the_old_test(dtype):
    """(16, 32, 32, 256) read as 4 statistics of 4 frames: one frame of 4 from the neighbouring statistic (randn data: all
    statistics look alike) and a variance off by 1 % both stay inside the old bound in bf16; the 1 % passes in bf16 only."""
    case = (16, 32, 32, 256, 0, True, None)
    x, gamma, beta, emb, _, _ = old_inputs(case, dtype)
    r = gn_ref64(x, gamma, beta, 4, 32, 1e-5, emb)
    ref = act64(r["pre"], ACT_SILU).float()
    got = faulty_gn(x, gamma, beta, 4, 32, 1e-5, emb, ACT_SILU, dtype, "neighbour").float()
    if dtype == BF:
        assert_close(got, ref, dtype, "neighbour", scale=4.0)
        got = faulty_gn(x, gamma, beta, 4, 32, 1e-5, emb, ACT_SILU, dtype, None, var_scale=1.01).float()
        assert_close(got, ref, dtype, "var * 1.01", scale=4.0)
    else:
        with pytest.raises(AssertionError):
            assert_close(got, ref, dtype, "neighbour", scale=4.0)


def _fails(f, *a, **k):
    with pytest.raises(AssertionError):
        f(*a, **k)


@pytest.mark.parametrize("dtype", BOTH, ids=lambda d: NAME[d])
@pytest.mark.parametrize("c", [EXACT[0], EXACT[2], EXACT[19], EXACT[21], EXACT[11], EXACT[12]], ids=str)
def test_faults_fail_the_balanced_check(c, dtype):
    """The model without a fault gives the expected bits; each fault leaves a nonzero where 0 belongs."""
    x, gamma, beta, film, pre = balanced_case(c)
    for act in (ACT_NONE, ACT_RELU):
        want = act64(pre, act).to(dtype)
        assert_bits_equal(faulty_gn(x, gamma, beta, c.frames, c.groups, 0.0, film, act, dtype, None), want, "no fault")
        for fault in FAULTS:
            if fault == "neighbour" and not 1 < c.frames < c.T:
                continue
            got = faulty_gn(x, gamma, beta, c.frames, c.groups, 0.0, film, act, dtype, fault)
            if fault == "neighbour" and bool((faulty_stats(x, c.frames, c.groups, fault)[0] == 0).all()):
                continue        # the borrowed frame happens to be balanced in every group: cannot happen with 64 pixels x 32 channels
            _fails(assert_bits_equal, got, want, f"{fault} {c}")


@pytest.mark.parametrize("dtype", BOTH, ids=lambda d: NAME[d])
@pytest.mark.parametrize("c", SPIKE, ids=str)
def test_faults_fail_the_spike_check(c, dtype):
    """The same models, and a variance off by 1 %, against the per-element bound of part 2 (act NONE); the model without
    a fault stays inside it."""
    x, gamma, beta, film = spike_case(c)
    r = gn_ref64(x, gamma, beta, c.frames, c.groups, 1e-5, film)
    bound = gn_bound(r["pre"], r, ACT_NONE, dtype)
    ok = faulty_gn(x, gamma, beta, c.frames, c.groups, 1e-5, film, ACT_NONE, dtype, None)
    ratio = assert_elem_close(ok, r["pre"], bound, 1.0, "no fault")
    print(f"f32 fold on the CPU, {c} {NAME[dtype]}: err/bound {ratio:.3f}")
    for fault in FAULTS:
        if fault == "neighbour" and not 1 < c.frames < c.T:
            continue
        _fails(assert_elem_close, faulty_gn(x, gamma, beta, c.frames, c.groups, 1e-5, film, ACT_NONE, dtype, fault), r["pre"],
               bound, 1.0, fault)
    _fails(assert_elem_close, faulty_gn(x, gamma, beta, c.frames, c.groups, 1e-5, film, ACT_NONE, dtype, None, var_scale=1.01),
           r["pre"], bound, 1.0, "var * 1.01")
