"""GPU: flair_niqe_luma and flair_niqe_moments against tests/niqe_ref.py -- the integer planes bit for bit, the MSCN map per
element, the block moments within the order-of-summation bound, the whole score within 1e-9 of the float64 definition,
flat regions, the same bits alone / in a batch / through the commands, and guarded views."""
import json
import math

import numpy as np
import pytest
import torch

from tests import niqe_ref as R
from tests import util

pytestmark = pytest.mark.gpu

PARAMS = R.synthetic_params()
SHAPES = [(1, 96, 192), (3, 200, 301), (2, 192, 96)]          # two blocks; odd sizes, a crop and a batch; a column of blocks
EPS = 2.0 ** -53
MSCN_FLOOR = 16 * EPS * 255                                   # sixteen roundings of a value of at most 255
SCORE_BOUND = 1e-9                                            # relative; float64 order noise is ~1e-13, one alpha cell 1.6e-4
ids = lambda s: "x".join(map(str, s))  # noqa: E731


parity = util.parity_log                                     # measured figures: printed and kept with the suite's other parity lines


@pytest.fixture(scope="module")
def model(dev):
    from flair_amd import niqe as Q
    return Q.NIQE(*PARAMS, dev)


def planes_ref(frames):
    y1 = np.stack([R.crop(R.luma(f)) for f in frames])
    return y1, np.stack([R.half_scale(y) for y in y1])


def run(model, u8):
    """The three launches on (N, H, W, 3) uint8 frames -> y1, y2, [mscn per scale], [moments per scale] as numpy arrays."""
    from flair_amd import ops
    y1, y2 = ops.niqe_luma(u8)
    maps = [torch.full(y.shape, math.nan, dtype=torch.float64, device=u8.device) for y in (y1, y2)]
    m1 = ops.niqe_moments(y1, 96, 1.0, model.window, mscn=maps[0])
    m2 = ops.niqe_moments(y2, 48, ops.NIQE_HALF_UNIT, model.window, mscn=maps[1])
    torch.cuda.synchronize()
    return y1.cpu().numpy(), y2.cpu().numpy(), [m.cpu().numpy() for m in maps], [m1.cpu().numpy(), m2.cpu().numpy()]


# ------------------------------------------------------------------------------------------- the integer planes
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_luma_planes_are_bit_exact(dev, shape):
    from flair_amd import ops
    frames = R.case(*shape)
    y1, y2 = ops.niqe_luma(torch.from_numpy(frames).to(dev))
    r1, r2 = planes_ref(frames)
    assert y1.dtype == torch.int32 and tuple(y1.shape) == r1.shape and tuple(y2.shape) == r2.shape
    assert np.array_equal(y1.cpu().numpy(), r1) and np.array_equal(y2.cpu().numpy(), r2)
    assert r1.min() >= 16 and r1.max() <= 235 and np.abs(r2).max() < 2 ** 25


def test_luma_on_rounding_ties_at_every_alignment(dev):
    """Frames tiled from the 580 byte triples on or next to a rounding tie, read through a byte pointer offset by 0 .. 3."""
    from flair_amd import ops
    ties = R.tie_triples()
    n = 2 * 100 * 197
    frames = ties[(np.arange(n) * 7) % len(ties)].reshape(2, 100, 197, 3)
    frames[1] = frames[1, ::-1, :, ::-1].copy()
    r1, r2 = planes_ref(frames)
    exact = R.luma(ties)                    # the 194 exact ties round to even
    t64 = ties.astype(np.int64)
    on = (65481 * t64[:, 0] + 128553 * t64[:, 1] + 24966 * t64[:, 2]) % 255000 == 127500
    assert on.sum() == 194 and np.all((exact[on] - 16) % 2 == 0)
    flat = torch.from_numpy(frames.reshape(-1)).to(dev)
    for off in range(4):
        buf = torch.full((flat.numel() + 8,), 255, dtype=torch.uint8, device=dev)
        buf[off:off + flat.numel()] = flat
        u8 = buf[off:off + flat.numel()].view(2, 100, 197, 3)
        assert u8.data_ptr() % 4 == off and u8.is_contiguous()
        y1, y2 = ops.niqe_luma(u8)
        assert np.array_equal(y1.cpu().numpy(), r1) and np.array_equal(y2.cpu().numpy(), r2), off


# ------------------------------------------------------------------------------------------- MSCN map and moments
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_mscn_map_and_moments(dev, model, shape):
    frames = R.case(*shape)
    ref, again = R.case_reference(*shape), R.case_reference(*shape, "restatement")
    _, _, maps, moms = run(model, torch.from_numpy(frames).to(dev))
    for n in range(shape[0]):
        for s, block in enumerate((96, 48)):
            d, r = ref[n]["mscn"][s], again[n]["mscn"][s]
            assert np.abs(d).min() > 1e-9                                    # no sign of the reference hangs on its rounding
            form = np.abs(r - d).max()
            bound = max(4 * form, MSCN_FLOOR)
            err = np.abs(maps[s][n] - d).max()
            parity(f"niqe mscn    {ids(shape)} frame {n} scale {s + 1}: max|kernel - definition| = {err:.3e}, "
                   f"max|restatement - definition| = {form:.3e}, bound = {bound:.3e}, kernel == restatement bits: "
                   f"{np.array_equal(maps[s][n], r)}")
            assert err <= bound
            got, want, other = moms[s][n], ref[n]["moments"][:, s], again[n]["moments"][:, s]
            assert got.shape == want.shape
            assert np.array_equal(got[..., :2], want[..., :2])               # counts, exactly
            assert np.all(got[..., 0] + got[..., 1] == block * block)
            terms = want[..., 2:]                                            # every term of s-, s+ and a is non-negative
            mbound = np.maximum(4 * np.abs(other[..., 2:] - want[..., 2:]), (block * block - 1) * EPS * terms)
            merr = np.abs(got[..., 2:] - want[..., 2:])
            parity(f"niqe moments {ids(shape)} frame {n} scale {s + 1}: max err / bound = {(merr / mbound).max():.3e}, "
                   f"max rel err = {(merr / terms).max():.3e}")
            assert np.all(merr <= mbound)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_whole_score_against_the_definition(dev, model, shape):
    frames = R.case(*shape)
    ref, again = R.case_reference(*shape), R.case_reference(*shape, "restatement")
    got = model(torch.from_numpy(frames).to(dev))
    feats = model.features(torch.from_numpy(frames).to(dev))
    for n in range(shape[0]):
        want = ref[n]["score"]
        assert not np.isnan(ref[n]["features"]).any()
        cells = int((np.abs(feats[n] - ref[n]["features"])[:, [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]] > 5e-4).sum())
        parity(f"niqe score   {ids(shape)} frame {n}: kernel {got[n]!r}, definition {want!r}, rel err {abs(got[n] - want) / want:.3e}, "
               f"restatement rel err {abs(again[n]['score'] - want) / want:.3e}, alpha cells off: {cells}")
        assert abs(got[n] - want) <= SCORE_BOUND * want


# ------------------------------------------------------------------------------------------- flat regions
def test_flat_blocks_give_zero_moments_and_drop_out(dev, model):
    """Columns below 112 constant: the two blocks left of column 96 are flat together with everything their windows and the
    half-scale filter reach (column 104), so their moments are exactly zero at both scales; the next two blocks are flat in
    part and hold exact zeros beside real values.  The frame's score is that of the blocks that have one."""
    from flair_amd import niqe as Q
    u8 = R.frame(192, 288, 40.0, 5)
    u8[:, :112] = 90
    want = R.analyse(u8, PARAMS, form="restatement")
    _, _, maps, moms = run(model, torch.from_numpy(u8[None]).to(dev))
    for s, block in enumerate((96, 48)):
        assert not moms[s][0, :2].any()                                      # blocks j nh + i = 0, 1: column 0
        assert not maps[s][0][:, :block].any()
        zeros = block * block - moms[s][0, 2:4, 0, 0] - moms[s][0, 2:4, 0, 1]
        assert np.all(zeros >= block) and np.all(zeros < block * block)  # partly flat: zeros in neither count
        assert np.array_equal(moms[s][0][..., :2], want["moments"][:, s][..., :2])
    feats = model.features(torch.from_numpy(u8[None]).to(dev))[0]
    assert np.isnan(feats[:2]).all() and not np.isnan(feats[2:]).any()
    got = model(torch.from_numpy(u8[None]).to(dev))[0]
    assert got == Q.score(feats[2:], PARAMS[0], PARAMS[1])                   # the flat blocks drop out of mean and covariance
    rest = R.score_of(want["features"][2:], PARAMS[0], PARAMS[1])
    assert want["score"] == rest and abs(got - rest) <= SCORE_BOUND * rest


def test_a_constant_frame_has_no_score(dev, model):
    u8 = torch.full((2, 96, 192, 3), 77, dtype=torch.uint8, device=dev)
    u8[1] = 255
    _, _, maps, moms = run(model, u8)
    assert not moms[0].any() and not moms[1].any() and not maps[0].any() and not maps[1].any()
    got = model(u8)
    assert len(got) == 2 and all(math.isnan(v) for v in got)


# ------------------------------------------------------------------------------------------- the same bits
def test_same_bits_alone_in_a_batch_and_through_the_commands(dev, model, tmp_path, monkeypatch, capsys):
    from flair_amd import __main__ as cli
    from flair_amd import io as fio
    from flair_amd import metrics
    frames = R.case(3, 200, 301)
    alone = model(torch.from_numpy(frames[0:1]).to(dev))[0]
    trio = model(torch.from_numpy(frames[[1, 0, 2]]).to(dev))
    again = model(torch.from_numpy(frames[0:1]).to(dev))[0]
    assert alone == trio[1] == again and not math.isnan(alone)
    m_alone = model.moments(torch.from_numpy(frames[0:1]).to(dev))
    m_trio = model.moments(torch.from_numpy(frames[[1, 0, 2]]).to(dev))
    assert torch.equal(util.bits(m_alone[:, 0]), util.bits(m_trio[:, 1]))
    for d in ("out", "truth"):
        (tmp_path / d).mkdir()
        for i, f in enumerate(frames[[1, 0, 2]]):
            fio.write_frame(str(tmp_path / d / f"{i:04d}.png"), f)
    res = metrics.evaluate_dirs(str(tmp_path / "out"), str(tmp_path / "truth"), dev, niqe=model)
    assert [f["niqe"] for f in res["frames"]] == trio and res["mean"]["niqe_frames"] == 3
    assert res["mean"]["niqe"] == sum(trio) / 3 and res["frames"][0]["psnr"] == math.inf
    assert metrics.format_report(res)[1] == f"0001.png  psnr inf  ssim 1.0000  niqe {alone:.4f}"
    params = tmp_path / "p.npz"
    np.savez(params, mu_pris_param=PARAMS[0].reshape(1, 36), cov_pris_param=PARAMS[1], gaussian_window=PARAMS[2])
    out = tmp_path / "scores.json"
    capsys.readouterr()
    with torch.enable_grad():                     # main() turns autograd off for the process; keep it to this test
        assert cli.main(["niqe", str(tmp_path / "out"), "--params", str(params), "--json", str(out), "--device", str(dev)]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines == [f"{i:04d}.png  niqe {v:.4f}" for i, v in enumerate(trio)] + [f"mean of 3 of 3 frames  niqe {sum(trio) / 3:.4f}"]
    assert [f["niqe"] for f in json.loads(out.read_text())["frames"]] == trio


# ------------------------------------------------------------------------------------------- guarded views
def test_guarded_views_come_back_untouched(dev, model):
    from flair_amd import ops
    frames = R.case(2, 192, 96)
    r1, r2 = planes_ref(frames)
    ubuf, u8, ubefore = util.flat_guarded(frames.shape, torch.uint8, dev, 255, src=torch.from_numpy(frames))
    b1, y1, k1 = util.flat_guarded((2, 192, 96), torch.int32, dev, -7777)
    b2, y2, k2 = util.flat_guarded((2, 96, 48), torch.int32, dev, -7777)
    ops.niqe_luma(u8, y1=y1, y2=y2)
    torch.cuda.synchronize()
    util.assert_flat_untouched(ubuf, ubefore, what="niqe_luma u8")
    util.assert_flat_untouched(b1, k1, view=y1, what="niqe_luma y1")
    util.assert_flat_untouched(b2, k2, view=y2, what="niqe_luma y2")
    assert np.array_equal(y1.cpu().numpy(), r1) and np.array_equal(y2.cpu().numpy(), r2)
    free = run(model, torch.from_numpy(frames).to(dev))
    for s, (y, block, unit) in enumerate(((y1, 96, 1.0), (y2, 48, ops.NIQE_HALF_UNIT))):
        # the plane between two poisoned neighbours: a read outside it would reach the moments and the map
        pbuf, plane, pbefore = util.flat_guarded(tuple(y.shape), torch.int32, dev, 1 << 30, src=y, pad=4096)
        wbuf, win, wbefore = util.flat_guarded((7, 7), torch.float64, dev, math.nan, src=model.window)
        obuf, out, obefore = util.flat_guarded((2, 2, 5, 5), torch.float64, dev, util.OUT_FILL)
        mbuf, mscn, mbefore = util.flat_guarded(tuple(y.shape), torch.float64, dev, util.OUT_FILL)
        ops.niqe_moments(plane, block, unit, win, out=out, mscn=mscn)
        torch.cuda.synchronize()
        util.assert_flat_untouched(pbuf, pbefore, what="niqe_moments y")
        util.assert_flat_untouched(wbuf, wbefore, what="niqe_moments window")
        util.assert_flat_untouched(obuf, obefore, view=out, what="niqe_moments out")
        util.assert_flat_untouched(mbuf, mbefore, view=mscn, what="niqe_moments mscn")
        assert np.array_equal(out.cpu().numpy(), free[3][s]) and np.array_equal(mscn.cpu().numpy(), free[2][s])
        # without a map nothing else changes
        ops.niqe_moments(plane, block, unit, win, out=out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), free[3][s])
