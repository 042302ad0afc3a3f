"""Generate tests/golden/g18_amt.npz: AMT-G frame interpolation, end to end, from the reference's own module.

Run it where the reference source tree is available (refimport.REFERENCE_ROOT, as for make_golden.py), from the repository
root:

    python tests/golden/make_golden_amt.py

guided_diffusion/amt.py and amt_blocks/ are imported through refimport (einops is installed, more_itertools is stubbed and
never called) and run unmodified, eval mode, 8 intra-op threads (tests/util.FIXTURE_THREADS).  The intermediate quantities
are read from the reference's run with hooks: forward hooks on feat_encoder and the decoders, pre-hooks on the decoders for
the flows that enter them, and wrappers around BidirCorrBlock.__call__ and multi_flow_combine.

Weights: name-seeded (tests/golden/weights.py), regenerated in the tests and never stored; the flow and mask channels of the
decoders' transposed convolutions and the last convolution of every flow_head are scaled (tests/amt_cpu.SCALES; the factors
are stored).  Asserted below on the reference's own output, per case and timestep: the full-resolution final flows have a
mean |flow| between 1 and 10 px; the sigmoid mask has a minimum below 0.1 and a maximum above 0.9; the output differs from
the plain blend by more than 100 x its stored deviation; and between 5 % and 40 % of the lookups' bilinear corner samples ON
THE FINEST LEVEL fall outside their plane.  Over all four levels that share cannot be brought under 40 % at sizes a fixture
can hold: the 8 x 8 corner patch of a 7 x 7 window is wider than the 4 x 4 and 2 x 2 planes of the coarse levels, so with
zero flow 55 % (16 x 16 and 16 x 18 grids) to 67 % (8 x 8 grid) of all corners are outside already; the share over all
levels is printed next to its zero-flow floor.

Case s32 also stores, in full, the inputs and outputs of decoder4 and update4 of its one timestep, with the deviation of
each block alone (the reference's f32 output against the restatement of that block in float64 on the same inputs).

Deviation.  A ``.double()`` copy of the reference cannot run (raft.py:199 casts the lookup to float32 and the next
convolution raises), so per quantity the stored deviation is THE REFERENCE'S F32 RESULT AGAINST THE RESTATEMENT
(tests/amt_cpu.py) RUN IN FLOAT64, the largest absolute difference over the whole quantity.  Before that the f32
restatement is shown to reproduce the reference's f32 run: the largest difference is printed and asserted to be at or below
the stored deviation.  The tests' bounds are multiples of these deviations.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import save  # noqa: E402
from tests import amt_cpu as ac  # noqa: E402


def reference_run(mod, m, f0, f1, factor):
    """The reference's forward with its intermediates recorded per timestep -> out, [dict per timestep]."""
    recs, cur = [], {}
    cat = lambda a, b: torch.cat([a, b], 1)      # noqa: E731
    handles = [m.feat_encoder.register_forward_hook(lambda _m, _i, o: cur.update(fmap0=o[0], fmap1=o[1])),
               m.decoder4.register_forward_hook(lambda _m, _i, o: cur.update(flow_dec4=cat(o[0], o[1]))),
               m.decoder3.register_forward_hook(lambda _m, _i, o: cur.update(flow_dec3=cat(o[0], o[1]))),
               m.decoder2.register_forward_hook(lambda _m, _i, o: cur.update(flow_dec2=cat(o[0], o[1]))),
               m.decoder3.register_forward_pre_hook(lambda _m, i: cur.update(flow4=cat(i[3], i[4]))),
               m.decoder2.register_forward_pre_hook(lambda _m, i: cur.update(flow3=cat(i[3], i[4]))),
               m.decoder1.register_forward_pre_hook(lambda _m, i: cur.update(flow2=cat(i[3], i[4]))),
               # one decoder and one update block with their own inputs, for the per-block tests
               m.decoder4.register_forward_hook(lambda _m, i, o: cur.update(blk_f0_4=i[0], blk_f1_4=i[1], blk_dec4=torch.cat(o, 1))),
               m.update4.register_forward_hook(lambda _m, i, o: cur.update(blk_net=i[0], blk_flow=i[1], blk_corr=i[2],
                                                                           blk_dnet=o[0], blk_dflow=o[1]))]
    block, combine = mod.BidirCorrBlock, mod.multi_flow_combine
    names = iter(())

    class Recording(block):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            nonlocal names
            names = iter(("lookup4", "lookup3", "lookup2"))
            cur["corr0"] = self.corr_pyramid[0][:, 0]

        def __call__(self, c0, c1):
            a, b = super().__call__(c0, c1)
            cur[next(names)] = torch.cat([a, b], 1)
            return a, b

    def recording_combine(comb, img0, img1, flow0, flow1, mask, img_res, mean):
        cur.update(flow1=cat(flow0, flow1), mask=mask)
        out = combine(comb, img0, img1, flow0, flow1, mask, img_res, mean)
        recs.append(dict(cur))
        return out
    mod.BidirCorrBlock, mod.multi_flow_combine = Recording, recording_combine
    try:
        out = m(f0.clone(), f1.clone(), factor)
    finally:
        mod.BidirCorrBlock, mod.multi_flow_combine = block, combine
        for h in handles:
            h.remove()
    return out, recs


def g18_amt():
    import refimport
    refimport.install_stubs()
    mod = refimport.ref("amt")
    m = mod.AMT().eval()
    sd = ac.seeded_state_dict(m)
    m.load_state_dict(sd)
    sd64 = {k: v.double() for k, v in sd.items()}
    n_params = sum(p.numel() for p in m.parameters())
    print("parameters:", n_params, "state-dict entries:", len(sd))
    arrays = dict(param_names=np.array(list(sd.keys())), param_shapes=np.array([";".join(map(str, v.shape)) for v in sd.values()]),
                  n_params=np.array(n_params), **{f"scale_{k}": np.array(v) for k, v in ac.SCALES.items()})
    for case, c in ac.CASES.items():
        u8 = ac.input_u8(case)
        f0, f1 = ac.frames(u8)
        out, recs = reference_run(mod, m, f0, f1, c["factor"])
        d32, d64 = [], []
        r32 = ac.amt_forward(sd, f0, f1, c["factor"], d32)
        r64 = ac.amt_forward(sd64, f0.double(), f1.double(), c["factor"], d64)
        ref = dict(recs[0], out=out)
        res32, res64 = dict(d32[0], out=r32), dict(d64[0], out=r64)
        arrays[f"{case}_u8"] = u8
        for q in ac.QUANTITIES:
            a = ref[q] if q != "corr0" else ref[q].reshape(res32[q][:, 0].shape)
            b32 = res32[q] if q != "corr0" else res32[q][:, 0]
            b64 = res64[q] if q != "corr0" else res64[q][:, 0]
            dev = (a.double() - b64).abs().max().item()
            same = (a - b32).abs().max().item()
            print(f"{case} {q}: shape {tuple(a.shape)}, max |ref| {a.abs().max().item():.3e}, f32-vs-f64 deviation {dev:.2e}, "
                  f"f32 restatement vs reference {same:.2e}")
            assert dev > 0 and same <= dev, (case, q, same, dev)
            arrays[f"{case}_{q}"] = ac.stored(case, q, a).numpy()
            arrays[f"{case}_dev_{q}"] = np.array(dev)
        if case == ac.BLOCK_CASE:
            # decoder4 and update4 of the first timestep on the reference's own inputs: outputs and their deviation from the
            # restatement of that block alone in float64 on the same inputs
            r, t0 = recs[0], ac.timesteps(c["factor"])[0]
            d64 = torch.cat(ac.init_decoder(sd64, "decoder4", r["blk_f0_4"].double(), r["blk_f1_4"].double(), t0), 1)
            n64, f64 = ac.update_block(sd64, "update4", r["blk_net"].double(), r["blk_flow"].double(), r["blk_corr"].double())
            for q in ac.BLOCK_INPUTS:
                arrays[f"{case}_{q}"] = r[q].numpy()
            for q, b64 in (("blk_dec4", d64), ("blk_dnet", n64), ("blk_dflow", f64)):
                dev = (r[q].double() - b64).abs().max().item()
                print(f"{case} {q}: shape {tuple(r[q].shape)}, max |ref| {r[q].abs().max().item():.3e}, per-block f32-vs-f64 deviation {dev:.2e}")
                assert dev > 0
                arrays[f"{case}_{q}"] = r[q].numpy()
                arrays[f"{case}_dev_{q}"] = np.array(dev)
        for k, (t, rec, r3) in enumerate(zip(ac.timesteps(c["factor"]).tolist(), recs, d32)):
            fl = rec["flow1"]
            mag = fl.view(fl.shape[0], -1, 2, *fl.shape[2:]).pow(2).sum(2).sqrt().mean().item()
            mask = rec["mask"]
            plain = (1 - t) * f0 + t * f1
            diff = (out[:, k] - plain).abs().max().item()
            print(f"  {case} t={t:.2f}: mean |final flow| {mag:.2f} px, mask min {mask.min().item():.4f} max {mask.max().item():.4f}, "
                  f"max |out - plain blend| {diff:.3f}; lookup corners outside, finest level "
                  + " ".join(f"{v:.3f}" for v in r3["outside0"]) + "; all levels " + " ".join(f"{v:.3f}" for v in r3["outside"])
                  + f" (zero-flow floor {r3['floor']:.3f})")
            assert 1.0 <= mag <= 10.0, mag
            assert mask.min().item() < 0.1 and mask.max().item() > 0.9
            assert diff > 100 * float(arrays[f"{case}_dev_out"]), (diff, arrays[f"{case}_dev_out"])
            assert all(0.05 <= v <= 0.40 for v in r3["outside0"]), r3["outside0"]
    save("g18_amt", **arrays)
    size = os.path.getsize(os.path.join(HERE, "g18_amt.npz"))
    print("g18_amt.npz:", size, "bytes")
    assert size < 1 << 20, size


def main():
    torch.set_num_threads(8)
    torch.set_grad_enabled(False)
    g18_amt()


if __name__ == "__main__":
    main()
