"""The host machinery the two video UNets share (flair_amd/guided_diffusion/clip_model.py), on the CPU: the flow cache's
key and eviction, what invalidation drops, the CPU refusal, and the batched-linear accumulator of packing.py."""
import pytest
import torch
import torch.nn as nn

from flair_amd.guided_diffusion.clip_model import ClipModel
from flair_amd.guided_diffusion.packing import LinearStack


class Stub(ClipModel, nn.Module):
    """Counts the misses of the flow cache."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def _compute_flows(self, rnn_clip, spec):
        self.calls.append((tuple(rnn_clip.shape), spec))
        return {spec: len(self.calls)}


def test_constructor_sets_the_clip_state():
    m = Stub()
    assert (m._flow_cache, m._graphs, m.use_hip_graph, m._flow_gen, m._trace) == ({}, {}, False, 0, None)
    assert m._packed_key is None and m.dtype == torch.float32


def test_flow_cache_hits_on_same_storage_version_and_spec():
    m = Stub()
    clip = torch.zeros(3, 3, 8, 8)
    first = m._flows_cached(clip, (8, 8))
    first["_prop"]["composed"] = 1
    again = m._flows_cached(clip, (8, 8))
    assert again is first and again["_prop"] == {"composed": 1} and len(m.calls) == 1


def test_flow_cache_misses_on_version_spec_and_shape():
    m = Stub()
    clip = torch.zeros(3, 3, 8, 8)
    first = m._flows_cached(clip, (8, 8))
    clip.add_(1.0)                                        # same storage, new version
    bumped = m._flows_cached(clip, (8, 8))
    assert bumped is not first and len(m.calls) == 2
    other_spec = m._flows_cached(clip, (4, 4))
    assert other_spec is not bumped and len(m.calls) == 3
    reshaped = m._flows_cached(clip.view(3, 3, 4, 16), (8, 8))       # same storage and version, another shape
    assert reshaped is not bumped and len(m.calls) == 4
    assert m._flows_cached(clip, (8, 8)) is bumped and len(m.calls) == 4
    assert all(f["_prop"] == {} for f in (first, bumped, other_spec, reshaped))


def test_flow_cache_clears_at_sixteen_entries():
    m = Stub()
    clips = [torch.zeros(2, 3, 4, 4) for _ in range(17)]
    sizes = []
    for c in clips:
        m._flows_cached(c, (4, 4))
        sizes.append(len(m._flow_cache))
    assert sizes == list(range(1, 17)) + [1] and max(sizes) <= 16
    assert all(kept is c for (_, kept), c in zip(m._flow_cache.values(), clips[16:]))   # the keyed storage is kept alive
    m._flows_cached(clips[0], (4, 4))                     # evicted with the rest: a miss again
    assert len(m.calls) == 18


def test_reset_flow_cache_empties_it_and_advances_the_chain_counter():
    m = Stub()
    m._flows_cached(torch.zeros(2, 3, 4, 4), (4, 4))
    gen = m._flow_gen
    m.reset_flow_cache()
    assert m._flow_cache == {} and m._flow_gen == gen + 1


def test_invalidation_drops_graphs_flows_and_the_packed_key():
    m = Stub()
    m._flows_cached(torch.zeros(2, 3, 4, 4), (4, 4))
    m._graphs["key"] = dict(graph=None)
    m._packed_key = (torch.float32, "cpu")
    m.invalidate_packed()
    assert m._flow_cache == {} and m._graphs == {} and m._packed_key is None
    m._graphs["key"] = dict(graph=None)
    assert m.enable_hip_graph(False) is m and m._graphs == {} and m.use_hip_graph is False
    m._graphs["key"] = dict(graph=None)
    m.enable_hip_graph()
    assert m._graphs == {} and m.use_hip_graph is True
    m._graphs["key"] = dict(graph=None)
    m.convert_to_fp16()                                   # the reference's name for the reduced precision
    assert m.dtype == torch.bfloat16 and m._graphs == {}


def _real_models():
    from flair_amd.guided_diffusion.sr3 import UNet
    from flair_amd.guided_diffusion.unet_new import UNetModel
    from tests.test_gpu_sr3 import SR3_SMALL
    from tests.test_gpu_unet import SMALL
    return {"unet_new": (lambda: UNetModel(**SMALL), 32, "flair_amd.UNetModel runs on the MI355X only (tensors must be "
                                                         "on 'cuda'); there is no CPU path"),
            "sr3": (lambda: UNet(**SR3_SMALL), 64, "flair_amd.sr3.UNet runs on the MI355X only (tensors must be on "
                                                   "'cuda'); there is no CPU path")}


@pytest.mark.parametrize("family", ["unet_new", "sr3"])
def test_run_clips_refuses_cpu_tensors(family):
    import re
    build, S, message = _real_models()[family]
    m = build()
    assert isinstance(m, ClipModel) and m._flow_gen == 0 and m._trace is None
    with pytest.raises(RuntimeError, match=re.escape(message)):
        m._run_clips(torch.zeros(2, 3, S, S), torch.zeros(2), torch.zeros(1, 2, 3, S, S), None, 2, True, 1.0)
    with pytest.raises(RuntimeError, match=re.escape(message)):     # and through each model's own argument order
        m(torch.zeros(2, 3, S, S), torch.zeros(2), low_res_input=torch.zeros(1, 2, 3, S, S), num_frames=2)
    assert m._packed_key is None                                      # refused before anything was packed


def test_linear_stack_offsets_and_concatenation():
    torch.manual_seed(0)
    lins = [nn.Linear(4, w) for w in (3, 5, 2)]
    stack = LinearStack()
    assert [stack.add(lin) for lin in lins] == [0, 3, 8]
    W, b = stack.cat("cpu")
    assert torch.equal(W, torch.cat([lin.weight for lin in lins])) and W.shape == (10, 4) and W.is_contiguous()
    assert torch.equal(b, torch.cat([lin.bias for lin in lins])) and b.shape == (10,)
    assert not W.requires_grad and not b.requires_grad
