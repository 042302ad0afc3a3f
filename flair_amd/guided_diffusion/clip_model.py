"""What the two video UNets (``unet_new.UNetModel``, ``sr3.UNet``) share on the host side: a forward over B clips is
one ``_forward_clip`` per clip, replayed from one captured hipGraph per clip when ``enable_hip_graph()`` is on, with the
clip's optical flows computed once and cached across the denoising steps ("Weight packing").

A model supplies ``_forward_clip(x, t, low_res, flows, enable_cross_frames, vsrpp_weights)`` and two hooks:
``_flow_spec(H, W, enable_cross_frames)``, the hashable description of which flows an H x W clip needs (falsy: none), and
``_compute_flows(rnn_clip, spec)``, which returns them as ``{level width: (forward, backward)}``.
"""
import torch

from .packing import PackedModel


class ClipModel(PackedModel):
    """Mixin in front of ``nn.Module`` (in place of ``PackedModel``).  ``_name`` is the class as messages spell it."""

    _name = "flair_amd.ClipModel"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._flow_cache = {}
        self._flow_cache_limit = 16   # entries before the cache clears itself; flair_amd.tiling raises it to its tiles for the length of a call
        self._graphs = {}
        self._graph_clip_limit = None   # clips of a batch replayed from graphs, the rest launched eagerly (None: all; flair_amd.tiling)
        self.use_hip_graph = False
        self._flow_gen = 0         # the sampler's chain counter (reset_flow_cache)
        self._trace = None         # tests: a list here receives per-stage activations (and turns graphs off)

    def enable_hip_graph(self, flag=True):
        """Replay one captured hipGraph per (clip shape, dtype, weight-map kind, clip index) instead of thousands of
        launches per forward.  Inputs are copied into static buffers; the returned tensor is overwritten by the next
        call (the sampler consumes it immediately)."""
        self.use_hip_graph = bool(flag)
        self._graphs = {}
        return self

    # the reference's name; bfloat16 is the reduced precision here (f32 accumulate; GroupNorm statistics, embeddings,
    # flows and SPyNet stay f32)
    convert_to_fp16 = PackedModel.convert_to_bf16

    def invalidate_packed(self):
        super().invalidate_packed()
        self._graphs, self._flow_cache = {}, {}      # captured launches and cached flows were made with the old copies

    def reset_flow_cache(self):
        """Forget cached SPyNet flows (the sampler calls this at the start of every chain: flows are a function of the
        conditioning clip, which only changes between chains)."""
        self._flow_cache = {}
        self._flow_gen += 1

    # ---- flows: once per (clip, spec) ---------------------------------------------------
    def _flows_cached(self, rnn_clip, spec):
        """rnn_clip: (T,3,h,w) f32 device tensor.  Flows are a pure function of the clip, so they are cached across the
        denoising steps, keyed on storage + version + shape + spec."""
        key = (rnn_clip.data_ptr(), rnn_clip._version, tuple(rnn_clip.shape), spec)
        hit = self._flow_cache.get(key)
        if hit is None:
            flows = self._compute_flows(rnn_clip, spec)
            flows["_prop"] = {}              # per-clip store of composed second-order flows (BasicVSRPP._propagate)
            if len(self._flow_cache) >= self._flow_cache_limit:
                self._flow_cache.clear()
            hit = (flows, rnn_clip)          # keep the keyed storage alive
            self._flow_cache[key] = hit
        return hit[0]

    def _clip_flows(self, rnn_clip, x, enable_cross_frames):
        spec = self._flow_spec(x.shape[-2], x.shape[-1], enable_cross_frames)
        return self._flows_cached(rnn_clip, spec) if spec else {}

    # ---- forward ------------------------------------------------------------------------
    def _run_clips(self, x, timesteps, low_res_input, rnn_input, num_frames, enable_cross_frames, vsrpp_weights):
        """x: (B*T, C, H, W) on the GPU; timesteps: (B*T,); low_res_input / rnn_input: (B, T, 3, H, W); vsrpp_weights: a
        number, None or a (B, T, 1, h, w) map.  Returns (B*T, out channels, H, W) f32."""
        if not x.is_cuda:
            raise RuntimeError(f"{self._name} runs on the MI355X only (tensors must be on 'cuda'); "
                               "there is no CPU path")
        self._ensure_packed(x.device)
        T = int(num_frames)
        B = x.shape[0] // T
        if rnn_input is None:
            rnn_input = low_res_input
        graphed = self.use_hip_graph and self._trace is None
        outs = []
        for b in range(B):
            xb, tb = (v[b * T:(b + 1) * T].float().contiguous() for v in (x, timesteps))
            lr, rnn = (v[b].float().contiguous() for v in (low_res_input, rnn_input))
            vw = vsrpp_weights[b] if isinstance(vsrpp_weights, torch.Tensor) else vsrpp_weights
            if graphed and (self._graph_clip_limit is None or b < self._graph_clip_limit):
                outs.append(self._forward_clip_graphed(xb, tb, lr, rnn, enable_cross_frames, vw, b))
            else:
                outs.append(self._forward_clip(xb, tb, lr, self._clip_flows(rnn, xb, enable_cross_frames),
                                               enable_cross_frames, vw))
        return outs[0] if B == 1 else torch.cat(outs, dim=0)

    def _forward_clip_graphed(self, x, t, low_res, rnn, enable_cross_frames, vsrpp_weights, clip):
        vw_t = vsrpp_weights if isinstance(vsrpp_weights, torch.Tensor) else None
        # one graph per clip of the batch: clips differ in their conditioning (rnn / low_res storage), so sharing one
        # entry would evict and re-capture it on every forward of every sampler step.  A per-pixel weight map is a
        # static input of the graph: it enters the key by shape only.
        key = (tuple(x.shape), self.dtype, bool(enable_cross_frames),
               tuple(vw_t.shape) if vw_t is not None else vsrpp_weights, x.device, clip)
        # conditioning identity: storage + torch version + the sampler's chain counter (kernels launched
        # through ctypes do not bump _version, so every new chain refreshes conditioning and flows once)
        src = (rnn.data_ptr(), rnn._version, low_res.data_ptr(), low_res._version, self._flow_gen,
               (vw_t.data_ptr(), vw_t._version) if vw_t is not None else None)
        ent = self._graphs.get(key)
        if ent is not None and ent["src"] != src:
            # a new clip / chain: the captured launches read this clip's flows AND the second-order flows composed
            # from them (BasicVSRPP._propagate's per-clip store): re-capture (one eager forward, once per chain)
            del self._graphs[key]
            ent = None
        if ent is None:
            st = dict(x=x.clone(), t=t.clone(), lr=low_res.clone(), rnn=rnn.clone(),
                      vw=vw_t.clone() if vw_t is not None else vsrpp_weights)
            flows = self._clip_flows(st["rnn"], x, enable_cross_frames)      # SPyNet runs eagerly, before capture
            args = (st["x"], st["t"], st["lr"], flows, enable_cross_frames, st["vw"])
            cur = torch.cuda.current_stream()
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):                    # warm-up (allocator, workspaces)
                self._forward_clip(*args)
            cur.wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            # thread_local: HIP calls of OTHER host threads (flair_amd.io's reader pins memory / uploads the next
            # window, its writer waits on events) must not invalidate this thread's capture
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                out = self._forward_clip(*args)
            ent = dict(graph=graph, st=st, out=out, src=src, flows=flows)
            self._graphs[key] = ent
        ent["st"]["x"].copy_(x)
        ent["st"]["t"].copy_(t)
        ent["graph"].replay()
        return ent["out"]
