"""Tiled denoising: frames larger than the network can take whole (or of a size it does not accept) are restored by running the
network on overlapping tiles of one valid size at every sampler step and blending the tile outputs into one whole-frame model
output.  Ours: the reference restores 512 x 512 frames only.

Tiling happens at the model call and nowhere else.  ``TiledModel`` wraps a ``ClipModel``; ``GaussianDiffusion.p_sample`` calls it
like the network and goes on with whole frames: x0, clipping, the data-consistency step, the face prior on detected faces,
``prev_recon`` pinning and the noise all see the frame, never a tile.

* ``plan_axis`` / ``make_plan``: the tile origins.  No padding: the last origin is clamped to the frame, so every tile lies inside it.
* ``ops.tile_gather`` / ``ops.tile_blend`` (csrc/tile.hip, include/flair_tile.h): the two HIP kernels, the weights' definition.
* ``TiledModel``: gather x and the conditioning, one call of the inner model with the tiles as a batch of clips, blend.

Limitations: a face cut by a seam gets the bicubic tasks' propagation weights from per-tile parses (the parser never sees the
whole frame); frames smaller than one tile are refused, not padded; tiles are not spread over several GPUs.
"""
import warnings

import torch

from . import ops

# restore --tile auto: a heuristic (the networks were trained at 512 x 512; 64 pixels is one cell of the deepest level), NOT
# validated on real footage
DEFAULT_TILE = (512, 512)
DEFAULT_OVERLAP = 64
# The most tile clips replayed from captured hipGraphs; the clips after them are launched eagerly.  Measured, not estimated: the
# 15 graphs of 1080 x 1920 (3 x 5 tiles of 512 x 512, 10 frames, bf16) reserve 113 GiB where eager launches reserve 18 GiB, and
# fit; no larger plan has been run, and graphs bought no time at this tile size ("Tiled denoising").
MAX_GRAPHED_TILES = 15


def plan_axis(L, t, min_overlap, g):
    """Tile origins along one axis of length ``L`` for tiles of side ``t`` whose neighbours share at least ``min_overlap``
    pixels, every origin a multiple of ``g``: ``[0]`` for L == t, else n = max(2, ceil((L - min_overlap) / (t - min_overlap)))
    tiles at o_i = floor(i (L - t) / (n - 1) / g) g, the last one exactly L - t.  L, t and min_overlap must be multiples of g
    (then flooring an origin to the grid never opens a gap or shrinks an overlap below min_overlap)."""
    L, t, min_overlap, g = int(L), int(t), int(min_overlap), int(g)
    if g < 1 or t < 1 or L < t:
        raise ValueError(f"plan_axis: tiles of {t} pixels on an axis of {L} (grid {g}): need 1 <= t <= L and g >= 1")
    if L % g or t % g:
        raise ValueError(f"plan_axis: the axis length {L} and the tile side {t} must be multiples of {g}")
    if L == t:
        return [0]
    if not 0 <= min_overlap < t or min_overlap % g:
        raise ValueError(f"plan_axis: overlap {min_overlap} must be a multiple of {g}, at least 0 and below the tile side {t}")
    n = max(2, -(-(L - min_overlap) // (t - min_overlap)))
    return [(i * (L - t)) // ((n - 1) * g) * g for i in range(n)]


def tile_side(L, requested, m):
    """The tile side used on an axis of length ``L``: the requested one, clipped to the largest multiple of ``m`` the axis holds."""
    return min(int(requested), int(L) // int(m) * int(m))


class TilePlan:
    """A tensor product of tile rows and tile columns: tile k = r * cols + c (row-major, "plan order") starts at (oy[r], ox[c])."""

    def __init__(self, frame_hw, tile_hw, overlap, g):
        (self.H, self.W), (self.th, self.tw) = (int(v) for v in frame_hw), (int(v) for v in tile_hw)
        self.overlap, self.g = int(overlap), int(g)
        if self.overlap < 1:
            raise ValueError(f"tile overlap {overlap}: at least 1 pixel (it is the blend's ramp)")
        self.oy = plan_axis(self.H, self.th, self.overlap, self.g)
        self.ox = plan_axis(self.W, self.tw, self.overlap, self.g)

    rows = property(lambda self: len(self.oy))
    cols = property(lambda self: len(self.ox))
    n_tiles = property(lambda self: len(self.oy) * len(self.ox))

    def origins(self):
        """[(oy, ox)] in plan order."""
        return [(a, b) for a in self.oy for b in self.ox]

    def pixels_ratio(self):
        """Pixels the network sees per frame pixel (what tiling costs)."""
        return self.n_tiles * self.th * self.tw / (self.H * self.W)

    def __repr__(self):
        return f"TilePlan({self.H}x{self.W}: {self.rows}x{self.cols} tiles of {self.th}x{self.tw}, overlap {self.overlap}, rows {self.oy}, columns {self.ox})"


def make_plan(frame_hw, tile_hw, overlap=DEFAULT_OVERLAP, g=1):
    return TilePlan(frame_hw, tile_hw, overlap, g)


class TiledModel:
    """``model`` (a ClipModel: unet_new.UNetModel or sr3.UNet) on the tiles of ``plan``.  The inner model stays reachable as
    ``.model`` (the sampler's ``getattr(model, "model", model)`` finds its ``reset_flow_cache`` there); ``dtype``, ``modules``,
    ``parameters``, ``enable_hip_graph`` and ``takes_noise_level`` are the inner model's.

    One call gathers x and -- once per conditioning clip, not once per step -- ``low_res_input`` and ``rnn_input`` into tiles
    (ops.tile_gather), calls the inner model ONCE with the tiles as a batch of n_tiles clips, so that its per-clip hipGraph key
    carries the tile index and nothing is captured again from step to step, and blends the outputs (ops.tile_blend).
    ``vsrpp_weights_fn`` (the bicubic tasks' per-pixel propagation weights): applied to every tile's init frames; without it a
    number or None is passed on as it is and a (B, T, 1, h, w) map is cut into the tiles' crops on its own grid.
    ``graph_tiles``: with hipGraphs on, the first so many tile clips replay captured graphs and the others are launched eagerly
    (MAX_GRAPHED_TILES; one warning when a plan has more)."""

    def __init__(self, model, plan, vsrpp_weights_fn=None, graph_tiles=MAX_GRAPHED_TILES):
        self.model, self.plan, self.vsrpp_weights_fn = model, plan, vsrpp_weights_fn
        self.graph_tiles, self._said = int(graph_tiles), False
        self._cond = None                 # (key, sources kept alive, low_res tiles, rnn tiles, weight maps)

    # ---- what the sampler and the window loop read off a model ----------------------------
    @property
    def dtype(self):
        return self.model.dtype

    @property
    def takes_noise_level(self):
        return getattr(self.model, "takes_noise_level", False)

    def modules(self):
        return self.model.modules()

    def parameters(self):
        return self.model.parameters()

    def enable_hip_graph(self, flag=True):
        self.model.enable_hip_graph(flag)
        return self

    # ---- tiles ------------------------------------------------------------------------------
    def _gather(self, frames, scale=1):
        """(N, C, H/scale, W/scale) -> (n_tiles * N, C, th/scale, tw/scale), the tile index major."""
        p = self.plan
        return ops.tile_gather(frames.float().contiguous(), [o // scale for o in p.oy], [o // scale for o in p.ox],
                               (p.th // scale, p.tw // scale))

    def _clips(self, clips):
        """(B, T, C, H, W) -> (n_tiles * B, T, C, th, tw): the B clips of tile 0, then those of tile 1, ..."""
        B, T = clips.shape[:2]
        tiles = self._gather(clips.reshape(B * T, *clips.shape[2:]))
        return tiles.reshape(self.plan.n_tiles * B, T, *tiles.shape[1:])

    def _weight_maps(self, vw, lr_tiles):
        if self.vsrpp_weights_fn is not None:
            return torch.cat([self.vsrpp_weights_fn(lr_tiles[k:k + 1]) for k in range(lr_tiles.shape[0])], 0)
        if not isinstance(vw, torch.Tensor):
            return vw
        p = self.plan
        B, T, _, h, w = vw.shape
        s = p.H // h if h and p.H % h == 0 else 0
        if not s or (h * s, w * s) != (p.H, p.W) or any(v % s for v in (p.th, p.tw, *p.oy, *p.ox)):
            raise ValueError(f"vsrpp_weights of {h}x{w} for frames of {p.H}x{p.W}: the map's grid must divide the frame, the tile "
                             f"size {p.th}x{p.tw} and every tile origin")
        tiles = self._gather(vw.reshape(B * T, 1, h, w), s)
        return tiles.reshape(p.n_tiles * B, T, 1, *tiles.shape[-2:])

    def _conditioning(self, low_res_input, rnn_input, vsrpp_weights):
        ident = lambda v: None if not isinstance(v, torch.Tensor) else (v.data_ptr(), v._version, tuple(v.shape))   # noqa: E731
        key = (ident(low_res_input), ident(rnn_input), ident(vsrpp_weights) if isinstance(vsrpp_weights, torch.Tensor) else vsrpp_weights,
               getattr(self.model, "_flow_gen", None))
        if self._cond is None or self._cond[0] != key:
            lr = self._clips(low_res_input)
            rnn = self._clips(rnn_input) if rnn_input is not None else None
            self._cond = (key, (low_res_input, rnn_input, vsrpp_weights), lr, rnn, self._weight_maps(vsrpp_weights, lr))
        return self._cond[2:]

    def __call__(self, x, timesteps, low_res_input=None, rnn_input=None, num_frames=None, enable_cross_frames=True,
                 vsrpp_weights=None, **kwargs):
        p = self.plan
        if tuple(x.shape[-2:]) != (p.H, p.W):
            raise ValueError(f"TiledModel: frames of {tuple(x.shape[-2:])}, planned for {p.H}x{p.W}")
        if low_res_input is None or num_frames is None:
            raise ValueError("TiledModel: low_res_input and num_frames are required")
        lr, rnn, vw = self._conditioning(low_res_input, rnn_input, vsrpp_weights)
        n_clips = lr.shape[0]
        tiles = self._gather(x)
        # every tile's flows stay cached for the chain: the cache's bound holds the tiles of this call, and is the inner model's
        # own again afterwards (a cache above its bound is only cleared by the next insertion, which a later chain makes)
        bound = getattr(self.model, "_flow_cache_limit", None)
        if bound is not None:
            self.model._flow_cache_limit = max(bound, n_clips)
        graphs = hasattr(self.model, "_graph_clip_limit")
        if graphs:
            self.model._graph_clip_limit = self.graph_tiles
            if n_clips > self.graph_tiles and getattr(self.model, "use_hip_graph", False) and not self._said:
                self._said = True
                warnings.warn(f"tiled denoising: {n_clips} tile clips; the first {self.graph_tiles} replay captured hipGraphs (the most "
                              "measured to fit: about 6.4 GiB of reserved memory each at 512x512 tiles of 10 frames), the others are "
                              "launched eagerly", stacklevel=2)
        try:
            out = self.model(tiles, timesteps.repeat(p.n_tiles), low_res_input=lr, rnn_input=rnn, num_frames=num_frames,
                             enable_cross_frames=enable_cross_frames, vsrpp_weights=vw, **kwargs)
        finally:
            if bound is not None:
                self.model._flow_cache_limit = bound
            if graphs:
                self.model._graph_clip_limit = None
        return ops.tile_blend(out.float().contiguous(), p.oy, p.ox, (p.H, p.W), p.overlap)
