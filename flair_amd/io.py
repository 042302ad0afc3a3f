"""Frame file I/O either side of the sampling path, and the streaming form of the window loop.

Mirror of the reference's ``scripts/video_sample.py:334-345`` (frame discovery with the glob
``*.[jJpP][pPnN][gG]`` in natural order, ``cv2.imread`` -> RGB -> float / 255, stacked to
``(1, N, 3, h, w)``) and ``:487-492`` (``(x * 255).byte()`` -> ``{i:04d}.png``), SURVEY.md section 8f
"next" row 2.  The reference decodes every frame up front, samples window after window, keeps all
results on the host and writes them at the end; here the three stages overlap:

  * a reader thread decodes the frames of window ``w + 1`` (PIL; ``cv2`` is not a dependency) into
    pinned host memory and uploads them on a side HIP stream while window ``w`` is being sampled;
  * finished frames leave the GPU with an asynchronous device-to-host copy and are PNG-encoded by a
    writer thread while the next window samples.

Windows of one video stay sequential (``prev_recon`` couples them); independent videos are the
clip-parallel unit (``flair_amd.parallel``).  Host-side glue only: no arithmetic of the hot path
happens here.

A path that ends in ``.y4m`` is a YUV4MPEG2 stream (flair_amd.y4m) wherever a directory of frame files stands: list_frames
gives one ``Y4MFrame`` per frame, the readers upload the file's payload bytes and turn them into RGB with
flair_yuv_to_rgb_u8 on the side stream, and the writer turns RGB bytes into payloads with flair_rgb_to_yuv_u8.
"""
import os
import queue
import re
import threading

import numpy as np
import torch

from . import video
from . import y4m
from .y4m import Y4MFrame, is_y4m

_FRAME_RE = re.compile(r".*\.[jJpP][pPnN][gG]$")          # the reference's glob: jpg / png / jng / pnG ...


def natural_key(name):
    """natsort's default ordering of the reference (``natsorted(video_path.glob(...))``): digit runs
    compare as integers, the rest as text."""
    return [int(tok) if tok.isdigit() else tok for tok in re.split(r"(\d+)", os.path.basename(str(name)))]


def list_frames(video_path):
    """Frame files of a directory in the reference's order (video_sample.py:334); for a ``.y4m`` path (any case) one
    Y4MFrame per frame of the stream."""
    if is_y4m(video_path):
        return y4m.frames_of(video_path)
    names = [n for n in os.listdir(video_path) if _FRAME_RE.match(n)]
    return [os.path.join(str(video_path), n) for n in sorted(names, key=natural_key)]


def _need_gpu(ref, device):
    if torch.device(device).type != "cuda":
        raise ValueError(f"{ref}: the frames of a .y4m stream become RGB in flair_yuv_to_rgb_u8 on the GPU; there is no CPU colour "
                         f"path (device {device})")


def _y4m_runs(refs):
    """Split a frame list into runs of one kind: (first, n, stream or None), Y4MFrames of one stream or frame files."""
    runs = []
    for i, r in enumerate(refs):
        s = r.stream if isinstance(r, Y4MFrame) else None
        if runs and runs[-1][2] is s:
            runs[-1][1] += 1
        else:
            runs.append([i, 1, s])
    return runs


def _y4m_payloads(refs):
    """The payloads of Y4MFrames of one stream in one pinned (n, payload) uint8 host tensor, one readinto per frame."""
    stream = refs[0].stream
    host = torch.empty((len(refs), stream.payload_bytes), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    rows = host.numpy()
    for k, r in enumerate(refs):
        stream.read_into(r.index, rows[k])
    return host


def _y4m_decode(refs, device, planar):
    """Y4MFrames of one stream -> (n, h, w, 3) or, planar, (n, 3, h, w) uint8 on ``device``, enqueued on the CURRENT stream:
    the upload of the file's bytes and flair_yuv_to_rgb_u8.  -> (device tensor, the pinned host tensor to keep alive)."""
    from . import ops
    stream = refs[0].stream
    host = _y4m_payloads(refs)
    dev = host.to(device, non_blocking=True)
    return ops.yuv_to_rgb_u8(dev, (stream.height, stream.width), stream.format, stream.matrix, stream.range, planar=planar), host


def _upload_group(refs, device, planar):
    """One group of a frame list on the current (side) stream -> (uint8 device tensor, [host tensors to keep alive])."""
    parts, keep = [], []
    for first, n, stream in _y4m_runs(refs):
        run = refs[first:first + n]
        if stream is not None:
            dev, host = _y4m_decode(run, device, planar)
        else:
            host = torch.from_numpy(np.stack([(decode_frame if planar else decode_frame_hwc)(p) for p in run])).pin_memory()
            dev = host.to(device, non_blocking=True)
        parts.append(dev)
        keep.append(host)
    return (parts[0] if len(parts) == 1 else torch.cat(parts)), keep


def decode_frame_hwc(path):
    """One frame file -> dense (h, w, 3) uint8 RGB, the layout of the files and of to_bytes.  A Y4MFrame goes through
    flair_yuv_to_rgb_u8 on the current device and comes back as host bytes: there is no CPU colour path."""
    if isinstance(path, Y4MFrame):
        if not torch.cuda.is_available():
            _need_gpu(path, "cpu")
        dev, _host = _y4m_decode([path], torch.device("cuda", torch.cuda.current_device()), False)
        return np.ascontiguousarray(dev[0].cpu().numpy())
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))


def decode_frame(path):
    """One frame file -> (3, h, w) uint8 RGB (what ``cv2.cvtColor(cv2.imread(p), COLOR_BGR2RGB)`` yields)."""
    return np.ascontiguousarray(decode_frame_hwc(path).transpose(2, 0, 1))


def read_frames(paths, pin=False):
    """Frame files -> (1, N, 3, h, w) float32 in [0, 1] on the host (video_sample.py:337-345)."""
    frames = np.stack([decode_frame(p) for p in paths])
    out = torch.from_numpy(frames).float().div_(255.0).unsqueeze(0)
    return out.pin_memory() if pin and torch.cuda.is_available() else out


def to_bytes(frames01):
    """(N, 3, H, W) float in [0, 1] -> (N, H, W, 3) uint8 exactly as ``(x * 255).byte()`` (truncation,
    video_sample.py:489) followed by the ``t c h w -> t h w c`` rearrange."""
    return (frames01.float() * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def write_frame(path, hwc_u8):
    from PIL import Image
    Image.fromarray(np.asarray(hwc_u8), mode="RGB").save(path, format="PNG")


class _Writer(threading.Thread):
    """Encodes finished frames in the background (PNG compression is host work that would otherwise sit
    between two windows).  An ``output_path`` ending in ``.y4m`` opens a stream instead of a directory: the frames become
    payloads in flair_rgb_to_yuv_u8 and the thread writes ``FRAME\\n`` and the payload in submission order (``first`` is not
    looked at).  ``y4m``: y4m.output_params(...) of the stream to write, None for those of no input stream."""

    def __init__(self, output_path, y4m=None):
        super().__init__(daemon=True)
        self.q = queue.Queue()
        self.output_path = str(output_path)
        self.error = None
        self.file = self.params = self.size = None
        if is_y4m(self.output_path):
            from . import y4m as _y4m
            self.params = dict(_y4m.output_params() if y4m is None else y4m)
            os.makedirs(os.path.dirname(os.path.abspath(self.output_path)), exist_ok=True)
            self.file = open(self.output_path, "wb")
        else:
            os.makedirs(self.output_path, exist_ok=True)
        self.start()

    def run(self):
        while True:
            item = self.q.get()
            if item is None:
                return
            first, host, event = item
            try:
                if event is not None:
                    event.synchronize()                    # the asynchronous D2H copy has landed
                if self.file is not None:
                    if first is None:                      # the stream's header line
                        self.file.write(host)
                    else:
                        for payload in host.numpy():
                            self.file.write(y4m.FRAME)
                            self.file.write(payload.data)
                    continue
                for i, frame in enumerate(host.numpy()):
                    write_frame(os.path.join(self.output_path, f"{first + i:04d}.png"), frame)
            except Exception as exc:                       # surfaced by close()
                self.error = exc

    def submit(self, first, frames01_dev):
        """frames01_dev: (n, 3, H, W) float on the GPU (or host)."""
        self.submit_bytes(first, to_bytes(frames01_dev))

    def submit_bytes(self, first, u8):
        """u8: (n, H, W, 3) uint8 on the GPU (or host), written as they are."""
        if self.file is not None:
            return self._submit_stream(u8)
        if u8.is_cuda:
            host = torch.empty(u8.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(u8, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.q.put((first, host, ev))
        else:
            self.q.put((first, u8, None))

    def _submit_stream(self, u8):
        """The frames as payloads of the stream: flair_rgb_to_yuv_u8 on the current stream (a host tensor is uploaded first),
        an asynchronous copy to pinned memory, and the bytes to the writer thread.  The header goes first, once."""
        from . import ops
        if u8.dim() != 4 or u8.shape[3] != 3 or u8.dtype != torch.uint8:
            raise ValueError(f"{self.output_path}: frames are (n, H, W, 3) uint8, got {tuple(u8.shape)} {u8.dtype}")
        if not u8.is_cuda:
            if not torch.cuda.is_available():
                raise ValueError(f"{self.output_path}: the frames of a .y4m stream are made in flair_rgb_to_yuv_u8 on the GPU; there is "
                                 "no CPU colour path")
            u8 = u8.pin_memory().to(torch.device("cuda", torch.cuda.current_device()), non_blocking=True)
        p, size = self.params, tuple(u8.shape[1:3])
        if self.size is None:
            self.size = size
            self.q.put((None, y4m.header_line(size[1], size[0], p["fps"], p["format"], p["range"], p["aspect"], p["extra"]), None))
        elif size != self.size:
            raise ValueError(f"{self.output_path}: frames of {size[0]}x{size[1]} in a stream of {self.size[0]}x{self.size[1]}")
        payload = ops.rgb_to_yuv_u8(u8.contiguous(), p["format"], p["matrix"], p["range"])
        host = torch.empty(payload.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(payload, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.q.put((0, host, ev))

    def close(self):
        self.q.put(None)
        self.join()
        if self.file is not None:
            self.file.close()
        if self.error is not None:
            raise self.error


def iter_windows(paths, device, length=video.FRAME_SLICE_LEN, overlap=video.OVERLAP, cuts=None):
    """Yield ``(indices, degraded01)`` per window with ``degraded01`` = (1, T, 3, h, w) float in [0, 1] on
    ``device``: the frames of the NEXT window are decoded and uploaded (pinned memory, side stream) while the
    caller works on the current one.  Frames shared by two windows are decoded once.  ``cuts``: the windows of
    video.window_plan (no window spans a cut) instead of video.window_indices."""
    wins = [idx for idx, _ in video.window_plan(len(paths), cuts, length, overlap)]
    cache, q = {}, queue.Queue(maxsize=2)
    on_gpu = torch.device(device).type == "cuda"
    side = torch.cuda.Stream(device=device) if on_gpu else None
    streamed = any(isinstance(p, Y4MFrame) for p in paths)
    if streamed:
        _need_gpu(next(p for p in paths if isinstance(p, Y4MFrame)), device)

    def produce():
        try:
            for w, idx in enumerate(wins):
                if streamed:                                   # the file's bytes go up as they are; a window re-reads its overlap
                    with torch.cuda.stream(side):
                        dev_u8, keep = _upload_group([paths[i] for i in idx], device, True)
                        ev = torch.cuda.Event()
                        ev.record(side)
                    q.put((idx, dev_u8, ev, keep))
                    continue
                for i in idx:
                    if i not in cache:
                        cache[i] = decode_frame(paths[i])
                host = torch.from_numpy(np.stack([cache[i] for i in idx]))
                ahead = set(wins[w + 1]) if w + 1 < len(wins) else ()
                for i in [k for k in cache if k not in ahead]:          # only the next window's frames are needed again
                    del cache[i]
                if on_gpu:
                    host = host.pin_memory()
                    with torch.cuda.stream(side):
                        dev_u8 = host.to(device, non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(side)
                    q.put((idx, dev_u8, ev, host))
                else:
                    q.put((idx, host, None, host))
            q.put(None)
        except Exception as exc:
            q.put(exc)

    threading.Thread(target=produce, daemon=True).start()
    while True:
        item = q.get()
        if item is None:
            return
        if isinstance(item, Exception):
            raise item
        idx, u8, ev, _keep = item
        if ev is not None:
            cur = torch.cuda.current_stream(device)
            cur.wait_event(ev)
            u8.record_stream(cur)        # allocated on the side stream, read here: keep the block until this read is done
        yield idx, (u8.float() / 255.0).unsqueeze(0)


def iter_frame_batches(path_lists, groups, device):
    """Yield ``(first, [u8, ...])`` per group ``(first, n)`` of ``groups``: ``u8[k]`` = (n, h, w, 3) uint8 on ``device``,
    frames ``first .. first + n - 1`` of ``path_lists[k]`` (the frames of one group share one size per list).  As in
    iter_windows the NEXT group is decoded into pinned memory and uploaded on a side stream while the caller works on the
    current one."""
    q = queue.Queue(maxsize=2)
    on_gpu = torch.device(device).type == "cuda"
    side = torch.cuda.Stream(device=device) if on_gpu else None
    streamed = [any(isinstance(p, Y4MFrame) for p in paths) for paths in path_lists]
    for paths, has in zip(path_lists, streamed):
        if has:
            _need_gpu(next(p for p in paths if isinstance(p, Y4MFrame)), device)

    def produce():
        try:
            for first, n in groups:
                if any(streamed):                              # lists one by one: a stream's payloads through the kernel, files through PIL
                    with torch.cuda.stream(side):
                        got = [_upload_group(paths[first:first + n], device, False) for paths in path_lists]
                        ev = torch.cuda.Event()
                        ev.record(side)
                    q.put((first, [d for d, _ in got], ev, [k for _, k in got]))
                    continue
                hosts = [torch.from_numpy(np.stack([decode_frame_hwc(p) for p in paths[first:first + n]]))
                         for paths in path_lists]
                if on_gpu:
                    hosts = [h.pin_memory() for h in hosts]
                    with torch.cuda.stream(side):
                        devs = [h.to(device, non_blocking=True) for h in hosts]
                        ev = torch.cuda.Event()
                        ev.record(side)
                    q.put((first, devs, ev, hosts))
                else:
                    q.put((first, hosts, None, hosts))
            q.put(None)
        except Exception as exc:
            q.put(exc)

    threading.Thread(target=produce, daemon=True).start()
    while True:
        item = q.get()
        if item is None:
            return
        if isinstance(item, Exception):
            raise item
        first, devs, ev, _keep = item
        if ev is not None:
            cur = torch.cuda.current_stream(device)
            cur.wait_event(ev)
            for d in devs:
                d.record_stream(cur)     # allocated on the side stream, read here
        yield first, devs


def frame_size(path):
    """(h, w) of a frame file; only its header is read.  A Y4MFrame answers from its stream's header."""
    if isinstance(path, Y4MFrame):
        return path.stream.height, path.stream.width
    from PIL import Image
    with Image.open(path) as im:
        w, h = im.size
    return h, w


def restore_video_files(task, video_path, output_path, model, diffusion, restore_fn_for, *, size, device,
                        length=video.FRAME_SLICE_LEN, overlap=video.OVERLAP, aligned=True, face_helper=None, cuts=None, **kw):
    """``scripts/video_sample.py:334-492`` end to end: frame files in, restored ``{i:04d}.png`` out, with
    decode / upload / sampling / download / encode overlapped.  ``kw`` goes to ``video.restore_window``
    (aux_model, vsrpp_weights_fn, hp, tau, t_start, noise_fn, q_noise_fn, faces, max_faces, and tile / tile_overlap: tiled
    denoising of frames the network cannot take whole, flair_amd.tiling).  ``aligned=False`` detects every window's
    faces on the main thread before its first step (video.window_faces) while the reader thread decodes the next
    window.  ``cuts`` (None = one shot): frames that start a new shot; every shot is windowed on its own and its first
    window gets no ``prev_recon`` (video.window_plan).  Returns the number of frames written."""
    paths = list_frames(video_path)
    plan = video.window_plan(len(paths), cuts, length, overlap)            # refuses bad cuts before anything is decoded
    writer = _Writer(output_path, y4m=y4m.output_params(y4m.stream_of(paths)))
    prev_recon, written = None, 0
    try:
        for wi, (idx, degraded01) in enumerate(iter_windows(paths, device, length, overlap, cuts=cuts)):
            if plan[wi][1]:
                prev_recon = None
            keep, prev_recon = video.restore_window(task, degraded01, model, diffusion, restore_fn_for, size=size,
                                                    prev_recon=prev_recon, overlap=overlap, window_index=wi, aligned=aligned,
                                                    face_helper=face_helper, frame_indices=idx, **kw)
            writer.submit(written, keep)
            written += keep.shape[0]
    finally:
        writer.close()
    return written
