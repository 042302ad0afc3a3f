"""YUV4MPEG2 (.y4m) streams: the uncompressed video interchange format every encoder reads and writes
(``ffmpeg -i clip.mp4 clip.y4m``; ``ffmpeg -i out.y4m out.mp4``).

A text header line ``YUV4MPEG2 W.. H.. F n:d I. A n:d C.. X..`` and then, per frame, the six bytes ``FRAME\\n`` and a dense
payload Y | U | V of a fixed size, so a file is randomly accessible.  This module is the host side only: the header, the
frame offsets, one ``readinto`` per frame, and the header a writer starts a file with.  The colour conversion and the chroma
resampling are the two kernels of include/flair_yuv.h (ops.yuv_to_rgb_u8, ops.rgb_to_yuv_u8); there is no CPU colour path.
flair_amd.io turns a ``.y4m`` path into one ``Y4MFrame`` per frame, which stands wherever a frame file's path stands.

A header says which chroma format a stream has and, with ``XCOLORRANGE``, which range; it does not say which matrix.  What it
leaves open comes from process-wide defaults (``set_defaults``: bt601, limited), and what a written stream takes from no
input stream from ``set_output`` (the command line's --y4m-chroma and --fps).
"""
import os
import threading

MAGIC = b"YUV4MPEG2"
FRAME = b"FRAME\n"
FORMATS = ("420jpeg", "420mpeg2", "422", "444", "mono")
MATRICES = ("bt601", "bt709")
RANGES = ("limited", "full")
DEFAULT_FPS = (25, 1)

_defaults = {"matrix": "bt601", "range": "limited"}
_output = {"chroma": None, "fps": None}


def set_defaults(matrix=None, range=None):          # noqa: A002  (the header's word)
    """The matrix and range of every stream whose header says nothing (process-wide; None leaves a value as it is)."""
    if matrix is not None:
        if matrix not in MATRICES:
            raise ValueError(f"y4m: matrix {matrix!r}, one of {', '.join(MATRICES)}")
        _defaults["matrix"] = matrix
    if range is not None:
        if range not in RANGES:
            raise ValueError(f"y4m: range {range!r}, one of {', '.join(RANGES)}")
        _defaults["range"] = range


def defaults():
    return dict(_defaults)


def set_output(chroma=None, fps=None):
    """What written streams take instead of their input stream's chroma format and rate (process-wide; None: the input's,
    else 420jpeg and 25:1).  fps: (n, d) or the text N[:D]."""
    if chroma is not None and chroma not in FORMATS:
        raise ValueError(f"y4m: chroma format {chroma!r}, one of {', '.join(FORMATS)}")
    _output["chroma"] = chroma
    _output["fps"] = None if fps is None else parse_fps(fps)


def parse_fps(text, what="y4m"):
    """'30', '30000:1001' or a pair -> (n, d), both positive."""
    try:
        if isinstance(text, str):
            n, _, d = text.partition(":")
            n, d = int(n), int(d) if d else 1
        else:
            n, d = (int(v) for v in text)
    except (TypeError, ValueError):
        n = d = 0
    if n < 1 or d < 1:
        raise ValueError(f"{what}: frame rate {text!r} is not N or N:D with positive integers")
    return n, d


def is_y4m(path):
    return str(path).lower().endswith(".y4m")


def chroma_size(fmt, height, width):
    """(hc, wc) of a format's chroma planes ((0, 0) for mono)."""
    if fmt == "mono":
        return 0, 0
    return ((height + 1) // 2 if fmt.startswith("420") else height), (width if fmt == "444" else (width + 1) // 2)


def payload_bytes(fmt, height, width):
    hc, wc = chroma_size(fmt, height, width)
    return height * width + 2 * hc * wc


def parse_header(line, what="y4m"):
    """The header line (bytes, without its newline) -> dict(width, height, fps, interlace, aspect, format, range, extra);
    fps (n, d) or None, aspect the text n:d or None, range None where no XCOLORRANGE says it, extra the other X tags."""
    try:
        tokens = line.decode("ascii").split(" ")
    except UnicodeDecodeError:
        tokens = [""]
    if tokens[0] != MAGIC.decode():
        raise ValueError(f"{what}: not a YUV4MPEG2 stream (the file does not start with 'YUV4MPEG2 ')")
    h = dict(width=None, height=None, fps=None, interlace="p", aspect=None, format="420jpeg", range=None, extra=[])
    for tok in filter(None, tokens[1:]):
        tag, val = tok[0], tok[1:]
        if tag in "WH":
            if not val.isdigit() or int(val) < 1:
                raise ValueError(f"{what}: header tag {tok!r} is not a positive size")
            h["width" if tag == "W" else "height"] = int(val)
        elif tag == "F":
            h["fps"] = parse_fps(val, what)
        elif tag == "I":
            if val in ("t", "b", "m"):
                raise ValueError(f"{what}: interlaced stream (I{val}); only progressive streams (Ip) are read")
            h["interlace"] = val
        elif tag == "A":
            h["aspect"] = val
        elif tag == "C":
            fmt = "420jpeg" if val == "420" else val
            if fmt not in FORMATS:
                raise ValueError(f"{what}: chroma format C{val} is not supported (8-bit {', '.join(FORMATS)} and the bare 420)")
            h["format"] = fmt
        elif tag == "X":
            if val.startswith("COLORRANGE="):
                rng = val[len("COLORRANGE="):].lower()
                if rng not in RANGES:
                    raise ValueError(f"{what}: header tag {tok!r} is neither FULL nor LIMITED")
                h["range"] = rng
            else:
                h["extra"].append(tok)
        else:
            raise ValueError(f"{what}: unknown header tag {tok!r}")
    for key, tag in (("width", "W"), ("height", "H")):
        if h[key] is None:
            raise ValueError(f"{what}: the header has no {tag} tag (the frame's {key})")
    return h


def header_line(width, height, fps, fmt, range, aspect=None, extra=()):          # noqa: A002
    """The header a written stream starts with, newline included: progressive, XCOLORRANGE always said."""
    n, d = fps
    parts = [MAGIC.decode(), f"W{width}", f"H{height}", f"F{n}:{d}", "Ip"] + ([f"A{aspect}"] if aspect else [])
    parts += [f"C{fmt}", f"XCOLORRANGE={range.upper()}"] + list(extra)
    return (" ".join(parts) + "\n").encode("ascii")


class Y4MStream:
    """A seekable .y4m file: its header and random access to its frames.  ``matrix`` and ``range`` are what the kernels are
    given for it: the header's XCOLORRANGE where it has one, the process-wide defaults otherwise (read when it is opened)."""

    def __init__(self, path):
        self.path = str(path)
        with open(self.path, "rb") as f:
            head = f.read(4096)
            size = os.fstat(f.fileno()).st_size
        end = head.find(b"\n")
        if not head.startswith(MAGIC + b" ") or end < 0:
            raise ValueError(f"{self.path}: not a YUV4MPEG2 stream (no 'YUV4MPEG2 ' header line in its first {len(head)} bytes)")
        h = parse_header(head[:end], self.path)
        self.width, self.height, self.fps, self.aspect = h["width"], h["height"], h["fps"], h["aspect"]
        self.format, self.extra, self.header_range = h["format"], h["extra"], h["range"]
        self.matrix, self.range = _defaults["matrix"], h["range"] or _defaults["range"]
        self.header_bytes = end + 1
        self.payload_bytes = payload_bytes(self.format, self.height, self.width)
        body, step = size - self.header_bytes, len(FRAME) + self.payload_bytes
        if body % step:
            raise ValueError(f"{self.path}: {body} bytes after the header are not whole frames of 6 + {self.payload_bytes} bytes "
                             f"({self.format}, {self.width}x{self.height}): a truncated file, or frames with parameters")
        self.frame_count = body // step
        self._file, self._lock = None, threading.Lock()

    def __len__(self):
        return self.frame_count

    def read_into(self, index, buffer):
        """Frame ``index``'s payload into ``buffer`` (a writable buffer of payload_bytes bytes, e.g. a row of a pinned
        tensor's numpy view) with one readinto at its offset."""
        if not 0 <= index < self.frame_count:
            raise IndexError(f"{self.path}: frame {index} of {self.frame_count}")
        view = memoryview(buffer).cast("B")
        if len(view) != self.payload_bytes:
            raise ValueError(f"{self.path}: a buffer of {len(view)} bytes for a payload of {self.payload_bytes}")
        with self._lock:
            if self._file is None:
                self._file = open(self.path, "rb", buffering=0)
            self._file.seek(self.header_bytes + index * (len(FRAME) + self.payload_bytes))
            mark = self._file.read(len(FRAME))
            if mark != FRAME:
                raise ValueError(f"{self.path}: frame {index} does not start with 'FRAME\\n' (got {mark!r}); per-frame "
                                 "parameters are not supported")
            got = self._file.readinto(view)
        if got != self.payload_bytes:
            raise ValueError(f"{self.path}: frame {index} ends after {got} of {self.payload_bytes} bytes")

    def close(self):
        with self._lock:
            if self._file is not None:
                self._file.close()
                self._file = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Y4MFrame(str):
    """One frame of a stream where a frame file's path stands: its text is ``<path>#0007``, so basenames, sorting and the
    names of JSON reports keep working; ``stream`` and ``index`` say where its bytes are."""

    def __new__(cls, stream, index):
        self = super().__new__(cls, f"{stream.path}#{index:04d}")
        self.stream, self.index = stream, int(index)
        return self


def frames_of(path):
    stream = Y4MStream(path)
    return [Y4MFrame(stream, k) for k in range(stream.frame_count)]


def stream_of(refs):
    """The stream of a frame list's first Y4MFrame (None for frame files or an empty list)."""
    return next((r.stream for r in refs if isinstance(r, Y4MFrame)), None)


def output_params(source=None, rate=1):
    """What a written stream's header says: dict(fps, aspect, format, matrix, range, extra).  ``source``: the input stream it
    inherits from (or None); ``rate``: interpolate's multiple of the frame rate.  set_output's values win over the source's."""
    fps = _output["fps"] or (source.fps if source is not None and source.fps else DEFAULT_FPS)
    return dict(fps=(fps[0] * int(rate), fps[1]), aspect=source.aspect if source is not None else None,
                format=_output["chroma"] or (source.format if source is not None else "420jpeg"), matrix=_defaults["matrix"],
                range=source.range if source is not None else _defaults["range"], extra=list(source.extra) if source is not None else [])
