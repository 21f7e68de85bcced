"""Video inference driver on the HIP path: a stream of Y'CbCr 4:2:0 frames in, the enhanced stream out, raw or YUV4MPEG2, files or pipes.
No reference counterpart (the reference walks a directory of PNGs); the forward is the LOL-Blur / LOL-v1 drivers' own:

    read (thread, pinned buffers)  ->  codec samples on the GPU  ->  fdn_pre_yuv420  ->  LPNet -> FDN  ->  fdn_post_yuv420  ->  write (thread)

so a frame goes from the decoder's samples straight to fp32 and back, rounded once, and 10-bit sources keep their bits.

    ffmpeg -i in.mp4 -f yuv4mpegpipe -strict -1 - | python inference_fdn_video.py --fdn F.pth --lpnet L.pth - - | ffmpeg -i - out.mp4
    python inference_fdn_video.py --fdn F.pth --lpnet L.pth --size 1280x720 --pix-fmt nv12 in.yuv out.yuv

IN / OUT: paths, `-` = stdin / stdout (binary); every message goes to stderr.  The output has the input's container and format: for Y4M
the input's header line is written back verbatim and `FRAME` precedes each frame.  Frames larger than one forward can take run with
--tile, as in the image drivers.  --ratio-smooth ALPHA filters the ratio FDN is fed across the frames (fdn_hip.temporal: against the flicker
of a ratio predicted frame by frame), --scene-cut FRACTION sets where it starts afresh.  --temporal-denoise STRENGTH filters the enhanced
frames themselves along block motion vectors, before they are rounded to samples (fdn_hip.mctf: against boiling noise; --denoise-threshold,
--denoise-radius and --denoise-cut shape it).  One process, one GPU.  Needs a ROCm GPU and the built libfdn_hip.so; there is no CPU fallback.
"""
import argparse
import os
import queue
import sys
import threading
from collections import namedtuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from inference_fdn_lolblur import add_tile_args, hint_hard_seam, hint_large_frame, load_params  # noqa: E402

Y4M_MAGIC = b"YUV4MPEG2 "
# Y4M colour-space tag -> (pix_fmt, chroma_loc); no tag at all means C420jpeg
Y4M_TAGS = {"420jpeg": ("yuv420p", "center"), "420": ("yuv420p", "center"), "420mpeg2": ("yuv420p", "left"), "420p10": ("yuv420p10le", "left")}
SAMPLE_BYTES = {"yuv420p": 1, "nv12": 1, "yuv420p10le": 2}

Y4MHeader = namedtuple("Y4MHeader", "line width height pix_fmt chroma_loc full_range")      # full_range: None when the header is silent


def frame_bytes(pix_fmt, width, height):
    """bytes of one 4:2:0 frame: width * height luma samples and half as many chroma samples"""
    if pix_fmt not in SAMPLE_BYTES:
        raise ValueError(f"pix_fmt {pix_fmt!r}: one of {', '.join(SAMPLE_BYTES)}")
    if width <= 0 or height <= 0 or width % 2 or height % 2:
        raise ValueError(f"a 4:2:0 frame needs even, positive sides, got {width}x{height}")
    return width * height * 3 // 2 * SAMPLE_BYTES[pix_fmt]


def parse_y4m_header(line):
    """The stream header line of a YUV4MPEG2 stream (bytes, with or without its newline) -> Y4MHeader.  Read: W, H, C, I and ffmpeg's
    XCOLORRANGE=FULL|LIMITED; anything else (F, A, other X) is carried along in `line`.  ValueError names what is not supported."""
    if not line.startswith(Y4M_MAGIC):
        raise ValueError("not a YUV4MPEG2 stream header")
    try:
        fields = line.rstrip(b"\n").decode("ascii").split(" ")[1:]
    except UnicodeDecodeError:
        raise ValueError("YUV4MPEG2 header is not ASCII")
    width = height = full_range = None
    tag = "420jpeg"
    for f in fields:
        if not f:
            continue
        key, val = f[0], f[1:]
        if key in "WH":
            if not val.isdigit():
                raise ValueError(f"YUV4MPEG2 header: bad size field {f!r}")
            width, height = (int(val), height) if key == "W" else (width, int(val))
        elif key == "C":
            tag = val
        elif key == "I" and val not in ("p", "?"):
            raise ValueError(f"YUV4MPEG2 header: interlaced material (I{val}) is not supported")
        elif f.startswith("XCOLORRANGE="):
            rng = f.split("=", 1)[1]
            if rng not in ("FULL", "LIMITED"):
                raise ValueError(f"YUV4MPEG2 header: unknown {f}")
            full_range = rng == "FULL"
    if tag not in Y4M_TAGS:
        raise ValueError(f"YUV4MPEG2 header: colour space C{tag} is not supported (C420jpeg, C420mpeg2, C420, C420p10 are)")
    if width is None or height is None:
        raise ValueError("YUV4MPEG2 header lacks W or H")
    pix_fmt, loc = Y4M_TAGS[tag]
    frame_bytes(pix_fmt, width, height)                                  # odd sides: refused here
    return Y4MHeader(line, width, height, pix_fmt, loc, full_range)


def auto_matrix(height):
    """--matrix auto, the usual player rule: BT.709 above 576 lines, BT.601 up to there"""
    return "bt709" if height > 576 else "bt601"


def video_format(height, pix_fmt="yuv420p", matrix="auto", full_range=False, chroma_loc="left"):
    from fdn_hip.harness import VideoFormat
    return VideoFormat(pix_fmt, auto_matrix(height) if matrix == "auto" else matrix, bool(full_range), chroma_loc)


def y4m_format(hdr, pix_fmt=None, matrix="auto", full_range=None, chroma_loc=None):
    """The VideoFormat of a Y4M stream: what its header says, unless a command-line flag (not None) says otherwise"""
    return video_format(hdr.height, pix_fmt or hdr.pix_fmt, matrix, (hdr.full_range or False) if full_range is None else full_range,
                        chroma_loc or hdr.chroma_loc)


class TruncatedInput(Exception):
    pass


def _read_exact(stream, view):
    """fill the writable byte view from a stream that may deliver short reads (a pipe) -> bytes read, short only at the end of the stream"""
    got = 0
    while got < len(view):
        n = stream.readinto(view[got:])
        if not n:
            break
        got += n
    return got


class FrameReader:
    """Frames of `nbytes` bytes from a binary stream, raw or Y4M (after its header line).  prefix: bytes already taken from the stream.
    read_batch(buf) fills rows of a uint8 array [n, nbytes] -> the number of complete frames, fewer than n only at the end; a stream that
    ends inside a frame raises TruncatedInput on the call after its last complete frame was handed out."""

    def __init__(self, stream, nbytes, y4m, prefix=b""):
        self.stream, self.nbytes, self.y4m, self.prefix = stream, nbytes, y4m, prefix
        self.frames = 0
        self.error = None

    def _take(self, view):
        k = min(len(self.prefix), len(view))
        view[:k] = self.prefix[:k]
        self.prefix = self.prefix[k:]
        return k + _read_exact(self.stream, view[k:])

    def _marker(self):
        """True after a FRAME line, False at a clean end of the stream"""
        line = bytearray()
        one = bytearray(1)
        while len(line) < 256 and self._take(memoryview(one)):
            line += one
            if one == b"\n":
                break
        if not line:
            return False
        if not line.startswith(b"FRAME") or not line.endswith(b"\n"):
            self.error = f"input ends or is damaged at frame {self.frames}: {len(line)} bytes where a FRAME line belongs"
            return False
        return True

    def read_batch(self, buf):
        if self.error:
            raise TruncatedInput(self.error)
        for i in range(buf.shape[0]):
            if self.y4m and not self._marker():
                return i
            got = self._take(memoryview(buf[i]).cast("B"))
            if got < self.nbytes:
                if got or self.y4m:
                    self.error = f"input ends inside frame {self.frames}: {got} of {self.nbytes} bytes"
                return i
            self.frames += 1
        return buf.shape[0]


def write_frames(stream, frames, y4m):
    """uint8 array [n, nbytes] -> the stream, `FRAME` before each frame of a Y4M stream"""
    for f in frames:
        if y4m:
            stream.write(b"FRAME\n")
        stream.write(memoryview(f).cast("B"))


def size_arg(s):
    try:
        w, h = (int(v) for v in s.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"{s!r} is not WxH")
    if w <= 0 or h <= 0 or w % 2 or h % 2:
        raise argparse.ArgumentTypeError(f"{s!r}: a 4:2:0 frame needs even, positive sides")
    return w, h


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def open_streams(a):
    """(input, output) binary streams.  With OUT = `-` the frames go to what was stdout.  Either way file descriptor 1 is then pointed at
    stderr, so that nothing but frames can reach a pipe and every message lands on stderr, whoever prints it."""
    src = sys.stdin.buffer if a.input == "-" else open(a.input, "rb")
    sys.stdout.flush()
    if a.output == "-":
        dst = os.fdopen(os.dup(1), "wb")
    else:
        os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
        dst = open(a.output, "wb")
    os.dup2(2, 1)
    return src, dst


def open_video(a, src):
    """-> (FrameReader, VideoFormat, width, height, the Y4M header line or None); SystemExit with one line on what cannot be read"""
    head = bytearray(len(Y4M_MAGIC))
    head = bytes(head[:_read_exact(src, memoryview(head))])
    y4m = a.format == "y4m" or (a.format == "auto" and head == Y4M_MAGIC)
    full = None if a.range is None else a.range == "full"
    try:
        if y4m:
            if head != Y4M_MAGIC:
                raise ValueError("--format y4m, but the input does not start with 'YUV4MPEG2 '")
            hdr = parse_y4m_header(head + src.readline(4096))
            if not hdr.line.endswith(b"\n"):
                raise ValueError("YUV4MPEG2 header line does not end")
            if a.size and a.size != (hdr.width, hdr.height):
                raise ValueError(f"--size {a.size[0]}x{a.size[1]} contradicts the stream's {hdr.width}x{hdr.height}")
            fmt, width, height, line, head = y4m_format(hdr, a.pix_fmt, a.matrix, full, a.chroma_loc), hdr.width, hdr.height, hdr.line, b""
        else:
            if not a.size:
                raise ValueError("raw input needs --size WxH")
            width, height = a.size
            fmt, line = video_format(height, a.pix_fmt or "yuv420p", a.matrix, bool(full), a.chroma_loc or "left"), None
        nbytes = frame_bytes(fmt.pix_fmt, width, height)
    except ValueError as e:
        raise SystemExit(f"inference_fdn_video.py: {e}")
    return FrameReader(src, nbytes, y4m, prefix=head), fmt, width, height, line


def stream_video(a, reader, dst, fmt, w, h, y4m_line, enhance, dev):
    """reader thread -> pinned batch -> enhance on the device -> pinned batch -> writer thread; -> the number of frames written"""
    n_in = fmt.frame_samples(h, w)
    pinned = lambda: torch.empty((a.batch, n_in), dtype=fmt.dtype).pin_memory()  # noqa: E731
    as_bytes = lambda t: t.numpy().view(np.uint8).reshape(a.batch, -1)  # noqa: E731
    free_in, free_out, filled, drain = queue.Queue(), queue.Queue(), queue.Queue(maxsize=1), queue.Queue()
    for _ in range(3):                                                    # one being filled, one waiting, one on its way to the GPU
        free_in.put(pinned())
    for _ in range(2):
        free_out.put(pinned())
    failed = []

    def read_loop():
        try:
            while True:
                buf = free_in.get()
                n = reader.read_batch(as_bytes(buf))
                filled.put((buf, n))
                if n < a.batch:
                    return
        except BaseException as e:  # noqa: BLE001  (handed to the main thread)
            filled.put(e)

    def write_loop():
        while True:
            item = drain.get()
            if item is None:
                return
            buf, n = item
            try:
                if not failed:
                    write_frames(dst, as_bytes(buf)[:n], y4m_line is not None)
            except BaseException as e:  # noqa: BLE001
                failed.append(e)
            free_out.put(buf)

    if y4m_line is not None:
        dst.write(y4m_line)
    threads = [threading.Thread(target=read_loop, daemon=True), threading.Thread(target=write_loop, daemon=True)]
    for t in threads:
        t.start()
    done = 0
    try:
        while not failed:
            item = filled.get()
            if isinstance(item, BaseException):
                raise item
            buf, n = item
            if n:
                out = enhance(buf[:n].to(dev, non_blocking=True))
                host = free_out.get()
                host[:n].copy_(out.view(fmt.dtype), non_blocking=True)
                torch.cuda.synchronize()
                drain.put((host, n))
                done += n
            free_in.put(buf)
            if n < a.batch:
                break
    finally:
        drain.put(None)
        threads[1].join()
    if failed:
        raise failed[0]
    dst.flush()
    if reader.error:                                                      # after the complete frames before it were written
        raise TruncatedInput(reader.error)
    return done


def unit_fraction(low_open):
    """argparse type of a value in (0, 1] (low_open) or [0, 1]"""
    def parse(s):
        try:
            v = float(s)
        except ValueError:
            raise argparse.ArgumentTypeError(f"{s!r} is not a number")
        if not (0.0 < v <= 1.0 if low_open else 0.0 <= v <= 1.0):
            raise argparse.ArgumentTypeError(f"{s!r} is not in {'(0, 1]' if low_open else '[0, 1]'}")
        return v
    return parse


def positive_float(s):
    try:
        v = float(s)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{s!r} is not a number")
    if not 0.0 < v < float("inf"):
        raise argparse.ArgumentTypeError(f"{s!r} is not a positive, finite number")
    return v


def radius_arg(s):
    try:
        v = int(s)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{s!r} is not an integer")
    if not 0 <= v <= 16:
        raise argparse.ArgumentTypeError(f"{s!r} is not in 0 .. 16")
    return v


DENOISE_DEFAULTS = {"denoise_threshold": 0.12, "denoise_radius": 8, "denoise_cut": 0.10}     # fdn_hip.mctf.TemporalDenoiser's own


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fdn", required=True, help="FDN checkpoint ({'params': state_dict})")
    ap.add_argument("--lpnet", required=True, help="LPNet checkpoint")
    ap.add_argument("--model", choices=("lolblur", "lolv1"), default="lolblur", help="the network and its ratio (default lolblur)")
    ap.add_argument("input", metavar="IN", help="input stream: a path, or - for stdin")
    ap.add_argument("output", metavar="OUT", help="output stream: a path, or - for stdout")
    ap.add_argument("--format", choices=("auto", "raw", "y4m"), default="auto",
                    help="auto: YUV4MPEG2 when the stream starts with its magic, else raw (which needs --size)")
    ap.add_argument("--size", type=size_arg, default=None, metavar="WxH", help="frame size of a raw stream")
    ap.add_argument("--pix-fmt", choices=tuple(SAMPLE_BYTES), default=None, help="sample layout (default: the Y4M header's, yuv420p for raw)")
    ap.add_argument("--matrix", choices=("auto", "bt601", "bt709"), default="auto", help="auto: bt709 above 576 lines, else bt601")
    ap.add_argument("--range", choices=("limited", "full"), default=None, help="default: the Y4M header's XCOLORRANGE, else limited")
    ap.add_argument("--chroma-loc", choices=("left", "center"), default=None, help="default: the Y4M header's, left for raw")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--ratio-smooth", type=unit_fraction(True), default=None, metavar="ALPHA",
                    help="filter the ratio FDN is fed across frames against flicker: ratio = previous + ALPHA * (this frame's - previous), "
                         "ALPHA in (0, 1], started afresh at a scene cut; 1 filters nothing but still counts cuts (default: off, every "
                         "frame on its own)")
    ap.add_argument("--scene-cut", type=unit_fraction(False), default=0.3, metavar="FRACTION",
                    help="with --ratio-smooth: a scene cut is where more than this fraction of the pixels changed their luma bin (of 256) "
                         "against the frame before; 1 = never (default 0.3)")
    ap.add_argument("--temporal-denoise", type=unit_fraction(True), default=None, metavar="STRENGTH",
                    help="filter the enhanced frames along block motion vectors against boiling noise: out = frame + k * (the previous "
                         "output, motion-compensated - frame), k = STRENGTH in (0, 1] where the prediction fits, falling to 0 where it does "
                         "not and at a scene cut (default: off)")
    ap.add_argument("--denoise-threshold", type=positive_float, default=None, metavar="T",
                    help="with --temporal-denoise: the local difference between a frame and its prediction, in units of the [0, 1] signal, at "
                         "which k reaches 0 (default 0.12, from synthetic noise, not tuned on footage)")
    ap.add_argument("--denoise-radius", type=radius_arg, default=None, metavar="R",
                    help="with --temporal-denoise: the block search looks R pixels each way, 0 .. 16 (default 8)")
    ap.add_argument("--denoise-cut", type=unit_fraction(False), default=None, metavar="FRACTION",
                    help="with --temporal-denoise: a frame whose best block matches miss by more than this fraction of the luma range on "
                         "average starts afresh, unfiltered; 1 = never (default 0.10)")
    add_tile_args(ap)
    a = ap.parse_args(argv)
    if a.batch < 1:
        ap.error("--batch must be at least 1")
    if a.ratio_smooth is not None and a.tile_ratio != "frame":
        ap.error("--ratio-smooth filters one ratio per frame: it needs --tile-ratio frame")
    for k, v in DENOISE_DEFAULTS.items():
        if getattr(a, k) is None:
            setattr(a, k, v)
        elif a.temporal_denoise is None:
            ap.error(f"--{k.replace('_', '-')} needs --temporal-denoise")
    return a


def main():
    a = parse_args()
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("inference_fdn_video.py runs as one process on one GPU: WORLD_SIZE > 1 is not supported")

    src, dst = open_streams(a)
    reader, fmt, w, h, y4m_line = open_video(a, src)
    say(f"{'y4m' if y4m_line is not None else 'raw'} {w}x{h} {fmt.pix_fmt} {fmt.matrix} {'full' if fmt.full_range else 'limited'} range, "
        f"chroma {fmt.chroma_loc}")

    from fdn_hip.harness import enhance_yuv420
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    if a.model == "lolv1":
        from basicsr.models.archs.fdnlol24_arch import FDN_lolv1 as Net
    else:
        from basicsr.models.archs.FDN_arch import FDN as Net
    from basicsr.models.archs.LPNet_arch import I_predict_net
    net, lp = Net().to(dev).eval(), I_predict_net().to(dev).eval()
    net.load_state_dict(load_params(a.fdn), strict=True)
    lp.load_state_dict(load_params(a.lpnet), strict=True)
    hint_large_frame(a.tile, h, w)
    hint_hard_seam(a.tile, a.tile_blend, a.tile_overlap, h, w)

    smooth = None
    if a.ratio_smooth is not None:                                       # one filter per run: the run is one stream of frames
        from fdn_hip.temporal import RatioFilter
        smooth = RatioFilter(h, w, fmt.bits, a.ratio_smooth, cut=a.scene_cut, device=dev)

    denoise = None
    if a.temporal_denoise is not None:                                   # as the ratio filter: one per run
        from fdn_hip.mctf import TemporalDenoiser
        denoise = TemporalDenoiser(h, w, fmt, a.temporal_denoise, a.denoise_threshold, a.denoise_radius, a.denoise_cut, device=dev)

    def enhance(frames):
        return enhance_yuv420(net, lp, frames, h, w, fmt, ratio_mode=a.model, tile=a.tile, ratio_from=a.tile_ratio, overlap=a.tile_overlap,
                              batch=a.batch, blend=a.tile_blend, temporal=smooth, denoise=denoise)

    try:
        done = stream_video(a, reader, dst, fmt, w, h, y4m_line, enhance, dev)
    except TruncatedInput as e:
        dst.flush()
        raise SystemExit(f"inference_fdn_video.py: {e}; {reader.frames} complete frames -> {a.output}")
    dst.close()
    say(f"{done} frames -> {a.output}" + (f", {smooth.cuts_seen()} scene cuts" if smooth is not None else ""))


if __name__ == "__main__":
    main()
