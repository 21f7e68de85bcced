"""Score an enhanced video stream on the HIP path, straight from its codec samples: per frame PSNR of Y / Cb / Cr and SSIM on luma against
a ground-truth stream, mean luma, scene cuts and the brightness flicker of the stream (fdn_hip.video_metrics).  The evaluation side of
inference_fdn_video.py: the same containers (raw or YUV4MPEG2) and sample layouts (yuv420p, nv12, yuv420p10le), opened by that driver's
own reader, and no detour through 8-bit RGB, so 10 bit is scored as 10 bit.  No reference counterpart (the reference scores PNGs).

    python calculate_video_metrics.py --ref gt.y4m enhanced.y4m --csv scores.csv
    ffmpeg -i out.mp4 -f yuv4mpegpipe -strict -1 - | python calculate_video_metrics.py --ref gt.y4m -
    python calculate_video_metrics.py --size 1280x720 --pix-fmt nv12 enhanced.yuv          # no ground truth: mean luma, cuts, flicker
    python calculate_video_metrics.py --ref gt.y4m enhanced.y4m --motion --motion-radius 12   # and the motion-compensated figures
    python calculate_video_metrics.py --ref gt.y4m enhanced.y4m --ms-ssim                     # and multi-scale SSIM on luma
    python calculate_video_metrics.py enhanced.y4m --piqe                                     # no ground truth: and PIQE on luma

REF and DIST are paths, DIST may be `-` for stdin.  PSNR is on the codes (peak 2^bits - 1) whatever the range of the stream, the `average`
pools the three planes as ffmpeg's psnr filter does; SSIM is the reference's _ssim_cly on the luma codes; mean_y and dmean (the change of
mean luma against the frame before, `-` at a scene cut) are in 8-bit code units; flicker = mean |dmean| over the frames that are no cut.
With --ref the cuts are found in REF.  stdout: one line per frame, `Average:` and `flicker:`; every message goes to stderr.  Streams of
--motion adds the motion-compensated temporal consistency (fdn_hip.motion.MotionScore, libfdn_motion.so): block vectors found in REF (in
DIST itself without one, which flatters it) by full search over +-N pixels (--motion-radius, default 8), and along them mc-PSNR (how well
the previous output frame predicts this one; `ref`: the same on REF, the ceiling), tc (the RMS difference of DIST's compensated change
against REF's, 8-bit code units: the local counterpart of the flicker figure) and the share of moving blocks; `-` at a scene cut.  Each
frame line, the CSV (mc_psnr, mc_psnr_ref, tc_rmse, moving, mean_mv) and one line `temporal:` after `flicker:` carry them; without
--motion stdout and the CSV are what they were.
--ms-ssim (needs --ref) adds the multi-scale SSIM of the luma planes (fdn_hip.msssim.MsSsimScore, libfdn_msssim.so; 10 bit scored as
10 bit): `, MS-SSIM-Y x.xxxxxx` at the end of each frame line and of the `Average:` line, and a last CSV column ms_ssim_y.  Five scales
need frames of at least 161x161; a smaller stream is refused.  Without --ms-ssim stdout and the CSV are what they were.
--piqe adds the no-reference PIQE of DIST's luma planes (fdn_hip.piqe.PiqeScore, libfdn_piqe.so; 0 best, 100 worst, exactly 100 for a
flat frame; 10-bit codes count as quarters of an 8-bit code) and with --ref that of REF's beside it: `, PIQE-Y x.xxxxxx` (`(ref
x.xxxxxx)`) at the very end of each frame line and of the `Average:` line, and the last CSV columns piqe_y (and piqe_y_ref).  It works
without --ref.  Without --piqe stdout and the CSV are what they were.  Streams of
unequal length: the common prefix is scored, both lengths are named and the exit status is 1.  One process, one GPU; needs a ROCm GPU
and the built libfdn_hip.so, there is no CPU fallback.
"""
import argparse
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from inference_fdn_video import SAMPLE_BYTES, open_video, say, size_arg, unit_fraction  # noqa: E402

ME = "calculate_video_metrics.py"
PIQE_COLUMNS = ("piqe_y", "piqe_y_ref")                                          # the very last columns, with --piqe; the second with --ref
MS_SSIM_COLUMNS = ("ms_ssim_y",)                                                # after every other column, with --ms-ssim
MS_SSIM_MIN_SIDE = 161                                                          # FDN_MSSSIM_MIN_SIDE of include/fdn_msssim.h
MOTION_COLUMNS = ("mc_psnr", "mc_psnr_ref", "tc_rmse", "moving", "mean_mv")     # after CSV_COLUMNS, with --motion
CSV_COLUMNS = ("frame", "psnr_y", "psnr_u", "psnr_v", "psnr_avg", "ssim_y", "mean_y_ref", "mean_y", "cut", "dmean_ref", "dmean")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ref", default=None, metavar="REF", help="ground-truth stream: a path (without it: mean luma, cuts and flicker only)")
    ap.add_argument("dist", metavar="DIST", help="the stream to score: a path, or - for stdin")
    ap.add_argument("--format", choices=("auto", "raw", "y4m"), default="auto",
                    help="auto: YUV4MPEG2 when a stream starts with its magic, else raw (which needs --size)")
    ap.add_argument("--size", type=size_arg, default=None, metavar="WxH", help="frame size of a raw stream")
    ap.add_argument("--pix-fmt", choices=tuple(SAMPLE_BYTES), default=None, help="sample layout (default: the Y4M header's, yuv420p for raw)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--scene-cut", type=unit_fraction(False), default=0.3, metavar="FRACTION",
                    help="a scene cut is where more than this fraction of the pixels changed their luma bin (of 256) against the frame "
                         "before; 1 = never (default 0.3)")
    ap.add_argument("--motion", action="store_true",
                    help="add the motion-compensated temporal consistency: mc-PSNR, tc, moving blocks (vectors from REF, else from DIST)")
    ap.add_argument("--motion-radius", type=int, default=None, metavar="N", help="search +-N pixels around every 16 x 16 block, 0 .. 16 (default 8)")
    ap.add_argument("--ms-ssim", action="store_true", help="add the multi-scale SSIM of the luma planes against REF (frames of at least 161x161)")
    ap.add_argument("--piqe", action="store_true", help="add the no-reference PIQE of the luma planes of DIST (and of REF, when given)")
    ap.add_argument("--csv", default=None, metavar="PATH", help="write the per-frame records there, floats as repr() writes them")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.batch < 1:
        ap.error("--batch must be at least 1")
    if a.motion_radius is not None and not a.motion:
        ap.error("--motion-radius needs --motion")
    if a.motion_radius is None:
        a.motion_radius = 8
    if not 0 <= a.motion_radius <= 16:
        ap.error("--motion-radius must be in 0 .. 16")
    if a.ms_ssim and a.ref is None:
        ap.error("--ms-ssim needs --ref: the score is of a pair")
    if a.ref == "-":
        ap.error("REF is a path: only DIST may be stdin")
    return a


DRIVER_PREFIX = "inference_fdn_video.py: "                              # what the driver's open_video puts before its one-line refusals


def close_streams(*readers):
    """close what open_stream opened (stdin is left alone)"""
    for r in readers:
        if r is not None and r.stream is not sys.stdin.buffer:
            r.stream.close()


def open_stream(a, path):
    """-> (FrameReader, VideoFormat, width, height) of one stream through the video driver's open_video; SystemExit with one line"""
    try:
        src = sys.stdin.buffer if path == "-" else open(path, "rb")
    except OSError as e:
        raise SystemExit(f"{ME}: {path}: {e.strerror}")
    try:
        return open_video(SimpleNamespace(format=a.format, size=a.size, pix_fmt=a.pix_fmt, matrix="auto", range=None, chroma_loc=None), src)[:4]
    except SystemExit as e:
        if src is not sys.stdin.buffer:
            src.close()
        msg = str(e.code)
        raise SystemExit(f"{ME}: {path}: {msg[len(DRIVER_PREFIX):] if msg.startswith(DRIVER_PREFIX) else msg}")


def open_pair(a):
    """both streams, checked against each other before anything touches the GPU -> (dist reader, ref reader or None, fmt, w, h)"""
    dist, fmt, w, h = open_stream(a, a.dist)
    ref = None
    try:
        if a.ref is not None:
            ref, rfmt, rw, rh = open_stream(a, a.ref)
            if (rw, rh) != (w, h):
                raise SystemExit(f"{ME}: the streams differ in size: {a.ref} is {rw}x{rh}, {a.dist} is {w}x{h}")
            if rfmt.pix_fmt != fmt.pix_fmt:
                raise SystemExit(f"{ME}: the streams differ in pix_fmt: {a.ref} is {rfmt.pix_fmt}, {a.dist} is {fmt.pix_fmt}")
    except SystemExit:
        close_streams(dist, ref)
        raise
    return dist, ref, fmt, w, h


def _num(v, spec):
    return "-" if v is None else format(v, spec)


def frame_line(i, r, has_ref):
    if has_ref:
        return (f"{i:6d}: PSNR y {r['psnr_y']:.4f} u {r['psnr_u']:.4f} v {r['psnr_v']:.4f} avg {r['psnr_avg']:.4f} dB, SSIM-Y {r['ssim_y']:.6f}, "
                f"mean_y {r['mean_y']:.3f} (ref {r['mean_y_ref']:.3f}), cut {int(r['cut'])}, dmean {_num(r['dmean'], '+.4f')} "
                f"(ref {_num(r['dmean_ref'], '+.4f')})")
    return f"{i:6d}: mean_y {r['mean_y']:.3f}, cut {int(r['cut'])}, dmean {_num(r['dmean'], '+.4f')}"


def motion_part(m, has_ref):
    """what --motion adds to a frame line"""
    ref = f" (ref {_num(m['mc_psnr_ref'], '.4f')})" if has_ref else ""
    tc = f", tc {_num(m['tc_rmse'], '.4f')}" if has_ref else ""
    return f", mc-PSNR {_num(m['mc_psnr'], '.4f')}{ref}{tc}, moving {_num(m['moving'], '.3f')}"


def ms_ssim_part(ms):
    """what --ms-ssim adds to a frame line and to the `Average:` line"""
    return f", MS-SSIM-Y {ms['ms_ssim_y']:.6f}"


def piqe_part(p, pr=None):
    """what --piqe adds to a frame line and to the `Average:` line; pr: the record of REF, when there is one"""
    return f", PIQE-Y {p['piqe_y']:.6f}" + (f" (ref {pr['piqe_y']:.6f})" if pr is not None else "")


def motion_cells(m):
    return ",".join("" if m[k] is None else repr(float(m[k])) for k in MOTION_COLUMNS)


def csv_row(i, r):
    def cell(k):
        v = i if k == "frame" else r[k]
        return "" if v is None else str(int(v)) if k in ("frame", "cut") else repr(float(v))
    return ",".join(cell(k) for k in CSV_COLUMNS)


def drain(reader, buf):
    """frames left in a stream whose partner has ended (counted, not scored)"""
    while reader.read_batch(buf) == buf.shape[0]:
        pass
    return reader.frames


def main(argv=None):
    a = parse_args(argv)
    dist, ref, fmt, w, h = open_pair(a)
    try:
        if a.ms_ssim and (w < MS_SSIM_MIN_SIDE or h < MS_SSIM_MIN_SIDE):
            raise SystemExit(f"{ME}: --ms-ssim: five scales need frames of at least {MS_SSIM_MIN_SIDE}x{MS_SSIM_MIN_SIDE}, the streams are {w}x{h}")
        score_streams(a, dist, ref, fmt, w, h)
    finally:
        close_streams(dist, ref)


def score_streams(a, dist, ref, fmt, w, h):
    say(f"{w}x{h} {fmt.pix_fmt}" + (f", {a.dist} against {a.ref}" if ref is not None else f", {a.dist} on its own"))

    import numpy as np
    import torch
    from fdn_hip.video_metrics import VideoScore
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    score = VideoScore(h, w, fmt, cut=a.scene_cut, device=dev)
    motion = None
    if a.motion:
        from fdn_hip.motion import MotionScore
        motion = MotionScore(h, w, fmt, radius=a.motion_radius, device=dev)
    msssim = None
    if a.ms_ssim:
        from fdn_hip.msssim import MsSsimScore
        msssim = MsSsimScore(h, w, fmt, device=dev)
    piqe = piqe_ref = None
    if a.piqe:
        from fdn_hip.piqe import PiqeScore
        piqe = PiqeScore(h, w, fmt, device=dev)
        piqe_ref = PiqeScore(h, w, fmt, device=dev) if ref is not None else None
    n = fmt.frame_samples(h, w)
    as_bytes = lambda t: t.numpy().view(np.uint8).reshape(a.batch, -1)  # noqa: E731
    buf_d = torch.empty((a.batch, n), dtype=fmt.dtype)
    buf_r = torch.empty((a.batch, n), dtype=fmt.dtype) if ref is not None else None
    out = open(a.csv, "w") if a.csv else None
    if out:
        out.write(",".join(CSV_COLUMNS + (MOTION_COLUMNS if motion else ()) + (MS_SSIM_COLUMNS if msssim else ())
                           + (PIQE_COLUMNS[:2 if piqe_ref else 1] if piqe else ())) + "\n")
    done = 0
    try:
        while True:
            nd = dist.read_batch(as_bytes(buf_d))
            nr = ref.read_batch(as_bytes(buf_r)) if ref is not None else nd
            k = min(nd, nr)
            if k:
                on_d, on_r = buf_d[:k].to(dev), (None if ref is None else buf_r[:k].to(dev))
                recs = score.update(on_d, on_r)
                mrecs = motion.update(on_d, on_r, cuts=[r["cut"] for r in recs]) if motion else [None] * k
                srecs = msssim.update(on_d, on_r) if msssim else [None] * k
                precs = piqe.update(on_d) if piqe else [None] * k
                prrecs = piqe_ref.update(on_r) if piqe_ref else [None] * k
                for r, m, ms, pq, pr in zip(recs, mrecs, srecs, precs, prrecs):
                    print(frame_line(done, r, ref is not None) + (motion_part(m, ref is not None) if motion else "") + (ms_ssim_part(ms) if msssim else "")
                          + (piqe_part(pq, pr) if piqe else ""))
                    if out:
                        out.write(csv_row(done, r) + ("," + motion_cells(m) if motion else "") + ("," + repr(ms["ms_ssim_y"]) if msssim else "")
                                  + ("," + repr(pq["piqe_y"]) + ("," + repr(pr["piqe_y"]) if pr is not None else "") if piqe else "") + "\n")
                    done += 1
            if nd < a.batch or nr < a.batch:
                break
        len_d = dist.frames if nd < a.batch else drain(dist, as_bytes(buf_d))
        len_r = len_d if ref is None else (ref.frames if nr < a.batch else drain(ref, as_bytes(buf_r)))
    finally:
        if out:
            out.close()
    s = score.summary()
    ptail = piqe_part(piqe.summary(), piqe_ref.summary() if piqe_ref else None) if piqe else ""
    if done:
        if ref is not None:
            print(f"Average: PSNR y {s['psnr_y']:.4f} u {s['psnr_u']:.4f} v {s['psnr_v']:.4f} avg {s['psnr_avg']:.4f} dB (over the stream: y "
                  f"{s['psnr_y_global']:.4f} avg {s['psnr_avg_global']:.4f} dB), SSIM-Y {s['ssim_y']:.6f}, mean_y {s['mean_y']:.3f} "
                  f"(ref {s['mean_y_ref']:.3f}), {s['cuts']} scene cuts in {done} frames" + (ms_ssim_part(msssim.summary()) if msssim else "") + ptail)
        else:
            print(f"Average: mean_y {s['mean_y']:.3f}, {s['cuts']} scene cuts in {done} frames" + ptail)
        if s["flicker"] == s["flicker"]:                                  # not nan: some frame followed a frame of its scene
            print(f"flicker: {s['flicker']:.4f}" + (f" (ref {s['flicker_ref']:.4f}, against ref {s['flicker_err']:.4f})" if ref is not None else "")
                  + " mean |dmean|, 8-bit code units")
        t = motion.summary() if motion else None
        if t and t["mc_psnr"] == t["mc_psnr"]:                            # not nan: some frame followed a frame of its scene
            print(f"temporal: mc-PSNR {t['mc_psnr']:.4f} dB (over the stream {t['mc_psnr_global']:.4f})"
                  + (f", ref {t['mc_psnr_ref']:.4f} dB (over the stream {t['mc_psnr_ref_global']:.4f}), tc {t['tc_rmse']:.4f} (over the stream "
                     f"{t['tc_rmse_global']:.4f}) RMS against ref, 8-bit code units" if ref is not None else "")
                  + f", moving {t['moving']:.3f}, mean |mv| {t['mean_mv']:.3f}, search +-{a.motion_radius}")
    sys.stdout.flush()
    for rd, path in ((dist, a.dist), (ref, a.ref)):
        if rd is not None and rd.error:                                   # a stream cut mid-frame, as the video driver words it
            raise SystemExit(f"{ME}: {path}: {rd.error}; {done} frames scored")
    if len_d != len_r:
        raise SystemExit(f"{ME}: the streams differ in length: {a.ref} has {len_r} frames, {a.dist} has {len_d}; the first {done} were scored")
    say(f"{done} frames scored" + (f" -> {a.csv}" if a.csv else ""))


if __name__ == "__main__":
    main()
