"""numpy restatement of the motion-compensated temporal consistency (include/fdn_motion.h, fdn_hip/motion.py), written from the header's
definitions and not from the kernels: for each candidate in rank order the absolute difference against the clamped shift of the previous
frame, summed over the blocks, and the strict-< minimum kept (the first wins, which is the lexicographic rule); the residual sums as plain
integers; the records of MotionScore on Fractions.  The yardstick of tests/test_gpu_motion.py; tests/test_motion_cpu.py judges it on its
own, by hand."""
import math
from fractions import Fraction

import numpy as np

from yuv_ref import PIX_FMTS, sample_dtype  # noqa: F401  (the frame helpers, shared)

BLOCK = 16
# shapes of the GPU tests (h, w, B, R): see the table in tests/test_gpu_motion.py
SHAPES = [(2, 2, 2, 8), (16, 16, 2, 16), (18, 34, 3, 1), (34, 50, 3, 8), (70, 130, 2, 16), (34, 50, 2, 0)]


def block_grid(h, w):
    return -(-h // BLOCK), -(-w // BLOCK)


def luma(frames, h, w, pix_fmt):
    """frames [B, h*w*3/2] (or one frame [h*w*3/2]) -> int64 [B,h,w], a 10-bit word above 1023 counted as 1023"""
    frames = np.asarray(frames)
    if frames.ndim == 1:
        frames = frames[None]
    top = 2 ** PIX_FMTS[pix_fmt][1] - 1
    return np.minimum(frames[:, :h * w].astype(np.int64), top).reshape(-1, h, w)


def candidates(R):
    """the displacements of [-R, R]^2 in the order (dy^2 + dx^2, dy, dx)"""
    return sorted(((dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)), key=lambda d: (d[0] * d[0] + d[1] * d[1], d[0], d[1]))


def shifted(prev, dy, dx):
    """prev(clamp(y + dy), clamp(x + dx)) at every (y, x); dy, dx scalars or [h,w] arrays"""
    h, w = prev.shape
    yy = np.clip(np.arange(h)[:, None] + dy, 0, h - 1)
    xx = np.clip(np.arange(w)[None, :] + dx, 0, w - 1)
    return prev[yy, xx]


def block_sums(a):
    """[h,w] -> [nby,nbx]: the sum over each 16 x 16 block's pixels inside the frame"""
    h, w = a.shape
    nby, nbx = block_grid(h, w)
    p = np.zeros((nby * BLOCK, nbx * BLOCK), dtype=np.int64)
    p[:h, :w] = a
    return p.reshape(nby, BLOCK, nbx, BLOCK).sum(axis=(1, 3))


def search_pair(cur, prev, R):
    """two luma planes -> (mv int64 [nby,nbx,2] = (dy, dx), sad int64 [nby,nbx,2] = (chosen, zero vector))"""
    nby, nbx = block_grid(*cur.shape)
    best = np.full((nby, nbx), np.iinfo(np.int64).max, dtype=np.int64)
    mv = np.zeros((nby, nbx, 2), dtype=np.int64)
    for dy, dx in candidates(R):
        s = block_sums(np.abs(cur - shifted(prev, dy, dx)))
        if (dy, dx) == (0, 0):
            zero = s
        better = s < best
        best = np.where(better, s, best)
        mv[better] = (dy, dx)
    return mv, np.stack([best, zero], axis=-1)


def search(guide, prev, h, w, pix_fmt, R):
    """-> (mv int16 [B,nby,nbx,2], sad int64 [B,nby,nbx,2], stats: B tuples of 4 Python ints); prev None: frame 0's rows are 0"""
    g = luma(guide, h, w, pix_fmt)
    p = None if prev is None else luma(prev, h, w, pix_fmt)[0]
    nby, nbx = block_grid(h, w)
    mvs, sads, stats = [], [], []
    for i in range(g.shape[0]):
        before = g[i - 1] if i else p
        if before is None:
            mv, sad = np.zeros((nby, nbx, 2), dtype=np.int64), np.zeros((nby, nbx, 2), dtype=np.int64)
        else:
            mv, sad = search_pair(g[i], before, R)
        mvs.append(mv)
        sads.append(sad)
        stats.append((int(sad[..., 0].sum()), int(sad[..., 1].sum()), int(np.abs(mv).sum()), int((mv != 0).any(axis=-1).sum())))
    return np.stack(mvs).astype(np.int16), np.stack(sads), stats


def residual(frames, frames_prev, guide, guide_prev, mv, h, w, pix_fmt):
    """-> B tuples of 5 Python ints (sum |rD|, sum rD^2, sum |rG|, sum rG^2, sum (rD - rG)^2); both prevs None: frame 0's row is 0"""
    f, g = luma(frames, h, w, pix_fmt), luma(guide, h, w, pix_fmt)
    fp = None if frames_prev is None else luma(frames_prev, h, w, pix_fmt)[0]
    gp = None if guide_prev is None else luma(guide_prev, h, w, pix_fmt)[0]
    assert (fp is None) == (gp is None)
    out = []
    for i in range(f.shape[0]):
        fb, gb = (f[i - 1], g[i - 1]) if i else (fp, gp)
        if fb is None:
            out.append((0, 0, 0, 0, 0))
            continue
        per_pixel = np.repeat(np.repeat(mv[i].astype(np.int64), BLOCK, axis=0), BLOCK, axis=1)[:h, :w]
        rd = f[i] - shifted(fb, per_pixel[..., 0], per_pixel[..., 1])
        rg = g[i] - shifted(gb, per_pixel[..., 0], per_pixel[..., 1])
        out.append(tuple(int(v) for v in (np.abs(rd).sum(), (rd * rd).sum(), np.abs(rg).sum(), (rg * rg).sum(), ((rd - rg) ** 2).sum())))
    return out


def psnr(sse, n, bits):
    if sse == 0:
        return float("inf")
    L = 2 ** bits - 1
    return 10.0 * math.log10(L * L * n / sse)


def records(dist, ref, h, w, pix_fmt, R=8, cuts=None):
    """the per-frame records of MotionScore for a whole stream -> (list of dicts, summary dict).  The guide is ref, or dist itself without
    one (then only mc_psnr, moving and mean_mv are figures); frame 0 and every frame with cuts[t] is a cut: every figure None."""
    bits = PIX_FMTS[pix_fmt][1]
    guide = dist if ref is None else ref
    mv, _, ss = search(guide, None, h, w, pix_fmt, R)
    rs = residual(dist, None, guide, None, mv, h, w, pix_fmt)
    n, unit = h * w, h * w * 4 ** (bits - 8)
    nblk = block_grid(h, w)[0] * block_grid(h, w)[1]
    recs = []
    for t, (s, r) in enumerate(zip(ss, rs)):
        rec = dict.fromkeys(("mc_psnr", "mc_psnr_ref", "tc_rmse", "moving", "mean_mv"))
        if t and not (cuts is not None and cuts[t]):
            rec.update(mc_psnr=psnr(r[1], n, bits), moving=float(Fraction(s[3], nblk)), mean_mv=float(Fraction(s[2], nblk)))
            if ref is not None:
                rec.update(mc_psnr_ref=psnr(r[3], n, bits), tc_rmse=math.sqrt(float(Fraction(r[4], unit))))
        recs.append(rec)
    live = [t for t, rec in enumerate(recs) if rec["mc_psnr"] is not None]
    nan = float("nan")

    def mean(k):
        v = [recs[t][k] for t in live if recs[t][k] is not None]
        return math.fsum(v) / len(v) if v else nan
    summary = {"frames": len(recs), "cuts": len(recs) - len(live)}
    summary.update({k: mean(k) for k in ("mc_psnr", "mc_psnr_ref", "tc_rmse", "moving", "mean_mv")})
    summary["mc_psnr_global"] = psnr(sum(rs[t][1] for t in live), len(live) * n, bits) if live else nan
    both = live and ref is not None
    summary["mc_psnr_ref_global"] = psnr(sum(rs[t][3] for t in live), len(live) * n, bits) if both else nan
    summary["tc_rmse_global"] = math.sqrt(float(Fraction(sum(rs[t][4] for t in live), len(live) * unit))) if both else nan
    return recs, summary


# ---- test data --------------------------------------------------------------------------------------------------------------------
def frames_of(lumas, pix_fmt, seed=0):
    """int luma planes [B,h,w] (codes; written as they are, so a 10-bit plane may hold words above 1023) -> frames [B, h*w*3/2] with random
    chroma, which nothing here may read"""
    lumas = np.asarray(lumas)
    B, h, w = lumas.shape
    top = 2 ** PIX_FMTS[pix_fmt][1]
    c = np.random.default_rng(seed).integers(0, top, size=(B, h * w // 2))
    return np.concatenate([lumas.reshape(B, -1), c], axis=1).astype(sample_dtype(pix_fmt))


def top_of(pix_fmt):
    return 2 ** PIX_FMTS[pix_fmt][1] - 1


def random_lumas(B, h, w, pix_fmt, seed):
    """independent random planes over the whole code range; for 10 bit one word in 16 lies above 1023 (up to 65535)"""
    g = np.random.default_rng(seed)
    y = g.integers(0, top_of(pix_fmt) + 1, size=(B, h, w))
    if PIX_FMTS[pix_fmt][1] == 10:
        y = np.where(g.random((B, h, w)) < 1 / 16, g.integers(1024, 65536, size=(B, h, w)), y)
    return y


def texture(hh, ww, pix_fmt, seed):
    """a random texture smoothed a little, so that a wrong vector costs something everywhere but neighbours are not independent"""
    g = np.random.default_rng(seed)
    t = g.integers(0, top_of(pix_fmt) + 1, size=(hh, ww)).astype(np.int64)
    return (2 * t + np.roll(t, 1, axis=0) + np.roll(t, 1, axis=1)) // 4


def shifted_stream(B, h, w, pix_fmt, step, seed, noise=0):
    """B frames cut from one texture, the content moving by step = (sy, sx) per frame (so every vector found is -step away from the
    border), plus independent noise of +-noise codes per frame, clipped to the code range"""
    sy, sx = step
    m = (B - 1) * max(abs(sy), abs(sx), 1)
    big = texture(h + 2 * m, w + 2 * m, pix_fmt, seed)
    g = np.random.default_rng(seed + 1)
    out = []
    for t in range(B):
        y0, x0 = m - t * sy, m - t * sx                           # content at p in frame t-1 is at p + step in frame t
        f = big[y0:y0 + h, x0:x0 + w]
        if noise:
            f = f + g.integers(-noise, noise + 1, size=f.shape)
        out.append(np.clip(f, 0, top_of(pix_fmt)))
    return np.stack(out)


def stripes(B, h, w, pix_fmt, move=1):
    """vertical stripes of period 4 (codes 0, 1/3, 2/3, 1 of the range), frame t moved by t * move columns: SAD ties 4 columns apart"""
    top = top_of(pix_fmt)
    x = np.arange(w)[None, :] + np.zeros((h, 1), dtype=np.int64)
    return np.stack([((x - t * move) % 4) * (top // 3) for t in range(B)])
