"""float32 numpy restatement of the motion-compensated temporal denoising (include/fdn_mctf.h, fdn_hip/mctf.py), written from the header's
definition and not from the kernel: whole-frame arrays, one numpy operation per operation of the definition, each on float32 operands and
so rounded once, in the header's order.  The yardstick of tests/test_gpu_mctf.py, which holds the device to it bit for bit;
tests/test_mctf_cpu.py judges it on its own, by its properties and on a synthetic noisy stream."""
import numpy as np

import motion_ref

BLOCK = 16
F = np.float32
# shapes of the GPU tests (h, w, H, W, B): see the table in tests/test_gpu_mctf.py
SHAPES = [(1, 1, 1, 1, 2), (2, 2, 2, 2, 2), (16, 16, 16, 16, 2), (18, 34, 32, 64, 3), (34, 50, 64, 64, 3), (70, 130, 70, 130, 3),
          (17, 65, 17, 65, 2), (16, 128, 16, 128, 2)]


def block_grid(h, w):
    return -(-h // BLOCK), -(-w // BLOCK)


def clamp01(x):
    """fminf(fmaxf(x, 0), 1): a NaN becomes 0"""
    return np.fmin(np.fmax(np.asarray(x, dtype=F), F(0)), F(1))


def axis_terms(n, nb):
    """along one axis of n pixels and nb blocks -> (b0, b1 int [n], w0, w1 float32 [n]): the two blocks of every pixel and their weights"""
    p = np.arange(n)
    b0 = np.floor_divide(p - 8, BLOCK)
    r = np.mod(p + 8, BLOCK)
    w1 = (2 * r + 1).astype(F) / F(32)                                               # exact
    return np.clip(b0, 0, nb - 1), np.clip(b0 + 1, 0, nb - 1), F(1) - w1, w1


def predict(P, mv, h, w):
    """P float32 [3,h,w], mv int [nby,nbx,2] -> pred float32 [3,h,w]: the overlapped-block prediction, four terms in the header's order"""
    nby, nbx = block_grid(h, w)
    mv = np.asarray(mv).astype(np.int64).reshape(nby, nbx, 2)
    by0, by1, wy0, wy1 = axis_terms(h, nby)
    bx0, bx1, wx0, wx1 = axis_terms(w, nbx)
    yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
    pred = np.zeros((3, h, w), dtype=F)
    for by, wy in ((by0, wy0), (by1, wy1)):
        for bx, wx in ((bx0, wx0), (bx1, wx1)):
            d = mv[by[:, None], bx[None, :]]                                          # [h,w,2]
            sy, sx = np.clip(yy + d[..., 0], 0, h - 1), np.clip(xx + d[..., 1], 0, w - 1)
            wt = wy[:, None] * wx[None, :]                                            # float32, a multiple of 1 / 1024
            pred = pred + wt[None] * P[:, sy, sx]
    return pred


def mean3x3(d):
    """float32 [h,w] -> s * (1 / 9), s the sum over the 3 x 3 neighbourhood with a replicated border, row-major from 0"""
    h, w = d.shape
    p = np.pad(d, 1, mode="edge")
    s = np.zeros((h, w), dtype=F)
    for dy in range(3):
        for dx in range(3):
            s = s + p[dy:dy + h, dx:dx + w]
    return s * (F(1) / F(9))


def blend_frame(c, P, mv, strength, inv_threshold):
    """c = clamp01(cur) float32 [3,h,w], P the predecessor -> (out [3,h,w], k [h,w], D [h,w], pred [3,h,w]): steps 3 - 7"""
    _, h, w = c.shape
    pred = predict(np.asarray(P, dtype=F), mv, h, w)
    a = np.abs(c - pred)
    D = mean3x3(np.fmax(np.fmax(a[0], a[1]), a[2]))
    t = D * F(inv_threshold)
    k = F(strength) * np.fmax(F(1) - t * t, F(0))
    return c + k[None] * (pred - c), k, D, pred


def blend(cur, prev, mv, stats, h, w, strength, inv_threshold, cut_limit):
    """cur [B,3,H,W], prev [3,h,w] or None, mv [B,nby,nbx,2], stats [B,4] (word 0 read) -> (out float32 [B,3,h,w], k float32 [B,h,w])"""
    cur = np.asarray(cur, dtype=F)
    outs, ks = [], []
    P = None if prev is None else np.asarray(prev, dtype=F)
    for b in range(cur.shape[0]):
        c = clamp01(cur[b, :, :h, :w])
        if P is None or int(stats[b][0]) > cut_limit:
            o, k = c, np.zeros((h, w), dtype=F)
        else:
            o, k = blend_frame(c, P, mv[b], strength, inv_threshold)[:2]
        outs.append(o)
        ks.append(k)
        P = o
    return np.stack(outs), np.stack(ks)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def inv_of(threshold):
    """what fdn_hip.mctf.inv_threshold gives: 1 / threshold in double, rounded to float32 once"""
    return F(1.0 / float(threshold))


# ---- test data --------------------------------------------------------------------------------------------------------------------
def luma_codes(rgb):
    """float [3,h,w] in [0,1] -> rint(255 * luma), BT.709 weights, int64: the plane the block search runs on"""
    y = 0.2126 * rgb[0].astype(np.float64) + 0.7152 * rgb[1] + 0.0722 * rgb[2]
    return np.rint(255.0 * y).astype(np.int64)


def smooth_texture(hh, ww, seed):
    """a smooth random R'G'B' texture in [0, 1], float64 [3,hh,ww]: white noise box-filtered twice (5 x 5, wrapping), stretched to [0.1, 0.9]"""
    g = np.random.default_rng(seed)
    t = g.random((3, hh, ww))
    for _ in range(2):
        t = sum(np.roll(np.roll(t, dy, axis=1), dx, axis=2) for dy in range(-2, 3) for dx in range(-2, 3)) / 25.0
    lo, hi = t.min(), t.max()
    return 0.1 + 0.8 * (t - lo) / (hi - lo)


def noisy_stream(n, h, w, step, sigma, seed):
    """n frames of h x w cropped from one larger texture, the crop moving by step = (sy, sx) pixels a frame -> (clean, noisy) float32
    [n,3,h,w]; noisy = clip(clean + iid Gaussian noise of sigma)"""
    sy, sx = step
    m = (n - 1) * max(abs(sy), abs(sx), 1)
    big = smooth_texture(h + 2 * m, w + 2 * m, seed)
    g = np.random.default_rng(seed + 1)
    clean = np.stack([big[:, m + t * sy:m + t * sy + h, m + t * sx:m + t * sx + w] for t in range(n)])
    noisy = np.clip(clean + g.normal(0.0, sigma, size=clean.shape), 0.0, 1.0)
    return clean.astype(F), noisy.astype(F)


def filter_stream(noisy, strength, threshold, R=8, cut_limit=None):
    """what TemporalDenoiser does to a stream, with motion_ref.search_pair on rint(255 luma) of the NOISY frames -> (out [n,3,h,w], k)"""
    n, _, h, w = noisy.shape
    nby, nbx = block_grid(h, w)
    mvs, stats = [np.zeros((nby, nbx, 2), dtype=np.int64)], [(0, 0, 0, 0)]
    for t in range(1, n):
        mv, sad = motion_ref.search_pair(luma_codes(noisy[t]), luma_codes(noisy[t - 1]), R)
        mvs.append(mv)
        stats.append((int(sad[..., 0].sum()), 0, 0, 0))
    limit = 255 * h * w if cut_limit is None else cut_limit
    return blend(noisy, None, np.stack(mvs), stats, h, w, strength, inv_of(threshold), limit)


def psnr(a, b):
    return 10.0 * np.log10(1.0 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
