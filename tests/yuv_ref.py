"""float64 restatement of the video frame conversions (include/fdn_video.h): Y'CbCr 4:2:0 frames <-> R'G'B' planes, written from the
formulas of DESIGN.md with numpy, sample positions as coordinates rather than as the kernels' cases.  The yardstick of tests/test_gpu_yuv.py;
tests/test_yuv_cpu.py judges it on its own."""
import numpy as np

PIX_FMTS = {"yuv420p": (0, 8), "nv12": (1, 8), "yuv420p10le": (0, 10)}       # -> (layout, bits)
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}            # -> (Kr, Kb)


def sample_dtype(pix_fmt):
    return np.uint8 if PIX_FMTS[pix_fmt][1] == 8 else np.uint16


def unpack(frames, h, w, pix_fmt):
    """frames [B, h*w*3/2] -> integer planes y [B,h,w], u, v [B,h/2,w/2]"""
    B = frames.shape[0]
    frames = frames.astype(np.int64)
    y = frames[:, :h * w].reshape(B, h, w)
    c = frames[:, h * w:]
    if PIX_FMTS[pix_fmt][0] == 1:
        c = c.reshape(B, h // 2, w // 2, 2)
        return y, c[..., 0], c[..., 1]
    c = c.reshape(B, 2, h // 2, w // 2)
    return y, c[:, 0], c[:, 1]


def pack(y, u, v, pix_fmt):
    """planes -> frames [B, h*w*3/2] of the format's sample type"""
    B = y.shape[0]
    c = np.stack([u, v], axis=-1) if PIX_FMTS[pix_fmt][0] == 1 else np.stack([u, v], axis=1)
    return np.concatenate([y.reshape(B, -1), c.reshape(B, -1)], axis=1).astype(sample_dtype(pix_fmt))


def _ranges(bits, full_range):
    """(luma offset, luma scale, chroma offset, chroma scale) in codes"""
    s, top = 2.0 ** (bits - 8), 2.0 ** bits - 1
    return (0.0, top, 2.0 ** (bits - 1), top) if full_range else (16 * s, 219 * s, 128 * s, 224 * s)


def _taps(n_luma, n_chroma, offset):
    """Linear interpolation of chroma samples sitting at luma coordinate 2 k + offset, at every luma coordinate 0 .. n_luma - 1:
    -> (lower index, upper index, weight of the upper), indices clamped to the frame"""
    pos = (np.arange(n_luma, dtype=np.float64) - offset) / 2.0
    lo = np.floor(pos)
    frac = pos - lo
    lo = lo.astype(np.int64)
    return np.clip(lo, 0, n_chroma - 1), np.clip(lo + 1, 0, n_chroma - 1), frac


def _reflect(n, N):
    """source index of every padded index: F.pad(mode='reflect') bottom / right"""
    i = np.arange(N)
    return np.where(i < n, i, 2 * (n - 1) - i)


def pre64(frames, h, w, H, W, pix_fmt, matrix, full_range, chroma_loc):
    """frames -> float64 [B,3,H,W] R', G', B' in [0,1], the padding the reflection of the converted image"""
    bits = PIX_FMTS[pix_fmt][1]
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    y, u, v = unpack(np.minimum(frames.astype(np.int64), 2 ** bits - 1), h, w, pix_fmt)
    yo, ys, co, cs = _ranges(bits, full_range)
    Y = (y - yo) / ys
    jl, ju, jf = _taps(h, h // 2, 0.5)                                       # chroma row j sits on luma row 2 j + 0.5
    kl, ku, kf = _taps(w, w // 2, 0.0 if chroma_loc == "left" else 0.5)

    def up(c):
        c = (c - co) / cs
        rows = c[:, jl] * (1 - jf)[None, :, None] + c[:, ju] * jf[None, :, None]
        return rows[:, :, kl] * (1 - kf) + rows[:, :, ku] * kf
    Cb, Cr = up(u), up(v)
    R = Y + 2 * (1 - kr) * Cr
    Bl = Y + 2 * (1 - kb) * Cb
    G = Y - (2 * kb * (1 - kb) / kg) * Cb - (2 * kr * (1 - kr) / kg) * Cr
    rgb = np.clip(np.stack([R, G, Bl], axis=1), 0.0, 1.0)
    return rgb[:, :, _reflect(h, H)][:, :, :, _reflect(w, W)]


def post64(res, h, w, pix_fmt, matrix, full_range, chroma_loc):
    """[B,3,H,W] -> (frames [B, h*w*3/2] of codes, float64 [B, h*w*3/2]: the values before rounding, in code units)"""
    bits = PIX_FMTS[pix_fmt][1]
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    rgb = np.clip(res[:, :, :h, :w].astype(np.float64), 0.0, 1.0)           # the crop first: nothing below sees the padding
    R, G, Bl = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    Y = kr * R + kg * G + kb * Bl
    yo, ys, co, cs = _ranges(bits, full_range)

    def down(c):
        c = (c[:, 0::2] + c[:, 1::2]) / 2
        if chroma_loc == "center":
            return (c[:, :, 0::2] + c[:, :, 1::2]) / 2
        k = np.arange(0, w, 2)
        return (c[:, :, np.clip(k - 1, 0, w - 1)] + 2 * c[:, :, k] + c[:, :, np.clip(k + 1, 0, w - 1)]) / 4
    Cb, Cr = down((Bl - Y) / (2 * (1 - kb))), down((R - Y) / (2 * (1 - kr)))
    B = res.shape[0]
    planes = [Y * ys + yo, Cb * cs + co, Cr * cs + co]
    c = np.stack(planes[1:], axis=-1) if PIX_FMTS[pix_fmt][0] == 1 else np.stack(planes[1:], axis=1)
    exact = np.concatenate([planes[0].reshape(B, -1), c.reshape(B, -1)], axis=1)
    return np.clip(np.rint(exact), 0, 2 ** bits - 1).astype(sample_dtype(pix_fmt)), exact


def near_tie(exact, window=1e-3):
    """where the value before rounding lies within `window` code units of a half"""
    return np.abs(exact - np.floor(exact) - 0.5) <= window


def random_frames(seed, B, h, w, pix_fmt, lo=0, hi=None):
    """codes uniform over [lo, hi] (default: the whole code range)"""
    bits = PIX_FMTS[pix_fmt][1]
    hi = 2 ** bits - 1 if hi is None else hi
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(B, h * w * 3 // 2)).astype(sample_dtype(pix_fmt))


def random_planes(seed, B, H, W):
    """float32 [B,3,H,W] uniform in [-0.2, 1.2]: the input of the post tests"""
    return (np.random.default_rng(seed).random((B, 3, H, W)) * 1.4 - 0.2).astype(np.float32)


# shapes of the GPU tests: (h, w, H, W, B)
SHAPES = [(2, 2, 2, 2, 1), (2, 4, 2, 4, 1), (18, 22, 32, 32, 1), (34, 38, 64, 64, 1), (34, 514, 64, 544, 2)]
FORMATS = [(p, m, f, c) for p in PIX_FMTS for m in MATRICES for f in (False, True) for c in ("left", "center")]
POST_SEED = 0
