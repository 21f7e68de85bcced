"""Restatement of the ratio filter across frames (include/fdn_temporal.h), written from its specification with numpy and plain loops: the
luma histogram as np.bincount on the clamped, shifted luma plane, the histograms' distance in integers, the filter in np.float32 with one
rounding per operation.  The yardstick of tests/test_gpu_temporal.py; tests/test_temporal_cpu.py judges it on its own."""
import numpy as np

STATE_WORDS = 258            # [0..255] last histogram, [256] bits of the last finite filtered ratio, [257] flags: 1 has a frame, 2 has a ratio


def luma_hist(frames, h, w, bits):
    """frames [B, h*w*3/2] (uint8, or uint16 for 10 bit) -> uint32 [B, 256]: only the first h*w samples of a frame count"""
    y = frames[:, :h * w].astype(np.int64)
    if bits == 10:
        y = np.minimum(y, 1023)
    y >>= bits - 8
    return np.stack([np.bincount(row, minlength=256) for row in y]).astype(np.uint32)


def zero_state():
    return np.zeros(STATE_WORDS, dtype=np.uint32)


def cut_above(cut, h, w):
    """floor(cut * 2 h w) with cut taken as the exact value of the double"""
    from fractions import Fraction
    import math
    return math.floor(Fraction(float(cut)) * (2 * h * w))


def _bits(f):
    return np.array([f], dtype=np.float32).view(np.uint32)[0]


def _float(u):
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def smooth(hist, ratio, state, alpha, cut_above):
    """-> (ratio_out float32 [B], dist uint32 [B], cut int32 [B], the state after these frames); `state` is left as it is"""
    hist = np.asarray(hist, dtype=np.uint32)
    ratio = np.asarray(ratio, dtype=np.float32)
    state = np.array(state, dtype=np.uint32)
    alpha = np.float32(alpha)
    B = hist.shape[0]
    out, dist, cut = np.empty(B, np.float32), np.zeros(B, np.uint32), np.zeros(B, np.int32)
    has_frame, has_ratio = bool(state[257] & 1), bool(state[257] & 2)
    prev_hist, prev = state[:256].astype(np.int64), _float(state[256])
    with np.errstate(all="ignore"):
        for t in range(B):
            cur = hist[t].astype(np.int64)
            d = int(np.abs(cur - prev_hist).sum()) if has_frame else 0
            dist[t] = d
            cut[t] = 1 if (not has_frame or d > cut_above) else 0
            r = ratio[t]
            o = r
            if not cut[t] and has_ratio and np.isfinite(r) and alpha != np.float32(1):
                diff = np.float32(r - prev)                       # float32 operands: each operation rounds once
                move = np.float32(alpha * diff)
                o = np.float32(prev + move)
            out[t] = o
            if np.isfinite(o):
                prev, has_ratio = o, True
            prev_hist, has_frame = cur, True
    state[:256] = prev_hist
    if has_ratio:
        state[256] = _bits(prev)
    state[257] = 1 | (2 if has_ratio else 0)
    return out, dist, cut, state


def scene_frames(seed=7, h=34, w=38, bits=8):
    """Four yuv420p frames [4, h*w*3/2]: two of one random dark image with noise of +-1 code (x 2^(bits - 8)), then two of another, brighter
    one: a cut at frame 0 (the first) and at frame 2"""
    s = 2 ** (bits - 8)
    rng = np.random.default_rng(seed)
    frames = []
    for lo, hi in ((20, 70), (90, 140)):
        y = rng.integers(lo * s, hi * s, size=h * w)
        c = rng.integers(120 * s, 136 * s, size=h * w // 2)
        for _ in range(2):
            frames.append(np.concatenate([y + rng.integers(-s, s + 1, size=h * w), c]))
    return np.stack(frames).astype(np.uint8 if bits == 8 else np.uint16)
