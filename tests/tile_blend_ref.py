"""The two tile merges restated in float64 numpy, for tests/test_tile_blend_cpu.py and tests/test_gpu_tile_blend.py: the uniform average of
the reference's grids_inverse and the feathered merge of fdn_tiles_merge_w, out = sum(w_t x_t) / sum(w_t) with w_t = wy[t][dy] * wx[t][dx]."""
import numpy as np


def merge64(outs, idx, h, w, wy=None, wx=None):
    """outs [T,C,ch,cw], origins [(i, j)], optional weight vectors wy [T,ch] / wx [T,cw] (any float dtype; None: all ones, the average)
    -> (merged float64 [C,h,w], covering tiles per pixel int [h,w], largest |x| over the covering tiles float64 [C,h,w])"""
    outs = np.asarray(outs, dtype=np.float64)
    T, C, ch, cw = outs.shape
    acc, den = np.zeros((C, h, w)), np.zeros((h, w))
    cover, amax = np.zeros((h, w), dtype=np.int64), np.zeros((C, h, w))
    for t, (i, j) in enumerate(idx):
        wgt = np.ones((ch, cw)) if wy is None else np.outer(np.asarray(wy[t], dtype=np.float64), np.asarray(wx[t], dtype=np.float64))
        acc[:, i:i + ch, j:j + cw] += wgt * outs[t]
        den[i:i + ch, j:j + cw] += wgt
        cover[i:i + ch, j:j + cw] += 1
        amax[:, i:i + ch, j:j + cw] = np.maximum(amax[:, i:i + ch, j:j + cw], np.abs(outs[t]))
    assert cover.min() >= 1, "a pixel without a tile"
    return acc / den, cover, amax


def largest_step(img):
    """the largest difference between horizontally or vertically adjacent pixels of [C,h,w]"""
    return max(float(np.abs(np.diff(img, axis=1)).max(initial=0.0)), float(np.abs(np.diff(img, axis=2)).max(initial=0.0)))
