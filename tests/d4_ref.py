"""The self-ensemble of include/fdn_ensemble.h restated with numpy / torch index operations, for tests/test_ensemble_cpu.py and
tests/test_gpu_ensemble.py: the eight transforms and their inverses, the reflect-pad rule, and the ordered fp32 mean."""
import numpy as np
import torch

MASKS = {1: 0x01, 2: 0x03, 4: 0x0F, 8: 0xFF}


def codes(mask):
    return [k for k in range(8) if mask >> k & 1]


def _ops(a):
    if isinstance(a, torch.Tensor):
        return (lambda t, ax: t.flip(ax)), (lambda t, r, c: t.transpose(r, c))
    return (lambda t, ax: np.flip(t, ax)), (lambda t, r, c: np.swapaxes(t, r, c))


def transform(a, k, axes):
    """T_k of a (numpy array or torch tensor) over axes = (rows, cols): mirror the columns if k & 1, the rows if k & 2, then transpose
    if k & 4"""
    rows, cols = axes
    flip, swap = _ops(a)
    t = a
    if k & 1:
        t = flip(t, cols)
    if k & 2:
        t = flip(t, rows)
    if k & 4:
        t = swap(t, rows, cols)
    return t


def inverse(a, k, axes):
    """T_k^-1: transpose first, then the same mirrors"""
    rows, cols = axes
    flip, swap = _ops(a)
    t = a
    if k & 4:
        t = swap(t, rows, cols)
    if k & 1:
        t = flip(t, cols)
    if k & 2:
        t = flip(t, rows)
    return t


def d4_shape(k, h, w):
    return (w, h) if k & 4 else (h, w)


def reflect_index(n, N):
    """the source index of each of N outputs along an axis of length n: i < n ? i : 2 (n - 1) - i (F.pad mode='reflect', bottom / right)"""
    i = np.arange(N)
    assert N - n < n, "reflect padding needs pad < size"
    return np.where(i < n, i, 2 * (n - 1) - i)


def reflect_pad(t, H, W):
    """torch tensor [..., h, w] -> [..., H, W], reflected bottom / right"""
    h, w = t.shape[-2:]
    iy, ix = torch.from_numpy(reflect_index(h, H)), torch.from_numpy(reflect_index(w, W))
    return t.index_select(-2, iy).index_select(-1, ix)


def ordered_mean(terms):
    """fp32 tensors of one shape -> ((t0 + t1) + t2 ...) / float32(K): every add and the one division rounded to fp32"""
    acc = terms[0].clone()
    assert acc.dtype == torch.float32
    for t in terms[1:]:
        acc = acc + t
    return acc / torch.tensor(float(len(terms)), dtype=torch.float32)


def mean_back(results, mask, h, w):
    """results: {k: fp32 tensor [B,3,>=h',>=w']} for the codes of mask -> [B,3,h,w]: crop, T_k^-1, ordered mean in ascending k"""
    terms = []
    for k in codes(mask):
        hp, wp = d4_shape(k, h, w)
        terms.append(inverse(results[k][..., :hp, :wp], k, (-2, -1)).contiguous())
    return ordered_mean(terms)
