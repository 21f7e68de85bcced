"""Golden values for NIQE, the reference's no-reference metric (basicsr/metrics/niqe.py:1-205, calculate_niqe :158-205).
The function bodies are lifted out of the reference by AST (niqe.py: estimate_aggd_param, compute_feature, niqe, calculate_niqe;
metric_util.py: reorder_image, to_y_channel; utils/matlab_functions.py: bgr2ycbcr and its two range helpers; the modules
themselves import cv2, absent here) and executed with stand-ins for what they import:
  convolve      = scipy.ndimage.convolve (what niqe.py:4 imports);
  cv2.resize    = at exactly half size (the only size niqe.py:136 asks for) the 2x2 mean, ((a + b) + c) + d) * 0.25 in float32,
                  a, b the upper pair - both OpenCV routes (INTER_LINEAR and the INTER_AREA fast path it switches to) take the mean;
                  the order of OpenCV's float32 adds is not pinned here and is left to the tolerance;
  cv2.cvtColor  = COLOR_BGR2GRAY per OpenCV's documentation, Y = 0.299 R + 0.587 G + 0.114 B, summed B, G, R in float32.
calculate_niqe loads its parameters from a relative path (niqe.py:186), so the lift runs with the reference checkout as the working
directory; the same parameters are stored next to this file as niqe_pris_params.npz (a data fixture).  The input frames are not
stored: tests/niqe_ref.py synth_u8 makes them again, bit for bit, from integer arithmetic.
Run:  python tests/golden/make_golden_niqe.py"""
import ast
import contextlib
import json
import os
import shutil
import sys
import types
import warnings
import zlib

import numpy as np
import scipy.ndimage
import scipy.special

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _refload import REF_ROOT  # noqa: E402
from niqe_ref import synth_u8  # noqa: E402

COLOR_BGR2GRAY = 6
INTER_LINEAR = 1


def resize_half(img, dsize, interpolation=None):
    w2, h2 = dsize
    assert img.dtype == np.float32 and img.shape == (2 * h2, 2 * w2) and interpolation == INTER_LINEAR
    a, b, c, d = img[0::2, 0::2], img[0::2, 1::2], img[1::2, 0::2], img[1::2, 1::2]
    return (((a + b) + c) + d) * np.float32(0.25)


def cvt_color(img, code):
    assert code == COLOR_BGR2GRAY and img.ndim == 3 and img.shape[2] == 3
    img = img.astype(np.float32)
    return (img[..., 0] * np.float32(0.114) + img[..., 1] * np.float32(0.587)) + img[..., 2] * np.float32(0.299)


def lift(path, names, ns):
    tree = ast.parse(open(path).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(fns) == len(names), (path, names)
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)


@contextlib.contextmanager
def cwd(path):
    old = os.getcwd()
    os.chdir(path)
    try:
        yield
    finally:
        os.chdir(old)


def lifted():
    ns = {"np": np, "math": __import__("math"), "convolve": scipy.ndimage.convolve, "gamma": scipy.special.gamma,
          "cv2": types.SimpleNamespace(resize=resize_half, INTER_LINEAR=INTER_LINEAR, cvtColor=cvt_color, COLOR_BGR2GRAY=COLOR_BGR2GRAY)}
    lift(os.path.join(REF_ROOT, "basicsr", "utils", "matlab_functions.py"), ("bgr2ycbcr", "_convert_input_type_range", "_convert_output_type_range"), ns)
    lift(os.path.join(REF_ROOT, "basicsr", "metrics", "metric_util.py"), ("reorder_image", "to_y_channel"), ns)
    lift(os.path.join(REF_ROOT, "basicsr", "metrics", "niqe.py"), ("estimate_aggd_param", "compute_feature", "niqe", "calculate_niqe"), ns)
    return ns


def main():
    ns = lifted()
    rec = {}
    niqe0, feat0 = ns["niqe"], ns["compute_feature"]

    def niqe_rec(img, *a, **k):
        rec["plane"] = img.copy()
        return niqe0(img, *a, **k)

    def feat_rec(block):
        f = feat0(block)
        rec.setdefault("blocks", []).append(block.copy())
        rec.setdefault("feats", []).append(f)
        return f

    ns["niqe"], ns["compute_feature"] = niqe_rec, feat_rec
    # The inputs are not stored: each is a window of a synth_u8 frame (tests/niqe_ref.py, integer arithmetic only), named in meta "src"
    # as [seed, frame h, frame w, dark, channel or None, y0, x0, h, w], with a CRC-32 of the frame.  The Y plane and both MSCN planes
    # are stored for "planes" alone (1 x 3 blocks: every edge of the plane inside one row of blocks).
    big, dark = (2025, 480, 672, False), (2026, 384, 576, True)
    cases = (  # name, src, crop_border, input_order, convert_to
        ("tex", big + (None, 0, 0, 288, 480), 0, "CHW", "y"),
        ("crop", big + (None, 180, 172, 300, 500), 4, "CHW", "y"),      # 292 x 492 after the crop: not a multiple of 96
        ("dark", dark + (None, 0, 0, 384, 576), 0, "CHW", "y"),
        ("hw", big + (1, 0, 0, 288, 480), 0, "HW", "y"),                # a grey (H, W) input: the G plane of "tex"
        ("gray", big + (None, 0, 0, 288, 480), 0, "CHW", "gray"),
        ("big", big + (None, 0, 0, 480, 672), 0, "CHW", "y"),
        ("planes", big + (None, 96, 192, 96, 288), 0, "CHW", "y"),
    )
    out, meta = {}, {}
    with cwd(REF_ROOT), warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)       # the empty means of the NaN blocks, as the reference's script does
        for name, src, border, order, conv in cases:
            seed, fh, fw, dk, c, y0, x0, h, w = src
            frame = synth_u8(seed, fh, fw, dk)
            img = frame[:, y0:y0 + h, x0:x0 + w] if c is None else frame[c, y0:y0 + h, x0:x0 + w]
            rec.clear()
            q = ns["calculate_niqe"](img, border, input_order=order, convert_to=conv)
            feats = np.array(rec["feats"], dtype=np.float64)
            nb = feats.shape[0] // 2
            dist = np.concatenate([feats[:nb], feats[nb:]], axis=1)
            dropped = np.nonzero(np.isnan(dist).any(axis=1))[0]
            meta[name] = {"src": src, "crc32": zlib.crc32(frame.tobytes()), "crop_border": border, "input_order": order, "convert_to": conv, "niqe": float(np.asarray(q).item()),
                          "dropped_rows": dropped.tolist()}
            out[name + "_feat1"], out[name + "_feat2"] = feats[:nb], feats[nb:]
            if name == "planes":
                ph, pw = rec["plane"].shape
                nbh, nbw = ph // 96, pw // 96
                for s, bs, blocks in ((1, 96, rec["blocks"][:nb]), (2, 48, rec["blocks"][nb:])):
                    m = np.empty((nbh * bs, nbw * bs), dtype=np.float32)
                    for i, blk in enumerate(blocks):                    # block order: idx_w outer, idx_h inner (niqe.py:120-121)
                        bw, bh = divmod(i, nbh)
                        m[bh * bs:(bh + 1) * bs, bw * bs:(bw + 1) * bs] = blk
                    out[f"planes_mscn{s}"] = m
                out["planes_y"] = rec["plane"]
            print(name, meta[name], "nan rows", len(dropped), "of", nb)
    out["cases_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "niqe.npz"), **out)
    shutil.copyfile(os.path.join(REF_ROOT, "basicsr", "metrics", "niqe_pris_params.npz"), os.path.join(HERE, "niqe_pris_params.npz"))


if __name__ == "__main__":
    main()
