"""CPU: the definition and the host side of the motion-compensated temporal denoising.  The float32 numpy restatement of tests/mctf_ref.py
is held to the properties the definition promises (strength 0 only clamps; identical frames give k = strength; a pixel whose D reaches
the threshold is returned unchanged; the scene cut is `>`; one block is a four-term sum of one vector) and to its purpose: on a synthetic
noisy stream, still or moving, every filtered frame after the first is closer to the clean one than the noisy frame is.  The entry point of
include/fdn_mctf.h in libfdn_mctf.so is checked for its version, its generated prototype table and every argument refusal before any
launch; fdn_hip.mctf for its refusals without a device; and the command line of inference_fdn_video.py for the four new options.  No GPU
compute."""
import ctypes
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
import mctf_ref as ref
from fdn_hip import harness, mctf  # noqa: E402  (the module under test: without it nothing here has a subject)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
NAMES = ["fdn_mctf_abi_version", "fdn_mctf_blend"]
F = np.float32


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(mctf.lib_path()):
        entry.build()
    return mctf.lib()


def same_bits(a, b):
    return np.array_equal(ref.bits(a), ref.bits(b))


def random_case(h, w, B, seed, lo=-0.2, hi=1.2):
    g = np.random.default_rng(seed)
    nby, nbx = ref.block_grid(h, w)
    cur = g.uniform(lo, hi, size=(B, 3, h, w)).astype(F)
    prev = g.uniform(0.0, 1.0, size=(3, h, w)).astype(F)
    mv = g.integers(-9, 10, size=(B, nby, nbx, 2))
    return cur, prev, mv


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement, by its properties
# ---------------------------------------------------------------------------------------------------------------------------------
def test_clamp_and_weights():
    x = np.array([-0.5, -0.0, 0.25, 1.0, 1.5, np.nan, np.inf, -np.inf], dtype=F)
    assert ref.clamp01(x).tolist() == [0.0, 0.0, 0.25, 1.0, 1.0, 0.0, 1.0, 0.0]                # a NaN becomes 0
    b0, b1, w0, w1 = ref.axis_terms(40, 3)
    assert b0[:8].tolist() == [0] * 8 and b1[:8].tolist() == [0] * 8                            # above the first block's centre: one block twice
    assert (b0[8:24] == 0).all() and (b1[8:24] == 1).all() and (b0[24:40] == 1).all() and (b1[24:40] == 2).all()
    assert w1[8] == F(1 / 32) and w1[23] == F(31 / 32) and w1[24] == F(1 / 32) and w1[7] == F(31 / 32) and w1[0] == F(17 / 32)
    assert np.all(w0 + w1 == 1) and np.all((w1 * 32) % 1 == 0)
    # every product of two weights is a multiple of 1 / 1024 in (0, 1): exact in float32
    prod = (w0[:, None] * w1[None, :]).astype(np.float64) * 1024
    assert np.all(prod == np.rint(prod)) and np.all(prod == w0[:, None].astype(np.float64) * w1[None, :].astype(np.float64) * 1024)
    b0, b1, _, _ = ref.axis_terms(5, 1)
    assert not b0.any() and not b1.any()


def test_strength_zero_only_clamps():
    cur, prev, mv = random_case(18, 34, 2, seed=1)
    out, k = ref.blend(cur, prev, mv, [(0, 0, 0, 0)] * 2, 18, 34, 0.0, ref.inv_of(0.12), 10 ** 9)
    assert same_bits(out, ref.clamp01(cur)) and not k.any()
    assert out.min() == 0.0 and out.max() == 1.0                                                # the clamp acted


def test_identical_frames_zero_vectors_give_k_equal_strength():
    g = np.random.default_rng(2)
    one = g.uniform(0.0, 1.0, size=(3, 34, 50)).astype(F)
    cur = np.repeat(one[None], 3, axis=0)
    mv = np.zeros((3, 3, 4, 2), dtype=np.int64)
    out, k = ref.blend(cur, one, mv, [(0, 0, 0, 0)] * 3, 34, 50, 0.6, ref.inv_of(0.12), 0)
    # the four weighted terms sum to the frame up to their roundings (1e-7), so t * t is far below 2^-24 and 1 - t * t is 1 exactly
    assert np.all(k == F(0.6)) and np.abs(out.astype(np.float64) - cur).max() < 1e-6


def test_pixel_at_or_above_threshold_is_unchanged():
    """cur = prev + a step of 0.25 over the right half, zero vectors, threshold 0.125 (its reciprocal, 8, is exact): up to roundings of
    1e-7, d = 0.25 on the right and 0 on the left, so D is 0.25 deep in the right half, 0 deep in the left half, and 1/3 and 2/3 of 0.25 in
    the two columns at the step.  D >= threshold gives k = 0 and the pixel back unchanged; D = 0.25 / 3 lies below the threshold"""
    h, w = 20, 40
    g = np.random.default_rng(3)
    prev = g.uniform(0.0, 0.5, size=(3, h, w)).astype(F)
    cur = prev.copy()
    cur[:, :, w // 2:] += F(0.25)
    mv = np.zeros((1, 2, 3, 2), dtype=np.int64)
    out, k, D, pred = ref.blend_frame(ref.clamp01(cur), prev, mv[0], 0.6, ref.inv_of(0.125))
    assert np.abs(pred.astype(np.float64) - prev).max() < 5e-7
    hot = D >= F(0.125)
    assert hot[:, w // 2:].all() and not hot[:, :w // 2].any()                                  # 2/3 of 0.25 is above 0.125, 1/3 below
    assert not k[hot].any() and same_bits(out[:, hot], cur[:, hot])
    assert np.all(k[:, :w // 2 - 1] == F(0.6))
    edge = k[:, w // 2 - 1]                                                                     # t = 2/3: k = 0.6 * 5/9
    assert np.all(np.abs(edge - 0.6 * 5 / 9) < 1e-5)
    # a threshold of 0.0625 = 1 / 16 catches the left column of the step too: 0.25 / 3 >= 0.0625
    out, k, D, _ = ref.blend_frame(ref.clamp01(cur), prev, mv[0], 0.6, ref.inv_of(0.0625))
    hot = D >= F(0.0625)
    assert hot[:, w // 2 - 1:].all() and not hot[:, :w // 2 - 1].any() and not k[hot].any() and same_bits(out[:, hot], cur[:, hot])


def test_scene_cut_is_strictly_above_the_limit():
    cur, prev, mv = random_case(18, 34, 3, seed=4, lo=0.0, hi=1.0)
    limit = 1234
    out, k = ref.blend(cur, prev, mv, [(limit, 0, 0, 0), (limit + 1, 9, 9, 9), (limit, 0, 0, 0)], 18, 34, 0.6, ref.inv_of(1.0), limit)
    assert k[0].all() and not same_bits(out[0], cur[0])                                         # at the limit: filtered (D < 1 = threshold)
    assert not k[1].any() and same_bits(out[1], cur[1])                                         # one above: a cut, returned unchanged
    want = ref.blend_frame(cur[2], cur[1], mv[2], 0.6, ref.inv_of(1.0))[0]
    assert same_bits(out[2], want)                                                              # and the next frame is filtered against it
    # no predecessor at all: frame 0 is returned clamped, frame 1 filtered against it
    out0, k0 = ref.blend(cur, None, mv, [(0, 0, 0, 0)] * 3, 18, 34, 0.6, ref.inv_of(1.0), limit)
    assert not k0[0].any() and same_bits(out0[0], cur[0]) and k0[1].all()


def test_one_block_is_a_four_term_sum_of_one_vector():
    """nby = nbx = 1: both blocks of every pixel are block 0, so pred is the sum of the four weighted copies of one shifted frame - in float32,
    term by term, not the shifted frame itself"""
    h, w = 11, 14
    g = np.random.default_rng(5)
    P = g.uniform(0.0, 1.0, size=(3, h, w)).astype(F)
    for dy, dx in ((0, 0), (2, -3), (-32768, 32767), (32767, -32768)):
        pred = ref.predict(P, np.array([[[dy, dx]]]), h, w)
        sy, sx = np.clip(np.arange(h) + dy, 0, h - 1), np.clip(np.arange(w) + dx, 0, w - 1)
        S = P[:, sy][:, :, sx]
        _, _, wy0, wy1 = ref.axis_terms(h, 1)
        _, _, wx0, wx1 = ref.axis_terms(w, 1)
        want = np.zeros_like(S)
        for wy in (wy0, wy1):
            for wx in (wx0, wx1):
                want = want + (wy[:, None] * wx[None, :])[None] * S
        assert same_bits(pred, want)
        assert np.abs(pred.astype(np.float64) - S).max() < 5e-7                                 # the weights sum to 1: S up to four roundings


@pytest.mark.parametrize("step", [(0, 0), (2, -3)], ids=["static", "moving"])
@pytest.mark.parametrize("sigma", [0.02, 0.05])
def test_filter_helps_on_the_synthetic_stream(sigma, step):
    """a smooth random texture of 48 x 80 cropped from a larger one, 8 frames, the crop still or moving by (2, -3) a frame, iid Gaussian
    noise added and clipped; vectors from motion_ref.search_pair on rint(255 luma) of the NOISY frames, R = 8; the defaults.  From the
    second frame on the filtered frame is closer to the clean one than the noisy frame is.  (DESIGN.md records the figures.)"""
    clean, noisy = ref.noisy_stream(8, 48, 80, step, sigma, seed=7)
    out, k = ref.filter_stream(noisy, 0.6, 0.12)
    noisy_db = [ref.psnr(noisy[t], clean[t]) for t in range(8)]
    out_db = [ref.psnr(out[t], clean[t]) for t in range(8)]
    print(f"sigma {sigma} step {step}: " + ", ".join(f"{a:.2f} -> {b:.2f}" for a, b in zip(noisy_db, out_db)) + f"; mean k {k[1:].mean():.3f}")
    assert same_bits(out[0], noisy[0]) and not k[0].any()
    for t in range(1, 8):
        assert out_db[t] > noisy_db[t], (t, noisy_db[t], out_db[t])


# ---------------------------------------------------------------------------------------------------------------------------------
# the library's host side
# ---------------------------------------------------------------------------------------------------------------------------------
def test_version_and_generated_table(lib, monkeypatch):
    spec = importlib.util.spec_from_file_location("gen_abi_table", os.path.join(ROOT, "tools", "gen_abi_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    from fdn_hip import _abi_mctf as table
    protos, names, members, versions = gen.build_table(headers=["fdn_mctf.h"])
    assert table.PROTOTYPES == protos and table.ARG_NAMES == names and list(protos) == members["fdn_mctf.h"] == NAMES
    assert table.VERSION == versions["fdn_mctf.h"] == ("fdn_mctf_abi_version", 1)
    assert "fdn_mctf.h" not in gen.HEADERS                                         # the one table of libfdn_hip.so stays what it was
    assert lib.fdn_mctf_abi_version() == 1 == mctf.ABI_VERSION
    assert lib.fdn_mctf_blend.argtypes == [ctypes.c_void_p] * 6 + [ctypes.c_int] * 5 + [ctypes.c_float] * 2 + [ctypes.c_long, ctypes.c_void_p]
    assert table.ARG_NAMES["fdn_mctf_blend"] == ["cur", "prev", "mv", "stats", "out", "kmap", "B", "h", "w", "H", "W", "strength", "inv_threshold",
                                                 "cut_limit", "stream"]
    import fdn_hip
    from fdn_hip import correct, fusion, motion, sharpness
    for other in (fdn_hip.lib(), correct.lib(), sharpness.lib(), fusion.lib(), motion.lib()):   # no other library holds the entry point
        assert not hasattr(other, "fdn_mctf_blend") and not hasattr(other, "fdn_mctf_abi_version")
    monkeypatch.setattr(mctf, "_lib", None)
    monkeypatch.setattr(mctf, "ABI_VERSION", 2)
    with pytest.raises(ImportError, match=r"libfdn_mctf\.so has mctf ABI version 1, this binding needs 2: rebuild with build\.sh"):
        mctf.lib()
    assert mctf._lib is None


GOOD = dict(B=2, h=34, w=50, H=64, W=64, strength=0.6, inv_threshold=8.0, cut_limit=1000)
BAD = [dict(B=0), dict(B=-1), dict(B=65536), dict(h=0), dict(w=0), dict(h=-2), dict(w=-4), dict(H=33), dict(W=49), dict(H=0), dict(W=-1),
       dict(h=32768, w=32768, H=32768, W=32768), dict(h=1, w=2 ** 30, H=1, W=2 ** 30), dict(h=2, w=2 ** 29, H=2, W=2 ** 29),
       dict(strength=-0.001), dict(strength=1.001), dict(strength=math.nan), dict(strength=math.inf), dict(strength=-math.inf),
       dict(inv_threshold=0.0), dict(inv_threshold=-8.0), dict(inv_threshold=math.inf), dict(inv_threshold=-math.inf),
       dict(inv_threshold=math.nan), dict(cut_limit=-1), dict(cut_limit=-2 ** 63)]


def check_argument_errors(lib):
    """every refusal of include/fdn_mctf.h returns FDN_ERR_ARG = 1 before any launch (the pointers are never dereferenced, and a machine
    without a GPU has nothing to launch on)"""
    p = ctypes.c_void_p(64)                                                        # never dereferenced

    def blend(ptrs=None, **kw):
        a = {**GOOD, **kw}
        q = dict(cur=p, prev=p, mv=p, stats=p, out=p, kmap=p)
        q.update(ptrs or {})
        return lib.fdn_mctf_blend(q["cur"], q["prev"], q["mv"], q["stats"], q["out"], q["kmap"], a["B"], a["h"], a["w"], a["H"], a["W"],
                                  a["strength"], a["inv_threshold"], a["cut_limit"], None)

    for bad in BAD:
        assert blend(**bad) == 1, bad
    for k in ("cur", "mv", "stats", "out"):
        assert blend({k: None}) == 1, k
        assert blend({k: None, "prev": None, "kmap": None}) == 1, k


def test_entry_point_validates_arguments_without_gpu(lib):
    check_argument_errors(lib)


def test_module_refuses_without_a_device(lib):
    from fdn_hip import FdnHipError
    fmt = harness.VideoFormat("yuv420p")
    cur = torch.zeros((2, 3, 64, 64))
    mv = torch.zeros((2, 3, 4, 2), dtype=torch.int16)
    stats = torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(FdnHipError, match="ROCm"):                                  # no host fallback
        mctf.blend(cur, None, mv, stats, 34, 50, 0.6, 0.12, 0)
    with pytest.raises(FdnHipError, match="cannot filter 65x50"):
        mctf.blend(cur, None, mv, stats, 65, 50, 0.6, 0.12, 0)
    with pytest.raises(FdnHipError, match="cur must be a float32 tensor"):
        mctf.blend(cur.double(), None, mv, stats, 34, 50, 0.6, 0.12, 0)
    for strength in (-0.1, 1.5, math.nan, None, True, "0.5"):
        with pytest.raises(ValueError, match="denoise strength"):
            mctf.blend(cur, None, mv, stats, 34, 50, strength, 0.12, 0)
        with pytest.raises(ValueError, match="denoise strength"):
            mctf.TemporalDenoiser(34, 50, fmt, strength=strength, device="cpu")
    for threshold in (0.0, -1.0, math.inf, math.nan, None, True, 1e-50, 1e50):       # the last two: the reciprocal leaves float32
        with pytest.raises(ValueError, match="denoise threshold"):
            mctf.blend(cur, None, mv, stats, 34, 50, 0.6, threshold, 0)
        with pytest.raises(ValueError, match="denoise threshold"):
            mctf.TemporalDenoiser(34, 50, fmt, threshold=threshold, device="cpu")
    with pytest.raises(ValueError, match="cut_limit"):
        mctf.blend(cur, None, mv, stats, 34, 50, 0.6, 0.12, -1)
    for radius in (-1, 17, 2.0, None):
        with pytest.raises(ValueError, match="motion radius"):
            mctf.TemporalDenoiser(34, 50, fmt, radius=radius, device="cpu")
    for cut in (-0.1, 1.1):
        with pytest.raises(ValueError, match="denoise cut"):
            mctf.TemporalDenoiser(34, 50, fmt, cut=cut, device="cpu")
    for kw in (dict(h=33), dict(w=49), dict(h=0), dict(h=32768, w=32768)):
        args = dict(h=34, w=50)
        args.update(kw)
        with pytest.raises(ValueError):
            mctf.TemporalDenoiser(args["h"], args["w"], fmt, device="cpu")
    d = mctf.TemporalDenoiser(34, 50, fmt, device="cpu")
    assert (d.strength, d.threshold, d.radius, d.cut) == (0.6, 0.12, 8, 0.10) and d.cut_limit == math.floor(0.10 * 255 * 34 * 50) == 43350
    assert d.matches(34, 50, 8) and not d.matches(34, 50, 10) and not d.matches(50, 34, 8)
    assert mctf.TemporalDenoiser(34, 50, harness.VideoFormat("yuv420p10le"), cut=1.0, device="cpu").cut_limit == 1023 * 34 * 50
    with pytest.raises(FdnHipError, match="ROCm"):
        d.step(cur)
    assert mctf.inv_threshold(0.125) == 8.0 and mctf.inv_threshold(0.12) == float(ref.inv_of(0.12)) == float(F(1 / 0.12))
    assert "NOT tuned on footage" in mctf.TemporalDenoiser.__doc__                    # where the defaults come from is said
    src = open(os.path.join(PKG, "fdn_hip", "mctf.py")).read()
    assert "oracle" not in src and "tests" not in src.replace("tests/", "")           # the product path stands without the yardsticks


def test_enhance_refuses_a_denoiser_of_another_stream():
    fmt = harness.VideoFormat("yuv420p")
    d = mctf.TemporalDenoiser(34, 50, fmt, device="cpu")
    frames = torch.zeros((1, 36 * 50 * 3 // 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match="temporal denoiser is for 34x50 8-bit frames, these are 36x50 8-bit"):
        harness.enhance_yuv420(None, None, frames, 36, 50, fmt, denoise=d)


# ---------------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def test_command_line(capsys):
    sys.path.insert(0, PKG)
    import inference_fdn_video as tool
    base = ["--fdn", "f.pth", "--lpnet", "l.pth", "-", "-"]
    a = tool.parse_args(base)
    assert a.temporal_denoise is None and (a.denoise_threshold, a.denoise_radius, a.denoise_cut) == (0.12, 8, 0.10)
    a = tool.parse_args(base + ["--temporal-denoise", "0.6"])
    assert a.temporal_denoise == 0.6 and (a.denoise_threshold, a.denoise_radius, a.denoise_cut) == (0.12, 8, 0.10)
    a = tool.parse_args(base + ["--temporal-denoise", "1", "--denoise-threshold", "0.2", "--denoise-radius", "16", "--denoise-cut", "1"])
    assert (a.temporal_denoise, a.denoise_threshold, a.denoise_radius, a.denoise_cut) == (1.0, 0.2, 16, 1.0)
    assert tool.parse_args(base + ["--temporal-denoise", "0.5", "--denoise-radius", "0", "--denoise-cut", "0"]).denoise_radius == 0
    # the defaults are TemporalDenoiser's own
    d = mctf.TemporalDenoiser(34, 50, harness.VideoFormat("yuv420p"), device="cpu")
    assert tool.DENOISE_DEFAULTS == {"denoise_threshold": d.threshold, "denoise_radius": d.radius, "denoise_cut": d.cut}
    for extra in (["--temporal-denoise", "0"], ["--temporal-denoise", "1.5"], ["--temporal-denoise", "x"], ["--temporal-denoise"],
                  ["--denoise-threshold", "0.2"], ["--denoise-radius", "8"], ["--denoise-cut", "0.1"],
                  ["--temporal-denoise", "0.5", "--denoise-threshold", "0"], ["--temporal-denoise", "0.5", "--denoise-threshold", "inf"],
                  ["--temporal-denoise", "0.5", "--denoise-radius", "17"], ["--temporal-denoise", "0.5", "--denoise-radius", "-1"],
                  ["--temporal-denoise", "0.5", "--denoise-radius", "2.5"], ["--temporal-denoise", "0.5", "--denoise-cut", "1.5"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + extra)
        assert "denoise" in capsys.readouterr().err
