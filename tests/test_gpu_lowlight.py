"""GPU: the low-light evaluation (include/fdn_lowlight.h, fdn_hip.lowlight) against the numpy restatement of tests/lowlight_ref.py.
LOE is an integer and must be EQUAL to the restatement's (which tests/test_lowlight_cpu.py ties to the brute-force pair count).
CIEDE2000 is a float64 formula; its bound is formed here from the restatement's own error: E = the largest |float64 - longdouble| of the
restatement on the case's inputs, and every per-pixel value of the device must lie within 32 max(E, 1.5e-14) of the float64 restatement
(1.5e-14: one float64 ulp at dE = 100; 32: a device maths library good to a few ulp rather than correctly rounded, over about ten chained
calls per pixel).  The per-pixel float64 values are read by scoring every pixel as a 1 x 1 image of a batch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
import lowlight_ref as ref
from common import fdn_weights

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fdn-tip2025_amd")

DEV = "cuda:0"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def rand_pair(h, w, seed, lo=0, hi=256):
    g = np.random.default_rng(seed)
    return g.integers(lo, hi, (h, w, 3), dtype=np.uint8), g.integers(lo, hi, (h, w, 3), dtype=np.uint8)


# ---- LOE ----
LOE_SHAPES = [(37, 53, 0), (16, 16, 50), (51, 50, 50), (64, 90, 50), (120, 67, 50), (96, 160, 0), (512, 512, 0)]


@pytest.mark.parametrize("shape", LOE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-size{s[2]}")
def test_loe_equals_the_restatement(shape):
    """a dark image against its brightened version and two unrelated images: numerator and m as integers, the map sample by sample"""
    from fdn_hip import lowlight
    h, w, size = shape
    for a, b in (ref.dark_pair(h, w, 11), rand_pair(h, w, 12)):
        want = ref.loe_hist(a, b, size)
        num, m = lowlight.loe_counts_u8(dev(a[None]), dev(b[None]), size)
        assert (num[0], m) == want, (num, m, want)
        assert lowlight.loe_u8(dev(a[None]), dev(b[None]), size) == [want[0] / want[1]]
        rd = lowlight.loe_map_u8(dev(a[None]), dev(b[None]), size)
        md, nd = ref.sample_dims(h, w, size)
        assert rd.dtype == torch.uint32 and tuple(rd.shape) == (1, md, nd)
        got = rd.cpu().numpy().astype(np.int64)[0]
        assert (got == ref.loe_map(a, b, size)).all() and int(got.sum()) == want[0]
    if shape == (512, 512, 0):
        assert ref.loe_hist(*rand_pair(h, w, 12), 0)[0] > 2 ** 32              # the sums this shape is here for


def test_loe_batch_slots_do_not_leak():
    """B = 3 with three different pairs: every slot equals the pair scored alone and the restatement, at a sampled and at the full grid"""
    from fdn_hip import lowlight
    pairs = [ref.dark_pair(64, 90, 21), rand_pair(64, 90, 22), rand_pair(64, 90, 23, 100, 140)]
    a, b = dev(np.stack([p[0] for p in pairs])), dev(np.stack([p[1] for p in pairs]))
    for size in (50, 0):
        num, m = lowlight.loe_counts_u8(a, b, size)
        assert [(n, m) for n in num] == [ref.loe_hist(x, y, size) for x, y in pairs]
        assert num == [lowlight.loe_counts_u8(a[k:k + 1], b[k:k + 1], size)[0][0] for k in range(3)]
        rd = lowlight.loe_map_u8(a, b, size).cpu().numpy().astype(np.int64)
        assert rd.shape == (3,) + ref.sample_dims(64, 90, size)
        for k, (x, y) in enumerate(pairs):
            assert (rd[k] == ref.loe_map(x, y, size)).all()


def test_loe_launch_zeroes_its_own_workspace():
    """the same call twice on ONE workspace, then another pair on it, then the first again, through the C interface: the counts do not pile up"""
    import ctypes
    import fdn_hip
    lib, h, w = fdn_hip.lib(), 37, 53
    (a1, b1), (a2, b2) = ref.dark_pair(h, w, 31), rand_pair(h, w, 32)
    ws = torch.full((lib.fdn_loe_ws(1, h, w, 0),), -1, dtype=torch.int64, device=DEV)           # no caller-zeroed memory
    out = torch.zeros((1, 2), dtype=torch.int64, device=DEV)
    got = []
    for a, b in ((a1, b1), (a1, b1), (a2, b2), (a1, b1)):
        ta, tb = dev(a[None]), dev(b[None])
        fdn_hip.check(lib.fdn_loe_u8(ctypes.c_void_p(ta.data_ptr()), ctypes.c_void_p(tb.data_ptr()), 1, h, w, 0, ctypes.c_void_p(ws.data_ptr()),
                                     ctypes.c_void_p(out.data_ptr()), fdn_hip.stream()), "fdn_loe_u8")
        got.append(tuple(out.cpu().tolist()[0]))
    w1, w2 = ref.loe_hist(a1, b1, 0), ref.loe_hist(a2, b2, 0)
    assert got == [w1, w1, w2, w1]
    # the tables stay in the workspace as the header lays them out: J, C, R, K as uint32
    t = ws.cpu().numpy().view(np.uint32)
    J, C, R, K = ref.loe_tables(*ref.loe_sets(a1, b1, 0))
    assert (t[:65536].reshape(256, 256) == J).all() and (t[65536:131072].reshape(256, 256) == C).all()
    assert (t[131072:131328] == R).all() and (t[131328:131584] == K).all()


def test_loe_edges():
    """identical images score 0; a constant input against a varying output; pairs that hold lightness 0 and 255 (the two ends of the
    prefix sums); a constant pair of 512 x 512, where one bin of a workgroup's private histogram takes every sample"""
    from fdn_hip import lowlight
    a, b = rand_pair(45, 70, 41)
    assert lowlight.loe_counts_u8(dev(a[None]), dev(a[None]), 0) == ([0], 45 * 70)
    assert int(lowlight.loe_map_u8(dev(a[None]), dev(a[None]), 0).cpu().numpy().astype(np.int64).sum()) == 0
    const = np.full_like(a, 9)
    for x, y in ((const, b), (b, const)):
        want = ref.loe_hist(x, y, 0)
        assert want[0] > 0 and lowlight.loe_counts_u8(dev(x[None]), dev(y[None]), 0) == ([want[0]], want[1])
    e1, e2 = a.copy(), b.copy()
    e1[::2, ::3], e1[1::2, 1::3], e2[::3, ::2], e2[1::3, 1::2] = 0, 255, 255, 0
    for x, y in ((e1, e2), (e1 // 255 * 255, e2 // 255 * 255)):              # the second pair holds nothing but 0 and 255
        want = ref.loe_hist(x, y, 0)
        assert lowlight.loe_counts_u8(dev(x[None]), dev(y[None]), 0) == ([want[0]], want[1])
        assert (lowlight.loe_map_u8(dev(x[None]), dev(y[None]), 0).cpu().numpy().astype(np.int64)[0] == ref.loe_map(x, y, 0)).all()
    big = np.full((512, 512, 3), 200, np.uint8)
    vary = rand_pair(512, 512, 42)[0]
    assert lowlight.loe_counts_u8(dev(big[None]), dev(big[None]), 0) == ([0], 512 * 512)
    want = ref.loe_hist(big, vary, 0)
    assert lowlight.loe_counts_u8(dev(big[None]), dev(vary[None]), 0) == ([want[0]], want[1])


# ---- CIEDE2000 ----
def cube_corners():
    c = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    return np.repeat(c, 8, 0).reshape(8, 8, 3), np.tile(c, (8, 1)).reshape(8, 8, 3)          # every corner against every corner


def grey_pair():
    g = np.random.default_rng(52)
    return tuple(np.repeat(g.integers(0, 256, (64, 64, 1), dtype=np.uint8), 3, 2) for _ in range(2))


DE_CASES = {
    "random-64x64": lambda: rand_pair(64, 64, 51),
    "random-37x53": lambda: rand_pair(37, 53, 53),
    "greys": grey_pair,
    "cube-corners": cube_corners,
    "black-white": lambda: (np.zeros((2, 2, 3), np.uint8), np.full((2, 2, 3), 255, np.uint8)),
}


@pytest.mark.parametrize("case", list(DE_CASES))
def test_deltae_within_the_measured_bound(case):
    from fdn_hip import lowlight
    a, b = DE_CASES[case]()                                                    # R, G, B
    h, w = a.shape[:2]
    want = ref.deltae_u8(a, b)
    E = float(np.abs(want - ref.deltae_u8(a, b, np.longdouble)).max())
    unit = max(E, 1.5e-14)
    bound = 32 * unit
    # every pixel as an image of its own: sum = max = the pixel's float64 value
    pa, pb = dev(a.reshape(-1, 1, 1, 3)), dev(b.reshape(-1, 1, 1, 3))
    mean1, max1 = lowlight.deltae00_u8(pa, pb, bgr=False)
    px = np.array(mean1).reshape(h, w)
    assert mean1 == max1
    err = float(np.abs(px - want).max())
    # the image: sum / (h w), the maximum, the map
    means, maxima, dmap = lowlight.deltae00_u8(dev(a[None]), dev(b[None]), bgr=False, want_map=True)
    ratios = (err / unit, abs(means[0] - want.mean()) / unit, abs(maxima[0] - want.max()) / unit)
    print(f"{case}: E = {E:.3e}, per-pixel |device - float64| / max(E, 1.5e-14) = {ratios[0]:.3f}, mean {ratios[1]:.3f}, "
          f"max {ratios[2]:.3f}")
    assert err <= bound, (err, bound)
    assert abs(means[0] - want.mean()) <= bound and abs(maxima[0] - want.max()) <= bound
    assert maxima[0] == px.max()                                               # the maximum is one of the per-pixel values, bit for bit
    got = dmap.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (1, h, w)
    assert (got[0] == px.astype(np.float32)).all()                             # the float64 value rounded once
    assert (np.abs(got[0].astype(np.float64) - want) <= 0.5 * np.spacing(want.astype(np.float32)).astype(np.float64) + bound).all()
    if case == "black-white":
        assert abs(means[0] - 100.0) < 1e-5                                    # Y of white is 1.0000001 with this matrix


def test_deltae_identical_images_are_exactly_zero():
    from fdn_hip import lowlight
    for a in (rand_pair(37, 53, 61)[0], grey_pair()[0], cube_corners()[0]):
        for bgr in (False, True):
            means, maxima, dmap = lowlight.deltae00_u8(dev(a[None]), dev(a[None]), bgr=bgr, want_map=True)
            assert means == [0.0] and maxima == [0.0] and not dmap.cpu().numpy().any()


def _bits(means, maxima):
    return np.array([means, maxima], np.float64).view(np.uint64).tolist()


def test_deltae_batch_slots_calls_and_channel_order_give_the_same_bits():
    """B = 3 against each image scored alone, the same call twice, and bgr = 1 on the channel-swapped bytes: the same float64 bits, and
    the same map; 96 x 100 has more than one tile per image and a partial last tile"""
    from fdn_hip import lowlight
    pairs = [rand_pair(96, 100, 71), rand_pair(96, 100, 72, 0, 60), rand_pair(96, 100, 73, 180, 256)]
    a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    m3, x3, map3 = lowlight.deltae00_u8(dev(a), dev(b), bgr=False, want_map=True)
    again = lowlight.deltae00_u8(dev(a), dev(b), bgr=False)
    assert _bits(m3, x3) == _bits(*again)
    for k in range(3):
        m1, x1, map1 = lowlight.deltae00_u8(dev(a[k:k + 1]), dev(b[k:k + 1]), bgr=False, want_map=True)
        assert _bits(m1, x1) == _bits(m3[k:k + 1], x3[k:k + 1])
        assert torch.equal(map1[0], map3[k])
    ms, xs, maps = lowlight.deltae00_u8(dev(a[..., ::-1]), dev(b[..., ::-1]), bgr=True, want_map=True)
    assert _bits(ms, xs) == _bits(m3, x3) and torch.equal(maps, map3)
    assert _bits(*lowlight.deltae00_u8(dev(a), dev(b), bgr=True)) != _bits(m3, x3)              # the flag is not ignored
    want = [ref.deltae_u8(x, y).mean() for x, y in pairs]
    assert np.allclose(m3, want, rtol=1e-12, atol=0)


def test_lowlight_metrics_end_to_end():
    """a batch with and without ground truth: the dicts hold what the single functions give"""
    from fdn_hip import lowlight
    pairs = [ref.dark_pair(64, 90, 81), ref.dark_pair(64, 90, 82)]
    gts = [rand_pair(64, 90, 83)[0], pairs[1][1]]                              # the second image is its own ground truth
    inp, enh, gt = dev(np.stack([p[0] for p in pairs])), dev(np.stack([p[1] for p in pairs])), dev(np.stack(gts))
    res = lowlight.lowlight_metrics(inp, enh)
    assert [set(r) for r in res] == [{"loe", "loe_numerator", "loe_samples"}] * 2
    for r, (x, y) in zip(res, pairs):
        num, m = ref.loe_hist(x, y, 50)
        assert (r["loe_numerator"], r["loe_samples"], r["loe"]) == (num, m, num / m)
    full = lowlight.lowlight_metrics(inp, enh, gt, size=0, bgr=False)
    means, maxima = lowlight.deltae00_u8(gt, enh, bgr=False)
    for k, r in enumerate(full):
        num, m = ref.loe_hist(*pairs[k], 0)
        assert (r["loe_numerator"], r["loe_samples"]) == (num, m) and r["deltae"] == means[k] and r["deltae_max"] == maxima[k]
    assert full[1]["deltae"] == 0.0 and abs(full[0]["deltae"] - ref.deltae_u8(gts[0], pairs[0][1]).mean()) < 1e-11
    one = lowlight.lowlight_metrics(inp[0], enh[0], gt[0], size=0, bgr=False)           # a single (h, w, 3) image is a batch of one
    assert one == full[:1]
    both, rd = lowlight.lowlight_metrics(inp, enh, gt, size=50, bgr=False, want_loe_map=True)    # the map from the tables of the same launch
    assert [r["loe_numerator"] for r in both] == [r["loe_numerator"] for r in res] and torch.equal(rd, lowlight.loe_map_u8(inp, enh, 50))
    assert [int(x) for x in rd.cpu().numpy().astype(np.int64).sum(axis=(1, 2))] == [r["loe_numerator"] for r in res]


def _run(script, *args):
    out = subprocess.run([sys.executable, os.path.join(PKG, script), *args], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stderr
    return out.stdout


def test_command_lines(tmp_path):
    """calculate_lowlight_metrics.py and validate_fdn.py --lowlight on a few small PNGs, in child processes: the printed lines, the means,
    the csv and the RD / m pictures are the Python API's"""
    from PIL import Image
    from basicsr.models.archs.FDN_arch import FDN
    from fdn_hip import harness, lowlight
    import calculate_lowlight_metrics as tool
    pairs = [ref.dark_pair(64, 90, 91 + i) for i in range(3)]
    lq, rs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    gt = np.stack([rand_pair(64, 90, 95 + i, 40, 220)[0] for i in range(3)])
    small = ref.dark_pair(24, 40, 99)                                            # a pair of another size: its own batch
    for d in ("lq", "gt", "rs"):
        (tmp_path / d).mkdir()
    for i in range(3):
        for d, arr in (("lq", lq), ("gt", gt), ("rs", rs)):
            Image.fromarray(arr[i]).save(tmp_path / d / f"f{i}.png")
    Image.fromarray(small[0]).save(tmp_path / "lq" / "f3.png")
    Image.fromarray(small[1]).save(tmp_path / "rs" / "f3.png")
    Image.fromarray(small[1]).save(tmp_path / "gt" / "f3.png")
    globs = [str(tmp_path / d / "*.png") for d in ("lq", "rs", "gt")]

    text = _run("calculate_lowlight_metrics.py", "--input", globs[0], "--restored", globs[1], "--gt", globs[2], "--batch", "2",
                "--csv", str(tmp_path / "ll.csv"), "--save-loe-map", str(tmp_path / "maps"))
    want = lowlight.lowlight_metrics(dev(lq), dev(rs), dev(gt), bgr=False) + lowlight.lowlight_metrics(dev(small[0]), dev(small[1]), dev(small[1]), bgr=False)
    rows = re.findall(r"^ *(\d+): (\S+) *\. \tLOE: (\S+), dE00: (\S+) \(max (\S+)\)$", text, re.M)
    assert [r[1] for r in rows] == ["f0", "f1", "f2", "f3"]
    for r, m in zip(rows, want):
        assert r[2:] == (f"{m['loe']:.6f}", f"{m['deltae']:.6f}", f"{m['deltae_max']:.6f}")
    assert want[3]["deltae"] == 0.0 and want[0]["loe"] == ref.loe_hist(lq[0], rs[0], 50)[0] / ref.loe_hist(lq[0], rs[0], 50)[1]
    assert f"Average: LOE: {sum(m['loe'] for m in want) / 4:.6f}, dE00: {sum(m['deltae'] for m in want) / 4:.6f}\n" in text
    lines = (tmp_path / "ll.csv").read_text().splitlines()
    assert lines[0] == "input,restored,loe,loe_numerator,loe_samples,gt,deltae,deltae_max" and len(lines) == 5
    for k, m in enumerate(want):
        c = lines[1 + k].split(",")
        assert c[0].endswith(f"lq/f{k}.png") and c[1].endswith(f"rs/f{k}.png") and c[5].endswith(f"gt/f{k}.png")
        assert (float(c[2]), int(c[3]), int(c[4]), float(c[6]), float(c[7])) == (m["loe"], m["loe_numerator"], m["loe_samples"], m["deltae"], m["deltae_max"])
    for k in range(3):
        px = np.array(Image.open(tmp_path / "maps" / f"f{k}.png"))
        assert px.dtype == np.uint8 and px.shape == ref.sample_dims(64, 90, 50)
        assert (px == tool.map_bytes(ref.loe_map(lq[k], rs[k], 50), want[k]["loe_samples"])).all()
    # without --gt: LOE only, at full resolution
    text = _run("calculate_lowlight_metrics.py", "--input", globs[0], "--restored", globs[1], "--loe-size", "0")
    assert "dE00" not in text
    full = [ref.loe_hist(a, b, 0) for a, b in pairs + [small]]
    assert re.findall(r"\tLOE: (\S+)$", text, re.M) == [f"{n / m:.6f}" for n, m in full]

    torch.save({"params": fdn_weights(tame=0.03)}, tmp_path / "fdn.pth")
    common = ["--fdn", str(tmp_path / "fdn.pth"), "--lq", str(tmp_path / "lq" / "f[012].png"), "--gt", str(tmp_path / "gt" / "f[012].png"), "--batch", "2"]
    text = _run("validate_fdn.py", *common, "--csv", str(tmp_path / "val.csv"), "--lowlight", "--loe-size", "0")
    net = FDN()
    net.load_state_dict(fdn_weights(tame=0.03), strict=True)
    net = net.to(DEV).eval()
    out, psnr, ssim, ratio = harness.validate_u8(net, None, dev(lq), dev(gt), ratio_mode="gt", bgr=False)
    want = lowlight.lowlight_metrics(dev(lq), out, dev(gt), size=0, bgr=False)
    rows = re.findall(r"^ *(\d+): (\S+) *\. \tPSNR: (\S+) dB, \tSSIM: (\S+), \tLOE: (\S+), dE00: (\S+)$", text, re.M)
    assert [r[1:] for r in rows] == [(f"f{i}", f"{psnr[i]:.6f}", f"{ssim[i]:.6f}", f"{want[i]['loe']:.6f}", f"{want[i]['deltae']:.6f}") for i in range(3)]
    assert (f"Average: PSNR: {sum(psnr) / 3:.6f} dB, SSIM: {sum(ssim) / 3:.6f}, LOE: {sum(m['loe'] for m in want) / 3:.6f}, "
            f"dE00: {sum(m['deltae'] for m in want) / 3:.6f}\n") in text
    lines = (tmp_path / "val.csv").read_text().splitlines()
    assert lines[0] == "frame,psnr,ssim,ratio,loe,deltae"
    for i in range(3):
        c = lines[1 + i].split(",")
        assert c[0].endswith(f"lq/f{i}.png") and (float(c[1]), float(c[2]), float(c[4]), float(c[5])) == (psnr[i], ssim[i], want[i]["loe"], want[i]["deltae"])
