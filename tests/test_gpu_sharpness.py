"""GPU: the deblurring evaluation (include/fdn_sharpness.h, fdn_hip.sharpness, csrc/sharpness.hip in libfdn_sharpness.so,
harness.validate_u8(sharpness=True), calculate_sharpness_metrics.py and validate_fdn.py --sharpness) against the numpy restatement of
tests/sharpness_ref.py, which tests/test_sharpness_cpu.py ties to a dense-matrix G U G, to the reference's EdgeLoss and to the GMSD
authors' MATLAB code.

Integers must be EQUAL: the edge residual N (int32) and the gradient energy A (int64).

The floating-point bounds, with u = 2^-53 and every reference sum exactly rounded (math.fsum, one more u):
  edge sum   n = 3 h w non-negative terms added in any order cost (n - 1) u relative; a term is a divide, a square, an add and a square
             root, 4 ulp = 8 u:  |S - S_ref| <= (n + 8) u S_ref.
  q          per grid point within 32 max(E, 2^-52) of the restatement, E = the restatement's own largest |float64 - longdouble| on the
             case and 2^-52 one ulp of 1.0 (the rule of tests/test_gpu_lowlight.py).  The device hands q out rounded once to float32, so
             what is held is that the float32 lies between the float32 roundings of the two ends of that interval: no wider, and exact
             wherever the interval does not straddle a float32 rounding boundary.
  GMSD sums  n = hd wd terms: sum of q (a product, a root, an add, a divide: 4 ulp) <= (n + 8) u; sum of q^2 (twice that and the square:
             9 ulp) <= (n + 18) u; sums of m (a root and a divide: 2 ulp) <= (n + 4) u, all relative to the reference sum.

Shapes: all 25 of 1 .. 5 rows and columns; one less than, equal to and one more than the tile in each axis; several tiles; batches whose
image size is odd, so that the second image starts at an odd address; and a batch whose last image lies past byte 2^31 (all but that
image black: the kernels' time on 2 GB of bytes, and nothing on the host)."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import sharpness_ref as ref
from common import fdn_weights
from test_sharpness_cpu import check_argument_errors

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
U = 2.0 ** -53
T = 32                                                    # FDN_EDGE_TILE = FDN_GMSD_TILE (asserted below)


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()   # fail loudly if the HIP extension is not built
    from fdn_hip import sharpness
    sharpness.lib()
    assert sharpness.EDGE_TILE == sharpness.GMSD_TILE == T
    return sharpness


def cuda(a):
    return (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).to("cuda:0").contiguous()


def batch2(h, w, seed):
    """a soft pair and an unrelated pair of one size: uint8 [2][h][w][3] each"""
    (a0, b0), (a1, b1) = ref.soft_pair(h, w, seed), ref.random_pair(h, w, seed + 1)
    return np.stack([a0, a1]), np.stack([b0, b1])


def check_edge(S, a, b):
    """the residual as integers and the sum within its bound, for every image of the batch a, b"""
    B, h, w, _ = a.shape
    n = 3 * h * w
    resid = S.edge_residual_u8(cuda(a), cuda(b))
    assert resid.dtype == torch.int32 and tuple(resid.shape) == a.shape
    resid = resid.cpu().numpy()
    sums = S.edge_sums_u8(cuda(a), cuda(b))
    for i in range(B):
        want = ref.edge_residual(a[i], b[i])
        bad = np.argwhere(resid[i] != want)
        assert bad.size == 0, (h, w, i, len(bad), bad[:4].tolist(), resid[i][tuple(bad[0])], want[tuple(bad[0])])
        s_ref = ref.edge_sum(a[i], b[i])
        print(f"{h}x{w} image {i}: edge sum {sums[i]!r}, restatement {s_ref!r}, diff {sums[i] - s_ref:+.2e}, bound {(n + 8) * U * s_ref:.2e}")
        assert abs(sums[i] - s_ref) <= (n + 8) * U * s_ref
    assert S.edge_error_u8(cuda(a), cuda(b)) == [s / n for s in sums]


def test_edge_residual_on_all_small_shapes(S):
    for h in range(1, 6):
        for w in range(1, 6):
            check_edge(S, *batch2(h, w, seed=10 * h + w))


@pytest.mark.parametrize("shape", [(T - 1, 40), (T, 40), (T + 1, 40), (40, T - 1), (40, T), (40, T + 1), (70, 133)])
def test_edge_residual_at_the_tile_edge_and_on_several_tiles(S, shape):
    check_edge(S, *batch2(*shape, seed=shape[0] * 1000 + shape[1]))


def check_gmsd(S, a, b, bgr=True):
    """the gradient energy as integers, q per grid point and the four sums within their bounds, for every image of the batch a, b"""
    B, h, w, _ = a.shape
    hd, wd = ref.gmsd_dims(h, w)
    n = hd * wd
    assert S.gmsd_dims(h, w) == (hd, wd)
    grad2 = S.gradient_energy_u8(cuda(a), cuda(b), bgr)
    assert grad2.dtype == torch.int64 and tuple(grad2.shape) == (B, 2, hd, wd)
    grad2 = grad2.cpu().numpy()
    qmap = S.gmsd_map_u8(cuda(a), cuda(b), bgr)
    assert qmap.dtype == torch.float32 and tuple(qmap.shape) == (B, hd, wd)
    qmap = qmap.cpu().numpy()
    rows, n_dev = S.gmsd_sums_u8(cuda(a), cuda(b), bgr)
    assert n_dev == n
    got_gmsd, (got_ma, got_mb) = S.gmsd_u8(cuda(a), cuda(b), bgr), S.mean_gradient_u8(cuda(a), cuda(b), bgr)
    for i in range(B):
        for k, img in enumerate((a[i], b[i])):
            assert np.array_equal(grad2[i, k], ref.grad2(img, bgr)), (h, w, i, k)
        q = ref.gms_map(a[i], b[i], bgr)
        E = float(np.abs(q - ref.gms_map(a[i], b[i], bgr, np.longdouble)).max())
        bound = 32 * max(E, 2.0 ** -52)
        lo, hi = (q - bound).astype(np.float32), (q + bound).astype(np.float32)
        assert ((lo <= qmap[i]) & (qmap[i] <= hi)).all(), (h, w, i, float(np.abs(qmap[i] - q).max()))
        s1, s2, _ = ref.gmsd_sums(a[i], b[i], bgr)
        ma, mb = (math.fsum(ref.gradient_terms(img, bgr).ravel().tolist()) for img in (a[i], b[i]))
        print(f"{h}x{w} image {i}: E {E:.1e}; sums {rows[i]!r}; restatement {(s1, s2, ma, mb)!r}")
        assert abs(rows[i][0] - s1) <= (n + 8) * U * s1
        assert abs(rows[i][1] - s2) <= (n + 18) * U * s2
        assert abs(rows[i][2] - ma) <= (n + 4) * U * ma and abs(rows[i][3] - mb) <= (n + 4) * U * mb
        assert got_gmsd[i] == ref.std_from_sums(rows[i][0], rows[i][1], n)               # the host step, on the device's sums
        assert (got_ma[i], got_mb[i]) == (rows[i][2] / n, rows[i][3] / n)
        # the figure itself: the difference S2 - S1^2 / n cancels, so its error is that of the sums over the variance
        var = (s2 - s1 * s1 / n) / (n - 1)
        if var > 1e-6:
            assert abs(got_gmsd[i] - ref.gmsd(a[i], b[i], bgr)) <= 4 * (n + 18) * U * s2 / ((n - 1) * math.sqrt(var))


@pytest.mark.parametrize("shape", [(1, 3), (3, 1), (3, 5), (64, 90), (2 * T - 3, 20), (2 * T, 20), (2 * T + 1, 20), (20, 2 * T - 3), (20, 2 * T),
                                   (20, 2 * T + 1), (2 * T + 6, 4 * T + 5)])
@pytest.mark.parametrize("bgr", [True, False])
def test_gradient_energy_and_similarity(S, shape, bgr):
    """grids of 31, 32 and 33 points in each axis sit at one less than, equal to and one more than the tile; 70 x 133 has 2 x 3 tiles"""
    check_gmsd(S, *batch2(*shape, seed=shape[0] * 1000 + shape[1]), bgr=bgr)


def test_a_grid_of_one_point_is_refused(S):
    """2 x 2 pixels are one grid point, and one point has no standard deviation: FDN_ERR_ARG whatever the batch.  (The batch of two
    2 x 2 pairs is therefore refused like the single pair: n counts the points of ONE image, as every image is scored on its own.)"""
    from fdn_hip import FdnHipError
    l = S.lib()
    for B in (1, 2):
        a, b = (cuda(x) for x in ref.random_pair(2, 2, seed=1, n=B))
        out = torch.full((B, 4), -1.0, dtype=torch.float64, device="cuda:0")
        ws = torch.full((64,), -1.0, dtype=torch.float64, device="cuda:0")
        grad2 = torch.full((B, 2, 1, 1), -1, dtype=torch.int64, device="cuda:0")
        assert l.fdn_gmsd_ws(B, 2, 2) == 0
        assert l.fdn_gmsd_u8(a.data_ptr(), b.data_ptr(), B, 2, 2, 1, grad2.data_ptr(), None, ws.data_ptr(), out.data_ptr(), None) == 1
        torch.cuda.synchronize()
        assert (out == -1).all() and (grad2 == -1).all() and (ws == -1).all()            # nothing was launched
        with pytest.raises(FdnHipError, match="needs at least two"):
            S.gmsd_u8(a, b)
    a, b = batch2(2, 4, seed=5)                                                          # the smallest batch of two that has a GMSD
    check_gmsd(S, a, b)
    check_edge(S, *batch2(2, 2, seed=6))                                                 # the edge error of 2 x 2 is defined


def test_equal_images(S):
    for h, w in ((5, 4), (64, 90), (70, 133)):
        a, _ = batch2(h, w, seed=h)
        d = cuda(a)
        hd, wd = ref.gmsd_dims(h, w)
        assert not S.edge_residual_u8(d, d).any()
        assert (S.gmsd_map_u8(d, d) == 1.0).all()
        rows, n = S.gmsd_sums_u8(d, d)
        assert all(r[0] == n and r[1] == n and r[2] == r[3] for r in rows)               # exact sums of ones
        assert S.gmsd_u8(d, d) == [0.0, 0.0]
        for m in S.sharpness_metrics(d, d):
            assert m["gmsd"] == 0.0 and m["grad_ratio"] == 1.0 and abs(m["edge"] - 0.001) <= (3 * h * w + 8) * U * 0.001


def test_batch_slots_do_not_leak(S):
    pairs = [ref.soft_pair(33, 47, seed=1), ref.random_pair(33, 47, seed=2), ref.soft_pair(33, 47, seed=3)]
    a, b = cuda(np.stack([p[0] for p in pairs])), cuda(np.stack([p[1] for p in pairs]))
    all3 = S.sharpness_metrics(a, b)
    assert len(all3) == 3 and set(all3[0]) == {"edge", "gmsd", "grad_gt", "grad_restored", "grad_ratio"}
    assert all3 == S.sharpness_metrics(a, b)                                             # a repeated call: the same bits
    resid, grad2, qmap = S.edge_residual_u8(a, b), S.gradient_energy_u8(a, b), S.gmsd_map_u8(a, b)
    for i in range(3):
        assert all3[i] == S.sharpness_metrics(a[i:i + 1], b[i:i + 1])[0], i              # alone
        assert torch.equal(resid[i], S.edge_residual_u8(a[i], b[i])[0]) and torch.equal(grad2[i], S.gradient_energy_u8(a[i], b[i])[0])
        assert torch.equal(qmap[i], S.gmsd_map_u8(a[i], b[i])[0])
        assert all3[i]["edge"] == S.edge_error_u8(a[i], b[i]) and all3[i]["gmsd"] == S.gmsd_u8(a[i], b[i])
        assert all3[i]["grad_restored"] == S.mean_gradient_u8(b[i]) and all3[i]["grad_ratio"] == all3[i]["grad_restored"] / all3[i]["grad_gt"]
    order = [2, 0]                                                                       # other neighbours, another place
    assert S.sharpness_metrics(a[order], b[order]) == [all3[i] for i in order]
    assert len({m["gmsd"] for m in all3}) == len({m["edge"] for m in all3}) == 3
    assert all3[0]["grad_ratio"] < 1 and all3[2]["grad_ratio"] < 1                       # the blurred copies are softer than their sources


def test_one_dirty_workspace_repeated_and_interleaved(S):
    """the C entry points on one workspace pre-filled with -1, the two interleaved and repeated: a launch writes what it later reads"""
    l = S.lib()
    a, b = (cuda(x) for x in batch2(70, 133, seed=4))
    B, h, w, _ = a.shape
    nws = max(l.fdn_edge_ws(B, h, w), l.fdn_gmsd_ws(B, h, w))
    assert l.fdn_edge_ws(B, h, w) == 2 * 3 * 5 and l.fdn_gmsd_ws(B, h, w) == 4 * 2 * 2 * 3 == nws
    ws = torch.full((nws,), -1.0, dtype=torch.float64, device="cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def edge():
        out = torch.full((B,), -1.0, dtype=torch.float64, device="cuda:0")
        assert l.fdn_edge_u8(p(a), p(b), B, h, w, None, p(ws), p(out), st) == 0
        return out.cpu().tolist()

    def gmsd():
        out = torch.full((B, 4), -1.0, dtype=torch.float64, device="cuda:0")
        assert l.fdn_gmsd_u8(p(a), p(b), B, h, w, 1, None, None, p(ws), p(out), st) == 0
        return out.cpu().tolist()

    e0, g0 = edge(), gmsd()
    assert e0 == S.edge_sums_u8(a, b) and g0 == S.gmsd_sums_u8(a, b)[0]
    assert [edge(), gmsd(), gmsd(), edge(), edge(), gmsd()] == [e0, g0, g0, e0, e0, g0]


def test_bgr_flag(S):
    a, b = batch2(33, 47, seed=9)
    flip = lambda x: np.ascontiguousarray(x[..., ::-1])
    as_bgr, as_rgb = S.sharpness_metrics(cuda(a), cuda(b), bgr=True), S.sharpness_metrics(cuda(a), cuda(b), bgr=False)
    for m, n in zip(as_bgr, as_rgb):
        assert m["edge"] == n["edge"]                                                    # no gray in the edge figure
        assert m["gmsd"] != n["gmsd"] and m["grad_gt"] != n["grad_gt"]                   # R and B weigh 299 and 114
    swapped = S.sharpness_metrics(cuda(flip(a)), cuda(flip(b)), bgr=False)               # the same pixels handed over as R, G, B
    for m, n in zip(as_bgr, swapped):
        assert {k: m[k] for k in m if k != "edge"} == {k: n[k] for k in n if k != "edge"}
        assert abs(m["edge"] - n["edge"]) <= 2 * (a[0].size + 8) * U * m["edge"]         # the same terms, the channels added in another order
    assert torch.equal(S.gradient_energy_u8(cuda(a), cuda(b), bgr=True), S.gradient_energy_u8(cuda(flip(a)), cuda(flip(b)), bgr=False))


def test_an_image_past_byte_2_31(S):
    """718 images of 1000 x 1000: the last one starts past byte 2^31 of both buffers; it scores what it scores alone, and the black
    images before it score what black images score"""
    h = w = 1000
    B = 718
    assert (B - 1) * h * w * 3 > 2 ** 31
    a1, b1 = ref.soft_pair(h, w, seed=12)
    a = torch.zeros((B, h, w, 3), dtype=torch.uint8, device="cuda:0")
    b = torch.zeros((B, h, w, 3), dtype=torch.uint8, device="cuda:0")
    a[-1], b[-1] = cuda(a1), cuda(b1)
    got = S.sharpness_metrics(a, b)
    alone = S.sharpness_metrics(cuda(a1), cuda(b1))[0]
    assert got[-1] == alone and alone["gmsd"] > 0 and alone["grad_ratio"] < 1
    for m in (got[0], got[B - 2]):
        assert m["gmsd"] == 0.0 and m["grad_gt"] == m["grad_restored"] == 0.0 and math.isnan(m["grad_ratio"]) and m["edge"] == got[0]["edge"]
    assert abs(got[0]["edge"] - 0.001) <= (3 * h * w + 8) * U * 0.001
    del a, b
    torch.cuda.empty_cache()


def test_argument_errors_on_the_device(S):
    """the refusals of tests/test_sharpness_cpu.py, where a launch would have had a GPU to run on"""
    check_argument_errors(S.lib())
    torch.cuda.synchronize()


def test_validate_u8_with_sharpness(S):
    from basicsr.models.archs.FDN_arch import FDN
    from fdn_hip import harness
    net = FDN()
    net.load_state_dict(fdn_weights(tame=0.03), strict=True)
    net = net.to("cuda:0").eval()
    gt, lq = (cuda(x) for x in batch2(64, 64, seed=8))
    plain = harness.validate_u8(net, None, lq, gt, ratio_mode="gt", bgr=False)
    more = harness.validate_u8(net, None, lq, gt, ratio_mode="gt", bgr=False, sharpness=True)
    both = harness.validate_u8(net, None, lq, gt, ratio_mode="gt", bgr=False, correct="gt_mean", sharpness=True)
    assert len(plain) == 4 and len(more) == 5 and len(both) == 7
    assert torch.equal(plain[0], more[0]) and plain[1:3] == more[1:3] == both[1:3] and torch.equal(plain[3], more[3])
    assert more[4] == both[6] == S.sharpness_metrics(gt, more[0], bgr=False)


def _run(script, *args):
    out = subprocess.run([sys.executable, os.path.join(PKG, script), *args], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stderr
    return out.stdout


FIG = r"edge: (\S+), GMSD: (\S+), grad ratio: (\S+)"


def test_command_lines(S, tmp_path):
    """each command line once, as a child process, on a folder of three 20 x 24 PNGs (validate_fdn.py's reflect padding refuses 16 rows)"""
    from PIL import Image
    from basicsr.models.archs.FDN_arch import FDN
    from fdn_hip import harness
    for d in ("gt", "rs"):
        (tmp_path / d).mkdir()
    pairs = [ref.soft_pair(20, 24, seed=60 + i) for i in range(3)]
    for i, (a, b) in enumerate(pairs):
        Image.fromarray(a).save(tmp_path / "gt" / f"f{i}.png")
        Image.fromarray(b).save(tmp_path / "rs" / f"f{i}.png")
    gt, rs = cuda(np.stack([p[0] for p in pairs])), cuda(np.stack([p[1] for p in pairs]))
    want = S.sharpness_metrics(gt, rs, bgr=False)
    text = _run("calculate_sharpness_metrics.py", "--gt", str(tmp_path / "gt" / "*.png"), "--restored", str(tmp_path / "rs" / "*.png"),
                "--batch", "2", "--csv", str(tmp_path / "sharp.csv"), "--save-gms-map", str(tmp_path / "maps"))
    rows = re.findall(r"^ *(\d+): (\S+) *\. \t" + FIG + r" \(gt (\S+), restored (\S+)\)$", text, re.M)
    assert [r[1:] for r in rows] == [(f"f{i}", f"{m['edge']:.6f}", f"{m['gmsd']:.6f}", f"{m['grad_ratio']:.6f}", f"{m['grad_gt']:.6f}",
                                      f"{m['grad_restored']:.6f}") for i, m in enumerate(want)]
    avg = re.search(r"^Average: " + FIG + "$", text, re.M)
    assert avg and avg.group(2) == f"{sum(m['gmsd'] for m in want) / 3:.6f}"
    csv = (tmp_path / "sharp.csv").read_text().splitlines()
    assert csv[0] == "restored,grad_restored,gt,edge,gmsd,grad_gt,grad_ratio" and len(csv) == 4
    for i, line in enumerate(csv[1:]):
        r, gr, g, e, q, gg, ratio = line.split(",")
        assert r.endswith(f"rs/f{i}.png") and g.endswith(f"gt/f{i}.png")
        assert (float(gr), float(e), float(q), float(gg), float(ratio)) == tuple(want[i][k] for k in ("grad_restored", "edge", "gmsd", "grad_gt", "grad_ratio"))
    qmap = S.gmsd_map_u8(gt, rs, bgr=False).cpu().numpy()
    for i in range(3):
        png = np.array(Image.open(tmp_path / "maps" / f"f{i}.png"))
        assert png.dtype == np.uint8 and np.array_equal(png, np.rint(np.clip(qmap[i].astype(np.float64), 0, 1) * 255).astype(np.uint8))
    # without a ground truth: the restored images' own mean gradient
    text = _run("calculate_sharpness_metrics.py", "--restored", str(tmp_path / "rs" / "*.png"))
    assert re.findall(r"\tgrad: (\S+)$", text, re.M) == [f"{m['grad_restored']:.6f}" for m in want] and "GMSD" not in text

    torch.save({"params": fdn_weights(tame=0.03)}, tmp_path / "fdn.pth")
    base = ["--fdn", str(tmp_path / "fdn.pth"), "--lq", str(tmp_path / "rs" / "*.png"), "--gt", str(tmp_path / "gt" / "*.png")]
    text = _run("validate_fdn.py", *base, "--sharpness", "--csv", str(tmp_path / "scores.csv"))
    net = FDN()
    net.load_state_dict(fdn_weights(tame=0.03), strict=True)
    net = net.to("cuda:0").eval()
    out, psnr, ssim, ratio, sm = harness.validate_u8(net, None, rs, gt, ratio_mode="gt", bgr=False, sharpness=True)
    rows = re.findall(r"^ *(\d+): (\S+) *\. \tPSNR: (\S+) dB, \tSSIM: (\S+?), \t" + FIG + "$", text, re.M)
    assert [r[1:] for r in rows] == [(f"f{i}", f"{psnr[i]:.6f}", f"{ssim[i]:.6f}", f"{m['edge']:.6f}", f"{m['gmsd']:.6f}", f"{m['grad_ratio']:.6f}")
                                     for i, m in enumerate(sm)]
    assert re.search(r"^Average: PSNR: \S+ dB, SSIM: \S+, " + FIG + "$", text, re.M)
    csv = (tmp_path / "scores.csv").read_text().splitlines()
    assert csv[0] == "frame,psnr,ssim,ratio,edge,gmsd,grad_ratio" and len(csv) == 4
    for i, line in enumerate(csv[1:]):
        f, p, s, r, e, q, gr = line.rsplit(",", 6)
        assert f.endswith(f"f{i}.png") and (float(p), float(s), float(e), float(q), float(gr)) == (psnr[i], ssim[i], sm[i]["edge"], sm[i]["gmsd"], sm[i]["grad_ratio"])
    # without the flag the output is what it was: no figure of this module in it
    plain = _run("validate_fdn.py", *base)
    assert "edge:" not in plain and [l.split(", \tedge:")[0] for l in text.splitlines() if l[:3].strip().isdigit()] == \
        [l for l in plain.splitlines() if l[:3].strip().isdigit()]
