"""GPU: PIQE (include/fdn_piqe.h, csrc/piqe.hip, fdn_hip.piqe) against the ordered numpy restatement of tests/piqe_ref.py, compared with
==, never with a tolerance: the MSCN plane, the block variances, the class bytes, D, NHSA and the score.  The header fixes every order of
summation, sqrt and the divisions are IEEE on both sides, and contraction is off in the kernel, so there is nothing to tolerate.

Shapes are the smallest at which the kernel can go wrong: one block without padding (16 x 16), padding on both sides (17 x 33), odd
sizes (47 x 95), every class present and more than one tile in both directions (161 x 257), and one pixel (33 x 65) and one block
(48 x 80) past the header's 32 x 64 tile.  The input is the four-quadrant synthetic of piqe_ref.quadrants (ramp, white noise, smoothed
texture, its 8 x 8 block means); at 161 x 257 every one of the five classes holds at least 3 % of the blocks, so no branch goes untested.

Then: a batch of three different images (each the bits it has alone), the same input twice, optional outputs NULL and not NULL, a
workspace the test filled with -1, guard words behind every buffer, luma at 8 and 10 bit with codes above 1023, the refusals, and the
three command lines through main(argv)."""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

import piqe_ref as ref
from common import fdn_weights
from test_piqe_cpu import check_argument_errors

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
TILE_H, TILE_W = 32, 64                                   # FDN_PIQE_TILE_H, FDN_PIQE_TILE_W (asserted below)
SHAPES = [(16, 16), (17, 33), (47, 95), (161, 257), (TILE_H + 1, TILE_W + 1), (TILE_H + 16, TILE_W + 16)]


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()   # fail loudly if the HIP extension is not built
    from fdn_hip import piqe
    piqe.lib()
    assert (piqe.TILE_H, piqe.TILE_W, piqe.BLOCK) == (TILE_H, TILE_W, 16)
    return piqe


@pytest.fixture(scope="module")
def Hn(S):
    from fdn_hip import harness
    return harness


def cuda(a):
    """numpy -> a contiguous tensor on the GPU; 16-bit samples travel as int16"""
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
    return a.to("cuda:0").contiguous()


@functools.lru_cache(maxsize=None)
def image(shape, seed=0):
    """the input and the restatement's result: computed once, never changed"""
    img = ref.quadrants(*shape, seed=seed)
    return img, ref.result_u8(img)


def check_plane(what, want, rec, maps, i=0):
    """one plane of the device against the restatement, every figure printed before anything is asserted"""
    mscn, var, cls = (maps[k][i].cpu().numpy() for k in ("mscn", "var", "cls"))
    bad = {"mscn": int((mscn != want["mscn"]).sum()), "var": int((var != want["v"]).sum()), "cls": int((cls != want["cls"]).sum())}
    print(f"{what}: differing mscn {bad['mscn']} of {mscn.size} (max |d| {float(np.abs(mscn - want['mscn']).max()):.3g}), var {bad['var']} of "
          f"{var.size}, cls {bad['cls']}; D {rec['d']!r} / {want['D']!r}, NHSA {rec['nhsa']} / {want['nhsa']}, PIQE {rec['piqe']!r} / {want['piqe']!r}")
    assert mscn.shape == want["mscn"].shape and var.shape == cls.shape == want["v"].shape and cls.dtype == np.uint8
    assert np.array_equal(mscn, want["mscn"]), what
    assert np.array_equal(var, want["v"]) and np.array_equal(cls, want["cls"]), what
    assert rec["d"] == want["D"] and rec["nhsa"] == want["nhsa"] and rec["piqe"] == want["piqe"], what


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_shape(S, shape):
    img, want = image(shape)
    recs, maps = S.piqe_u8(cuda(img), maps=True)
    assert len(recs) == 1 and maps["mscn"].shape == (1,) + ref.dims(*shape)[:2]
    check_plane("%dx%d" % shape, want, recs[0], maps)
    assert S.piqe_u8(cuda(img)) == recs                                               # optional outputs NULL: the same D
    if shape == (161, 257):
        for c in (0, 1, 3, 5, 7):                                                     # every class holds at least 3 % of the blocks
            assert (want["cls"] == c).sum() >= 0.03 * want["cls"].size, c


def test_batch_of_three_and_repeats(S):
    """three different images in one call: each has the bits it has alone, wherever it sits; the same input twice: the same bits"""
    shape = (47, 95)
    imgs = [image(shape, seed=s) for s in (0, 1, 2)]
    assert len({w["piqe"] for _, w in imgs}) == 3
    batch = cuda(np.stack([i for i, _ in imgs]))
    recs, maps = S.piqe_u8(batch, maps=True)
    for k, (_, want) in enumerate(imgs):
        check_plane(f"batch[{k}]", want, recs[k], maps, k)
        assert S.piqe_u8(batch[k]) == [recs[k]]
    assert S.piqe_u8(batch[[2, 0, 1]]) == [recs[2], recs[0], recs[1]]
    again, maps2 = S.piqe_u8(batch, maps=True)
    assert again == recs and all(torch.equal(maps[k], maps2[k]) for k in maps)


def test_bgr_flat_and_padding(S):
    img, want = image((47, 95))
    flip = np.ascontiguousarray(img[..., ::-1])
    a = S.piqe_u8(cuda(img))[0]
    assert S.piqe_u8(cuda(flip), bgr=True) == [a] and S.piqe_u8(cuda(flip))[0]["d"] != a["d"]
    for value in (0, 37, 255):                                                        # no active block: exactly 100.0
        recs, maps = S.piqe_u8(cuda(np.full((40, 50, 3), value, np.uint8)), maps=True)
        assert recs == [{"piqe": 100.0, "d": 0.0, "nhsa": 0}] and not maps["cls"].any()
    small, _ = image((17, 33))
    padded = np.pad(small, ((0, 15), (0, 15), (0, 0)), mode="edge")
    (ra, ma), (rb, mb) = S.piqe_u8(cuda(small), maps=True), S.piqe_u8(cuda(padded), maps=True)
    assert ra == rb and all(torch.equal(ma[k], mb[k]) for k in ma)


def raw_call(S, src, B, h, w, entry, guard=64, optional=True, fill=-1.0, **kw):
    """one C entry point on exactly sized buffers, each followed by `guard` words of -1 -> (status, sizes, out, ws, mscn, var, cls) as
    host arrays, guards included"""
    l = S.lib()
    H, W, nby, nbx, ty, tx = ref.dims(max(h, 1), max(w, 1))
    nws = max(int(l.fdn_piqe_ws(B, h, w)), 1)
    sizes = dict(out=2 * B, ws=nws, mscn=B * H * W, var=B * nby * nbx, cls=B * nby * nbx)
    out = torch.full((sizes["out"] + guard,), -1.0, dtype=torch.float64, device="cuda:0")
    ws = torch.full((nws + guard,), fill, dtype=torch.float64, device="cuda:0")
    mscn = torch.full((sizes["mscn"] + guard,), -1.0, dtype=torch.float64, device="cuda:0")
    var = torch.full((sizes["var"] + guard,), -1.0, dtype=torch.float64, device="cuda:0")
    cls = torch.full((sizes["cls"] + guard,), 255, dtype=torch.uint8, device="cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if optional or t is ws or t is out else None      # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    taps = ctypes.c_void_p(S._TAPS.ctypes.data)
    if entry == "u8":
        code = l.fdn_piqe_u8(ctypes.c_void_p(src.data_ptr()), B, h, w, kw.get("bgr", 0), taps, p(mscn), p(var), p(cls), p(ws), p(out), st)
    else:
        code = l.fdn_piqe_luma(ctypes.c_void_p(src.data_ptr()), B, h, w, kw["bits"], kw["stride"], taps, p(mscn), p(var), p(cls), p(ws), p(out), st)
    torch.cuda.synchronize()
    return (code, sizes) + tuple(t.cpu().numpy() for t in (out, ws, mscn, var, cls))


def test_workspace_and_outputs_are_the_stated_sizes(S):
    """the C entry points on buffers of exactly the stated sizes with guard words behind each: every stated word is written, no guard
    word is; a workspace that held -1 or NaN gives the same bits; with the optional outputs NULL nothing but out and ws is written; the
    luma entry with a frame stride that is no multiple of anything, on an odd shape, 8 and 10 bit"""
    h, w, B = 47, 95, 2
    (a, wa), (b, wb) = image((h, w), 0), image((h, w), 1)
    src = cuda(np.stack([a, b]))
    H, W, nby, nbx, ty, tx = ref.dims(h, w)
    code, n, out, ws, mscn, var, cls = raw_call(S, src, B, h, w, "u8")
    assert code == 0 and n["ws"] == S.lib().fdn_piqe_ws(B, h, w) == 2 * B * ty * tx
    for t, k in ((out, "out"), (ws, "ws"), (mscn, "mscn"), (var, "var")):
        assert (t[n[k]:] == -1).all() and t[n[k]:].size == 64, k                       # nothing behind the stated size
    assert (cls[n["cls"]:] == 255).all() and (cls[:n["cls"]] <= 7).all() and not np.isnan(mscn[:n["mscn"]]).any() and (var[:n["var"]] >= 0).all()
    for i, want in enumerate((wa, wb)):                                                 # the stated layout
        assert np.array_equal(mscn[:n["mscn"]].reshape(B, H, W)[i], want["mscn"]) and np.array_equal(var[:n["var"]].reshape(B, nby, nbx)[i], want["v"])
        assert np.array_equal(cls[:n["cls"]].reshape(B, nby, nbx)[i], want["cls"]) and out[:4].reshape(B, 2)[i].tolist() == [want["D"], float(want["nhsa"])]
    assert (ws[:n["ws"]].reshape(B, ty * tx, 2)[..., 1].sum(axis=1) == [wa["nhsa"], wb["nhsa"]]).all()      # one partial per tile
    code, _, out2, ws2, mscn2, var2, cls2 = raw_call(S, src, B, h, w, "u8", optional=False, fill=float("nan"))
    assert code == 0 and np.array_equal(out2, out) and np.array_equal(ws2[:n["ws"]], ws[:n["ws"]]) and np.isnan(ws2[n["ws"]:]).all()
    assert (mscn2 == -1).all() and (var2 == -1).all() and (cls2 == 255).all()           # NULL: not written
    recs = S.piqe_u8(src)                                                               # the wrapper's workspace was poisoned
    assert [[r["d"], float(r["nhsa"])] for r in recs] == out[:4].reshape(B, 2).tolist()
    own = torch.full((n["ws"],), -1.0, dtype=torch.float64, device="cuda:0")            # a workspace pre-filled with -1 by the test
    got, _ = S.piqe_sums_u8(src, ws=own)
    assert got.cpu().numpy().ravel().tolist() == out[:4].tolist() and np.array_equal(own.cpu().numpy(), ws[:n["ws"]])
    # luma through the C entry: an odd shape, a stride of h w + 7 samples
    stride = h * w + 7
    for bits, dt in ((8, np.uint8), (10, np.uint16)):
        g = np.random.default_rng(bits)
        f = g.integers(0, 256 if bits == 8 else 1400, (B, stride)).astype(dt)
        f[:, :h * w] = np.stack([ref.plane_u8(x)[0].ravel() * (4 if bits == 10 else 1) for x in (a, b)])
        if bits == 10:
            f[:, 5:h * w:97] = 1500                                                     # above 1023: counts as 1023
        code, n, out, ws, mscn, var, cls = raw_call(S, cuda(f), B, h, w, "luma", bits=bits, stride=stride)
        assert code == 0
        for i in range(B):
            want = ref.plane_result(*ref.plane_luma(f[i], h, w, bits))
            assert np.array_equal(mscn[:n["mscn"]].reshape(B, H, W)[i], want["mscn"]), (bits, i)
            assert np.array_equal(var[:n["var"]].reshape(B, nby, nbx)[i], want["v"]) and np.array_equal(cls[:n["cls"]].reshape(B, nby, nbx)[i], want["cls"])
            assert out[:4].reshape(B, 2)[i].tolist() == [want["D"], float(want["nhsa"])], (bits, i)


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("shape", [(48, 80), (162, 258)], ids=lambda s: "%dx%d" % s)
def test_luma(S, Hn, shape, bits):
    """4:2:0 frames with stride h * w * 3 / 2; the 10-bit fixture holds codes above 1023"""
    h, w = shape
    fmt = Hn.VideoFormat("yuv420p10le" if bits == 10 else "yuv420p", "bt709", False, "left")
    f = ref.luma_frames(2, h, w, bits)
    assert f.shape == (2, h * w * 3 // 2) and (bits == 8 or (f[:, :h * w] > 1023).any())
    want = [ref.plane_result(*ref.plane_luma(x, h, w, bits)) for x in f]
    recs, maps = S.piqe_luma(cuda(f), h, w, fmt, maps=True)
    for i in range(2):
        check_plane(f"luma {bits} bit {h}x{w} [{i}]", want[i], recs[i], maps, i)
    assert S.piqe_luma(cuda(f), h, w, fmt) == recs and S.piqe_luma(cuda(f[1]), h, w, fmt) == recs[1:]
    score = S.PiqeScore(h, w, fmt, device="cuda:0")
    got = score.update(cuda(f[:1])) + score.update(cuda(f[1:]))
    assert got == score.frames == [{"piqe_y": r["piqe"], "nhsa": r["nhsa"]} for r in recs]
    assert score.summary() == {"frames": 2, "piqe_y": math.fsum(r["piqe"] for r in recs) / 2}
    if bits == 10 and shape == (48, 80):                                              # codes 4 c score the bits of the 8-bit codes c
        c = ref.plane_u8(ref.quadrants(h, w))[0]
        f8 = np.concatenate([c.ravel().astype(np.uint8), np.zeros(h * w // 2, np.uint8)])[None]
        f10 = np.concatenate([(4 * c).ravel().astype(np.uint16), np.zeros(h * w // 2, np.uint16)])[None]
        fmt8 = Hn.VideoFormat("yuv420p", "bt709", False, "left")
        assert S.piqe_luma(cuda(f10), h, w, fmt) == S.piqe_luma(cuda(f8), h, w, fmt8)


def test_refusals_leave_everything_untouched(S):
    """FDN_ERR_ARG before any launch - out, the workspace and the optional outputs keep what they held"""
    a = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device="cuda:0")
    for h, w, entry, kw in ((0, 16, "u8", {}), (16, 0, "u8", {}), (16, 16, "luma", dict(bits=9, stride=256)), (16, 16, "luma", dict(bits=8, stride=255))):
        code, _, out, ws, mscn, var, cls = raw_call(S, a, 1, h, w, entry, **kw)
        assert code == 1 and all((t == -1).all() for t in (out, ws, mscn, var)) and (cls == 255).all(), (h, w, entry, kw)
    check_argument_errors(S.lib())                                                    # where a launch would have had a GPU to run on
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# the command lines, through main(argv)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clis(S):
    sys.path.insert(0, PKG)
    import calculate_piqe
    import calculate_video_metrics
    import validate_fdn
    return calculate_piqe, calculate_video_metrics, validate_fdn


def test_calculate_piqe(S, clis, tmp_path, capsys):
    from PIL import Image
    tool = clis[0]
    imgs = {"a": image((47, 95), 0)[0], "b": image((47, 95), 1)[0], "c": image((33, 65), 0)[0]}
    (tmp_path / "in").mkdir()
    for k, v in imgs.items():
        Image.fromarray(v).save(tmp_path / "in" / f"{k}.png")
    want = {k: ref.result_u8(v) for k, v in imgs.items()}
    tool.main(["--input", str(tmp_path / "in"), "--batch", "2", "--csv", str(tmp_path / "p.csv"), "--masks", str(tmp_path / "m")])
    text = capsys.readouterr().out.splitlines()
    assert text[:3] == [f"{i+1:3d}: {k:25}. \tPIQE: {want[k]['piqe']:.6f} ({want[k]['nhsa']} active blocks)" for i, k in enumerate("abc")]
    assert text[3] == str(tmp_path / "in") and text[4] == f"Average: PIQE: {sum(want[k]['piqe'] for k in 'abc') / 3:.6f}" and len(text) == 5
    lines = (tmp_path / "p.csv").read_text().splitlines()
    assert lines[0] == "image,piqe,active_blocks" and [l.split(",")[1:] for l in lines[1:]] == [[repr(want[k]["piqe"]), str(want[k]["nhsa"])] for k in "abc"]
    for k, v in imgs.items():
        for name, bit in (("active", 1), ("wndc", 2), ("wnc", 4)):
            png = np.array(Image.open(tmp_path / "m" / f"{k}_{name}.png"))
            up = np.repeat(np.repeat(((want[k]["cls"] & bit) != 0).astype(np.uint8) * 255, 16, 0), 16, 1)[:v.shape[0], :v.shape[1]]
            assert png.dtype == np.uint8 and np.array_equal(png, up), (k, name)


def test_validate_fdn(S, clis, tmp_path, capsys):
    from PIL import Image
    from basicsr.models.archs.FDN_arch import FDN
    from fdn_hip import harness
    tool = clis[2]
    for d in ("gt", "lq"):
        (tmp_path / d).mkdir()
    gts = [image((48, 64), s)[0] for s in (3, 4)]
    lqs = [(g // 3).astype(np.uint8) for g in gts]
    for i in range(2):
        Image.fromarray(gts[i]).save(tmp_path / "gt" / f"f{i}.png")
        Image.fromarray(lqs[i]).save(tmp_path / "lq" / f"f{i}.png")
    torch.save({"params": fdn_weights(tame=0.03)}, tmp_path / "fdn.pth")
    base = ["--fdn", str(tmp_path / "fdn.pth"), "--lq", str(tmp_path / "lq" / "*.png"), "--gt", str(tmp_path / "gt" / "*.png")]
    tool.main(base + ["--csv", str(tmp_path / "plain.csv")])
    plain = capsys.readouterr().out.splitlines()
    tool.main(base + ["--piqe", "--csv", str(tmp_path / "piqe.csv")])
    more = capsys.readouterr().out.splitlines()
    net = FDN()
    net.load_state_dict(fdn_weights(tame=0.03), strict=True)
    net = net.to("cuda:0").eval()
    gt, lq = cuda(np.stack(gts)), cuda(np.stack(lqs))
    out, psnr, ssim, ratio = harness.validate_u8(net, None, lq, gt, ratio_mode="gt", bgr=False)
    pr, pg = [r["piqe"] for r in S.piqe_u8(out)], [ref.result_u8(g)["piqe"] for g in gts]
    assert [r["piqe"] for r in S.piqe_u8(gt)] == pg
    old = [f"{i+1:3d}: {'f%d' % i:25}. \tPSNR: {psnr[i]:.6f} dB, \tSSIM: {ssim[i]:.6f}" for i in range(2)] + \
          [f"Average: PSNR: {sum(psnr) / 2:.6f} dB, SSIM: {sum(ssim) / 2:.6f}"]
    assert plain == old                                                                  # without the flag the output is what it was
    assert more == [l + f", \tPIQE: {a:.6f} (gt {b:.6f})" for l, a, b in zip(old[:2], pr, pg)] + [old[2] + f", PIQE: {sum(pr) / 2:.6f} (gt {sum(pg) / 2:.6f})"]
    lines, plain_csv = (tmp_path / "piqe.csv").read_text().splitlines(), (tmp_path / "plain.csv").read_text().splitlines()
    assert lines[0] == "frame,psnr,ssim,ratio,piqe,piqe_gt" and plain_csv[0] == "frame,psnr,ssim,ratio"
    assert lines[1:] == [l + f",{a!r},{b!r}" for l, a, b in zip(plain_csv[1:], pr, pg)]


def y4m(frames, w, h, bits):
    tag = b"C420p10" if bits == 10 else b"C420"
    return b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 %s\n" % (w, h, tag) + b"".join(b"FRAME\n" + f.astype("<u2" if bits == 10 else np.uint8).tobytes() for f in frames)


@pytest.mark.parametrize("with_ref", [False, True], ids=["alone", "ref"])
@pytest.mark.parametrize("bits", [8, 10])
def test_calculate_video_metrics(S, Hn, clis, tmp_path, capsys, bits, with_ref):
    """a 3-frame 48 x 80 Y4M stream, with and without --ref, with and without --piqe: without the flag stdout and the CSV are the lines
    the tool's own (unchanged) frame_line and csv_row form from VideoScore's records; with it every frame line and the Average line gain
    `, PIQE-Y` at the very end, the CSV its last columns, and nothing else changes"""
    from fdn_hip import video_metrics as vm
    tool = clis[1]
    h, w, pix = 48, 80, "yuv420p10le" if bits == 10 else "yuv420p"
    df, gf = ref.luma_frames(3, h, w, bits, seed=5), ref.luma_frames(3, h, w, bits, seed=9)
    if bits == 10:                                                                      # a Y4M stream holds codes up to 1023
        df, gf = np.minimum(df, np.uint16(1023)), np.minimum(gf, np.uint16(1023))
    (tmp_path / "dist.y4m").write_bytes(y4m(df, w, h, bits))
    (tmp_path / "ref.y4m").write_bytes(y4m(gf, w, h, bits))
    argv = (["--ref", str(tmp_path / "ref.y4m")] if with_ref else []) + [str(tmp_path / "dist.y4m"), "--batch", "2"]
    outs = {}
    for flag in (False, True):
        tool.main(argv + ["--csv", str(tmp_path / f"c{int(flag)}.csv")] + (["--piqe"] if flag else []))
        cap = capsys.readouterr()
        assert "3 frames scored" in cap.err
        outs[flag] = (cap.out.rstrip("\n").split("\n"), (tmp_path / f"c{int(flag)}.csv").read_text().splitlines())
    (plain, plain_csv), (more, more_csv) = outs[False], outs[True]
    fmt = Hn.VideoFormat(pix, "bt601", False, "left")
    recs = vm.VideoScore(h, w, fmt, device="cuda:0").update(cuda(df), cuda(gf) if with_ref else None)
    assert plain[:3] == [tool.frame_line(i, r, with_ref) for i, r in enumerate(recs)] and plain[3].startswith("Average: ")
    assert plain_csv == [",".join(tool.CSV_COLUMNS)] + [tool.csv_row(i, r) for i, r in enumerate(recs)]
    pd = [ref.plane_result(*ref.plane_luma(f, h, w, bits))["piqe"] for f in df]
    pg = [ref.plane_result(*ref.plane_luma(f, h, w, bits))["piqe"] for f in gf] if with_ref else [None] * 3
    tail = lambda a, b: f", PIQE-Y {a:.6f}" + (f" (ref {b:.6f})" if with_ref else "")      # noqa: E731
    assert more[:3] == [l + tail(a, b) for l, a, b in zip(plain[:3], pd, pg)]
    assert more[3] == plain[3] + tail(math.fsum(pd) / 3, math.fsum(pg) / 3 if with_ref else None) and more[4:] == plain[4:]
    assert more_csv[0] == plain_csv[0] + ",piqe_y" + (",piqe_y_ref" if with_ref else "")
    assert more_csv[1:] == [l + "," + repr(a) + ("," + repr(b) if with_ref else "") for l, a, b in zip(plain_csv[1:], pd, pg)]
