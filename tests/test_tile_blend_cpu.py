"""CPU: the host side of the feathered tile merge (fdn_hip.tiling.feather_weights, blend=, the drivers' --tile-blend) and what it is for -
no step at a tile seam - shown on a float64 restatement of both merges (tests/tile_blend_ref.py).  No GPU compute: the weights are
arithmetic, and fdn_tiles_merge_w / fdn_tiles_merge_w_u8 refuse bad arguments before any launch."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
from tile_blend_ref import largest_step, merge64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import fdn_hip
    if not os.path.isfile(fdn_hip.lib_path()):
        entry.build()
    return fdn_hip.lib()


def _ramps(org, c):
    """(lo, hi) per tile along an axis with sorted unique origins org"""
    lo = [0] + [max(0, a + c - b) for a, b in zip(org, org[1:])]
    hi = [max(0, a + c - b) for a, b in zip(org, org[1:])] + [0]
    return list(zip(lo, hi))


# frame, tile, overlap: no pixel under more than two tiles per axis in the first two; up to four per axis in the third
CASES = [((70, 90), (32, 32), 8), ((40, 50), (32, 32), 0), ((70, 90), (32, 32), 20), ((64, 96), (32, 32), 0), ((32, 32), (32, 32), 0),
         ((3000, 4000), (736, 1280), 0)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-v{c[2]}")
def test_feather_weights(case):
    """positive; 1 outside the ramps and on sides at the frame border or without an overlapping neighbour; float64 formula rounded once;
    where exactly two tiles share a band their ramps sum to 1 within 1e-6 (exact in float64, 2^-24 of rounding on each float32 weight)"""
    from fdn_hip import tiling
    (h, w), (ch, cw), v = case
    idx = tiling.tile_origins(h, w, ch, cw, v)
    wy, wx = tiling.feather_weights(idx, ch, cw)
    assert wy.dtype == wx.dtype == torch.float32 and wy.shape == (len(idx), ch) and wx.shape == (len(idx), cw)
    assert float(wy.min()) > 0 and float(wx.min()) > 0 and float(wy.max()) == 1.0 == float(wx.max())
    for wgt, c, n, pick in ((wy, ch, h, 0), (wx, cw, w, 1)):
        org = sorted({o[pick] for o in idx})
        ramps = dict(zip(org, _ramps(org, c)))
        for t, o in enumerate(idx):
            lo, hi = ramps[o[pick]]
            got = wgt[t].numpy()
            d = np.arange(c, dtype=np.float64)
            want = np.ones(c)
            if lo:
                want[:lo] = np.minimum(want[:lo], (d[:lo] + 0.5) / lo)
            if hi:
                want[c - hi:] = np.minimum(want[c - hi:], (c - d[c - hi:] - 0.5) / hi)
            assert np.array_equal(got, want.astype(np.float32)), (t, o)
            assert np.all(got[lo:c - hi] == 1.0)                                           # outside the ramps
            if o[pick] == 0:
                assert lo == 0 and got[0] == 1.0                                           # the frame's border
            if o[pick] == n - c:
                assert hi == 0 and got[-1] == 1.0
        # along the axis: where exactly two tiles cover a position, their weights sum to 1
        first = {o[pick]: t for t, o in reversed(list(enumerate(idx)))}
        for p in range(n):
            over = [o for o in org if o <= p < o + c]
            if len(over) == 2:
                s = sum(float(wgt[first[o]][p - o]) for o in over)
                assert abs(s - 1.0) <= 1e-6, (p, over, s)


def test_ramp_lengths_of_a_twelve_megapixel_frame():
    """3000 x 4000 under --tile auto: 5 x 4 tiles of 736 x 1280, overlap bands of 170 rows and 373 / 373 / 374 columns"""
    from fdn_hip import tiling
    idx = tiling.tile_origins(3000, 4000, 736, 1280)
    assert len(idx) == 20
    wy, wx = tiling.feather_weights(idx, 736, 1280)

    def ramp_lengths(wgt):
        below = (wgt < 1).numpy()
        lo = [int(np.argmax(~r)) if r[0] else 0 for r in below]
        hi = [int(np.argmax(~r[::-1])) if r[-1] else 0 for r in below]
        return lo, hi
    lo, hi = ramp_lengths(wy)
    assert lo[::4] == [0, 170, 170, 170, 170] and hi[::4] == [170, 170, 170, 170, 0]
    lo, hi = ramp_lengths(wx)
    assert lo[:4] == [0, 373, 373, 374] and hi[:4] == [373, 373, 374, 0]
    assert float(wy[4][0]) == np.float32(0.5 / 170) and float(wx[3][0]) == np.float32(0.5 / 374)


def test_feather_weights_need_the_full_grid():
    from fdn_hip import FdnHipError, tiling
    idx = tiling.tile_origins(70, 90, 32, 32, 8)
    for bad in (idx[:-1], idx[1:], idx + [idx[0]], idx + [(5, 7)], []):
        with pytest.raises(FdnHipError, match="full grid"):
            tiling.feather_weights(bad, 32, 32)
    wy, wx = tiling.feather_weights(torch.tensor(idx, dtype=torch.int32).tolist(), 32, 32)       # as merge() passes them
    assert wy.shape == (len(idx), 32)


@pytest.mark.parametrize("case", CASES[:2], ids=["70x90-v8", "40x50-v0"])
def test_feathering_removes_the_step_at_a_seam(case):
    """Constant tiles delta_t, both merges in float64.  Feathered, the output moves along a ramp of length L by at most the spread of the
    tiles, in steps of 1/L of it (a half step where the ramp begins): the largest difference between adjacent pixels is at most
    (max delta - min delta) / (smallest ramp).  This needs at most two tiles over a pixel per axis (the output is then the bilinear
    blend of four constants), which both shapes have - 70 x 90 at overlap 20 does not, and is not asserted.  Averaged, a row that lies in
    one tile row only jumps from (A + B) / 2 to B where A ends: half of |delta_A - delta_B|, for every pair of neighbours."""
    from fdn_hip import tiling
    (h, w), (ch, cw), v = case
    idx = tiling.tile_origins(h, w, ch, cw, v)
    rows, cols = sorted({i for i, _ in idx}), sorted({j for _, j in idx})
    assert max(len([o for o in rows if o <= p < o + ch]) for p in range(h)) == 2
    assert max(len([o for o in cols if o <= p < o + cw]) for p in range(w)) == 2
    smallest = min(r for org, c in ((rows, ch), (cols, cw)) for lo, hi in _ramps(org, c) for r in (lo, hi) if r)
    wy, wx = tiling.feather_weights(idx, ch, cw)
    for seed in range(5):
        delta = np.random.default_rng(seed).random(len(idx))
        outs = np.broadcast_to(delta[:, None, None, None], (len(idx), 1, ch, cw))
        feather = largest_step(merge64(outs, idx, h, w, wy.numpy(), wx.numpy())[0])
        average = largest_step(merge64(outs, idx, h, w)[0])
        bound = (delta.max() - delta.min()) / smallest
        at = dict(zip(idx, delta))
        neighbours = [abs(at[(i, a)] - at[(i, b)]) for i in rows for a, b in zip(cols, cols[1:])] + \
                     [abs(at[(a, j)] - at[(b, j)]) for j in cols for a, b in zip(rows, rows[1:])]
        print(f"{h}x{w} overlap {v} seed {seed}: feathered step {feather:.4f} <= {bound:.4f} (smallest ramp {smallest}); averaged step "
              f"{average:.4f} >= {max(neighbours) / 2:.4f}")
        assert feather <= bound * (1 + 1e-6)                       # the float32 weights' rounding, 2^-24 each
        assert average >= max(neighbours) / 2 * (1 - 1e-12)


def test_weighted_entry_points_validate_arguments_without_gpu(lib):
    """NULL pointers / bad sizes are rejected before any launch (FDN_ERR_ARG = 1); the ABI version has not moved"""
    import ctypes
    import fdn_hip
    assert lib.fdn_abi_version() == fdn_hip.ABI_VERSION == 22
    p = ctypes.c_void_p(64)                          # never dereferenced: every call below fails its argument check
    for f, mid in ((lib.fdn_tiles_merge_w, (3,)), (lib.fdn_tiles_merge_w_u8, ())):
        def call(ptrs=(p, p, p, p, p), T=4, h=70, w=90, ch=64, cw=64):
            tail = (1,) if not mid else ()
            return f(*ptrs, T, *mid, h, w, ch, cw, *tail, None)
        for k in range(5):
            assert call(ptrs=tuple(None if n == k else p for n in range(5))) == 1, k
        assert call(T=0) == 1 and call(T=65536) == 1
        assert call(h=0) == 1 and call(w=-1) == 1 and call(ch=0) == 1 and call(cw=0) == 1
        assert call(ch=96) == 1 and call(cw=96) == 1                                       # ch > H, cw > W
    assert lib.fdn_tiles_merge_w(p, p, p, p, p, 4, 0, 70, 90, 64, 64, None) == 1 and lib.fdn_tiles_merge_w(p, p, p, p, p, 4, 65536, 70, 90, 64, 64, None) == 1


def test_abi_table_holds_the_new_entry_points():
    """the weighted merges in fdn_hip/_abi.py (tests/test_host_cpu.py holds the table to the headers, in their order)"""
    from fdn_hip._abi import ARG_NAMES, HEADERS, PROTOTYPES
    assert PROTOTYPES["fdn_tiles_merge_w"] == ("I", ["P"] * 5 + ["I"] * 6 + ["P"])
    assert PROTOTYPES["fdn_tiles_merge_w_u8"] == ("I", ["P"] * 5 + ["I"] * 6 + ["P"])
    assert ARG_NAMES["fdn_tiles_merge_w"] == ["tiles", "out", "ij", "wy", "wx", "T", "C", "H", "W", "ch", "cw", "stream"]
    assert ARG_NAMES["fdn_tiles_merge_w_u8"] == ["tiles", "out", "ij", "wy", "wx", "T", "h", "w", "ch", "cw", "swap_rb", "stream"]
    assert len(HEADERS["fdn_hip.h"]) == 74


def test_blend_keyword_is_checked_before_anything_runs(lib):
    """every function that takes blend= defaults to "average" and refuses another word with ValueError, without a GPU"""
    import inspect
    from fdn_hip import harness, tiling
    for fn in (tiling.merge, tiling.merge_u8, tiling.forward_tiled, harness.enhance_frame_tiled, harness.enhance_u8, harness.validate_u8):
        assert inspect.signature(fn).parameters["blend"].default == "average", fn.__name__
    outs, ij, img = torch.zeros(4, 3, 32, 32), torch.zeros(4, 2, dtype=torch.int32), torch.zeros(64, 64, 3, dtype=torch.uint8)
    for bad in ("linear", "Feather", None):
        for call in (lambda: tiling.merge(outs, ij, 64, 64, blend=bad), lambda: tiling.merge_u8(outs, ij, 64, 64, blend=bad),
                     lambda: tiling.forward_tiled(None, None, torch.zeros(1, 3, 64, 64), 32, 32, blend=bad),
                     lambda: harness.enhance_frame_tiled(None, None, img, (32, 32), blend=bad),
                     lambda: harness.enhance_u8(None, None, img, tile=(32, 32), blend=bad),
                     lambda: harness.enhance_u8(None, None, img, blend=bad),
                     lambda: harness.validate_u8(None, None, img, img, tile=(32, 32), blend=bad)):
            with pytest.raises(ValueError, match="blend"):
                call()
    # the feathered merge has no host fallback either
    with pytest.raises(tiling.FdnHipError, match="ROCm"):
        tiling.merge(outs, torch.tensor(tiling.tile_origins(64, 64, 32, 32), dtype=torch.int32), 64, 64, blend="feather")


class _Parsed(Exception):
    pass


def _parse(monkeypatch, main, argv):
    """the namespace a driver's main() parses from argv; main() is stopped there"""
    real = argparse.ArgumentParser.parse_args

    def grab(self, args=None, namespace=None):
        raise _Parsed(real(self, args, namespace))
    with monkeypatch.context() as m:
        m.setattr(argparse.ArgumentParser, "parse_args", grab)
        m.setattr(sys, "argv", ["driver"] + argv)
        with pytest.raises(_Parsed) as e:
            main()
    return e.value.args[0]


def test_tile_blend_flag_in_the_four_command_lines(monkeypatch, capsys):
    import inference_fdn_lolblur
    import inference_fdn_lolv1
    import inference_fdn_multi_r
    import validate_fdn
    walk = ["--fdn", "x.pth", "--lpnet", "y.pth", "--input", "in/*.png", "--output", "out"]
    drivers = [(inference_fdn_lolblur.main, walk), (inference_fdn_lolv1.main, walk),
               (inference_fdn_multi_r.main, ["--fdn", "x.pth", "--input", "f.png"]),
               (validate_fdn.main, ["--fdn", "x.pth", "--lq", "lq/*.png", "--gt", "gt/*.png"])]
    for main, base in drivers:
        a = _parse(monkeypatch, main, base)
        assert (a.tile, a.tile_overlap, a.tile_blend) == (None, 0, "average"), main.__module__
        assert _parse(monkeypatch, main, base + ["--tile-blend", "feather"]).tile_blend == "feather"      # without --tile: accepted, unused
        a = _parse(monkeypatch, main, base + ["--tile", "64x64", "--tile-overlap", "16", "--tile-blend", "feather"])
        assert (a.tile, a.tile_overlap, a.tile_blend) == ((64, 64), 16, "feather")
        assert _parse(monkeypatch, main, base + ["--tile", "auto", "--tile-blend", "average"]).tile_blend == "average"
        for bad in ("linear", "Feather", ""):
            with monkeypatch.context() as m:
                m.setattr(sys, "argv", ["driver"] + base + ["--tile-blend", bad])
                with pytest.raises(SystemExit) as e:
                    main()
            assert e.value.code == 2 and "--tile-blend" in capsys.readouterr().err
    ap = argparse.ArgumentParser()
    inference_fdn_lolblur.add_tile_args(ap, ratio_default=None)
    assert ap.parse_args([]).tile_blend == "average"


def test_hard_seam_hint(capsys):
    import inference_fdn_lolblur as drv
    drv._seam_hinted = False
    drv.hint_hard_seam(None, "feather", 0, 128, 128)                # no --tile: nothing to say
    drv.hint_hard_seam((64, 64), "average", 0, 128, 128)            # the reference's merge: its seams are the reference's
    drv.hint_hard_seam((64, 64), "feather", 16, 128, 128)           # an overlap on both axes
    drv.hint_hard_seam((64, 64), "feather", 0, 70, 90)              # the reference's walk overlaps whenever a side is no multiple
    drv.hint_hard_seam((64, 64), "feather", 0, 64, 64)              # one tile
    drv.hint_hard_seam("auto", "feather", 0, 720, 1280)             # left whole
    drv.hint_hard_seam((64, 64), "feather", 0, 20, 90)              # too small to tile: that error is enhance_u8's
    assert capsys.readouterr().err == ""
    drv.hint_hard_seam((64, 64), "feather", 0, 70, 128)             # columns 0, 64: no shared pixel
    drv.hint_hard_seam((64, 64), "feather", 0, 128, 128)            # once per run
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "--tile-overlap" in err and "columns" in err
    drv._seam_hinted = False
    drv.hint_hard_seam((64, 64), "feather", 0, 128, 90)
    assert "rows" in capsys.readouterr().err
    drv._seam_hinted = False
