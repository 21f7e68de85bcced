"""CPU: the host side of tiled inference from uint8 frames (fdn_hip.tiling / fdn_hip.harness, the drivers' --tile flags, and the tiles of
one frame over two gloo ranks).  No GPU compute: origins are arithmetic, the two ABI 21 entry points refuse bad arguments before any
launch, and run_tiles_sharded is scatter / gather plumbing around an injected torch forward."""
import argparse
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
import fdn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")

# frame, tile, row origins | column origins: the shapes of tests/test_gpu_tiled.py, computed with the reference's rule
SHAPES = [((70, 90), (64, 64), [0, 6], [0, 26]),
          ((33, 65), (32, 32), [0, 1], [0, 17, 33]),
          ((100, 200), (64, 96), [0, 36], [0, 52, 104]),
          ((96, 128), (64, 64), [0, 32], [0, 64]),
          ((96, 160), (96, 160), [0], [0])]


@pytest.fixture(scope="module")
def lib():
    import fdn_hip
    if not os.path.isfile(fdn_hip.lib_path()):
        entry.build()
    return fdn_hip.lib()


def test_tile_origins_without_overlap_are_the_reference_rule():
    from fdn_hip import tiling
    for (h, w), (ch, cw), rows, cols in SHAPES:
        assert tiling.tile_origins(h, w, ch, cw) == [(i, j) for i in rows for j in cols]
    n = 0
    for h in range(32, 300, 7):
        for w in range(32, 420, 11):
            for ch in range(32, h + 1, 32):
                for cw in range(32, w + 1, 64):
                    assert tiling.tile_origins(h, w, ch, cw) == tiling.tile_origins(h, w, ch, cw, overlap=0) == O.grids_indices(h, w, ch, cw)[2]
                    n += 1
    assert n > 5000


def _axis(n, c, v):
    """the origins along one axis: a frame n x c cut with tiles c x c has one column, so its rows are the axis"""
    from fdn_hip import tiling
    return [i for i, _ in tiling.tile_origins(n, c, c, c, overlap=v)]


def test_tile_origins_with_overlap():
    """every n in 32..699, every crop that is a multiple of 32, v in {8, 16, 31}: ceil((n - v) / (c - v)) tiles, the first at 0, the last at
    n - c, the axis covered, neighbours sharing at least v pixels"""
    for v in (8, 16, 31):
        for n in range(32, 700):
            for c in range(32, n + 1, 32):
                org = _axis(n, c, v)
                want = 1 if c >= n else -(-(n - v) // (c - v))
                assert len(org) == want, (n, c, v, org)
                assert org[0] == 0 and org[-1] == n - c and org == sorted(set(org)), (n, c, v, org)
                assert all(b - a <= c - v for a, b in zip(org, org[1:])), (n, c, v, org)      # no gap, and >= v shared pixels
    # the reason for the parameter: the reference's rule leaves no overlap when the side is a multiple of the crop
    assert _axis(128, 64, 0) == [0, 64] and _axis(128, 64, 16) == [0, 32, 64]
    from fdn_hip import FdnHipError, tiling
    for bad in (-1, 32, 40):
        with pytest.raises(FdnHipError, match="overlap"):
            tiling.tile_origins(96, 96, 32, 64, overlap=bad)


def test_auto_tile_and_the_effective_crop():
    from fdn_hip import FdnHipError, harness, tiling
    assert tiling.WHOLE_FRAME_MAX_PIXELS == 1088 * 1920
    assert tiling.auto_tile(1088, 1920) is None and tiling.auto_tile(1080, 1920) is None          # pads to the constant: still whole
    assert tiling.auto_tile(1089, 1920) == (736, 1280) and tiling.auto_tile(1088, 1921) == (736, 1280)
    assert tiling.auto_tile(3000, 4000) == (736, 1280)
    assert tiling.auto_tile(700, 4000) == (672, 1280) and tiling.auto_tile(5000, 1000) == (736, 992)   # clipped to whole 32-pixel blocks
    assert len(tiling.tile_origins(3000, 4000, 736, 1280)) == 20
    assert harness.resolve_tile(None, 3000, 4000) is None and harness.resolve_tile("auto", 720, 1280) is None
    assert harness.resolve_tile("auto", 3000, 4000) == (736, 1280) and harness.resolve_tile((64, 96), 720, 1280) == (64, 96)
    with pytest.raises(ValueError):
        harness.resolve_tile("on", 64, 64)
    # a tile larger than the frame is clipped per axis to the frame's whole blocks
    assert tiling.effective_crop(70, 90, 64, 64) == (64, 64) and tiling.effective_crop(40, 72, 64, 64) == (32, 64)
    assert tiling.effective_crop(33, 65, 736, 1280) == (32, 64) and tiling.effective_crop(96, 160, 96, 160) == (96, 160)
    for h, w in ((31, 90), (70, 20)):
        with pytest.raises(FdnHipError, match="untiled path"):
            tiling.effective_crop(h, w, 64, 64)
    for ch, cw in ((48, 64), (64, 0), (-32, 64)):
        with pytest.raises(FdnHipError, match="multiples of 32"):
            tiling.effective_crop(70, 90, ch, cw)
    # the uint8 pair has no host fallback either
    with pytest.raises(FdnHipError, match="ROCm"):
        tiling.split_u8(torch.zeros(70, 90, 3, dtype=torch.uint8), 64, 64)
    with pytest.raises(FdnHipError):
        tiling.merge_u8(torch.zeros(4, 3, 64, 64), torch.zeros(4, 2, dtype=torch.int32), 70, 90)
    with pytest.raises(FdnHipError, match=r"\[5,1\]"):
        tiling.run_tiles(None, torch.zeros(5, 3, 32, 32), torch.zeros(4, 1))


def test_u8_tile_entry_points_validate_arguments_without_gpu(lib):
    """NULL pointers / bad sizes are rejected before any launch (FDN_ERR_ARG = 1)"""
    import ctypes
    import fdn_hip
    assert lib.fdn_abi_version() == fdn_hip.ABI_VERSION == 22
    p = ctypes.c_void_p(64)                          # never dereferenced: every call below fails its argument check
    for f in (lib.fdn_tiles_gather_u8, lib.fdn_tiles_merge_u8):
        assert f(None, p, p, 4, 70, 90, 64, 64, 1, None) == 1
        assert f(p, None, p, 4, 70, 90, 64, 64, 1, None) == 1
        assert f(p, p, None, 4, 70, 90, 64, 64, 1, None) == 1
        assert f(p, p, p, 0, 70, 90, 64, 64, 1, None) == 1
        assert f(p, p, p, 65536, 70, 90, 64, 64, 1, None) == 1
        assert f(p, p, p, 4, 0, 90, 64, 64, 1, None) == 1 and f(p, p, p, 4, 70, -1, 64, 64, 1, None) == 1
        assert f(p, p, p, 4, 70, 90, 0, 64, 1, None) == 1 and f(p, p, p, 4, 70, 90, 64, 0, 1, None) == 1
        assert f(p, p, p, 4, 70, 90, 96, 64, 1, None) == 1 and f(p, p, p, 4, 70, 90, 64, 96, 1, None) == 1     # ch > h, cw > w


def test_tile_flag_parsing(tmp_path, capsys):
    import inference_fdn_lolblur as drv
    import validate_fdn
    assert drv.tile_arg("384x640") == (384, 640) and drv.tile_arg("64X96") == (64, 96)
    assert drv.tile_arg("auto") == "auto" and drv.tile_arg("off") is None
    for bad in ("100x100", "64", "64x", "0x64", "-32x64", "64x96x3", "big"):
        with pytest.raises(argparse.ArgumentTypeError):
            drv.tile_arg(bad)
    ap = argparse.ArgumentParser()
    drv.add_tile_args(ap)
    a = ap.parse_args([])
    assert (a.tile, a.tile_overlap, a.tile_ratio) == (None, 0, "frame")
    a = ap.parse_args(["--tile", "384x640", "--tile-overlap", "16", "--tile-ratio", "tile"])
    assert (a.tile, a.tile_overlap, a.tile_ratio) == ((384, 640), 16, "tile")
    with pytest.raises(SystemExit):
        ap.parse_args(["--tile", "100x100"])
    assert "multiples of 32" in capsys.readouterr().err
    sweep = argparse.ArgumentParser()
    drv.add_tile_args(sweep, ratio_default=None)                   # the sweep driver: its ratio is fixed
    assert not hasattr(sweep.parse_args(["--tile", "auto"]), "tile_ratio")
    # validate_fdn.py: val.grids takes the ratio per tile
    from PIL import Image
    import numpy as np
    for d in ("lq", "gt"):
        (tmp_path / d).mkdir()
        Image.fromarray(np.zeros((40, 72, 3), np.uint8)).save(tmp_path / d / "f0.png")
    base = ["--fdn", "x.pth", "--lq", str(tmp_path / "lq" / "*.png"), "--gt", str(tmp_path / "gt" / "*.png")]
    a = validate_fdn.parse_args(base)
    assert (a.tile, a.tile_overlap, a.tile_ratio) == (None, 0, "tile")
    a = validate_fdn.parse_args(base + ["--tile", "64x64", "--tile-ratio", "frame"])
    assert (a.tile, a.tile_ratio) == ((64, 64), "frame")
    with pytest.raises(SystemExit):
        validate_fdn.parse_args(base + ["--tile", "100x100"])


def test_large_frame_hint(capsys):
    import inference_fdn_lolblur as drv
    drv._hinted = False
    drv.hint_large_frame(None, 70, 90)
    drv.hint_large_frame(None, 1080, 1920)
    drv.hint_large_frame("auto", 3000, 4000)
    drv.hint_large_frame((736, 1280), 3000, 4000)
    assert capsys.readouterr().err == ""
    drv.hint_large_frame(None, 3000, 4000)
    drv.hint_large_frame(None, 3000, 4000)                          # once per run
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "--tile auto" in err
    drv._hinted = False


def _forward(tiles, ratio):
    return tiles * ratio.view(-1, 1, 1, 1) + 1


def _sharded_worker(rank, world, port, q):
    sys.path.insert(0, PKG)
    from fdn_hip import tiling
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    seen, results = [], []

    def forward(t, r):
        seen.append((t.shape[0], r.shape[0]))
        return _forward(t, r)

    for T in (1, 5, 8):                                            # T = 1: rank 1 receives nothing
        g = torch.Generator().manual_seed(T)
        tiles, ratio = torch.rand(T, 3, 32, 64, generator=g), torch.rand(T, 1, generator=g)
        out = tiling.run_tiles_sharded(dist, forward, T, torch.empty(1, 3, 32, 64), tiles if rank == 0 else None, ratio if rank == 0 else None)
        results.append(out is None if rank else torch.equal(out, _forward(tiles, ratio)))
    want_seen = [(1, 1), (3, 3), (4, 4)] if rank == 0 else [(2, 2), (4, 4)]
    # the drivers' protocol on the same group: the root announces each frame's (T, ch, cw) and None at the end
    if rank == 0:
        for T, ch, cw in ((3, 32, 32), (1, 64, 32)):
            g = torch.Generator().manual_seed(10 + T)
            tiles, ratio = torch.rand(T, 3, ch, cw, generator=g), torch.rand(T, 1, generator=g)
            results.append(torch.equal(tiling.run_tiles_root(dist, _forward, tiles, ratio), _forward(tiles, ratio)))
        tiling.end_serving(dist)
    else:
        tiling.serve_tiles(dist, _forward, torch.device("cpu"))
    flags = [None] * world
    dist.all_gather_object(flags, all(results) and seen == want_seen)
    if rank == 0:
        q.put(flags)
    dist.destroy_process_group()


def test_run_tiles_sharded_over_two_gloo_ranks():
    """T in {1, 5, 8} over two ranks: bit-equal to the direct call on the root, None elsewhere, every rank's forward sees exactly its own
    tiles and ratios (none at all on a rank without a tile); then serve_tiles / run_tiles_root / end_serving, the drivers' loop"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35300 + os.getpid() % 2000
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    flags = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
    assert flags == [True, True]
