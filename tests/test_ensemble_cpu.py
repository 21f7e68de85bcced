"""CPU: the host side of the geometric self-ensemble - the restatement of tests/d4_ref.py judged on its own, the entry points of
include/fdn_ensemble.h (version, prototype table, every refusal before any launch), what fdn_hip.ensemble and the `ensemble` keyword of
fdn_hip.harness / fdn_hip.tiling refuse before anything runs, and the drivers' --ensemble.  No GPU compute."""
import argparse
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
import d4_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fdn_ensemble_abi_version", "fdn_d4_pre_u8", "fdn_d4_apply", "fdn_d4_mean", "fdn_d4_post_u8"]


@pytest.fixture(scope="module")
def lib():
    import fdn_hip
    if not os.path.isfile(fdn_hip.lib_path()):
        entry.build()
    return fdn_hip.lib()


def test_eight_codes_are_distinct_and_invert():
    a = np.arange(3 * 5 * 7).reshape(3, 5, 7)
    seen = [ref.transform(a, k, (1, 2)) for k in range(8)]
    for k, t in enumerate(seen):
        assert t.shape == (3,) + ref.d4_shape(k, 5, 7)
        assert np.array_equal(ref.inverse(t, k, (1, 2)), a), k
        for j in range(k):
            assert seen[j].shape != t.shape or not np.array_equal(seen[j], t), (j, k)
    # the definition, element by element: mirrors first, then the transposition
    assert seen[1][0, 0, 0] == a[0, 0, 6] and seen[2][0, 0, 0] == a[0, 4, 0] and seen[3][0, 0, 0] == a[0, 4, 6]
    assert seen[4][0, 1, 2] == a[0, 2, 1] and seen[5][0, 1, 2] == a[0, 2, 5] and seen[6][0, 1, 2] == a[0, 2, 1] and seen[7][0, 1, 2] == a[0, 2, 5]
    assert seen[5][0, 0, 0] == a[0, 0, 6] and seen[6][0, 0, 0] == a[0, 4, 0]
    # the same on torch tensors, and with the axes named from the end
    t = torch.from_numpy(a)
    for k in range(8):
        assert np.array_equal(ref.transform(t, k, (-2, -1)).numpy(), seen[k])
        assert torch.equal(ref.inverse(ref.transform(t, k, (1, 2)), k, (1, 2)), t)


def test_restatement_padding_and_mean():
    assert list(ref.reflect_index(5, 8)) == [0, 1, 2, 3, 4, 3, 2, 1]
    assert list(ref.reflect_index(33, 35)) == list(range(33)) + [31, 30]
    with pytest.raises(AssertionError):
        ref.reflect_index(5, 10)
    x = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 4)
    want = torch.nn.functional.pad(x[None], (0, 3, 0, 2), mode="reflect")[0]
    assert torch.equal(ref.reflect_pad(x, 5, 7), want)
    # the ordered sum is not the exact one: 1e8 + 3 + 3 + 3 in fp32 stays 1e8, the other order does not
    t = [torch.tensor([v], dtype=torch.float32) for v in (1e8, 3.0, 3.0, 3.0)]
    assert ref.ordered_mean(t).item() == np.float32(1e8) / np.float32(4)
    assert ref.ordered_mean(t[::-1]).item() != ref.ordered_mean(t).item()
    third = ref.ordered_mean([torch.tensor([v], dtype=torch.float32) for v in (0.1, 0.2, 0.4)]).item()
    assert third == np.float32(np.float32(np.float32(0.1) + np.float32(0.2)) + np.float32(0.4)) / np.float32(3)
    # mean_back of transformed copies of one image is that image
    img = torch.rand(2, 3, 5, 7)
    res = {k: ref.reflect_pad(ref.transform(img, k, (-2, -1)), *[n + 2 for n in ref.d4_shape(k, 5, 7)]) for k in range(8)}
    assert torch.allclose(ref.mean_back(res, 0xFF, 5, 7), img, atol=1e-6)
    assert torch.equal(ref.mean_back(res, 0x10, 5, 7), img)


def test_masks_and_shapes():
    from fdn_hip import ensemble as ens
    assert ens.MASKS == ref.MASKS == {1: 0x01, 2: 0x03, 4: 0x0F, 8: 0xFF}
    for k in range(8):
        assert ens.d4_shape(k, 33, 65) == ref.d4_shape(k, 33, 65) == ((65, 33) if k >= 4 else (33, 65))
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            ens.d4_shape(bad, 3, 4)
    assert ens.codes(0xFF) == list(range(8)) and ens.codes(0x0B) == [0, 1, 3] and ens.codes(0x80) == [7]
    for bad in (0, 256, -1, 1.0, True, None):
        with pytest.raises(ValueError):
            ens.codes(bad)
    for e, m in ens.MASKS.items():
        assert ens.check_ensemble(e) == m and len(ens.codes(m)) == e


def test_version_and_prototype_table(lib):
    """the entry points of include/fdn_ensemble.h in the one table (tests/test_host_cpu.py holds it to the headers): names, signatures"""
    from fdn_hip._abi import HEADERS, PROTOTYPES
    assert HEADERS["fdn_ensemble.h"] == NAMES
    assert PROTOTYPES["fdn_d4_pre_u8"] == ("I", ["P", "P"] + ["I"] * 7 + ["P"])
    assert PROTOTYPES["fdn_d4_apply"] == ("I", ["P", "P"] + ["I"] * 6 + ["P"])
    assert PROTOTYPES["fdn_d4_mean"] == ("I", ["P", "P", "P"] + ["I"] * 8 + ["P"])
    assert PROTOTYPES["fdn_d4_post_u8"] == ("I", ["P", "P", "P"] + ["I"] * 9 + ["P"])
    assert lib.fdn_d4_mean.argtypes == [ctypes.c_void_p] * 3 + [ctypes.c_int] * 8 + [ctypes.c_void_p]
    build_sh = open(os.path.join(ROOT, "fdn-tip2025_amd", "build.sh")).read()
    assert "../include/*.h" in [ln for ln in build_sh.splitlines() if ln.startswith("NEWEST_HDR=")][0]      # the header triggers a rebuild


def test_entry_points_validate_arguments_without_gpu(lib):
    """every refusal of include/fdn_ensemble.h returns FDN_ERR_ARG = 1 before any launch"""
    p = ctypes.c_void_p(64)                          # never dereferenced: every call below fails its argument check

    def pre(img=p, out=p, B=1, h=33, w=65, H=64, W=96, mask=0x0F, swap_rb=1):
        return lib.fdn_d4_pre_u8(img, out, B, h, w, H, W, mask, swap_rb, None)

    def app(x=p, out=p, B=1, h=33, w=65, H=64, W=96, mask=0x0F):
        return lib.fdn_d4_apply(x, out, B, h, w, H, W, mask, None)
    for f in (pre, app):
        assert f(**{"img" if f is pre else "x": None}) == 1 and f(out=None) == 1
        assert f(B=0) == 1 and f(B=-1) == 1 and f(B=65536) == 1
        assert f(h=0) == 1 and f(w=0) == 1 and f(h=-3) == 1 and f(w=-3) == 1
        for mask in (0, 256, -1, 0x1FF, 0x100):
            assert f(mask=mask) == 1, mask
        for mask in (0x11, 0xFF, 0x18, 0x81, 0x3C):                                    # codes on both sides of bit 4
            assert f(mask=mask) == 1, mask
        assert f(H=32) == 1 and f(W=64) == 1                                           # H < h', W < w'
        assert f(mask=0xF0, H=64, W=96) == 1 and f(mask=0x10, H=96, W=32) == 1         # transposed: h' x w' = 65 x 33
        assert f(h=5, w=7, H=32, W=32) == 1 and f(h=5, w=7, H=10, W=7) == 1 and f(h=5, w=7, H=5, W=14) == 1      # pad >= size
        assert f(h=5, w=7, H=7, W=10, mask=0x40) == 1 and f(h=5, w=7, H=14, W=5, mask=0x40) == 1
        assert f(h=40000, w=8, H=65536, W=8) == 1 and f(h=8, w=40000, H=65536, W=8, mask=0x20) == 1            # grid limit

    def mean(a=p, b=p, out=p, B=1, h=33, w=65, Ha=64, Wa=96, Hb=96, Wb=64, mask=0xFF):
        return lib.fdn_d4_mean(a, b, out, B, h, w, Ha, Wa, Hb, Wb, mask, None)

    def post(a=p, b=p, out=p, B=1, h=33, w=65, Ha=64, Wa=96, Hb=96, Wb=64, mask=0xFF, swap_rb=0):
        return lib.fdn_d4_post_u8(a, b, out, B, h, w, Ha, Wa, Hb, Wb, mask, swap_rb, None)
    for f in (mean, post):
        assert f(out=None) == 1
        assert f(B=0) == 1 and f(B=-2) == 1 and f(B=65536) == 1
        assert f(h=0) == 1 and f(w=0) == 1 and f(h=-1) == 1
        for mask in (0, 256, -1, 0x1FF):
            assert f(mask=mask) == 1, mask
        assert f(a=None) == 1 and f(b=None) == 1 and f(a=None, b=None) == 1            # a buffer missing against the mask
        assert f(mask=0x0F) == 1 and f(mask=0xF0) == 1                                 # a buffer present against the mask
        assert f(a=None, mask=0x0F) == 1 and f(b=None, mask=0xF0) == 1 and f(a=None, b=None, mask=0x01) == 1
        assert f(Ha=32) == 1 and f(Wa=64) == 1 and f(Hb=64) == 1 and f(Wb=32) == 1     # H < h', W < w' on either side
        assert f(b=None, mask=0x03, Ha=32) == 1 and f(a=None, mask=0x30, Wb=32) == 1
        assert f(h=65536, w=8, Ha=65536, Wa=8, Hb=8, Wb=65536) == 1                     # grid limit


def test_wrappers_refuse_cpu_tensors_and_wrong_dtypes():
    from fdn_hip import FdnHipError
    from fdn_hip import ensemble as ens
    u8, f32 = torch.zeros(2, 33, 65, 3, dtype=torch.uint8), torch.zeros(2, 3, 32, 32)
    with pytest.raises(FdnHipError, match="ROCm"):
        ens.pre_u8(u8, 0x0F)
    with pytest.raises(FdnHipError, match="ROCm"):
        ens.apply(f32, 0xF0)
    with pytest.raises(FdnHipError, match="uint8"):
        ens.pre_u8(torch.zeros(2, 33, 65, 3), 0x01)
    with pytest.raises(FdnHipError, match="float32"):
        ens.apply(f32.double(), 0x01)
    with pytest.raises(FdnHipError, match=r"\[B,h,w,3\]"):
        ens.pre_u8(torch.zeros(33, 65, 3, dtype=torch.uint8), 0x01)
    with pytest.raises(FdnHipError, match=r"\[N,3,h,w\]"):
        ens.apply(torch.zeros(2, 4, 32, 32), 0x01)
    with pytest.raises(ValueError, match="both sides"):
        ens.pre_u8(u8, 0xFF)
    with pytest.raises(ValueError):
        ens.apply(f32, 0)
    with pytest.raises(FdnHipError, match="pad < size"):
        ens.pre_u8(torch.zeros(1, 5, 7, 3, dtype=torch.uint8), 0x01)
    res_a, res_b = torch.zeros(4, 2, 3, 64, 96), torch.zeros(4, 2, 3, 96, 64)
    for fn in (ens.mean, ens.post_u8):
        with pytest.raises(FdnHipError, match="ROCm"):
            fn(res_a, res_b, 0xFF, 33, 65)
        with pytest.raises(FdnHipError, match="float32"):
            fn(res_a.double(), res_b, 0xFF, 33, 65)
        with pytest.raises(FdnHipError, match="exactly when"):
            fn(res_a, None, 0xFF, 33, 65)
        with pytest.raises(FdnHipError, match="exactly when"):
            fn(res_a, res_b, 0x0F, 33, 65)
        with pytest.raises(ValueError):
            fn(res_a, res_b, 0, 33, 65)
    with pytest.raises(FdnHipError, match="ratio"):
        ens.forward_ensemble(None, u8, torch.ones(3, 1), 2)
    with pytest.raises(FdnHipError, match="batch"):
        ens.forward_ensemble(None, u8, torch.ones(2, 1), 2, batch=0)


def test_ensemble_outside_the_set_raises():
    from fdn_hip import ensemble as ens
    from fdn_hip import harness, tiling
    u8 = torch.zeros(1, 33, 65, 3, dtype=torch.uint8)
    for fn in (harness.enhance_u8, harness.validate_u8, harness.enhance_frame_tiled, tiling.run_tiles, tiling.forward_tiled):
        assert inspect.signature(fn).parameters["ensemble"].default == 1, fn.__name__
    for bad in (0, 3, 5, 16, -2, 2.5, "8", None, True):
        with pytest.raises(ValueError, match="ensemble"):
            ens.check_ensemble(bad)
        with pytest.raises(ValueError, match="ensemble"):
            ens.forward_ensemble(None, u8, torch.ones(1, 1), bad)
        with pytest.raises(ValueError, match="ensemble"):
            harness.enhance_u8(None, None, u8, ensemble=bad)
        with pytest.raises(ValueError, match="ensemble"):
            harness.enhance_u8(None, None, u8, tile=(32, 32), ensemble=bad)
        with pytest.raises(ValueError, match="ensemble"):
            harness.validate_u8(None, None, u8, u8, ensemble=bad)
        with pytest.raises(ValueError, match="ensemble"):
            harness.enhance_frame_tiled(None, None, u8[0], (32, 32), ensemble=bad)
        with pytest.raises(ValueError, match="ensemble"):
            tiling.run_tiles(None, torch.zeros(1, 3, 32, 32), torch.ones(1, 1), ensemble=bad)
        with pytest.raises(ValueError, match="ensemble"):
            tiling.forward_tiled(None, None, torch.zeros(1, 3, 64, 64), 32, 32, ensemble=bad)
    # a caller's run= serves one tile shape: refused with one line, before anything is read
    for e in (2, 4, 8):
        with pytest.raises(ValueError, match="run="):
            harness.enhance_frame_tiled(None, None, u8[0], (32, 32), run=lambda t, r: t, ensemble=e)


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


def test_ensemble_flag_in_the_four_command_lines(monkeypatch, capsys):
    import inference_fdn_lolblur
    import inference_fdn_lolv1
    import inference_fdn_multi_r
    import validate_fdn
    walk = ["--fdn", "x.pth", "--lpnet", "y.pth", "--input", "in/*.png", "--output", "out"]
    drivers = [(inference_fdn_lolblur.main, walk), (inference_fdn_lolv1.main, walk),
               (inference_fdn_multi_r.main, ["--fdn", "x.pth", "--input", "f.png"]),
               (validate_fdn.main, ["--fdn", "x.pth", "--lq", "lq/*.png", "--gt", "gt/*.png"])]
    for main, base in drivers:
        assert _parse(monkeypatch, main, base).ensemble == 1, main.__module__
        for e in (1, 2, 4, 8):
            assert _parse(monkeypatch, main, base + ["--ensemble", str(e)]).ensemble == e
        a = _parse(monkeypatch, main, base + ["--ensemble", "8", "--tile", "64x64", "--tile-blend", "feather"])
        assert (a.ensemble, a.tile, a.tile_blend) == (8, (64, 64), "feather")
        for bad in ("3", "0", "16", "x", "2.0", ""):
            with monkeypatch.context() as m:
                m.setattr(sys, "argv", ["driver"] + base + ["--ensemble", bad])
                with pytest.raises(SystemExit) as e:
                    main()
            assert e.value.code == 2 and "--ensemble" in capsys.readouterr().err, bad
    # more than one rank: refused with one line, before any model is built
    for main in (inference_fdn_lolblur.main, inference_fdn_lolv1.main):
        with monkeypatch.context() as m:
            m.setenv("WORLD_SIZE", "2")
            m.setattr(sys, "argv", ["driver"] + walk + ["--tile", "64x64", "--ensemble", "2"])
            with pytest.raises(SystemExit) as e:
                main()
        assert e.value.code == 2 and "one GPU" in capsys.readouterr().err
