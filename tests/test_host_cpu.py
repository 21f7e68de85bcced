"""CPU: host-side logic of the drop-in modules and the C-ABI library (no GPU compute)."""
import ctypes
import os
import re

import pytest
import torch

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
from common import fdn_shapes, fdn_weights, lpnet_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import fdn_hip
    if not os.path.isfile(fdn_hip.lib_path()):
        entry.build()
    return fdn_hip.lib()


def test_library_exports_every_declared_symbol(lib):
    hdr = open(os.path.join(ROOT, "include", "fdn_hip.h")).read()
    names = sorted(set(re.findall(r"\b(fdn_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"libfdn_hip.so does not export {n}"
    assert lib.fdn_abi_version() >= 1
    assert lib.fdn_error_string(1).decode().startswith("invalid argument")


@pytest.fixture(scope="module")
def gen():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_abi_table", os.path.join(ROOT, "tools", "gen_abi_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# header -> (entry points, version function, version): a new header is one row here and one entry of tools/gen_abi_table.py HEADERS
ABI = {"fdn_hip.h": (74, "fdn_abi_version", 22), "fdn_video.h": (3, "fdn_video_abi_version", 1),
       "fdn_temporal.h": (3, "fdn_temporal_abi_version", 1), "fdn_vmetrics.h": (4, "fdn_vmetrics_abi_version", 1),
       "fdn_ensemble.h": (5, "fdn_ensemble_abi_version", 1), "fdn_spectral.h": (5, "fdn_spectral_abi_version", 1),
       "fdn_lowlight.h": (7, "fdn_lowlight_abi_version", 1)}


@pytest.mark.parametrize("header", list(ABI))
def test_version_and_prototype_table(lib, gen, header):
    """fdn_hip/_abi.py holds, for every header of include/, exactly what it declares, in the headers' order and then the declarations';
    the library, the table and this test agree on each header's version"""
    import fdn_hip
    from fdn_hip._abi import ARG_NAMES, HEADERS, PROTOTYPES, VERSIONS
    assert list(HEADERS) == list(VERSIONS) == list(ABI) == gen.HEADERS
    count, fn, version = ABI[header]
    path = os.path.join(ROOT, "include", header)
    at = sum(ABI[h][0] for h in list(ABI)[:list(ABI).index(header)])
    assert HEADERS[header] == list(gen.parse_header(path)) and len(HEADERS[header]) == count
    assert list(PROTOTYPES.items())[at:at + count] == list(gen.parse_header(path).items())
    assert list(ARG_NAMES.items())[at:at + count] == list(gen.parse_names(path).items())
    assert len(PROTOTYPES) == len(ARG_NAMES) == sum(c for c, _, _ in ABI.values()) == 101
    assert VERSIONS[header] == (fn, version) == gen.parse_version(path) and fn in HEADERS[header]
    assert getattr(lib, fn)() == version
    assert fdn_hip.ABI_VERSION == 22
    assert fdn_hip.PART_ABI_VERSIONS == {"video": 1, "temporal": 1, "vmetrics": 1, "ensemble": 1, "spectral": 1, "lowlight": 1}


def test_generator_refuses_a_name_declared_twice(gen, tmp_path):
    """the tables of two headers cannot share a name: the generator raises instead of letting the later declaration win"""
    for h in ("fdn_hip.h", "fdn_video.h"):
        (tmp_path / h).write_text(open(os.path.join(ROOT, "include", h)).read())
    assert len(gen.build_table(["fdn_hip.h", "fdn_video.h"], str(tmp_path))[0]) == 77
    with open(tmp_path / "fdn_video.h", "a") as f:
        f.write("\nint fdn_chan_stats(int n);\n")
    with pytest.raises(ValueError, match="fdn_chan_stats"):
        gen.build_table(["fdn_hip.h", "fdn_video.h"], str(tmp_path))


def test_version_mismatch_is_refused(lib, monkeypatch):
    """a library that answers another version than the table's is refused by name and number, and nothing stays loaded"""
    import fdn_hip
    from fdn_hip import _abi
    monkeypatch.setattr(fdn_hip, "_lib", None)                   # (lib() afresh; the loaded library comes back when the test ends)
    monkeypatch.setitem(_abi.VERSIONS, "fdn_temporal.h", ("fdn_temporal_abi_version", 7))
    with pytest.raises(ImportError) as e:
        fdn_hip.lib()
    assert str(e.value) == f"{fdn_hip.lib_path()} has temporal ABI version 1, this binding needs 7: rebuild with build.sh"
    assert fdn_hip._lib is None
    monkeypatch.setitem(_abi.VERSIONS, "fdn_temporal.h", ("fdn_temporal_abi_version", 1))
    monkeypatch.setitem(_abi.VERSIONS, "fdn_hip.h", ("fdn_abi_version", 21))
    with pytest.raises(ImportError, match=r"libfdn_hip\.so has ABI version 22, this binding needs 21: rebuild with build\.sh$"):
        fdn_hip.lib()
    assert fdn_hip._lib is None


def test_ctypes_prototypes_match_header(lib, gen):
    """fdn_hip/_abi.py (argtypes of every entry point) holds exactly what include/fdn_hip.h declares, and the loader applied it."""
    import ctypes as C
    from fdn_hip._abi import HEADERS, PROTOTYPES
    assert {n: PROTOTYPES[n] for n in HEADERS["fdn_hip.h"]} == gen.parse_header(os.path.join(ROOT, "include", "fdn_hip.h"))
    assert lib.fdn_fdsa_fused.argtypes is not None and len(lib.fdn_fdsa_fused.argtypes) == len(PROTOTYPES["fdn_fdsa_fused"][1])
    with pytest.raises(C.ArgumentError):
        lib.fdn_fdsa_core(None, None, None, None, 1.5, 38, 32, 32, None)            # a float where an int belongs
    with pytest.raises(TypeError):
        lib.fdn_fdsa_core(None, None, None, None, 1, 38, 32, 32)          # one argument short


def test_argument_validation_without_gpu(lib):
    # NULL pointers / bad sizes are rejected before any launch
    assert lib.fdn_fdsa_core(None, None, None, None, 1, 38, 32, 32, None) == 1
    assert lib.fdn_rfft_rows(None, None, ctypes.c_long(4), 16, ctypes.c_long(0), None) == 1
    # (round 6) the one-launch FDSA route: sizes of its operand image / ring are host arithmetic, a width without a form has none
    assert lib.fdn_fdsa_fused_tail(None, ctypes.c_long(0), None, None, None, None, None, None, None, None, None, None, 1, 32, 38, 32, 32, 0, 0, None) == 1
    assert lib.fdn_fdsa_tail_pack_floats(32, 38, 32, 0) == 4096 and lib.fdn_fdsa_tail_pack_floats(32, 38, 32, 86) > 4096
    assert lib.fdn_fdsa_tail_pack_floats(64, 76, 64, 0) == 512 + 3 * 5 * 2 * 3 * 64 * 4 and lib.fdn_fdsa_tail_pack_floats(128, 153, 128, 0) == 0
    assert lib.fdn_fdsa_tail_pack_floats(48, 57, 48, 129) == 0                      # no project_in behind the C = 48 tail
    ring = lib.fdn_fdsa_scratch_floats(8, 38, 736, 1280)
    assert ring == lib.fdn_fdsa_scratch_floats(1, 38, 64, 64) == 16384 + 4096 * 4 * 38 * 256      # a ring: independent of the image
    # (ABI 16) the CU budget: below 0 or above the device's count is refused (without a device every non-zero budget is above it),
    # and the Python wrapper keeps no record of a refused one
    import fdn_hip
    assert lib.fdn_set_cu_budget(-1) == 1 and lib.fdn_set_cu_budget(1 << 20) == 1
    before = dict(fdn_hip._cu_budgets)
    for n in (-1, 1 << 20):
        with pytest.raises(fdn_hip.FdnHipError):
            fdn_hip.set_cu_budget(n)
    assert fdn_hip._cu_budgets == before


def test_state_dict_layout_matches_reference():
    from basicsr.models.archs.FDN_arch import FDN
    from basicsr.models.archs.LPNet_arch import I_predict_net
    net = FDN()
    sd = net.state_dict()
    ref = fdn_shapes()                      # key -> shape table captured from the reference FDN()
    assert len(sd) == 1503 and set(sd) == set(ref)
    assert all(tuple(sd[k].shape) == tuple(ref[k]) for k in ref)
    net.load_state_dict(fdn_weights(), strict=True)
    assert sum(p.numel() for p in net.parameters()) == 8030489
    assert not any(p.requires_grad for p in net.net_a.parameters())      # FDN_arch.py:858-859
    lp = I_predict_net()
    lp.load_state_dict(lpnet_weights(), strict=True)
    assert len(lp.state_dict()) == 292


def test_star_import_surface():
    ns = {}
    exec("from basicsr.models.archs.FDN_arch import *\nfrom basicsr.models.archs.LPNet_arch import *", ns)
    for name in ("FDN", "F", "torch", "nn", "np", "rearrange", "I_predict_net", "transforms"):
        assert name in ns, name
    from basicsr.models.archs import define_network
    assert type(define_network({"type": "FDN"})).__name__ == "FDN"


def test_no_cpu_fallback():
    from basicsr.models.archs.FDN_arch import FDN
    from basicsr.models.archs.LPNet_arch import I_predict_net
    import fdn_hip
    with pytest.raises(fdn_hip.FdnHipError):
        FDN().eval()(torch.rand(1, 3, 32, 32), ratio_i=torch.rand(1, 1))
    with pytest.raises(fdn_hip.FdnHipError):
        I_predict_net().eval()(torch.rand(1, 3, 32, 32))
    with pytest.raises(ValueError):
        FDN().eval()(torch.rand(1, 3, 32, 32))


def test_product_path_never_imports_oracle():
    pkg = os.path.join(ROOT, "fdn-tip2025_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".hpp", ".sh")):
                txt = open(os.path.join(dp, f)).read()
                assert "fdn_oracle" not in txt and "oracle/" not in txt, os.path.join(dp, f)


def test_harness_rejects_cpu_tensors():
    """The GPU pre/post stage has no host fallback either: CPU tensors are refused before any library call."""
    import torch
    import fdn_hip
    from fdn_hip import harness
    assert harness.padded_size(720, 1280) == (736, 1280) and harness.padded_size(64, 96) == (64, 96)
    with pytest.raises(fdn_hip.FdnHipError):
        harness.preprocess(torch.zeros(1, 40, 40, 3, dtype=torch.uint8))
    with pytest.raises(fdn_hip.FdnHipError):
        harness.postprocess(torch.zeros(1, 3, 64, 64), 40, 40)


def test_lolv1_state_dict_layout_matches_reference():
    """FDN_lolv1 (dim 24): same 1503 keys / shapes as the reference module, so its checkpoint loads strict."""
    from basicsr.models.archs.fdnlol24_arch import FDN_lolv1
    from common import lolv1_shapes, lolv1_weights
    net = FDN_lolv1()
    sd, ref = net.state_dict(), lolv1_shapes()
    assert len(sd) == 1503 and set(sd) == set(ref)
    assert all(tuple(sd[k].shape) == tuple(ref[k]) for k in ref)
    assert sd["net_p.patch_embed.proj.weight"].shape[0] == 24 and "net_a.net.Encoder.0.cat.weight" in sd
    net.load_state_dict(lolv1_weights(), strict=True)


def test_tiling_origins_match_oracle_and_reject_cpu():
    import torch
    import fdn_hip
    import fdn_oracle as O
    from fdn_hip import tiling
    for (h, w, ch, cw) in ((720, 1280, 256, 256), (100, 150, 64, 64), (96, 96, 96, 96), (1088, 1920, 512, 640)):
        assert tiling.tile_origins(h, w, ch, cw) == O.grids_indices(h, w, ch, cw)[2]
    with pytest.raises(fdn_hip.FdnHipError):
        tiling.split(torch.zeros(1, 3, 64, 64), 32, 32)
    with pytest.raises(fdn_hip.FdnHipError):
        tiling.tile_origins(64, 64, 128, 32)


def test_sincos_large_argument_table():
    """The large-argument reduction of fdn_sincos (csrc/common.hpp) restated with exact rationals on the committed table
    (csrc/sincos_table.inc, made by tools/gen_sincos_table.py): x * 2/pi mod 4 = m * T[e] mod 4 for |x| = m * 2^e."""
    import math
    import os
    import struct
    from fractions import Fraction

    import numpy as np

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = []
    for line in open(os.path.join(root, "fdn-tip2025_amd", "csrc", "sincos_table.inc")):
        if line.startswith("{"):
            hi, lo = line.strip().strip("{},").split(",")
            rows.append((float.fromhex(hi.strip()), float.fromhex(lo.strip())))
    assert len(rows) == 115
    rng = np.random.default_rng(3)
    xs = np.concatenate([np.exp(rng.uniform(9.02, 88.7, 400)), [8192.0, 2.0 ** 40, 3.4028235e38]]).astype(np.float32)
    for x in xs:
        bits = struct.unpack("<I", struct.pack("<f", float(x)))[0]
        eb, m = bits >> 23, (bits & 0x7FFFFF) | 0x800000
        assert Fraction(m) * Fraction(2) ** (eb - 150) == Fraction(float(x))
        fh, fl = rows[eb - 140]
        exact = Fraction(m) * Fraction(fh)
        p = float(exact)                                   # the rounded fp64 product
        pe = float(exact - Fraction(p))                    # fma(m, fh, -p): exact
        kq = round(p)                                      # (ties cannot occur within the tolerance below)
        fr = (p - kq) + float(Fraction(m) * Fraction(fl) + Fraction(pe))
        r, q = fr * (math.pi / 2), kq & 3
        s, c = math.sin(r), math.cos(r)
        sn = (s, c, -s, -c)[q]
        cs = (c, -s, -c, s)[q]
        assert abs(sn - math.sin(float(x))) < 1e-12 and abs(cs - math.cos(float(x))) < 1e-12, float(x)


def test_ratio_sweep_grid_and_names_follow_the_reference():
    """inference_fdn_multi_r.py:55,84: `for i in np.arange(0, 1, 0.01)` ... `"./multi_r/{}.png".format(i)` - the driver's grid and the
    file names it writes are exactly those (format of the numpy float64 loop variable)."""
    import sys
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "fdn-tip2025_amd"))
    import inference_fdn_multi_r as M
    vals = M.sweep_values(0.0, 1.0, 0.01)
    ref = [i for i in np.arange(0, 1, 0.01)]
    assert len(vals) == 100 and all(float(a) == float(b) for a, b in zip(vals, ref))
    assert [M.output_name(v) for v in vals[:3]] == ["{}.png".format(i) for i in ref[:3]] == ["0.0.png", "0.01.png", "0.02.png"]
    assert M.output_name(vals[29]) == "{}.png".format(ref[29])


def test_no_waterfall_loops_in_the_patch_kernels(tmp_path):
    """The compiler wrapped every halo load of fdffn_mid's channel loop in a waterfall loop (the strength-reduced plane offset lived in a vector
    register: 12 loops, ~150 issue slots per channel).  Compile patchfft.hip to gfx950 assembly and hold the count at 0."""
    import importlib.util
    import subprocess
    root = ROOT
    out = tmp_path / "patchfft.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "--cuda-device-only", "-S",
                    os.path.join(root, "fdn-tip2025_amd", "csrc", "patchfft.hip"), "-o", str(out)], check=True, timeout=600)
    spec = importlib.util.spec_from_file_location("isa_waterfall", os.path.join(root, "tools", "isa_waterfall.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    stats = mod.waterfalls(str(out))
    kernels = [k for k in stats if "fdffn_mid_kernel" in k or "fdsa_fused_kernel" in k or "fdsa_core_kernel" in k]
    assert len(kernels) >= 10, sorted(stats)
    assert {k: stats[k][0] for k in kernels if stats[k][0]} == {}


def test_no_build_hooks_in_the_kernel_sources():
    """The kernels compile in one form only: no `FDN_*` switch that an A/B build could flip with -D (build.sh defines none)."""
    csrc = os.path.join(ROOT, "fdn-tip2025_amd", "csrc")
    hook = re.compile(r"#\s*(ifdef|ifndef|if)\s+FDN_")
    hits = [f"{name}:{i}: {line.strip()}" for name in sorted(os.listdir(csrc)) if name.endswith((".hip", ".hpp"))
            for i, line in enumerate(open(os.path.join(csrc, name)), 1) if hook.search(line)]
    assert hits == []


def test_reference_driver_imports_through_the_shadow(tmp_path):
    """this package FIRST on PYTHONPATH, a reference checkout after it.  The checkout here is a stub laid out like the
    reference (basicsr/ WITHOUT an __init__.py, basicsr/utils/__init__.py with the four helpers, basicsr/models/__init__.py that must NOT run,
    a reference-only arch module); the import lines are those of /root/reference/inference_fdn_lolblur.py:1-6, executed verbatim in a fresh
    interpreter.  FDN / I_predict_net must come from this package, the helpers from the checkout."""
    import subprocess
    import sys
    ck = tmp_path / "checkout"
    (ck / "basicsr" / "utils").mkdir(parents=True)
    (ck / "basicsr" / "models" / "archs").mkdir(parents=True)
    (ck / "basicsr" / "utils" / "__init__.py").write_text(
        "def get_root_logger(*a, **k): return 'logger'\ndef imwrite(*a, **k): return 'imwrite'\n"
        "def tensor2img(*a, **k): return 'tensor2img'\ndef img2tensor(*a, **k): return 'img2tensor'\ndef scandir(*a, **k): return []\n")
    (ck / "basicsr" / "models" / "__init__.py").write_text("raise RuntimeError('the training stack of the checkout must not be imported')\n")
    (ck / "basicsr" / "models" / "archs" / "__init__.py").write_text("raise RuntimeError('the registry of the checkout must not be imported')\n")
    (ck / "basicsr" / "models" / "archs" / "FDN_arch.py").write_text("raise RuntimeError('shadowing failed: the reference FDN_arch was imported')\n")
    (ck / "basicsr" / "models" / "archs" / "mar_arch.py").write_text("MAR_ONLY_IN_CHECKOUT = 1\n")
    driver_lines = (
        "from basicsr.utils import get_root_logger, imwrite, tensor2img\n"
        "\n"
        "from basicsr.models.archs.FDN_arch import *\n"
        "\n"
        "from basicsr.models.archs.LPNet_arch import *\n"
        "from basicsr.utils import img2tensor\n")
    check = (
        "import basicsr, os\n"
        "pkg = os.environ['FDN_PKG']\n"
        "assert FDN.__module__ == 'basicsr.models.archs.FDN_arch' and os.path.realpath(sys.modules[FDN.__module__].__file__).startswith(pkg), sys.modules[FDN.__module__].__file__\n"
        "assert os.path.realpath(sys.modules[I_predict_net.__module__].__file__).startswith(pkg)\n"
        "assert transforms is not None and F is torch.nn.functional and rearrange is not None and np is not None and nn is torch.nn\n"
        "assert get_root_logger() == 'logger' and imwrite() == 'imwrite' and tensor2img() == 'tensor2img' and img2tensor() == 'img2tensor'\n"
        "from basicsr.models.archs.fdnlol24_arch import FDN_lolv1\n"
        "from basicsr.models.archs import mar_arch, define_network\n"
        "assert mar_arch.MAR_ONLY_IN_CHECKOUT == 1\n"
        "assert type(define_network({'type': 'FDN'})).__name__ == 'FDN'\n"
        "print('shadow ok')\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([entry.PKG, str(ck)]), FDN_PKG=os.path.realpath(entry.PKG))
    r = subprocess.run([sys.executable, "-c", "import sys\n" + driver_lines + check], env=env, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0 and "shadow ok" in r.stdout, r.stderr[-2000:]


def test_reference_model_registry_is_reached_on_demand(tmp_path):
    """`from basicsr.models import create_model` (the reference's test.py / train.py) - the shadow package runs the checkout's
    basicsr/models/__init__.py the first time one of its names is asked for, and says so when that fails or when no checkout follows."""
    import subprocess
    import sys
    ck = tmp_path / "checkout"
    (ck / "basicsr" / "models").mkdir(parents=True)
    (ck / "basicsr" / "models" / "__init__.py").write_text("def create_model(opt):\n    return ('model of the checkout', opt)\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([entry.PKG, str(ck)]))
    code = ("from basicsr.models import create_model\nassert create_model(3) == ('model of the checkout', 3)\n"
            "import basicsr.models as m\n"
            "try:\n    m.no_such_name\nexcept AttributeError as e:\n    assert 'drop-in' in str(e)\nelse:\n    raise SystemExit('no error')\nprint('registry ok')\n")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0 and "registry ok" in r.stdout, r.stderr[-2000:]
    (ck / "basicsr" / "models" / "__init__.py").write_text("import a_module_the_training_stack_needs\n")
    code = ("try:\n    from basicsr.models import create_model\nexcept ImportError as e:\n"
            "    assert 'on demand' in str(e) and 'a_module_the_training_stack_needs' in str(e), str(e)\n    print('clear error')\n")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0 and "clear error" in r.stdout, r.stderr[-2000:]
    code = ("import basicsr.models as m\ntry:\n    m.create_model\nexcept AttributeError as e:\n    assert 'no reference checkout' in str(e), str(e)\n    print('clear error')\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=entry.PKG), capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0 and "clear error" in r.stdout, r.stderr[-2000:]


def test_bench_describes_calls_by_name(gen):
    """bench.py's roofline figures come from the ARGUMENTS of the C-ABI calls it wraps.  They are read by NAME (fdn_hip/_abi.py ARG_NAMES,
    generated from the header), so an inserted or reordered parameter of a later ABI version cannot silently shift a shape: every parser gets
    a call built from the header's own prototype in which each integer parameter carries a distinct value, and the group key it returns must
    show the values of the parameters it names - then the same call with two parameters swapped IN THE TABLE must change the key or raise."""
    import bench
    from fdn_hip._abi import ARG_NAMES, HEADERS, PROTOTYPES
    assert {n: ARG_NAMES[n] for n in HEADERS["fdn_hip.h"]} == gen.parse_names(os.path.join(ROOT, "include", "fdn_hip.h"))
    assert set(ARG_NAMES) == set(PROTOTYPES) and all(len(ARG_NAMES[n]) == len(PROTOTYPES[n][1]) for n in PROTOTYPES)
    # every entry point the step's by_entry_point_ms can name either has a parser or is a helper without a shape figure; the heavy ones must have one
    heavy = ("fdn_conv1x1", "fdn_fdsa_fused", "fdn_fdsa_out", "fdn_fdsa_core", "fdn_fdffn_mid", "fdn_ffn_tail", "fdn_dwconv_gate", "fdn_conv2d",
             "fdn_fft_cols_fcaffn", "fdn_rfft_rows_ln", "fdn_irfft_rows", "fdn_rfft_rows", "fdn_fcaffn_in", "fdn_fcaffn_in_packed", "fdn_chan_stats")
    assert all(n in bench.DESCRIBERS for n in heavy)
    assert all(n in PROTOTYPES for n in bench.DESCRIBERS)
    shape_params = ("C", "E", "Hd", "G", "Cin", "Cout", "rows", "planes", "N", "H", "W", "P", "Wf")
    derived = {"fdn_rfft_rows_ln": {"C", "H"}}               # (shown as rows = B * C * H)
    for name, fn in bench.DESCRIBERS.items():
        if name == "fdn_conv1x1":
            continue                                             # one descriptor struct: fields are named by construction
        names, kinds = ARG_NAMES[name], PROTOTYPES[name][1]
        vals = {n: (None if k == "P" else 0 if n.endswith("bf16") or n in ("form", "pad") else 101 + 2 * i) for i, (n, k) in enumerate(zip(names, kinds))}
        if "stride" in vals:
            vals["stride"] = 1
        args = [ctypes.c_long(v) if k == "L" and v is not None else v for v, k in ((vals[n], k) for n, k in zip(names, kinds))]
        key, flops, byts = bench.describe_call(name, args)
        assert key.startswith(name + "[") and byts > 0, (name, key)
        for pn in shape_params:
            if pn in vals and vals[pn] is not None and pn not in derived.get(name, ()):
                assert re.search(r"(?<!\d)%d(?!\d)" % vals[pn], key), f"{name}: parameter {pn}={vals[pn]} not in key {key}"
        ints = [n for n in names if n in shape_params and n not in derived.get(name, ())]
        if len(ints) >= 2:                                       # a table in another order = a different ABI: the same positional call must not read the same
            swapped = list(names)
            i, j = names.index(ints[0]), names.index(ints[1])
            swapped[i], swapped[j] = swapped[j], swapped[i]
            ARG_NAMES[name] = swapped
            try:
                key2, _, byts2 = bench.describe_call(name, args)
            finally:
                ARG_NAMES[name] = names
            assert key2 != key, (name, key, key2)
    with pytest.raises(TypeError):
        bench.describe_call("fdn_fdsa_fused", [None] * 3)       # a call that does not match the declared parameter count is refused


def test_graph_key_covers_every_routing_switch():
    """A captured HIP graph replays the kernels of its capture: every process-wide switch that decides WHICH kernels a forward launches must be part of
    pipeline.weights_signature, or a holder would replay a stale route (ops.FFN_TAIL_MODE was missing).  Checked on CPU modules."""
    import torch
    from fdn_hip import ops, pipeline
    m = torch.nn.Linear(3, 3)
    base = pipeline.weights_signature(m)
    flips = {"FDSA_FULL": True, "FDSA_FULL_MAX_C": 64, "FDSA_TAIL": False, "FDSA_TAIL_PIN": False, "FFN_TAIL_MODE": "split", "SPECTRAL_MLP_FUSED": False,
             "GEMM_OWN_STATS": False, "UPCONV_GATHER": False, "AFF_MULTIRES": False}
    # every module-level switch of ops.py whose initial value is a bool or None (the routing switches; thresholds and width tables are constants)
    import re
    src = open(ops.__file__).read()
    switches = set(re.findall(r"^([A-Z][A-Z0-9_]*) = (?:True|False|None)\b", src, flags=re.M))
    assert switches <= set(flips), f"routing switches missing from this test (and maybe from the graph key): {sorted(switches - set(flips))}"
    for name, val in flips.items():
        old = getattr(ops, name)
        assert old != val, name
        setattr(ops, name, val)
        try:
            assert pipeline.weights_signature(m) != base, f"ops.{name} is not part of the graph key"
        finally:
            setattr(ops, name, old)
    assert pipeline.weights_signature(m) == base
    # (ABI 16) the CU budget decides the launch geometry of the persistent and channel-grouped kernels: a graph captured under one budget must
    # not replay under another (set directly: fdn_hip.set_cu_budget needs a device)
    import fdn_hip
    saved = dict(fdn_hip._cu_budgets)
    keys = set()
    try:
        for budgets in ({}, {0: 1}, {0: 7}, {1: 1}):
            fdn_hip._cu_budgets.clear()
            fdn_hip._cu_budgets.update(budgets)
            keys.add(pipeline.weights_signature(m))
    finally:
        fdn_hip._cu_budgets.clear()
        fdn_hip._cu_budgets.update(saved)
    assert len(keys) == 4, "fdn_hip.set_cu_budget is not part of the graph key"
    assert pipeline.weights_signature(m) == base
    with torch.no_grad():
        m.weight.add_(1.0)                      # an in-place weight update is seen too
    assert pipeline.weights_signature(m) != base
    # a graph holds raw pointers: two equal-shaped parameters that swap storages change what it reads and leave every sum over the tree alone
    two = torch.nn.Sequential(torch.nn.Linear(3, 3), torch.nn.Linear(3, 3))
    base2 = pipeline.weights_signature(two)
    assert pipeline.weights_signature(two) == base2
    two[0].weight.data, two[1].weight.data = two[1].weight.data, two[0].weight.data
    assert pipeline.weights_signature(two) != base2, "swapped storages are not seen by the graph key"
    two[0].weight.data, two[1].weight.data = two[1].weight.data, two[0].weight.data
    assert pipeline.weights_signature(two) == base2
    ops.forget_derived(two)                     # the way out after a write through .data moves the key as well
    assert pipeline.weights_signature(two) != base2


# ---- (ABI 17) the routes of the generic full-image FFT: fdn_fft_route is host arithmetic, the launchers decide by the same code ----
def _kernel_switch(name, marker):
    """{radix: lowest BIG at which it has a case} from the `switch (R)` of a device function in csrc/fft2d.hip: `case R: ...` = BIG 0,
    `case R: if (BIG) ...` = 1, `case R: if (BIG == 2) ...` = 2.  Read from the source, so the check below sees the device-side list."""
    src = open(os.path.join(ROOT, "fdn-tip2025_amd", "csrc", "fft2d.hip")).read()
    start = src.index(marker)
    body = src[start:src.index("\n}\n", start)]
    cases = {}
    for r, cond in re.findall(r"case (\d+):\s*(if \(BIG(?: == 2)?\))?", body):
        cases[int(r)] = 0 if not cond else 2 if "== 2" in cond else 1
    assert cases, name
    return cases


def _rader_length(p):
    """Rader applies: p a prime >= 29 and p - 1 a product of the radices with an in-place / BIG-1 register butterfly (2, 3, 5, 7, 17, 23)."""
    if p < 29 or any(p % f == 0 for f in range(2, int(p ** 0.5) + 1)):
        return False
    m = p - 1
    for f in (2, 3, 5, 7, 17, 23):
        while m % f == 0:
            m //= f
    return m == 1


def _lds_bytes(kind, n, rt):
    """LDS of one workgroup of the generic kernels at the route's tc / rpb (fft2d.hip: launch_cols, fdn_rfft_rows, fdn_irfft_rows)."""
    if kind == 2:
        return (n * rt["width"] + n) * 8 if rt["route"] == "inplace" else (2 * n * rt["width"] + n) * 8
    M = n // 2
    return (2 * rt["width"] * M + n + (M + rt["width"] if rt["route"] == "rader" else 0)) * 8


def test_fft_route_pins_the_lengths_the_gpu_tests_use(lib):
    from common import FFT_COL_ROUTES, FFT_ROW_ROUTES
    from fdn_hip import ops
    for H, (route, big, tc, gather) in FFT_COL_ROUTES.items():
        rt = ops.fft_route(ops.FFT_COLS, H)
        assert (rt["route"], rt["big"], rt["width"], rt["gather"]) == (route, big, tc, gather), (H, rt)
    for W, (route, big, rpb, gather, p) in FFT_ROW_ROUTES.items():
        rt = ops.fft_route(ops.FFT_ROWS, W)
        assert (rt["route"], rt["big"], rt["width"], rt["gather"], rt["rader"]) == (route, big, rpb, gather, p), (W, rt)
        inv = ops.fft_route(ops.FFT_IROWS, W)                   # no Rader on the inverse: a prime half-length gathers
        assert inv["route"] == ("refused" if route == "refused" else "pingpong") and inv["rader"] == 0, (W, inv)
        if p:
            assert inv["gather"] == (p,) and inv["width"] == rpb, (W, inv)
    # the compile-time plans and where they hand over
    assert ops.fft_route(ops.FFT_COLS, 736) == {"route": "planned", "big": 0, "width": 8, "rader": 0, "radices": (23, 32), "gather": ()}
    assert ops.fft_route(ops.FFT_ROWS, 1280)["radices"] == (20, 32) and ops.fft_route(ops.FFT_IROWS, 1120)["radices"] == (35, 16)
    assert ops.fft_route(ops.FFT_ROWS, 152)["route"] == "pingpong"            # 2 x 19 x 4: not planned (include/fdn_hip.h)


def test_fft_route_sweep_invariants(lib):
    """Every column length 1..4600 and every even row width 2..10260: the plan is a factorisation, an in-place plan uses only radices
    fft_run_inplace has a case for (at its BIG), register radices imply their BIG tier, a Rader sub-plan has no gather stage, tc / rpb
    are within their bounds, and a length is refused exactly where the LDS of a workgroup (160 KiB) runs out.  The lengths answered
    "planned" are exactly PLANNED_H / PLANNED_W (tests/common.py), each as its factors (R, P)."""
    from common import PLANNED_H, PLANNED_W
    from fdn_hip import ops
    inplace = _kernel_switch("fft_run_inplace", "__device__ void fft_run_inplace(")
    reg = _kernel_switch("fft_pass", "__device__ void fft_pass(")
    reg.update({2: 0, 4: 0})                                   # fft_pass: radix 2 and 4 are the butterflies after the switch
    assert set(inplace) >= {2, 3, 4, 5, 7}
    lds_max = 160 * 1024
    seen = set()
    planned = {ops.FFT_COLS: set(), ops.FFT_ROWS: set(), ops.FFT_IROWS: set()}
    for kind, lengths in ((ops.FFT_COLS, range(1, 4601)), (ops.FFT_ROWS, range(2, 10262, 2)), (ops.FFT_IROWS, range(2, 10262, 2))):
        for n in lengths:
            rt = ops.fft_route(kind, n)
            seen.add((kind, rt["route"], rt["big"]))
            N = n if kind == ops.FFT_COLS else n // 2
            if rt["route"] == "planned":
                planned[kind].add(n)
                R, P = rt["radices"]
                assert R * P == N and (rt["big"], rt["rader"], rt["gather"]) == (0, 0, ()), (kind, n, rt)
                if kind == ops.FFT_COLS:
                    assert rt["width"] == 256 // P, (n, rt)
                continue
            if kind == ops.FFT_COLS:
                # no column length <= 4096 needs more than tc 2 of ping-pong buffers and the table; 4097 and up do
                assert (rt["route"] == "refused") == (n > 4096), (n, rt)
            else:
                rpb = min(8, max(1, 32 * 1024 // (16 * N)))     # pick_rpb
                rader = kind == ops.FFT_ROWS and _rader_length(N)
                need = (2 * rpb * N + n + (N + rpb if rader else 0)) * 8
                assert (rt["route"] == "refused") == (need > lds_max), (n, rt, need)
                assert rt["route"] in ("refused", "rader" if rader else "pingpong"), (n, rt)
                assert rt["route"] == "refused" or rt["width"] == rpb, (n, rt)
            if rt["route"] == "refused":
                continue
            assert _lds_bytes(kind, n, rt) <= lds_max, (kind, n, rt)
            radices = rt["radices"]
            prod = 1
            for r in radices:
                prod *= r
            if rt["route"] == "rader":
                assert kind == ops.FFT_ROWS and rt["rader"] == N and prod == N - 1, (n, rt)
                assert rt["gather"] == () and all(reg.get(r, 99) <= 1 and r in inplace for r in radices), (n, rt)
            else:
                assert prod == N and rt["rader"] == 0, (kind, n, rt)
            if rt["route"] == "inplace":
                assert kind == ops.FFT_COLS and rt["width"] in (32, 16, 8) and rt["width"] * n <= 256 * 24, (n, rt)
                for r in radices:
                    assert r in inplace and inplace[r] <= rt["big"], f"H = {n}: radix {r} at BIG {rt['big']} has no case in fft_run_inplace {sorted(inplace)}"
                    assert (n // r) * rt["width"] <= 256 * (36 // r), (n, rt)
            if kind == ops.FFT_COLS and rt["route"] == "pingpong":
                assert rt["width"] in (16, 8, 4, 2), (n, rt)
            if kind != ops.FFT_COLS:
                assert 1 <= rt["width"] <= 8 and rt["big"] in (0, 1), (n, rt)
            # BIG tiers: 17 / 23 need BIG >= 1, 13 / 37 / 41 run in registers only on a BIG == 2 column plan; BIG is the least that covers them
            want_big = 1 if any(r in (17, 23) for r in radices) else 0
            if kind == ops.FFT_COLS and rt["route"] == "pingpong" and any(r in (13, 37, 41) for r in radices):
                want_big = 2
            assert rt["big"] == want_big, (kind, n, rt)
            if rt["route"] != "inplace":
                assert rt["gather"] == tuple(r for r in radices if reg.get(r, 99) > rt["big"]), (kind, n, rt)
    assert planned[ops.FFT_COLS] == set(PLANNED_H) and len(PLANNED_H) == 13
    assert planned[ops.FFT_ROWS] == set(PLANNED_W) and planned[ops.FFT_IROWS] == set(PLANNED_W) and len(PLANNED_W) == 11
    # every route and BIG tier the kernels have is reached by some length
    for want in [(2, "inplace", 0), (2, "inplace", 1), (2, "pingpong", 0), (2, "pingpong", 1), (2, "pingpong", 2), (2, "refused", 0),
                 (0, "pingpong", 0), (0, "pingpong", 1), (0, "rader", 0), (0, "rader", 1), (0, "refused", 0), (1, "pingpong", 0), (1, "pingpong", 1)]:
        assert want in seen, want


def test_rows_ln_ok_follows_the_planned_widths(lib):
    """ops.rows_ln_ok asks the library: true for a (1, 3, 8, W) tensor exactly when W has a compile-time plan (only .shape is read)."""
    from common import PLANNED_W
    from fdn_hip import ops
    for W in range(2, 2049, 2):
        assert ops.rows_ln_ok(torch.empty(1, 3, 8, W, device="meta")) == (W in PLANNED_W), W
    assert not ops.rows_ln_ok(torch.empty(1, 3, 8, 641, device="meta"))                     # an odd width is no error here
    assert not ops.rows_ln_ok(torch.empty(2 ** 20, 3, 8, 1280, device="meta"))              # statistics past 2 GB


def test_fft_route_argument_validation(lib):
    desc = (ctypes.c_int * 37)()
    assert lib.fdn_fft_route(2, 64, desc, 37) == 0 and desc[0] == 2         # FDN_FFT_INPLACE
    for kind, n, nd in ((-1, 64, 37), (3, 64, 37), (2, 0, 37), (0, -2, 37), (2, 64, 36), (0, 1282, 5), (0, 35, 37), (1, 9, 37)):
        assert lib.fdn_fft_route(kind, n, desc, nd) == 1, (kind, n, nd)
    assert lib.fdn_fft_route(2, 64, None, 37) == 1
    assert lib.fdn_fft_route(2, 35, desc, 37) == 0                          # odd column lengths are fine
    from fdn_hip import FdnHipError, ops
    with pytest.raises(FdnHipError):
        ops.fft_route(ops.FFT_ROWS, 641)
    assert ops.fft_route(ops.FFT_COLS, 4097)["route"] == "refused"           # a refusal is an answer, not an error


# ---- (ABI 22) the routes of fdn_conv1x1: fdn_conv1x1_route is host arithmetic on the descriptor, fdn_conv1x1 launches what it answers ----
def _route_name(fields):
    from common import conv1x1_route_name, conv1x1_route_of
    return conv1x1_route_name(conv1x1_route_of(fields))


def test_conv1x1_route_sweep_matches_the_recorded_routes(lib):
    """tests/conv1x1_routes.txt: every descriptor of tools/gen_conv1x1_route_cases.py (K and N across every threshold of the route, odd /
    huge P, prologues, epilogues, segments, bf16 storage, misaligned pointers and strides, both matrix-pipe modes) with the route the
    if-ladder of fdn_conv1x1 took before the table existed.  Every line must still get that answer, field for field."""
    import importlib.util
    from common import CONV1X1_ROUTE_FIELDS, conv1x1_route_of
    spec = importlib.util.spec_from_file_location("gen_conv1x1_route_cases", os.path.join(ROOT, "tools", "gen_conv1x1_route_cases.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    path = os.path.join(ROOT, "tests", "conv1x1_routes.txt")
    assert os.path.getsize(path) < 200 * 1024
    lines = [ln.split("|") for ln in open(path) if not ln.startswith("#")]
    assert [a.strip() for a, _ in lines] == gen.cases()                    # the committed descriptors are the generator's
    forms, wrong = set(), []
    for a, b in lines:
        want = tuple(int(v) for v in b.split())
        got = conv1x1_route_of([int(v) for v in a.split()])
        assert len(want) == len(CONV1X1_ROUTE_FIELDS)
        forms.add((want[1], want[0]))
        if got != want:
            wrong.append((a.strip(), want, got))
    assert not wrong, (len(wrong), wrong[:5])
    # every form, and both kinds of refusal, are in the sweep
    assert forms >= {(f, 0) for f in range(1, 11)} | {(0, 1), (0, 4)}, sorted(forms)


def test_conv1x1_route_pins_the_network_shapes(lib):
    from common import CONV1X1_NET_ROUTES, conv1x1_fields
    P = 84 * 131
    for what, kw, plain, packed in CONV1X1_NET_ROUTES:
        kw = dict({"P": P}, **kw)
        assert _route_name(conv1x1_fields(**kw)) == plain, what
        assert _route_name(conv1x1_fields(wpk=1, **kw)) == (packed or plain), what
        for wpk in (0, 1):                                           # the f32 pipe: no split-bf16 form, packed weights or not
            assert _route_name(conv1x1_fields(wpk=wpk, pipe=1, **kw)) == plain, what


def test_conv1x1_route_pins_the_cases_of_the_gpu_tests(lib):
    """Each conv1x1 case of tests/test_gpu_geometry.py, tests/test_gpu_kernel_forms.py and tests/test_gpu_parity.py still reaches the kernel it was chosen for (the GPU tests
    assert the same on the descriptor they really pass)."""
    import importlib
    from common import (CONV1X1_GEOMETRY_ROUTES, CONV1X1_SPLIT_ROUTES, CONV1X1_TWO_INPUT_ROUTES, CONV1X1_VARIANT_ROUTES, conv1x1_fields,
                        conv1x1_route_name, conv1x1_route_of)
    cases = importlib.import_module("test_gpu_geometry").CONV1X1
    assert set(cases) == set(CONV1X1_GEOMETRY_ROUTES)
    for name, (K, N, H, W, pro, epi, act, want_stats, _sliced) in cases.items():
        rt = conv1x1_route_of(conv1x1_fields(K, N, H * W, pro, epi, act=act, so=int(want_stats)))
        assert (conv1x1_route_name(rt), rt[11], rt[12]) == CONV1X1_GEOMETRY_ROUTES[name], name
    assert len({r[0] for r in CONV1X1_GEOMETRY_ROUTES.values()}) == len(CONV1X1_GEOMETRY_ROUTES)        # no two cases on one instantiation
    for (K, N, H, W, pro), (plain, cached) in CONV1X1_VARIANT_ROUTES.items():
        for wpk, want in ((0, plain), (1, cached)):
            assert _route_name(conv1x1_fields(K, N, H * W, pro, "res", so=int(N <= 160), wpk=wpk)) == want, (K, N, pro, wpk)
    for (K, N, H, W, pro, epi), want in CONV1X1_SPLIT_ROUTES.items():
        assert want.startswith("split")
        assert _route_name(conv1x1_fields(K, N, H * W, pro, epi, so=int(N <= 128 and K >= 96), wpk=1)) == want, (K, N, pro, epi)
    for (K0, K1, N, H, W), want in CONV1X1_TWO_INPUT_ROUTES.items():
        assert _route_name(conv1x1_fields(K0 + K1, N, H * W, segs=(K0, K1), so=int(N <= 128), wpk=1, B=2 if H < 100 else 1)) == want, (K0, K1, N)
    forms = importlib.import_module("test_gpu_kernel_forms").CONV1X1
    for name, (K, N, H, W, pro, epi, act, want_stats, xbf, want) in forms.items():
        assert _route_name(conv1x1_fields(K, N, H * W, pro, epi, act=act, so=int(want_stats), xbf=xbf)) == want, name
    assert len({c[-1] for c in forms.values()}) == len(forms)                                            # no two cases on one instantiation


def test_conv1x1_route_argument_validation(lib):
    from common import CONV1X1_ROUTE_FIELDS, conv1x1_case_desc, conv1x1_fields
    from fdn_hip import ops
    nd = len(CONV1X1_ROUTE_FIELDS)
    desc = (ctypes.c_int * nd)()
    d, _ = conv1x1_case_desc(conv1x1_fields(32, 152, 84 * 131, "ln"))
    assert lib.fdn_conv1x1_route(ctypes.byref(d), desc, nd) == 0 and desc[0] == 0 and ops.CONV1X1_FORMS[desc[1]] == "smallk_vec"
    assert lib.fdn_conv1x1_route(None, desc, nd) == 1
    assert lib.fdn_conv1x1_route(ctypes.byref(d), None, nd) == 1
    assert lib.fdn_conv1x1_route(ctypes.byref(d), desc, nd - 1) == 1
    assert lib.fdn_conv1x1(None, None) == 1

    def status(change, **kw):
        d, _ = conv1x1_case_desc(conv1x1_fields(**dict(dict(K=64, N=64, P=4096), **kw)))
        change(d)
        rt = ops.conv1x1_route(d)                                    # a refusal is an answer, not an exception
        if rt["status"]:
            assert rt["form"] == "refused" and not any(rt[k] for k in CONV1X1_ROUTE_FIELDS[2:]), rt
        return rt["status"]
    ARG, UNSUPPORTED = 1, 4
    assert status(lambda d: None) == 0
    for field in ("B", "K", "N", "P"):
        assert status(lambda d: setattr(d, field, 0)) == ARG, field
    for field in ("w", "out"):
        assert status(lambda d: setattr(d, field, None)) == ARG, field

    def no_x0(d):
        d.x[0] = None
    assert status(no_x0) == ARG

    def bad_segments(d):
        d.kseg[0] = 60
    assert status(bad_segments) == ARG                               # the segments do not add up to K

    def segment_without_tensor(d):
        d.x[1] = None
    assert status(segment_without_tensor, segs=(32, 32)) == ARG
    assert status(lambda d: setattr(d, "stats", None), pro="ln") == ARG              # only LN3_GATE / LN_MULADD may leave the statistics to the kernel
    assert status(lambda d: setattr(d, "gamma", None), pro="muladd") == ARG
    assert status(lambda d: setattr(d, "xb", None), pro="muladd") == ARG
    assert status(lambda d: setattr(d, "ln_group", 21), K=66, pro="ln3") == ARG      # 3 * ln_group != K
    assert status(lambda d: setattr(d, "res", None), epi="res") == ARG
    assert status(lambda d: setattr(d, "add", None), epi="muladd") == ARG
    assert status(lambda d: None, N=161, so=1) == ARG                                # statistics epilogue: N <= 160
    assert status(lambda d: setattr(d, "pro", 7)) == ARG                             # no such prologue (the generic form's switch)
    # refusals: 32-bit offsets, odd segments, bf16 storage without a form, statistics no kernel of the shape takes itself
    assert status(lambda d: None, K=64, N=64, P=12_000_000) == UNSUPPORTED           # (N + 200) planes past 4 GiB
    assert status(lambda d: None, K=345, N=64, P=3_000_000) == UNSUPPORTED           # (K + 40) planes past 4 GiB
    assert status(lambda d: None, K=66, N=64, segs=(33, 33)) == UNSUPPORTED
    assert status(lambda d: None, xbf=1, obf=1) == UNSUPPORTED
    assert status(lambda d: None, K=64, N=64, pro="ln", xbf=1) == UNSUPPORTED
    assert status(lambda d: None, K=128, N=128, pro="muladd", epi="muladd", st=0) == UNSUPPORTED            # no packed weights
    assert status(lambda d: None, K=128, N=128, pro="muladd", epi="muladd", st=0, wpk=1) == 0
    assert status(lambda d: None, K=128, N=128, pro="muladd", epi="muladd", st=0, wpk=1, pipe=0, P=4_200_000) == UNSUPPORTED   # 2^31 mask offset
    # the pointer values are read, never what they point to: the same descriptor at 4 bytes off takes the dword form
    d, _ = conv1x1_case_desc(conv1x1_fields(32, 152, 84 * 131, "ln")[:15] + [1, 0])
    assert ops.conv1x1_route(d)["form"] == "smallk"
