"""Shared helpers for the parity tests (fixtures, synthetic weights, tolerance policy)."""
import contextlib
import json
import os

import numpy as np
import torch
import torch.utils.deterministic

from weights import synth_state_dict

try:
    import pytest
except ImportError:         # bench.py, smoke() and the tools import this module for the weights: they need no fixture
    pytest = None

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 7  # tests/golden/make_golden.py


# ---- poisoned uninitialised memory (testing) ----
# The wrappers allocate outputs and workspace with torch.empty, and torch's caching allocator hands a freed block to the next request of its
# size: the second of two equal calls would find the first one's answer in its output.  Under poisoned() every torch.empty / empty_like /
# new_empty / empty_strided is filled with NaN (floating types) or the type's maximum (integers), so each assertion of a GPU module also says
# "every element was written and no unwritten element was read".
def _poison_state():
    return (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
            torch.utils.deterministic.fill_uninitialized_memory)


@contextlib.contextmanager
def _poison_set(mode, warn_only, fill):
    prev = _poison_state()
    torch.use_deterministic_algorithms(mode, warn_only=warn_only)
    torch.utils.deterministic.fill_uninitialized_memory = fill
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
        torch.utils.deterministic.fill_uninitialized_memory = prev[2]


def poisoned():
    """Context manager: torch fills uninitialised allocations (deterministic mode, warn_only so that an op without a deterministic form warns
    and runs).  Restores mode, warn_only and the fill flag on exit, also on an exception; nests."""
    return _poison_set(True, True, True)


def poisoned_off():
    """Context manager for a test listed in POISON_EXEMPT: torch's defaults (no deterministic mode, no fill) inside, the previous state after."""
    return _poison_set(False, False, False)


def poison_uninitialized():
    """Every tests/test_gpu_*.py imports this: module-scoped, so that module-scoped fixtures (models, weight files) are built under it too."""
    with poisoned():
        yield


if pytest is not None:
    poison_uninitialized = pytest.fixture(scope="module", autouse=True)(poison_uninitialized)


# test id ("<module>::<test function>") -> reason.  The only way out of the fixture: a `with poisoned_off():` inside that test.  The only
# admissible reason is that torch's deterministic mode changes or refuses a torch op the test or a wrapper uses, with the op named; a NaN
# that comes out of a library call is never one.  tests/test_poison_cpu.py holds the list to the modules.
POISON_EXEMPT = {
    # not a torch-mode side effect but the switch's own test: it has to see an allocation made while the fill is off
    "test_gpu_poison::test_the_block_a_freed_result_leaves_is_what_the_next_call_gets":
        "tests the switch itself: torch.empty outside poisoned() must hand back the freed block unfilled, and be forced again after",
}


def fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    out = {}
    for k in z.files:
        if k == "shapes_json":
            out["shapes"] = {kk: tuple(v) for kk, v in json.loads(bytes(z[k]).decode()).items()}
        else:
            out[k] = torch.from_numpy(z[k])
    return out


def fixture_weights(name, shapes, tame=None, po_scale=None):
    sd = synth_state_dict(shapes, SEED, prefix_key=name + "/", tame=tame)
    if po_scale is not None:
        for k in sd:
            if k.endswith("project_out.weight"):
                sd[k] = sd[k] * po_scale
    return sd


_fdn_shapes = None


def fdn_shapes():
    global _fdn_shapes
    if _fdn_shapes is None:
        _fdn_shapes = fixture("fdn_tamed_64")["shapes"]
    return _fdn_shapes


def fdn_weights(tame=0.03):
    return synth_state_dict(fdn_shapes(), SEED, prefix_key="fdn/", tame=tame)


def lpnet_weights(which="lolblur"):
    z = np.load(os.path.join(GOLDEN, f"lpnet_{which}_params.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


_lolv1_shapes = None


def lolv1_shapes():
    global _lolv1_shapes
    if _lolv1_shapes is None:
        _lolv1_shapes = fixture("lolv1_tamed_64")["shapes"]
    return _lolv1_shapes


def lolv1_weights(tame=0.03):
    """FDN_lolv1 (dim 24) synthetic state dict, the one tests/golden/make_golden_lolv1.py loaded into the reference."""
    return synth_state_dict(lolv1_shapes(), SEED, prefix_key="fdnlol/", tame=tame)


def rel_rms(a, b):
    a, b = a.double(), b.double()
    return (torch.sqrt(torch.mean((a - b) ** 2)) / (torch.sqrt(torch.mean(b ** 2)) + 1e-30)).item()


def assert_close_cond(got, ref32, truth64, what, factor=4.0, floor=2e-6):
    """Conditioning-aware tolerance: the candidate may be at most
    `factor` times as far from the fp64 truth as the fp32 reference itself is, plus a floor
    (relative RMS).  Also bounds the 99.9th percentile of |err| the same way."""
    got, ref32, truth64 = got.double().cpu(), ref32.double().cpu(), truth64.double().cpu()
    scale = torch.sqrt(torch.mean(truth64 ** 2)).item() + 1e-30
    e_got = torch.sqrt(torch.mean((got - truth64) ** 2)).item() / scale
    e_ref = torch.sqrt(torch.mean((ref32 - truth64) ** 2)).item() / scale
    q = lambda t: torch.quantile(t.abs().flatten()[:4_000_000], 0.999).item() / scale
    p_got, p_ref = q(got - truth64), q(ref32 - truth64)
    assert e_got <= factor * e_ref + floor, f"{what}: rel-RMS err {e_got:.3e} > {factor}*{e_ref:.3e}+{floor}"
    assert p_got <= factor * p_ref + 10 * floor, f"{what}: p99.9 err {p_got:.3e} > {factor}*{p_ref:.3e}+{10*floor}"
    return e_got, e_ref



def rd_replace(v):
    """replace_denormals (FDN_arch.py:548-553): components in (-1e-10, 1e-10) become 1e-10"""
    return torch.where((v < 1e-10) & (v > -1e-10), torch.full_like(v, 1e-10), v)


def fcaffn_ref(z, amp, pha, wxa, wxp, dtype=torch.float64):
    """Restatement of FDN_arch.py:411-418 for the column pass (forward FFT over H, modulation, unnormalised inverse) in `dtype`
    (float64: the truth; float32: what torch.fft computes in the reference's precision); the phase is formed in float32 like the
    kernel does, so that large phases compare bin for bin."""
    Z = torch.fft.fft(torch.view_as_complex(z.to(dtype)), dim=2)
    Zr = torch.complex(rd_replace(Z.real.float()).to(dtype), rd_replace(Z.imag.float()).to(dtype))
    A = torch.einsum("ci,bihw->bchw", wxa.to(dtype), amp.to(dtype))
    ph = torch.einsum("ci,bihw->bchw", wxp, pha).to(dtype) if wxp.abs().max() < 100 else (wxp[:, 0].view(1, -1, 1, 1) * pha[:, :1]).to(dtype)
    out = Zr * A * torch.polar(torch.ones_like(ph), -ph)
    return torch.view_as_real(torch.fft.ifft(out, dim=2) * Z.shape[2])


# The route each length of the generic-FFT tests is chosen to exercise, as fdn_fft_route reports it (include/fdn_hip.h).  The CPU suite pins
# these (a plan change that moves a length to another route fails there, not silently in a GPU test that no longer tests its route), and
# tests/test_gpu_fft_generic.py runs each length against float64.
# columns, length H: (route, BIG, tc, radices that run the gather pass)
FFT_COL_ROUTES = {
    18: ("inplace", 0, 32, ()), 98: ("inplace", 0, 32, ()), 120: ("inplace", 0, 32, ()),          # radix 3 / 7 / 5, tc 32
    240: ("inplace", 0, 16, ()), 224: ("inplace", 0, 16, ()), 480: ("inplace", 0, 8, ()),          # tc 16 / 8 (224: radix 7)
    112: ("inplace", 0, 32, ()),                                                                  # 224 x 352 frames, level 2
    34: ("inplace", 1, 32, ()), 322: ("inplace", 1, 16, ()), 578: ("inplace", 1, 8, ()),          # 17 / 23 in place
    690: ("inplace", 1, 8, ()),                                                                   # 23 * 5 * 3 * 2: at the job limit
    66: ("pingpong", 0, 16, (11,)), 114: ("pingpong", 0, 16, (19,)), 194: ("pingpong", 0, 16, (97,)),
    226: ("pingpong", 0, 8, (113,)), 242: ("pingpong", 0, 8, (11, 11)), 482: ("pingpong", 0, 8, (241,)),
    816: ("pingpong", 1, 8, ()), 1104: ("pingpong", 1, 8, ()),                                    # 17 / 23 beside radices too wide to run in place
    82: ("pingpong", 2, 16, ()), 296: ("pingpong", 2, 8, ()), 338: ("pingpong", 2, 8, ()), 546: ("pingpong", 2, 8, ()),   # 41 / 37 / 13
    2178: ("pingpong", 0, 4, (11, 11)), 4094: ("pingpong", 1, 2, (89,)), 4096: ("pingpong", 0, 2, ()),                      # 4K frames
    1: ("inplace", 0, 32, ()), 2: ("inplace", 0, 32, ()), 3: ("inplace", 0, 32, ()),
    4097: ("refused", 0, 0, ()), 4480: ("refused", 0, 0, ()), 4482: ("refused", 0, 0, ()),    # ping-pong buffers + table > 160 KiB of LDS
}
# the lengths with a compile-time plan (FDN_COL_PLANS / FDN_ROW_PLANS of csrc/fft_plan.hpp): the CPU suite checks that fdn_fft_route answers
# "planned" for exactly these, tests/test_gpu_fft_planned.py runs each
PLANNED_H = [736, 368, 184, 544, 272, 136, 1088, 640, 320, 160, 416, 208, 104]       # + the LOL-Blur (640 x 1120) and padded LOL-v1 (416 x 608) pyramids
PLANNED_W = [1280, 640, 320, 1920, 960, 480, 608, 304, 1120, 560, 280]      # (35 x 16 / 8 / 4: 7 / 7 / 6 row groups per workgroup, a partly filled first stage)
# rows, width W: (forward route, BIG, rpb, radices that run the gather pass, Rader prime)
FFT_ROW_ROUTES = {
    160: ("pingpong", 0, 8, (), 0), 224: ("pingpong", 0, 8, (), 0), 352: ("pingpong", 0, 8, (11,), 0), 546: ("pingpong", 0, 7, (13,), 0),
    176: ("pingpong", 0, 8, (11,), 0),                                                            # 224 x 352 frames, level 2
    322: ("pingpong", 1, 8, (), 0), 544: ("pingpong", 1, 7, (), 0),                             # BIG rows (23, 17)
    194: ("rader", 0, 8, (), 97), 226: ("rader", 0, 8, (), 113), 482: ("rader", 0, 8, (), 241), 1282: ("rader", 0, 3, (), 641),
    274: ("rader", 1, 8, (), 137),                                                                # 136 = 17 * 4 * 2: a BIG sub-plan
    26: ("pingpong", 0, 8, (13,), 0), 354: ("pingpong", 0, 8, (59,), 0), 178: ("pingpong", 0, 8, (89,), 0), 642: ("pingpong", 0, 6, (107,), 0),
    2: ("pingpong", 0, 8, (), 0), 4: ("pingpong", 0, 8, (), 0), 6: ("pingpong", 0, 8, (), 0),
    8192: ("pingpong", 0, 1, (), 0), 10240: ("pingpong", 0, 1, (), 0),
    10242: ("refused", 0, 0, (), 0),
}


# ---- the routes of fdn_conv1x1 (fdn_conv1x1_route, include/fdn_hip.h): what the CPU suite pins and the GPU tests assert ----
CONV1X1_ROUTE_FIELDS = ("status", "form", "n", "pro", "nw", "early", "xbf", "obf", "strip2", "own_stats", "bf16_pipe", "threads", "tile_px")


def conv1x1_case_desc(fields):
    """One descriptor line of tests/conv1x1_routes.txt (tools/gen_conv1x1_route_cases.py: B K N P pro epi act stats_out stats k0 k1 k2 wpk
    x_bf16 out_bf16 misaligned pipe) -> (Conv1x1Desc, pipe).  The pointers are made-up 16-byte aligned addresses (+ 4 where the
    `misaligned` bit says so): the route reads their values only."""
    from fdn_hip import Conv1x1Desc
    B, K, N, P, pro, epi, act, so, st, k0, k1, k2, wpk, xbf, obf, mis, pipe = fields
    d = Conv1x1Desc()
    ptr = lambda i, off=0: 0x10000000 + 0x1000000 * i + (4 if off else 0)
    for i, k in enumerate((k0, k1, k2)):
        d.kseg[i] = k
        if k > 0:
            d.x[i], d.xbs[i] = ptr(i, i == 0 and mis & 1), k * P + (1 if i == 0 and mis & 32 else 0)
    d.w, d.bias, d.out, d.obs = ptr(3), ptr(4), ptr(5, mis & 2), N * P + (1 if mis & 64 else 0)
    d.B, d.K, d.N, d.P, d.pro, d.ln_group, d.act, d.epi = B, K, N, P, pro, (K // 3 if pro == 2 else K), act, epi
    if st:
        d.stats = ptr(6, mis & 8)
    if pro >= 2:
        d.gamma, d.beta, d.xb, d.xbbs = ptr(7), ptr(8), ptr(9), (K // 3 if pro == 2 else K) * P
    if epi == 1:
        d.res, d.rbs = ptr(10, mis & 4), N * P + (1 if mis & 128 else 0)
    elif epi == 2:
        d.mul, d.add, d.mbs = ptr(11), ptr(12), N * P
    if so:
        d.stats_out = ptr(13, mis & 16)
    d.x_bf16, d.out_bf16 = xbf, obf
    if wpk:
        d.wpk = ptr(14)
    return d, pipe


def conv1x1_route_of(fields):
    """the 13 ints fdn_conv1x1_route answers for a descriptor line, under the line's matrix-pipe mode (restored afterwards)"""
    import ctypes
    import fdn_hip
    d, pipe = conv1x1_case_desc(fields)
    out = (ctypes.c_int * len(CONV1X1_ROUTE_FIELDS))()
    try:
        if pipe:
            fdn_hip.set_matrix_pipe("f32")
        assert fdn_hip.lib().fdn_conv1x1_route(ctypes.byref(d), out, len(out)) == 0
    finally:
        if pipe:
            fdn_hip.set_matrix_pipe("bf16")
    return tuple(out)


_PRO_NAMES = ("none", "ln", "ln3", "muladd")


def conv1x1_route_name(rt):
    """A route (the dict of ops.conv1x1_route, or the 13 ints) as the instantiation it stands for: "generic<MT,PRO,NW,EARLY>",
    "smallk<NCH,PRO>", "smallk_vec<NCH,PRO,obf=.>", "narrow_tail<NCH,xbf=.>", "kstream_vec<MT,xbf=.>", "smallk_stream<NCH,PRO>",
    "smallk_stream_vec<NCH,PRO>", "tile<PRO>", "split<PRO>", "split_strip<NKS,PRO,strip2=.>", "refused(status)"."""
    from fdn_hip import ops
    if not isinstance(rt, dict):
        rt = dict(zip(CONV1X1_ROUTE_FIELDS, rt))
        rt["form"] = ops.CONV1X1_FORMS[rt["form"]]
    f, n, pro = rt["form"], rt["n"], _PRO_NAMES[rt["pro"]]
    if f == "refused":
        return f"refused({rt['status']})"
    args = {"generic": f"{n},{pro},{rt['nw']},{rt['early']}", "smallk_vec": f"{n},{pro},obf={rt['obf']}", "narrow_tail": f"{n},xbf={rt['xbf']}",
            "kstream_vec": f"{n},xbf={rt['xbf']}", "tile": pro, "split": pro, "split_strip": f"{n},{pro},strip2={rt['strip2']}"}.get(f, f"{n},{pro}")
    return f"{f}<{args}>"


def conv1x1_fields(K, N, P, pro=None, epi=None, act=0, so=0, st=1, segs=None, wpk=0, xbf=0, obf=0, pipe=0, B=2):
    """a descriptor line (conv1x1_case_desc) from a test's parameters: pro None / "none" / "ln" / "ln3" / "muladd", epi None / "none" /
    "bias" / "res" / "muladd"; aligned pointers, as torch allocates them"""
    k = list(segs or (K,)) + [0, 0]
    return [B, K, N, P, _PRO_NAMES.index(pro or "none"), {"res": 1, "muladd": 2}.get(epi, 0), act, so, st,
            k[0], k[1], k[2], wpk, xbf, obf, 0, pipe]


# The kernel each conv1x1 case is chosen for, as conv1x1_route_name writes fdn_conv1x1_route's answer.  tests/test_host_cpu.py pins every table
# below without a GPU (a route change that moves a case to another kernel fails there), and the GPU tests assert the route before they run.
# All were recorded from the if-ladder that csrc/conv1x1_route.hpp replaced.
# The 1x1 convs of FDN (dim 32), FDN_lolv1 (dim 24) and the class default (dim 48), of MAR and of LPNet (FDN_arch.py, fdnlol24_arch.py,
# LPNet_arch.py): (what, conv1x1_fields arguments at P = 84 x 131, route without packed weights, route with them under the bf16 pipe or None =
# the same).  Under the f32 pipe packed weights change nothing: every case then takes its first route.
CONV1X1_NET_ROUTES = [
    ('FDSA to_hidden C=24', dict(K=24, N=112, pro='ln', epi=None), 'smallk_vec<1,ln,obf=0>', 'split_strip<2,ln,strip2=0>'),
    ('FDSA project_out C=24', dict(K=84, N=24, pro='ln3', epi='res', so=1), 'generic<1,ln3,8,0>', None),
    ('FDSA project_out C=24, statistics left to the kernel', dict(K=84, N=24, pro='ln3', epi='res', so=1, st=0), 'refused(4)', None),
    ('FDFFN project_in C=24', dict(K=24, N=64, pro='ln', epi=None), 'smallk_vec<1,ln,obf=0>', 'split_strip<2,ln,strip2=0>'),
    ('FDFFN project_out C=24', dict(K=64, N=24, pro=None, epi='res', so=1), 'narrow_tail<2,xbf=0>', None),
    ('FDFFN project_in C=24, bf16 hidden tensor', dict(K=24, N=64, pro='ln', epi=None, obf=1), 'smallk_vec<1,ln,obf=1>', None),
    ('FDFFN project_out C=24, bf16 hidden tensor', dict(K=64, N=24, pro=None, epi='res', so=1, xbf=1), 'narrow_tail<2,xbf=1>', None),
    ('FCAFFN project_in C=24', dict(K=24, N=24, pro='muladd', epi='muladd'), 'generic<1,muladd,4,1>', None),
    ('FCAFFN project_in C=24, statistics left to the kernel', dict(K=24, N=24, pro='muladd', epi='muladd', st=0), 'refused(4)', None),
    ('FDSA to_hidden C=32', dict(K=32, N=152, pro='ln', epi=None), 'smallk_vec<1,ln,obf=0>', 'split_strip<2,ln,strip2=0>'),
    ('FDSA project_out C=32', dict(K=114, N=32, pro='ln3', epi='res', so=1), 'generic<1,ln3,8,0>', None),
    ('FDSA project_out C=32, statistics left to the kernel', dict(K=114, N=32, pro='ln3', epi='res', so=1, st=0), 'refused(4)', None),
    ('FDFFN project_in C=32', dict(K=32, N=86, pro='ln', epi=None), 'smallk_vec<1,ln,obf=0>', 'split_strip<2,ln,strip2=0>'),
    ('FDFFN project_out C=32', dict(K=86, N=32, pro=None, epi='res', so=1), 'narrow_tail<3,xbf=0>', None),
    ('FDFFN project_in C=32, bf16 hidden tensor', dict(K=32, N=86, pro='ln', epi=None, obf=1), 'smallk_vec<1,ln,obf=1>', None),
    ('FDFFN project_out C=32, bf16 hidden tensor', dict(K=86, N=32, pro=None, epi='res', so=1, xbf=1), 'narrow_tail<3,xbf=1>', None),
    ('FCAFFN project_in C=32', dict(K=32, N=32, pro='muladd', epi='muladd'), 'generic<1,muladd,4,1>', None),
    ('FCAFFN project_in C=32, statistics left to the kernel', dict(K=32, N=32, pro='muladd', epi='muladd', st=0), 'refused(4)', None),
    ('FDSA to_hidden C=48', dict(K=48, N=228, pro='ln', epi=None), 'smallk<2,ln>', 'split_strip<3,ln,strip2=0>'),
    ('FDSA project_out C=48', dict(K=171, N=48, pro='ln3', epi='res', so=1), 'generic<2,ln3,4,0>', None),
    ('FDSA project_out C=48, statistics left to the kernel', dict(K=171, N=48, pro='ln3', epi='res', so=1, st=0), 'refused(4)', None),
    ('FDFFN project_in C=48', dict(K=48, N=129, pro='ln', epi=None), 'smallk_vec<2,ln,obf=0>', 'split_strip<3,ln,strip2=0>'),
    ('FDFFN project_out C=48', dict(K=129, N=48, pro=None, epi='res', so=1), 'kstream_vec<2,xbf=0>', None),
    ('FDFFN project_in C=48, bf16 hidden tensor', dict(K=48, N=129, pro='ln', epi=None, obf=1), 'smallk_vec<2,ln,obf=1>', None),
    ('FDFFN project_out C=48, bf16 hidden tensor', dict(K=129, N=48, pro=None, epi='res', so=1, xbf=1), 'kstream_vec<2,xbf=1>', None),
    ('FCAFFN project_in C=48', dict(K=48, N=48, pro='muladd', epi='muladd'), 'generic<2,muladd,4,1>', None),
    ('FCAFFN project_in C=48, statistics left to the kernel', dict(K=48, N=48, pro='muladd', epi='muladd', st=0), 'refused(4)', None),
    ('Fuse conv C=48', dict(K=48, N=48, pro=None, epi=None, so=1, segs=(24, 24)), 'generic<2,none,4,0>', None),
    ('Fuse conv2 C=48', dict(K=48, N=24, pro=None, epi=None, so=1), 'narrow_tail<2,xbf=0>', None),
    ('FDSA to_hidden C=64', dict(K=64, N=304, pro='ln', epi=None), 'smallk_stream_vec<2,ln>', 'split_strip<4,ln,strip2=0>'),
    ('FDSA project_out C=64', dict(K=228, N=64, pro='ln3', epi='res', so=1), 'generic<2,ln3,4,0>', None),
    ('FDSA project_out C=64, statistics left to the kernel', dict(K=228, N=64, pro='ln3', epi='res', so=1, st=0), 'refused(4)', None),
    ('FDFFN project_in C=64', dict(K=64, N=172, pro='ln', epi=None), 'smallk_vec<2,ln,obf=0>', 'split_strip<4,ln,strip2=0>'),
    ('FDFFN project_out C=64', dict(K=172, N=64, pro=None, epi='res', so=1), 'kstream_vec<2,xbf=0>', None),
    ('FDFFN project_in C=64, bf16 hidden tensor', dict(K=64, N=172, pro='ln', epi=None, obf=1), 'smallk_vec<2,ln,obf=1>', None),
    ('FDFFN project_out C=64, bf16 hidden tensor', dict(K=172, N=64, pro=None, epi='res', so=1, xbf=1), 'kstream_vec<2,xbf=1>', None),
    ('FCAFFN project_in C=64', dict(K=64, N=64, pro='muladd', epi='muladd'), 'generic<2,muladd,4,1>', None),
    ('FCAFFN project_in C=64, statistics left to the kernel', dict(K=64, N=64, pro='muladd', epi='muladd', st=0), 'refused(4)', None),
    ('Fuse conv C=64', dict(K=64, N=64, pro=None, epi=None, so=1, segs=(32, 32)), 'generic<2,none,4,0>', None),
    ('Fuse conv2 C=64', dict(K=64, N=32, pro=None, epi=None, so=1), 'narrow_tail<2,xbf=0>', None),
    ('FDSA to_hidden C=96', dict(K=96, N=460, pro='ln', epi=None), 'smallk_stream_vec<3,ln>', 'split_strip<6,ln,strip2=0>'),
    ('FDSA project_out C=96', dict(K=345, N=96, pro='ln3', epi='res', so=1), 'tile<ln3>', 'split<ln3>'),
    ('FDSA project_out C=96, statistics left to the kernel', dict(K=345, N=96, pro='ln3', epi='res', so=1, st=0), 'refused(4)', 'split<ln3>'),
    ('FDFFN project_in C=96', dict(K=96, N=259, pro='ln', epi=None), 'smallk_stream_vec<3,ln>', 'split_strip<6,ln,strip2=0>'),
    ('FDFFN project_out C=96', dict(K=259, N=96, pro=None, epi='res', so=1), 'tile<none>', 'split<none>'),
    ('FCAFFN project_in C=96', dict(K=96, N=96, pro='muladd', epi='muladd'), 'generic<3,muladd,8,0>', 'split<muladd>'),
    ('FCAFFN project_in C=96, statistics left to the kernel', dict(K=96, N=96, pro='muladd', epi='muladd', st=0), 'refused(4)', 'split<muladd>'),
    ('Fuse conv C=96', dict(K=96, N=96, pro=None, epi=None, so=1, segs=(48, 48)), 'generic<3,none,4,0>', None),
    ('Fuse conv2 C=96', dict(K=96, N=48, pro=None, epi=None, so=1), 'generic<2,none,4,0>', None),
    ('FDSA to_hidden C=128', dict(K=128, N=612, pro='ln', epi=None), 'smallk_stream_vec<4,ln>', 'split_strip<8,ln,strip2=1>'),
    ('FDSA project_out C=128', dict(K=459, N=128, pro='ln3', epi='res', so=1), 'tile<ln3>', 'split<ln3>'),
    ('FDSA project_out C=128, statistics left to the kernel', dict(K=459, N=128, pro='ln3', epi='res', so=1, st=0), 'refused(4)', 'split<ln3>'),
    ('FDFFN project_in C=128', dict(K=128, N=345, pro='ln', epi=None), 'smallk_stream_vec<4,ln>', 'split_strip<8,ln,strip2=1>'),
    ('FDFFN project_out C=128', dict(K=345, N=128, pro=None, epi='res', so=1), 'tile<none>', 'split<none>'),
    ('FCAFFN project_in C=128', dict(K=128, N=128, pro='muladd', epi='muladd'), 'generic<4,muladd,8,0>', 'split<muladd>'),
    ('FCAFFN project_in C=128, statistics left to the kernel', dict(K=128, N=128, pro='muladd', epi='muladd', st=0), 'refused(4)', 'split<muladd>'),
    ('Fuse conv C=128', dict(K=128, N=128, pro=None, epi=None, so=1, segs=(64, 64)), 'generic<4,none,4,0>', 'split<none>'),
    ('Fuse conv2 C=128', dict(K=128, N=64, pro=None, epi=None, so=1), 'kstream_vec<2,xbf=0>', None),
    ('FDSA to_hidden C=192', dict(K=192, N=920, pro='ln', epi=None), 'generic<1,ln,8,0>', 'split<ln>'),
    ('FDSA project_out C=192', dict(K=690, N=192, pro='ln3', epi='res', so=1), 'refused(1)', None),
    ('FDSA project_out C=192, statistics left to the kernel', dict(K=690, N=192, pro='ln3', epi='res', so=1, st=0), 'refused(1)', None),
    ('FDFFN project_in C=192', dict(K=192, N=518, pro='ln', epi=None), 'generic<1,ln,8,0>', 'split<ln>'),
    ('FDFFN project_out C=192', dict(K=518, N=192, pro=None, epi='res', so=1), 'refused(1)', None),
    ('FCAFFN project_in C=192', dict(K=192, N=192, pro='muladd', epi='muladd'), 'generic<3,muladd,8,0>', 'split<muladd>'),
    ('FCAFFN project_in C=192, statistics left to the kernel', dict(K=192, N=192, pro='muladd', epi='muladd', st=0), 'refused(4)', 'split<muladd>'),
    ('Fuse conv C=192', dict(K=192, N=192, pro=None, epi=None, so=0, segs=(96, 96)), 'generic<3,none,4,0>', 'split<none>'),
    ('Fuse conv2 C=192', dict(K=192, N=96, pro=None, epi=None, so=1), 'tile<none>', 'split<none>'),
    ('MAR FreBlock / process convs nc=12', dict(K=12, N=12, pro=None, epi=None), 'narrow_tail<1,xbf=0>', None),
    ('MAR process convs nc=12, LeakyReLU', dict(K=12, N=12, pro=None, epi=None, act=1), 'narrow_tail<1,xbf=0>', None),
    ('LOL-v1 ProcessBlock.cat nc=12', dict(K=12, N=12, pro=None, epi='res'), 'narrow_tail<1,xbf=0>', None),
    ('MAR FreBlock / process convs nc=24', dict(K=24, N=24, pro=None, epi=None), 'narrow_tail<1,xbf=0>', None),
    ('MAR process convs nc=24, LeakyReLU', dict(K=24, N=24, pro=None, epi=None, act=1), 'narrow_tail<1,xbf=0>', None),
    ('LOL-v1 ProcessBlock.cat nc=24', dict(K=24, N=24, pro=None, epi='res'), 'narrow_tail<1,xbf=0>', None),
    ('MAR FreBlock / process convs nc=48', dict(K=48, N=48, pro=None, epi=None), 'generic<2,none,4,0>', None),
    ('MAR process convs nc=48, LeakyReLU', dict(K=48, N=48, pro=None, epi=None, act=1), 'generic<2,none,4,0>', None),
    ('LOL-v1 ProcessBlock.cat nc=48', dict(K=48, N=48, pro=None, epi='res'), 'generic<2,none,4,1>', None),
    ('MAR stem 48->48', dict(K=48, N=48, pro=None, epi=None), 'generic<2,none,4,0>', None),
    ('MAR stem 12->24', dict(K=12, N=24, pro=None, epi=None), 'narrow_tail<1,xbf=0>', None),
    ('MAR stem 3->12', dict(K=3, N=12, pro=None, epi=None), 'narrow_tail<1,xbf=0>', None),
    ('MAR FAM1.merge1', dict(K=96, N=48, pro=None, epi=None, segs=(48, 48)), 'generic<2,none,4,0>', None),
    ('MAR FAM2.merge1', dict(K=48, N=24, pro=None, epi=None, segs=(24, 24)), 'generic<1,none,8,0>', None),
    ('MAR Convs[0]', dict(K=48, N=24, pro=None, epi=None, act=1, segs=(24, 24)), 'generic<1,none,8,0>', None),
    ('MAR Convs[1]', dict(K=24, N=12, pro=None, epi=None, act=1, segs=(12, 12)), 'generic<1,none,8,0>', None),
    ('MAR AFFs[0] fpre', dict(K=84, N=12, pro=None, epi=None, segs=(12, 24, 48)), 'generic<1,none,8,0>', None),
    ('MAR AFFs[1] fpre', dict(K=84, N=24, pro=None, epi=None, segs=(12, 24, 48)), 'generic<1,none,8,0>', None),
    ('MAR AFF multires 48->12', dict(K=48, N=12, pro=None, epi=None), 'narrow_tail<2,xbf=0>', None),
    ('MAR AFF multires 24->12 + res', dict(K=24, N=12, pro=None, epi='res'), 'narrow_tail<1,xbf=0>', None),
    ('MAR AFF multires 12->12 + res', dict(K=12, N=12, pro=None, epi='res'), 'narrow_tail<1,xbf=0>', None),
    ('MAR AFF multires 48->24', dict(K=48, N=24, pro=None, epi=None), 'narrow_tail<2,xbf=0>', None),
    ('MAR AFF multires [12|24]->24 + res', dict(K=36, N=24, pro=None, epi='res', segs=(12, 24)), 'generic<1,none,4,1>', None),
    ('LPNet SEBlock 16->16', dict(K=16, N=16, pro=None, epi=None, act=2), 'narrow_tail<1,xbf=0>', None),
    ('LPNet SEBlock 16->32', dict(K=16, N=32, pro=None, epi=None, act=0), 'narrow_tail<1,xbf=0>', None),
    ('LPNet SEBlock 32->16', dict(K=32, N=16, pro=None, epi=None, act=2), 'narrow_tail<1,xbf=0>', None),
    ('LPNet SEBlock 32->64', dict(K=32, N=64, pro=None, epi=None, act=0), 'smallk_vec<1,none,obf=0>', None),
    ('LPNet SEBlock 64->32', dict(K=64, N=32, pro=None, epi=None, act=2), 'narrow_tail<2,xbf=0>', None),
    ('LPNet SEBlock 64->128', dict(K=64, N=128, pro=None, epi=None, act=0), 'smallk_vec<2,none,obf=0>', None),
    ('LPNet SEBlock 128->64', dict(K=128, N=64, pro=None, epi=None, act=2), 'kstream_vec<2,xbf=0>', None),
    ('LPNet pooled 32->2', dict(K=32, N=2, pro=None, epi=None, act=2, P=1), 'generic<1,none,8,0>', None),
    ('LPNet pooled 2->32', dict(K=2, N=32, pro=None, epi=None, act=3, P=1), 'generic<1,none,8,0>', None),
    ('LPNet pooled 64->4', dict(K=64, N=4, pro=None, epi=None, act=2, P=1), 'generic<1,none,8,0>', None),
    ('LPNet pooled 4->64', dict(K=4, N=64, pro=None, epi=None, act=3, P=1), 'smallk<1,none>', None),
    ('LPNet pooled 128->8', dict(K=128, N=8, pro=None, epi=None, act=2, P=1), 'generic<1,none,8,0>', None),
    ('LPNet pooled 8->128', dict(K=8, N=128, pro=None, epi=None, act=3, P=1), 'smallk<1,none>', None),
    ('LPNet pooled 128->128', dict(K=128, N=128, pro=None, epi=None, act=0, P=1), 'tile<none>', 'split<none>'),
    ('LPNet pooled 128->1', dict(K=128, N=1, pro=None, epi=None, act=3, P=1), 'generic<1,none,8,0>', None),
    ("named in the route's comments: 32->152", dict(K=32, N=152, pro='ln', epi=None), 'smallk_vec<1,ln,obf=0>', 'split_strip<2,ln,strip2=0>'),
    ("named in the route's comments: 64->172", dict(K=64, N=172, pro='ln', epi=None), 'smallk_vec<2,ln,obf=0>', 'split_strip<4,ln,strip2=0>'),
    ("named in the route's comments: 64->304", dict(K=64, N=304, pro='ln', epi=None), 'smallk_stream_vec<2,ln>', 'split_strip<4,ln,strip2=0>'),
    ("named in the route's comments: 128->612", dict(K=128, N=612, pro='ln', epi=None), 'smallk_stream_vec<4,ln>', 'split_strip<8,ln,strip2=1>'),
    ("named in the route's comments: 128->345", dict(K=128, N=345, pro='ln', epi=None), 'smallk_stream_vec<4,ln>', 'split_strip<8,ln,strip2=1>'),
    ("named in the route's comments: 172->64", dict(K=172, N=64, pro=None, epi='res'), 'kstream_vec<2,xbf=0>', None),
    ("named in the route's comments: 345->128", dict(K=345, N=128, pro=None, epi='res'), 'tile<none>', 'split<none>'),
    ("named in the route's comments: 459->128", dict(K=459, N=128, pro='ln3', epi='res'), 'tile<ln3>', 'split<ln3>'),
]

CONV1X1_GEOMETRY_ROUTES = {   # case of test_gpu_geometry.CONV1X1: (instantiation, threads, pixels per tile)
    'smallk_res': ('smallk<1,ln>', 512, 256),
    'smallk_vec': ('smallk_vec<1,ln,obf=0>', 256, 256),
    'smallk_muladd': ('smallk<1,muladd>', 512, 256),
    'smallk_stream': ('smallk_stream<3,ln>', 512, 256),
    'stream_vec': ('smallk_stream_vec<3,none>', 512, 512),
    'ln3_resident': ('generic<1,ln3,8,0>', 512, 256),
    'ln3_streaming': ('generic<5,ln3,4,0>', 256, 128),
    'act_res_stats': ('generic<4,none,4,0>', 256, 128),
    'early_muladd': ('generic<1,muladd,4,1>', 256, 128),
    'kstream_vec': ('kstream_vec<2,xbf=0>', 256, 256),
    'narrow_tail': ('narrow_tail<3,xbf=0>', 256, 256),
}

# test_gpu_parity.test_conv1x1_variants (K, N, H, W, prologue): (without a weight cache, with one)
CONV1X1_VARIANT_ROUTES = {
    (32, 152, 24, 40, 'ln'): ('generic<5,ln,4,0>', 'generic<5,ln,4,0>'),
    (64, 304, 16, 24, 'ln'): ('smallk<2,ln>', 'smallk<2,ln>'),
    (128, 612, 8, 24, 'ln'): ('smallk_stream<4,ln>', 'split<ln>'),
    (96, 345, 8, 16, 'none'): ('smallk_stream<3,none>', 'split<none>'),
    (86, 32, 46, 21, 'none'): ('generic<1,none,8,0>', 'generic<1,none,8,0>'),
    (459, 128, 8, 16, 'ln3'): ('tile<ln3>', 'split<ln3>'),
    (114, 32, 24, 40, 'ln3'): ('generic<1,ln3,8,0>', 'generic<1,ln3,8,0>'),
    (32, 32, 16, 24, 'muladd'): ('generic<1,muladd,4,1>', 'generic<1,muladd,4,1>'),
    (300, 128, 9, 21, 'ln3'): ('tile<ln3>', 'split<ln3>'),
    (200, 100, 9, 21, 'none'): ('tile<none>', 'split<none>'),
    (345, 128, 23, 40, 'none'): ('tile<none>', 'split<none>'),
}

# test_gpu_parity.test_conv1x1_split_bf16_kernel (K, N, H, W, prologue, epilogue): the split-bf16 form the packed weights reach
CONV1X1_SPLIT_ROUTES = {
    (128, 612, 23, 40, 'ln', 'none'): 'split_strip<8,ln,strip2=1>',
    (128, 345, 184, 320, 'ln', 'none'): 'split_strip<8,ln,strip2=1>',
    (459, 128, 23, 41, 'ln3', 'res'): 'split<ln3>',
    (345, 128, 184, 320, 'none', 'res'): 'split<none>',
    (128, 128, 23, 40, 'muladd', 'muladd'): 'split<muladd>',
    (96, 96, 5, 7, 'none', 'bias'): 'split<none>',
    (100, 130, 9, 13, 'ln', 'res'): 'split<ln>',
    (345, 128, 8, 17, 'ln3', 'none'): 'split<ln3>',
    (128, 128, 184, 320, 'muladd', 'muladd'): 'split<muladd>',
    (96, 460, 9, 13, 'ln', 'none'): 'split_strip<6,ln,strip2=0>',
    (100, 300, 9, 13, 'none', 'bias'): 'split_strip<7,none,strip2=0>',
    (100, 300, 9, 13, 'ln', 'none'): 'split_strip<7,ln,strip2=0>',
    (128, 612, 184, 320, 'ln', 'bias'): 'split_strip<8,ln,strip2=1>',
    (32, 86, 23, 40, 'ln', 'none'): 'split_strip<2,ln,strip2=0>',
    (64, 172, 46, 80, 'ln', 'none'): 'split_strip<4,ln,strip2=0>',
    (48, 129, 9, 13, 'ln', 'bias'): 'split_strip<3,ln,strip2=0>',
    (24, 64, 9, 13, 'none', 'none'): 'split_strip<2,none,strip2=0>',
    (64, 172, 368, 640, 'ln', 'none'): 'split_strip<4,ln,strip2=0>',
}

# test_gpu_parity.test_conv1x1_two_inputs_on_the_split_bf16_kernel (K0, K1, N, H, W)
CONV1X1_TWO_INPUT_ROUTES = {
    (64, 64, 128, 23, 41): 'split<none>',
    (96, 32, 96, 9, 13): 'split<none>',
    (64, 64, 128, 368, 640): 'split<none>',
    (32, 96, 130, 8, 17): 'split<none>',
}
