"""Shared helpers for the parity tests (fixtures, synthetic weights, tolerance policy)."""
import json
import os

import numpy as np
import torch

from weights import synth_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 7  # tests/golden/make_golden.py


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
