"""Weight updates reach every derived operand and every captured graph.

The mirror modules keep derived weights (LayerNorm folds, concatenated gammas, split-bf16 packs, the fdsa / fcaffn operand images, BatchNorm
folds, tap-rearranged upsample weights, split fpre weights) in ops.WeightCache entries, each behind a hand-written list of source tensors;
the graph holders key their captures on pipeline.weights_signature.  A list that forgets a tensor is a model that keeps computing with
the old weights after a checkpoint is loaded into it, and a parity test on a fresh module cannot see that.

Criterion used throughout: WARM is a module that has run (its caches are full), COLD is copy.deepcopy(module) taken after the update
(WeightCache.__deepcopy__ gives it empty caches, a GraphedForward copies to None).  After an update warm(x) must equal cold(x) with
torch.equal: the same kernels on the same operands on one stream, a regime the suite pins as bit-stable (test_single_stream_bit_stable,
test_batch_independence_and_determinism).  Before a comparison is trusted two cold copies of the same weights are checked to agree bit for
bit, and the output after an update must differ from the output before it; the parameters for which it does not are listed in DEAD, each
with the line of the mirror that shows it is never read, and the tests assert that exactly those are dead."""
import contextlib
import copy
import pickle
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import lpips_ref as R
from common import fdn_shapes, fdn_weights, fixture, fixture_weights, lolv1_shapes, lolv1_weights, lpnet_weights
from weights import shapes_of, synth_state_dict

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()   # fail loudly if the HIP extension is not built
    from basicsr.models.archs import FDN_arch
    return FDN_arch


def dev(t):
    return t.to(DEV).contiguous()


def load(mod, sd):
    mod.load_state_dict(sd, strict=True)
    return mod.to(DEV).eval()


def _rnd(*s, seed):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------------------------------------------
OPS_SWITCHES = {"full": ("FDSA_FULL", True), "no_tail": ("FDSA_TAIL", False), "no_pin": ("FDSA_TAIL_PIN", False), "split": ("FFN_TAIL_MODE", "split"),
                "no_own_stats": ("GEMM_OWN_STATS", False), "no_gather": ("UPCONV_GATHER", False), "no_multires": ("AFF_MULTIRES", False)}
ROUTES = ("default", "f32pipe", "bf16store") + tuple(OPS_SWITCHES)


@contextlib.contextmanager
def route(name):
    """one routing switch away from the defaults; everything is restored on the way out (a leaked switch changes later tests' routes)"""
    import fdn_hip
    from fdn_hip import ops
    pipe, store = fdn_hip.matrix_pipe_mode(), fdn_hip.storage_dtype()
    saved = {k: getattr(ops, k) for k, _ in OPS_SWITCHES.values()}
    try:
        if name == "f32pipe":
            fdn_hip.set_matrix_pipe("f32")
        elif name == "bf16store":
            fdn_hip.set_storage_dtype("bf16")
        elif name != "default":
            setattr(ops, *OPS_SWITCHES[name])
        yield
    finally:
        fdn_hip.set_matrix_pipe(pipe)
        fdn_hip.set_storage_dtype(store)
        for k, v in saved.items():
            setattr(ops, k, v)


# ---------------------------------------------------------------------------------------------------------------------------------
# B. modules: name -> () -> (module on the device, call(module) -> tensor).  Inputs: the fixture's where tests/golden has one
# ---------------------------------------------------------------------------------------------------------------------------------
_inputs = {}


def _fx_inputs(name, keys):
    if name not in _inputs:
        fx = fixture(name)
        _inputs[name] = tuple(dev(fx[k]) for k in keys)
    return _inputs[name]


def _guided(key, B, C, H, W):
    """(x, amp, pha, img) in the layout of the fcaffn / tblock fixtures, seeded"""
    if key not in _inputs:
        g = torch.Generator().manual_seed(C + H + W)
        _inputs[key] = tuple(dev(t) for t in (torch.randn(B, C, H, W, generator=g), torch.rand(B, 3, H, W // 2 + 1, generator=g) * 2.0,
                                              torch.rand(B, 3, H, W // 2 + 1, generator=g) * 6.2 - 3.1, torch.rand(B, 3, H, W, generator=g)))
    return _inputs[key]


def _synth(mod, key, seed=7, po_scale=None):
    sd = synth_state_dict(shapes_of(mod), seed, prefix_key=key + "/")
    if po_scale is not None:
        sd = {k: v * po_scale if k.endswith("project_out.weight") else v for k, v in sd.items()}
    return sd


def _spec_fdsa(c):
    def make():
        from basicsr.models.archs.FDN_arch import FDSA
        name = f"fdsa_c{c}"
        x, = _fx_inputs(name, ("x",))
        return load(FDSA(c), fixture_weights(name, fixture(name)["shapes"])), lambda m: m(x)
    return make


def _spec_fdffn(c):
    def make():
        from basicsr.models.archs.FDN_arch import FDFFN
        name = f"fdffn_c{c}"
        x, = _fx_inputs(name, ("x",))
        return load(FDFFN(c), fixture_weights(name, fixture(name)["shapes"])), lambda m: m(x)
    return make


def _spec_fcaffn(c, name, shape=None):
    def make():
        from basicsr.models.archs.FDN_arch import FCAFFN
        args = _fx_inputs(name, ("x", "amp", "pha", "img")) if shape is None else _guided(("fcaffn", c) + shape, 1, c, *shape)
        return load(FCAFFN(c), fixture_weights(name, fixture(name)["shapes"])), lambda m: m(*args)
    return make


def _spec_tblock(dim, light):
    def make():
        from basicsr.models.archs.FDN_arch import TransformerBlock
        m = TransformerBlock(dim=dim, att=True, use_light=light, use_img=light)
        if dim == 32:
            name = "tblock_enc_c32" if light else "tblock_dec_c32"
            fx = fixture(name)
            sd = fixture_weights(name, fx["shapes"], po_scale=float(fx["po_scale"]))
            args = _fx_inputs(name, ("x", "amp", "pha", "img"))
        else:                                        # level-2 width at the level-2 fixtures' 16 x 24
            sd = _synth(m, f"tblock_c{dim}_{int(light)}", po_scale=0.1)
            args = _guided(("tblock", dim), 1, dim, 16, 24)
        return load(m, sd), lambda m: m(args)[0]
    return make


def _spec_fuse():
    from basicsr.models.archs.FDN_arch import Fuse
    enc, dnc = _fx_inputs("fuse_n32", ("enc", "dnc"))
    return load(Fuse(32), fixture_weights("fuse_n32", fixture("fuse_n32")["shapes"])), lambda m: m(enc, dnc)


def _spec_up():
    from basicsr.models.archs.FDN_arch import Upsample
    x, = _fx_inputs("upsample_c64", ("x",))
    return load(Upsample(64), fixture_weights("upsample_c64", fixture("upsample_c64")["shapes"])), lambda m: m(x)


def _spec_aff(which):
    """the two splits MAR_archa.forward feeds its fourier_fuse modules (FDN_arch.py:502-511): AFFs[0] takes (res1 | x2 res2 | x4 z),
    AFFs[1] takes (z12, res2 | x2 z); called as MAR_archa calls them, per source resolution or on the resized copies (ops.AFF_MULTIRES)"""
    def make():
        from basicsr.models.archs.FDN_arch import fourier_fuse
        from fdn_hip import ops
        c, H, W = 12, 16, 24
        m = fourier_fuse(7 * c, c if which == 0 else 2 * c)
        key = ("aff", which)
        if key not in _inputs:
            if which == 0:
                _inputs[key] = ([dev(_rnd(1, c, H, W, seed=1))], dev(_rnd(1, 2 * c, H // 2, W // 2, seed=2)), dev(_rnd(1, 4 * c, H // 4, W // 4, seed=3)))
            else:
                _inputs[key] = ([dev(_rnd(1, c, H, W, seed=4)), dev(_rnd(1, 2 * c, H, W, seed=5))], None, dev(_rnd(1, 4 * c, H // 2, W // 2, seed=6)))
        same, up1, up2 = _inputs[key]

        def call(m):
            if ops.AFF_MULTIRES:
                return m.forward_multires(same, up1, up2)
            big2 = ops.resample(up2, ops.RS_NEAREST_X2)
            if up1 is not None:
                return m(same[0], ops.resample(up1, ops.RS_NEAREST_X2), ops.resample(big2, ops.RS_NEAREST_X2))
            return m(same[0], same[1], big2)
        return load(m, _synth(m, f"aff{which}")), call
    return make


def _spec_se(shortcut):
    def make():
        from basicsr.models.archs.LPNet_arch import SEBlock
        m = SEBlock(16, (16, 16, 32), stride=2, is_1x1conv=True) if shortcut else SEBlock(32, (16, 16, 32), stride=1, is_1x1conv=False)
        key = ("se", shortcut)
        if key not in _inputs:
            _inputs[key] = dev(_rnd(2, 16 if shortcut else 32, 16, 24, seed=8))
        x = _inputs[key]
        sd = _synth(m, f"se{int(shortcut)}")
        sd["se.1.bias"] = torch.full_like(sd["se.1.bias"], 0.5)          # the gate's two hidden units stay on the live side of their ReLU
        return load(m, sd), lambda m: m(x)
    return make


def _spec_lpnet():
    from basicsr.models.archs.LPNet_arch import I_predict_net
    x, = _fx_inputs("lpnet_real", ("x",))
    return load(I_predict_net(), lpnet_weights()), lambda m: m(x)


SPECS = {
    "fdsa32": _spec_fdsa(32), "fdsa64": _spec_fdsa(64), "fdsa128": _spec_fdsa(128),
    "fdffn32": _spec_fdffn(32), "fdffn64": _spec_fdffn(64), "fdffn128": _spec_fdffn(128),
    "fcaffn32": _spec_fcaffn(32, "fcaffn_c32_32x32"), "fcaffn64": _spec_fcaffn(64, "fcaffn_c64_46x40"), "fcaffn128": _spec_fcaffn(128, "fcaffn_c128_16x16"),
    # W % 4 != 0: the "split" tail (fdn_dwconv_gate + the project_out GEMM with its cache entry) is what runs by default.  FCAFFN only:
    # fdn_fdffn_mid takes whole 8 x 8 patches (W % 8 == 0), so an FDFFN never meets such a width; its default "split" tail is fdffn128 (N > 64)
    "fcaffn32_w26": _spec_fcaffn(32, "fcaffn_c32_32x32", (18, 26)),
    "tblock32_light": _spec_tblock(32, True), "tblock32": _spec_tblock(32, False), "tblock64_light": _spec_tblock(64, True), "tblock64": _spec_tblock(64, False),
    "fuse32": _spec_fuse, "up64": _spec_up, "aff0": _spec_aff(0), "aff1": _spec_aff(1),
    "se_shortcut_s2": _spec_se(True), "se_plain_s1": _spec_se(False), "lpnet": _spec_lpnet,
}
# Which (module, route) pairs run.  A pair is skipped only where the switch cannot change that module's launches:
#   f32pipe      every module has matrix products that the library routes by the pipe mode: all run
#   bf16store    read by ops.block_storage alone, for FDSA / FDFFN of C <= 64: not fdsa128, fdffn128, FCAFFN, Upsample, fourier_fuse, LPNet
#   full         FDSA.fused with C <= ops.FDSA_FULL_MAX_C = 32 only: fdsa32 and the 32-wide blocks (Fuse's block has no FDSA)
#   no_tail      FDSA.fused with C in ops.FDSA_FUSED_C: fdsa32 / 64 and the blocks
#   no_pin       FDSA.fused with pin= and C <= ops.FDSA_TAIL_PIN_MAX_C = 32: the 32-wide blocks only
#   split        ops.ffn_tail where the default is not "split" already (N <= 64, W % 4 == 0): not the 128-wide modules, not fcaffn32_w26
#   no_own_stats FDSA's and FCAFFN's level-3 GEMMs: fdsa128, fcaffn128
#   no_gather    Upsample;  no_multires  fourier_fuse as MAR_archa calls it
RUNS = {
    "default": set(SPECS), "f32pipe": set(SPECS),
    "bf16store": {"fdsa32", "fdsa64", "fdffn32", "fdffn64", "tblock32_light", "tblock32", "tblock64_light", "tblock64", "fuse32"},
    "full": {"fdsa32", "tblock32_light", "tblock32"},
    "no_tail": {"fdsa32", "fdsa64", "tblock32_light", "tblock32", "tblock64_light", "tblock64"},
    "no_pin": {"tblock32_light", "tblock32"},
    "split": {"fdffn32", "fdffn64", "fcaffn32", "fcaffn64", "tblock32_light", "tblock32", "tblock64_light", "tblock64", "fuse32"},
    "no_own_stats": {"fdsa128", "fcaffn128"}, "no_gather": {"up64"}, "no_multires": {"aff0", "aff1"},
}
# Parameters / buffers whose update must NOT change the output, by regular expression on the name, with the line that shows they are never read.
DEAD = {
    r"(^|\.)num_batches_tracked$": "BatchNorm's step counter: _fold (LPNet_arch.py:43-52) reads weight, bias, running_mean, running_var only",
    r"^net_a\.net\..*\.cat\.(weight|bias)$": "FDN_arch.py:419 `self.cat = ...  # in the checkpoint, never called`; ProcessBlock.forward (:421-422) runs frequency_process only",
    r"^net_p\.reduce_chan_level2\.weight$": "FDN_arch.py:322 `# in the checkpoint, never called`; FDformer.forward (:332-344) goes through fuse2 instead",
    r"^net_p\.norm\.body\.(weight|bias)$": "FDN_arch.py:330 `# in the checkpoint, never called`; FDformer.forward (:332-344) never applies self.norm",
}
DEAD_LOLV1 = {k: v for k, v in DEAD.items() if ".cat." not in k}          # fdnlol24_arch.py:38: the LOL-v1 ProcessBlock applies its cat conv


def _is_dead(name, table=DEAD):
    return any(re.search(p, name) for p in table)


def _tensors(m, own_only=False):
    """every parameter and buffer of the tree (BatchNorm running statistics included); own_only: those of the root module's direct
    children that are not SEBlock stages (I_predict_net's stem and heads: its SEBlocks are swept on their own)"""
    named = list(m.named_parameters()) + list(m.named_buffers())
    if own_only:
        named = [(n, t) for n, t in named if re.match(r"(conv1|fc|fc2)\.", n)]
    return named


def _changed(t):
    return t * 1.25 + 0.01 if t.is_floating_point() else t + 1


def _owner(m, name):
    mod, _, leaf = name.rpartition(".")
    return (m.get_submodule(mod) if mod else m), leaf


def _replace(m, name):
    """the Parameter (or buffer tensor) object replaced by a new one with changed values"""
    own, leaf = _owner(m, name)
    old = getattr(own, leaf)
    new = _changed(old.detach().clone())
    setattr(own, leaf, nn.Parameter(new, requires_grad=old.requires_grad) if isinstance(old, nn.Parameter) else new)


def _cold(m):
    return copy.deepcopy(m)


def _precondition(m, call, what):
    """two cold copies of the same weights agree bit for bit (else a warm / cold difference would prove nothing) and are finite"""
    a, b = call(_cold(m)), call(_cold(m))
    assert torch.isfinite(a).all(), what
    assert torch.equal(a, b), f"{what}: two cold copies of the same weights differ - the comparison cannot be trusted"


def _sweep(m, call, what, names, dead_table=DEAD):
    """every tensor of `names`: updated in place, then its object replaced; warm must equal cold each time, and differ from before
    exactly for the tensors that are not dead.  Every tensor's turn starts from the module's first weights, loaded back into the warm
    module (updates piled on one another drive LPNet's sigmoid into saturation, where a small update no longer shows).  Returns the
    names found dead."""
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    found_dead = []
    with torch.no_grad():
        for name in names:
            m.load_state_dict(sd0, strict=True)
            before = call(m)
            own, leaf = _owner(m, name)
            t = getattr(own, leaf)
            t.copy_(_changed(t))
            got = call(m)
            assert torch.equal(got, call(_cold(m))), f"{what}: stale operands after an in-place update of {name}"
            dead = torch.equal(got, before)
            _replace(m, name)
            got2 = call(m)
            assert torch.equal(got2, call(_cold(m))), f"{what}: stale operands after {name} was replaced by a new object"
            assert torch.equal(got2, got) == dead, (what, name)
            if dead:
                found_dead.append(name)
            assert torch.isfinite(got2).all(), (what, name)
    assert sorted(found_dead) == sorted(n for n in names if _is_dead(n, dead_table)), f"{what}: the dead-parameter list is wrong"
    return found_dead


PAIRS = [(s, r) for r in ROUTES for s in SPECS if s in RUNS[r]]


@pytest.mark.parametrize("spec,rt", PAIRS, ids=[f"{s}-{r}" for s, r in PAIRS])
def test_module_sweep(A, spec, rt):
    """B: per module, per parameter / buffer, per route - in place, replaced object, then every tensor at once through load_state_dict"""
    with route(rt), torch.no_grad():
        m, call = SPECS[spec]()
        what = f"{spec} [{rt}]"
        _precondition(m, call, what)
        first = call(m)                                           # warm
        assert torch.equal(first, call(_cold(m))), f"{what}: warm and cold differ before any update"
        _sweep(m, call, what, [n for n, _ in _tensors(m, own_only=spec == "lpnet")])
        before = call(m)
        sd2 = {k: (v if not v.is_floating_point() else v + 0.05 * _rnd(*v.shape, seed=31 + i).to(v.device) * (v.abs().mean() + 0.01))
               for i, (k, v) in enumerate(m.state_dict().items())}                       # a second seeded state dict of the same shapes
        m.load_state_dict(sd2, strict=True)
        got = call(m)
        assert torch.equal(got, call(_cold(m))), f"{what}: stale operands after load_state_dict"
        assert not torch.equal(got, before) and torch.isfinite(got).all(), what


ROUTE_PAIRS = [("default", "full"), ("default", "f32pipe"), ("default", "split"), ("default", "bf16store")]          # (f32 storage, bf16 storage) is the last
ROUTE_PAIR_SPECS = {"full": ["fdsa32", "tblock32_light"], "f32pipe": ["tblock32_light", "tblock64_light", "fdsa128", "fdffn128", "fcaffn128", "up64"],
                    "split": ["tblock32_light", "tblock64_light", "fuse32"], "bf16store": ["tblock32_light", "tblock64", "fuse32"]}
RP_CASES = [(a, b, s) for a, b in ROUTE_PAIRS for s in ROUTE_PAIR_SPECS[b]] + [(b, a, s) for a, b in ROUTE_PAIRS for s in ROUTE_PAIR_SPECS[b]]


@pytest.mark.parametrize("r1,r2,spec", RP_CASES, ids=[f"{s}-{a}-{b}" for a, b, s in RP_CASES])
def test_route_change_over_a_warm_cache(A, r1, r2, spec):
    """Warm under R1, run under R2, update every tensor under R2 and run, back under R1: the entries R1 left behind (and R2 did not touch)
    must not be served.  Warm and cold are compared within one mode."""
    with torch.no_grad():
        with route(r1):
            m, call = SPECS[spec]()
            _precondition(m, call, f"{spec} [{r1}]")
            first = call(m)
        with route(r2):
            _precondition(m, call, f"{spec} [{r2}]")
            call(m)
            for _, t in _tensors(m):
                t.copy_(_changed(t))
            got2 = call(m)
            assert torch.equal(got2, call(_cold(m))), f"{spec}: stale operands under {r2} after an update (warmed under {r1})"
        with route(r1):
            got = call(m)
            assert torch.equal(got, call(_cold(m))), f"{spec}: back under {r1}, the operands built before the update under {r2} were served"
            assert not torch.equal(got, first)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. whole nets and the graph holders
# ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 3, 32, 32), (2, 3, 32, 64)]
SEED_B = 8


def _net_cls(kind):
    if kind == "fdn":
        from basicsr.models.archs.FDN_arch import FDN
        return FDN
    from basicsr.models.archs.fdnlol24_arch import FDN_lolv1
    return FDN_lolv1


def _sd(kind, which):
    """state dict A (the suite's tamed synthetic weights) or B (the same shapes and taming, another seed)"""
    if kind == "lpnet":
        return lpnet_weights() if which == "A" else synth_state_dict(shapes_of(lpnet_weights()), SEED_B, prefix_key="lpnet/")
    if which == "A":
        return fdn_weights(tame=0.03) if kind == "fdn" else lolv1_weights(tame=0.03)
    shapes, prefix = (fdn_shapes(), "fdn/") if kind == "fdn" else (lolv1_shapes(), "fdnlol/")
    return synth_state_dict(shapes, SEED_B, prefix_key=prefix, tame=0.03)


def _build(kind, which):
    from basicsr.models.archs.LPNet_arch import I_predict_net
    return load(I_predict_net() if kind == "lpnet" else _net_cls(kind)(), _sd(kind, which))


def _x(shape, seed=3):
    return dev(torch.rand(*shape, generator=torch.Generator().manual_seed(seed + shape[0] + shape[3])))


def _paths(net, lp):
    """the ways a forward is driven, each -> a result tensor for x; holders are made once so that they capture before the update"""
    from fdn_hip import harness, pipeline, tiling
    gf, gs = pipeline.GraphedForward(net, lp), pipeline.GraphedStep(net, lp, n_streams=1)
    return {
        "eager": lambda x: net(x, ratio_i=lp(x), device=x.device)[0],
        "run": lambda x: pipeline.run(net, lp, x),
        "GraphedForward": gf,
        "GraphedStep": gs,
        "enhance_u8": lambda x: harness.enhance_u8(net, lp, (x.permute(0, 2, 3, 1) * 255).round().to(torch.uint8).contiguous(), bgr=True),
        "forward_tiled": lambda x: tiling.forward_tiled(net, lp, x[:1, :, :, :64].contiguous(), 32, 32) if x.shape[3] >= 64 else None,
    }


@pytest.fixture(scope="module")
def want_B(A):
    """what nets built from state dict B give, per (kind, shape, path): computed once, shared, never changed"""
    out = {}
    with torch.no_grad():
        lp = _build("lpnet", "B")
        for kind in ("fdn", "lolv1"):
            net = _build(kind, "B")
            paths = _paths(net, lp)
            for shape in SHAPES:
                x = _x(shape)
                for name in ("eager", "enhance_u8", "forward_tiled"):          # (the graph paths are held to the eager result)
                    r = paths[name](x)
                    out[kind, shape, name] = None if r is None else r.clone()
                out["lpnet", shape] = lp(x).clone()
    torch.cuda.synchronize()
    return out


def _load_B(how, kind, mod):
    sd = {k: v.to(DEV) for k, v in _sd(kind, "B").items()}
    if how == "load_state_dict":
        mod.load_state_dict(sd, strict=True)
    elif how == "assign":
        mod.load_state_dict(sd, strict=True, assign=True)
    else:                                                      # parameter by parameter
        with torch.no_grad():
            for k, t in list(mod.named_parameters()) + list(mod.named_buffers()):
                t.copy_(sd[k])


# calls per path and phase: a holder's third call on a shape replays its graph; enhance_u8 goes through pipeline.run's holder on the model, which
# the "run" path in front of it has captured on the same shape, so its one call is a replay; the eager paths hold no state between calls
CALLS = {"eager": 1, "run": 3, "GraphedForward": 3, "GraphedStep": 3, "enhance_u8": 1, "forward_tiled": 1}


@pytest.mark.parametrize("how", ["load_state_dict", "assign", "copy_"])
@pytest.mark.parametrize("kind", ["fdn", "lolv1"])
def test_checkpoint_into_a_warmed_net(A, want_B, kind, how):
    """Checkpoint B loaded into nets warmed (and captured) on A gives, through every way a forward is driven, the bits of nets built from B"""
    with torch.no_grad():
        net, lp = _build(kind, "A"), _build("lpnet", "A")
        paths = _paths(net, lp)
        xs = {shape: _x(shape) for shape in SHAPES}
        on_A = {}
        for shape, x in xs.items():
            for name, fn in paths.items():
                for _ in range(CALLS[name]):                   # the graph holders: eager / capture / replay (GraphedStep: capture, replay, replay)
                    r = fn(x)
                on_A[shape, name] = None if r is None else r.clone()
            for name in ("run", "GraphedForward", "GraphedStep"):
                assert torch.equal(on_A[shape, name], on_A[shape, "eager"]), (name, shape)
        assert len(paths["GraphedForward"]._graphs) == len(SHAPES) and paths["GraphedStep"].captures == len(SHAPES)
        assert len(net.__dict__["_fdn_graphed"]._graphs) >= 1
        _load_B(how, kind, net)
        _load_B(how, "lpnet", lp)
        for shape, x in xs.items():
            assert torch.equal(lp(x), want_B["lpnet", shape]), (how, shape)
            for name, fn in paths.items():
                want = want_B[kind, shape, name if name in ("enhance_u8", "forward_tiled") else "eager"]
                if want is None:
                    continue
                for i in range(CALLS[name]):
                    assert torch.equal(fn(x), want), f"{kind} {how} {name} {shape} call {i}: not the result of a net built from B"
                assert not torch.equal(want, on_A[shape, name]), (name, shape)


# Indices that only select among INSTANCES of one module class are removed from a key: the block index inside a stage, the level of a stage,
# and the numbered containers and twins of MAR (Encoder / Decoder / AFFs / Convs / ConvsOut, f1..f3, FAM1/2, the down / up convs) and of the
# FDformer (fuse1/2, down1_2 / down2_3, up3_2 / up2_1, FDN's norm1..3).  Each instance has its own WeightCache, so updating all of them at once
# cannot hide a stale entry of one of them.  Indices INSIDE a module stay (attn.norm1..3, a block's norm1..3, space.0 / space.2,
# process1.0 / .2, fpre.0 / .1): those tensors feed the same module's entries, and updated together the one that a source list names would
# rebuild the entry for the one it forgot.
_INSTANCE_INDEX = [(r"^(net_p\.(?:encoder|decoder)_level)\d\.\d+\.", r"\1#.#."), (r"^(net_p\.refinement)\.\d+\.", r"\1.#."),
                   (r"^net_p\.fuse\d\.", "net_p.fuse#."), (r"^net_p\.down\d_\d\.", "net_p.down#."), (r"^net_p\.up\d_\d\.", "net_p.up#."),
                   (r"^(net_a\.net\.(?:Encoder|Decoder|AFFs|Convs|ConvsOut))\.\d+\.", r"\1.#."), (r"^net_a\.net\.f\d\.", "net_a.net.f#."),
                   (r"^net_a\.net\.FAM\d\.", "net_a.net.FAM#."), (r"^net_a\.net\.f\d_(down|up)\.", r"net_a.net.f#_\1."), (r"^norm\d\.", "norm#.")]


def _class_of(key):
    """all encoder_level*.*.attn.project_out.weight are one class"""
    for pat, rep in _INSTANCE_INDEX:
        key = re.sub(pat, rep, key)
    return key


def _fdn_classes():
    cls = {}
    for k in fdn_shapes():
        cls.setdefault(_class_of(k), []).append(k)
    return cls


N_CHUNKS = 6


def _fresh_caches(m):
    """every WeightCache of the tree replaced by a new, empty one"""
    from fdn_hip import ops
    for mod in m.modules():
        for k, v in list(mod.__dict__.items()):
            if isinstance(v, ops.WeightCache):
                mod.__dict__[k] = ops.WeightCache()


@pytest.fixture(scope="module")
def warm_fdn(A):
    """The one warmed FDN the class sweep updates, case after case (each class once), and the one cold tree it is compared with.
    A class is judged on the forward of the sub-net that owns it - MAR (net_a), the FDformer (net_p), or the whole FDN for FDN's own
    LayerNorms - on the arguments FDN.forward gave that sub-net in the warming forward (taken by a hook, then held fixed)."""
    with torch.no_grad():
        net, lp = _build("fdn", "A"), _build("lpnet", "A")
        x = _x(SHAPES[0])
        ratio = lp(x)
        full = lambda m: m(x, ratio_i=ratio, device=x.device)[0]
        _precondition(net, full, "FDN")
        args = {}
        hooks = [getattr(net, sub).register_forward_pre_hook(lambda mod, a, kw, sub=sub: args.__setitem__(sub, (a, kw)), with_kwargs=True)
                 for sub in ("net_a", "net_p")]
        full(net)                                              # warm: every cache of the tree is full now
        for h in hooks:
            h.remove()
        calls = {"net_a": lambda m: torch.cat([t.flatten() for t in m.net_a(*args["net_a"][0], **args["net_a"][1])]),
                 "net_p": lambda m: m.net_p(*args["net_p"][0], **args["net_p"][1]), "": full}
        cold = copy.deepcopy(net)
    return net, cold, calls


@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_fdn_parameter_class_sweep(A, warm_fdn, chunk):
    """Every parameter class of FDN (all instances of a module class at once, see _INSTANCE_INDEX), one class at a time in the warmed net,
    compared after each class with a cold tree: catches a cache site in a module that the module list above missed.  1 x 3 x 32 x 32.
    The cold tree is one deep copy that receives each class's changed tensors and gets new, empty caches before every comparison; at the
    end of a case it is held against a deep copy taken then.  The classes are dealt over the cases in turn, and every case updates the
    same warmed net on top of the cases before it (a case selected alone starts from the first weights instead)."""
    classes = _fdn_classes()
    assert sum(len(v) for v in classes.values()) == 1503 and 80 <= len(classes) <= 200, len(classes)
    mine = sorted(classes)[chunk::N_CHUNKS]
    net, cold, calls = warm_fdn
    state = f"case {chunk} of {N_CHUNKS}, on the net as the cases before it in this run left it"
    with torch.no_grad():
        params = dict(list(net.named_parameters()) + list(net.named_buffers()))
        cparams = dict(list(cold.named_parameters()) + list(cold.named_buffers()))
        dead = []
        for c in mine:
            call = calls[c.split(".")[0] if c.startswith("net_") else ""]
            before = call(net)
            for k in classes[c]:
                params[k].copy_(_changed(params[k]))
                cparams[k].copy_(params[k])
            got = call(net)
            _fresh_caches(cold)
            assert torch.equal(got, call(cold)), f"FDN: stale operands after an update of {c} ({state})"
            assert torch.isfinite(got).all(), (c, state)
            if torch.equal(got, before):
                dead.append(c)
        assert sorted(dead) == sorted(c for c in mine if _is_dead(c)), f"the dead-parameter list is wrong ({state})"
        _fresh_caches(cold)
        want = calls[""](copy.deepcopy(net))
        assert torch.equal(calls[""](cold), want), f"the kept cold tree is not what a deep copy of the net gives ({state})"
        assert torch.equal(calls[""](net), want), state


def test_deep_copy_of_a_warm_net(A):
    """copy.deepcopy of a net that has run (full caches, a GraphedForward on it): the same bits, its own results after the original's
    weights change, no graph holder shared"""
    from fdn_hip import pipeline
    with torch.no_grad():
        net, lp = _build("fdn", "A"), _build("lpnet", "A")
        x = _x(SHAPES[0])
        for _ in range(3):
            first = pipeline.run(net, lp, x).clone()
        assert net.__dict__.get("_fdn_graphed") is not None
        c = copy.deepcopy(net)
        assert c.__dict__.get("_fdn_graphed") is None
        caches = [v for mod in c.modules() for v in mod.__dict__.values() if hasattr(v, "versions")]
        assert len(caches) > 100 and all(v.versions() == () for v in caches)
        assert torch.equal(pipeline.run(c, lp, x), first)
        assert c.__dict__["_fdn_graphed"] is not net.__dict__["_fdn_graphed"] and c.__dict__["_fdn_graphed"].net is c
        for p in list(net.net_p.encoder_level1.parameters()) + list(net.net_p.up3_2.parameters()) + list(net.net_a.net.AFFs.parameters()):
            p.copy_(_changed(p))
        changed = pipeline.run(net, lp, x).clone()
        assert not torch.equal(changed, first)
        for _ in range(3):
            assert torch.equal(pipeline.run(c, lp, x), first)
        assert torch.equal(pipeline.run(net, lp, x), changed)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fixes that belong with it
# ---------------------------------------------------------------------------------------------------------------------------------
def test_writes_through_data_and_forget_derived_block(A):
    """The documented limit of WeightCache on the eager path: after writes through .data the warm result EQUALS the old result
    (asserted, so that a change of behaviour is noticed); ops.forget_derived is the way out.  TransformerBlock(32) on its default route,
    where the tensors written here reach the kernels through cache entries only: the outer norm1 gamma through FDSA's "pk" pack, the outer
    norm2 gamma, ffn.project_in, attn.project_out and the attn norms through the "tlp" tail image that also runs the FDFFN's project_in."""
    from fdn_hip import ops
    with torch.no_grad():
        m, call = SPECS["tblock32_light"]()
        old = call(m)
        for name in ("norm1.body.weight", "norm2.body.weight", "attn.project_out.weight", "ffn.project_in.weight", "attn.norm2.body.bias"):
            own, leaf = _owner(m, name)
            getattr(own, leaf).data.mul_(1.5)
        m.attn.to_hidden.weight.data.copy_(m.attn.to_hidden.weight.data * 0.5)
        want = call(_cold(m))
        assert not torch.equal(want, old)
        assert torch.equal(call(m), old), "a write through .data is now seen: update WeightCache's docstring and INTEGRATION.md"
        ops.forget_derived(m)
        assert torch.equal(call(m), want)


def test_writes_through_data_and_forget_derived_fdn(A):
    """The same on FDN through pipeline.run and the holders: after a write through .data the captured graphs replay the old result
    exactly; after ops.forget_derived every path gives the cold copy's bits."""
    from fdn_hip import ops, pipeline
    with torch.no_grad():
        net, lp = _build("fdn", "A"), _build("lpnet", "A")
        x = _x(SHAPES[0])
        gf, gs = pipeline.GraphedForward(net, lp), pipeline.GraphedStep(net, lp)
        for _ in range(3):
            old = pipeline.run(net, lp, x).clone()
            assert torch.equal(gf(x), old) and torch.equal(gs(x), old)
        for blk in net.net_p.encoder_level1:
            blk.attn.project_out.weight.data.mul_(1.5)
            blk.norm1.body.weight.data.mul_(1.1)
        net.net_p.up3_2.body[1].weight.data.mul_(1.5)
        lp.conv1[1].running_var.data.mul_(2.0)
        want = pipeline.forward_streams(_cold(net), _cold(lp), x, 1)
        assert not torch.equal(want, old)
        assert torch.equal(pipeline.run(net, lp, x), old) and torch.equal(gf(x), old) and torch.equal(gs(x), old)      # the documented limit
        captures = gs.captures
        ops.forget_derived(net, lp)
        assert net.__dict__.get("_fdn_graphed") is None
        for _ in range(3):
            assert torch.equal(pipeline.run(net, lp, x), want) and torch.equal(gf(x), want) and torch.equal(gs(x), want)
        assert gs.captures == captures + 1
        assert torch.equal(pipeline.forward_streams(net, lp, x, 1), want)


@pytest.mark.parametrize("what", ["fdsa32", "fdn"])
def test_pickle_of_a_warm_model(A, what, tmp_path):
    """pickle.dumps / torch.save of a model that has run: the caches' HIP events and the graph holder stay behind, the loaded module gives the original's bits"""
    from fdn_hip import pipeline
    with torch.no_grad():
        if what == "fdn":
            m, lp = _build("fdn", "A"), _build("lpnet", "A")
            x = _x(SHAPES[0])
            call = lambda mod: pipeline.run(mod, lp, x)
            for _ in range(3):
                first = call(m).clone()
        else:
            m, call = SPECS[what]()
            first = call(m)
        blob = pickle.dumps(m)
        c = pickle.loads(blob).to(DEV)
        assert all(v.versions() == () for mod in c.modules() for v in mod.__dict__.values() if hasattr(v, "versions"))
        assert torch.equal(call(c), first)
        torch.save(m, tmp_path / "m.pt")
        c2 = torch.load(tmp_path / "m.pt", weights_only=False).to(DEV)
        assert torch.equal(call(c2), first)
        assert torch.equal(call(m), first)


def test_lpips_model_follows_a_rewritten_weights_file(A, tmp_path, monkeypatch):
    """metrics.lpips_model keeps one model per weights file: a file rewritten in place (another size or modification time) is loaded
    again, an unchanged one is not"""
    import os
    from fdn_hip import lpips, metrics
    built = []
    real = lpips.LPIPS

    class Counting(real):
        def __init__(self, *a, **k):
            built.append(1)
            super().__init__(*a, **k)
    monkeypatch.setattr(lpips, "LPIPS", Counting)
    a = (R.images(1, 48, 64, seed=4).permute(0, 2, 3, 1).numpy() * 255).round().astype(np.uint8)[0]
    b = (R.distorted(R.images(1, 48, 64, seed=4), "distinct").permute(0, 2, 3, 1).numpy() * 255).round().astype(np.uint8)[0]
    _, paths = R.write_weight_files(str(tmp_path), "alex", seed=5)
    s1 = metrics.calculate_lpips(a, b, net="alex", weights=paths["lpips"], device=DEV)
    assert metrics.calculate_lpips(a, b, net="alex", weights=paths["lpips"], device=DEV) == s1
    assert len(built) == 1, "an unchanged file builds the model once"
    st = os.stat(paths["lpips"])
    _, paths2 = R.write_weight_files(str(tmp_path), "alex", seed=6)             # the same paths, other weights of the same size
    assert paths2 == paths and os.stat(paths["lpips"]).st_size == st.st_size
    os.utime(paths["lpips"], ns=(st.st_atime_ns, max(os.stat(paths["lpips"]).st_mtime_ns, st.st_mtime_ns) + 1_000_000))      # (a coarse file clock must not give both writes one stamp)
    s2 = metrics.calculate_lpips(a, b, net="alex", weights=paths["lpips"], device=DEV)
    assert len(built) == 2
    direct = metrics.calculate_lpips(a, b, model=real("alex", weights=paths["lpips"], device=DEV))
    assert s2 == direct and s2 != s1
    assert metrics.calculate_lpips(a, b, net="alex", weights=paths["lpips"], device=DEV) == s2 and len(built) == 2
