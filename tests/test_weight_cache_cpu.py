"""CPU: which weight changes ops.WeightCache and pipeline.weights_signature notice (plain CPU tensors, no library call).

The mirror modules keep every derived operand (LayerNorm folds, packed MFMA images, BatchNorm folds, ...) in a WeightCache keyed on the
sources' (pointer, version, device), and the graph holders key their captures on weights_signature.  A change that neither notices is a
model that keeps computing with the old weights.  The documented blind spot is a write THROUGH `.data`; ops.forget_derived is the way out."""
import copy
import gc
import pickle
import weakref

import pytest
import torch
import torch.nn as nn

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
from fdn_hip import ops, pipeline


class Holder(nn.Module):
    """A module with a cache on it, as the mirror modules have (module level: pickle needs to find the class)."""

    def __init__(self, bias=True):
        super().__init__()
        self.lin = nn.Linear(4, 3, bias=bias)
        self.conv = nn.Conv2d(3, 3, 1)
        self._c = ops.WeightCache()
        self.builds = 0

    def derived(self):
        """2 w + mean(bias), the stand-in for a fold: reads both sources"""
        def build():
            self.builds += 1
            w = self.lin.weight.detach() * 2
            return w if self.lin.bias is None else w + self.lin.bias.detach().mean()
        return self._c.get("d", [self.lin.weight, self.lin.bias], build)

    def fresh(self):
        w = self.lin.weight.detach() * 2
        return w if self.lin.bias is None else w + self.lin.bias.detach().mean()


def _other_state(m, seed=11):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(v.shape, generator=g) for k, v in m.state_dict().items()}


def _mul(m):
    with torch.no_grad():
        m.lin.weight.mul_(1.5)


def _mul_bias(m):
    with torch.no_grad():
        m.lin.bias.mul_(1.5)


def _detach_copy(m):
    m.lin.weight.detach().copy_(torch.full((3, 4), 0.25))


def _load(m):
    m.load_state_dict(_other_state(m))


def _load_assign(m):
    m.load_state_dict(_other_state(m), assign=True)


def _replace(m):
    m.lin.weight = nn.Parameter(m.lin.weight.detach().clone() + 1.0)


def _replace_bias(m):
    m.lin.bias = nn.Parameter(m.lin.bias.detach().clone() + 1.0)


def _set_data(m):
    m.lin.weight.data = torch.full((3, 4), -0.5)


UPDATES = {"no_grad mul_": _mul, "no_grad mul_ of the second source": _mul_bias, "detach().copy_": _detach_copy, "load_state_dict": _load,
           "load_state_dict(assign=True)": _load_assign, "replaced Parameter": _replace, "replaced second Parameter": _replace_bias,
           "p.data = new": _set_data}


@pytest.mark.parametrize("how", sorted(UPDATES))
def test_get_rebuilds_after(how):
    torch.manual_seed(0)
    m = Holder()
    first = m.derived().clone()
    assert m.builds == 1
    assert m.derived() is m.derived() and m.builds == 1          # nothing changed: the entry is served, build is not called
    sig = pipeline.weights_signature(m)
    assert pipeline.weights_signature(m) == sig
    UPDATES[how](m)
    got = m.derived()
    assert m.builds == 2, how
    assert torch.equal(got, m.fresh()) and not torch.equal(got, first), how
    assert pipeline.weights_signature(m) != sig, how              # the graph holders capture again too
    m.derived()
    assert m.builds == 2


def test_get_follows_a_source_that_appears_or_disappears():
    """a None source (a conv without bias) that becomes a tensor, and the reverse"""
    torch.manual_seed(0)
    m = Holder(bias=False)
    a = m.derived()
    assert m.builds == 1 and torch.equal(a, m.lin.weight.detach() * 2)
    m.lin.bias = nn.Parameter(torch.full((3,), 0.5))
    b = m.derived()
    assert m.builds == 2 and torch.equal(b, m.fresh()) and not torch.equal(a, b)
    m.derived()
    assert m.builds == 2
    m.lin.bias = None
    c = m.derived()
    assert m.builds == 3 and torch.equal(c, a)


def test_chained_entries_follow_the_first_source():
    """Entry B is built from entry A's output and keyed on it, as "up:taps" -> "up:z:pk" is; entry C is keyed on A's SOURCE and reads A's
    output, as FDSA's "g" / "b" -> "tl" are.  Both follow a change of A's source, each built once per change."""
    c = ops.WeightCache()
    w = nn.Parameter(torch.arange(6.0).reshape(2, 3))
    n = {"a": 0, "b": 0, "c": 0}

    def count(k, fn):
        def build():
            n[k] += 1
            return fn()
        return build

    def run():
        a = c.get("a", [w], count("a", lambda: w.detach().t().contiguous()))
        b = c.get("b", [a, None], count("b", lambda: a * 10))
        cc = c.get("c", [w], count("c", lambda: a.sum(1)))
        return a, b, cc

    a0, b0, c0 = run()
    run()
    assert n == {"a": 1, "b": 1, "c": 1}
    for i, update in enumerate((lambda: w.detach().mul_(2.0), lambda: w.detach().copy_(torch.ones(2, 3)))):
        update()
        a, b, cc = run()
        assert n == {"a": 2 + i, "b": 2 + i, "c": 2 + i}
        assert torch.equal(a, w.detach().t()) and torch.equal(b, w.detach().t() * 10) and torch.equal(cc, w.detach().t().sum(1))
    assert not torch.equal(b, b0) and not torch.equal(cc, c0)
    assert len(c.versions()) == 3


def test_an_entry_keeps_its_sources_alive():
    """The key is (pointer, version, device).  An entry holds references to its sources, so their storage cannot be freed and handed to a
    NEW tensor at the same address with the same version: shown through the references kept, not through an address coincidence."""
    c = ops.WeightCache()
    builds = []
    t = torch.randn(64)
    alive = weakref.ref(t)
    c.get("e", [t], lambda: builds.append(1) or t * 2)
    del t
    gc.collect()
    assert alive() is not None, "the entry let go of its source: a new tensor could take its address and version"
    old_ptr = alive().data_ptr()
    new = torch.randn(64)                      # same size, same (zero) version
    assert new.data_ptr() != old_ptr           # follows from the above: the old storage is still allocated
    got = c.get("e", [new], lambda: builds.append(1) or new * 2)
    assert len(builds) == 2 and torch.equal(got, new * 2)
    gc.collect()
    assert alive() is None                     # the replaced entry let the old source go
    # a replaced Parameter on a module: the old one lives exactly as long as the entry built from it
    m = Holder()
    m.derived()
    old = weakref.ref(m.lin.weight)
    m.lin.weight = nn.Parameter(torch.zeros(3, 4))
    gc.collect()
    assert old() is not None
    m.derived()
    gc.collect()
    assert old() is None and m.builds == 2


@pytest.mark.parametrize("how", ["pickle", "pickle protocol 1", "deepcopy", "copy"])
def test_a_copy_starts_with_an_empty_cache(how):
    torch.manual_seed(0)
    m = Holder()
    d = m.derived()
    assert len(m._c.versions()) == 1
    if how.startswith("pickle"):
        c = pickle.loads(pickle.dumps(m, protocol=1 if how.endswith("1") else pickle.DEFAULT_PROTOCOL))
    elif how == "copy":                         # a shallow copy of the CACHE: it must not share the entries either
        c = copy.deepcopy(m)
        c._c = copy.copy(m._c)
    else:
        c = copy.deepcopy(m)
    assert isinstance(c._c, ops.WeightCache) and c._c is not m._c
    assert c._c.versions() == (), "derived tensors (and their events) travelled with the copy"
    c.builds = 0
    dc = c.derived()
    assert c.builds == 1 and torch.equal(dc, d) and dc.data_ptr() != d.data_ptr()
    with torch.no_grad():
        m.lin.weight.add_(1.0)                  # the original's update does not reach the copy, and the reverse
    assert torch.equal(c.derived(), dc) and c.builds == 1 and not torch.equal(m.derived(), dc)
    assert len(m._c.versions()) == 1


def test_writes_through_data_need_forget_derived():
    """The documented limit: `p.data.mul_()` / `p.data.copy_()` change the values and neither the version nor the pointer, so the cache
    serves the old derived tensor and the graph key stands still (asserted, so that a change of this behaviour is noticed).
    ops.forget_derived empties the caches of the trees it is given, drops the GraphedForward pipeline.run keeps on a model and moves
    the key of every graph holder."""
    torch.manual_seed(0)
    m = nn.Sequential(Holder(), nn.Sequential(Holder()))
    h0, h1 = m[0], m[1][0]
    old0, old1 = h0.derived().clone(), h1.derived().clone()
    sig = pipeline.weights_signature(m)
    other = nn.Linear(2, 2)
    sig_other = pipeline.weights_signature(other)
    m.__dict__["_fdn_graphed"] = object()
    h0.lin.weight.data.mul_(3.0)
    h1.lin.weight.data.copy_(torch.ones(3, 4))
    assert torch.equal(h0.derived(), old0) and torch.equal(h1.derived(), old1) and (h0.builds, h1.builds) == (1, 1)
    assert pipeline.weights_signature(m) == sig
    ops.forget_derived(m)
    assert h0._c.versions() == () and h1._c.versions() == ()
    assert "_fdn_graphed" not in m.__dict__
    assert pipeline.weights_signature(m) != sig
    assert pipeline.weights_signature(other) != sig_other        # the counter is process-wide: every holder captures again
    assert torch.equal(h0.derived(), h0.fresh()) and torch.equal(h1.derived(), h1.fresh()) and (h0.builds, h1.builds) == (2, 2)
    assert not torch.equal(h0.derived(), old0) and not torch.equal(h1.derived(), old1)
    sig2 = pipeline.weights_signature(m)
    assert pipeline.weights_signature(m) == sig2
    ops.forget_derived(h0, h1)                                    # several trees in one call
    assert pipeline.weights_signature(m) != sig2 and h0._c.versions() == ()


def test_signature_sees_swapped_storages():
    """A captured graph holds raw pointers: two equal-shaped parameters that swap storages, or one pointer moving by +d while another
    moves by -d, change what every kernel reads and leave any SUM over the tree unchanged."""
    torch.manual_seed(0)
    m = Holder()
    a, b = m.lin.weight, nn.Parameter(torch.randn(3, 4))
    m.second = b
    sig = pipeline.weights_signature(m)
    assert pipeline.weights_signature(m) == sig
    va, vb, pa, pb = a._version, b._version, a.data_ptr(), b.data_ptr()
    a.data, b.data = b.data, a.data
    assert (a.data_ptr(), b.data_ptr()) == (pb, pa) and a._version + b._version == va + vb      # the sums stand still
    assert pipeline.weights_signature(m) != sig
    a.data, b.data = b.data, a.data
    assert pipeline.weights_signature(m) == sig                   # swapped back: the same pointers and versions again
    # +d / -d: views into one buffer
    buf = torch.arange(48.0)
    a.data, b.data = buf[0:12].view(3, 4), buf[24:36].view(3, 4)
    sig = pipeline.weights_signature(m)
    s = a.data_ptr() + b.data_ptr()
    a.data, b.data = buf[12:24].view(3, 4), buf[12:24].view(3, 4)
    assert a.data_ptr() + b.data_ptr() == s
    assert pipeline.weights_signature(m) != sig
