"""CPU: the switch that poisons uninitialised memory in the GPU tests (tests/common.py poisoned(), poison_uninitialized, POISON_EXEMPT),
and the rules that keep every tests/test_gpu_*.py under it: each module installs the fixture, a test leaves it only through a
`with poisoned_off():` of its own and a POISON_EXEMPT entry, no module is exempt as a whole, and the one buffer a kernel waits on
(the slot flags of fdn_fdsa_fused_tail's scratch ring: csrc/patchfft.hip spins until a flag reads 0) comes from torch.zeros."""
import ast
import glob
import inspect
import os

import pytest
import torch

import common
from common import POISON_EXEMPT, poisoned, poisoned_off
from common import poison_uninitialized  # noqa: F401  (installed here the way the GPU modules install it: test_the_import_installs_the_fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
FLOATS = (torch.float32, torch.float64, torch.bfloat16)
INTS = (torch.uint8, torch.int16, torch.int64)
GPU_MODULES = sorted(glob.glob(os.path.join(HERE, "test_gpu_*.py")))


def _state():
    return (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
            torch.utils.deterministic.fill_uninitialized_memory)


def _allocations(dtype):
    base = torch.zeros(3, 5, dtype=dtype)
    return {"empty": torch.empty(37, 5, dtype=dtype), "empty_like": torch.empty_like(base), "new_empty": base.new_empty((7, 3)),
            "empty_strided": torch.empty_strided((3, 5), (5, 1), dtype=dtype)}


@pytest.mark.parametrize("dtype", FLOATS + INTS, ids=lambda d: str(d).split(".")[-1])
def test_fill_on_the_cpu(dtype):
    before = _state()
    with poisoned():
        assert _state() == (True, True, True)
        for how, t in _allocations(dtype).items():
            if dtype in FLOATS:
                assert bool(torch.isnan(t).all()), (how, dtype)
            else:
                assert bool((t == torch.iinfo(dtype).max).all()), (how, dtype)
        assert bool((torch.zeros(37, 5, dtype=dtype) == 0).all())
    assert _state() == before


@pytest.mark.parametrize("start", [(False, False, True), (True, False, False), (True, True, True), (False, True, False)])
def test_all_three_settings_are_restored(start):
    """after a normal exit, after an exception and after nesting, from any state: (mode, warn_only, fill flag)"""
    saved = _state()
    try:
        torch.use_deterministic_algorithms(start[0], warn_only=start[1])
        torch.utils.deterministic.fill_uninitialized_memory = start[2]
        assert _state() == start
        with poisoned():
            assert _state() == (True, True, True)
        assert _state() == start
        with pytest.raises(KeyError):
            with poisoned():
                raise KeyError("inside")
        assert _state() == start
        with poisoned():
            with poisoned_off():
                assert _state() == (False, False, False)
                with poisoned():
                    assert _state() == (True, True, True)
                assert _state() == (False, False, False)
            assert _state() == (True, True, True)
            with pytest.raises(KeyError):
                with poisoned():
                    raise KeyError("nested")
            assert _state() == (True, True, True)
        assert _state() == start
    finally:
        torch.use_deterministic_algorithms(saved[0], warn_only=saved[1])
        torch.utils.deterministic.fill_uninitialized_memory = saved[2]


def test_an_op_without_a_deterministic_form_warns_and_runs():
    """warn_only: reference code and wrappers keep running (torch.kthvalue on a CUDA tensor, scatter_add ... only warn); on the CPU the
    flag is what can be observed"""
    with poisoned():
        assert torch.is_deterministic_algorithms_warn_only_enabled()
        x = torch.arange(6.0)
        assert torch.equal(torch.zeros(3).index_add(0, torch.tensor([0, 1, 1, 2, 2, 2]), x), torch.tensor([0.0, 3.0, 12.0]))


def test_the_import_installs_the_fixture():
    """this module imports poison_uninitialized as every tests/test_gpu_*.py does, and nothing else turns the switch on"""
    assert _state() == (True, True, True)
    assert bool(torch.isnan(torch.empty(5)).all())


def test_the_fixture_is_module_scoped_and_autouse():
    mark = getattr(common.poison_uninitialized, "_fixture_function_marker", None) or common.poison_uninitialized._pytestfixturefunction
    assert mark.scope == "module" and mark.autouse


# ---------------------------------------------------------------------------------------------------------------------------------
# every GPU module is under the fixture
# ---------------------------------------------------------------------------------------------------------------------------------
def _tree(path):
    with open(path) as f:
        return ast.parse(f.read(), path)


def _installs_fixture(tree):
    for node in tree.body:                                       # module level only: an import inside a function installs nothing
        if isinstance(node, ast.ImportFrom) and node.module == "common":
            if any(a.name == "poison_uninitialized" and a.asname in (None, "poison_uninitialized") for a in node.names):
                return True
    return False


def _uses_poisoned_off(fn):
    return any(isinstance(n, ast.Name) and n.id == "poisoned_off" or isinstance(n, ast.Attribute) and n.attr == "poisoned_off"
               for n in ast.walk(fn))


def test_every_gpu_module_installs_the_fixture():
    assert len(GPU_MODULES) >= 31
    missing = [os.path.basename(p) for p in GPU_MODULES if not _installs_fixture(_tree(p))]
    assert not missing, f"GPU test modules that do not import common.poison_uninitialized: {missing}"


def test_no_gpu_module_rebinds_the_fixture_or_the_switch():
    """a module-level `poison_uninitialized = ...` / `def poison_uninitialized` (or of poisoned / poisoned_off) would replace what was imported"""
    names = {"poison_uninitialized", "poisoned", "poisoned_off"}
    for p in GPU_MODULES:
        for node in ast.walk(_tree(p)):
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                assert node.name not in names, (os.path.basename(p), node.name)
            elif isinstance(node, ast.Name) and isinstance(node.ctx, (ast.Store, ast.Del)):
                assert node.id not in names, (os.path.basename(p), node.id)
        src = open(p).read()
        for attr in ("use_deterministic_algorithms", "fill_uninitialized_memory"):          # the switch is thrown in tests/common.py only
            assert attr not in src or os.path.basename(p) == "test_gpu_poison.py", (os.path.basename(p), attr)


def test_exemptions_name_tests_and_are_the_only_way_out():
    print(f"POISON_EXEMPT ({len(POISON_EXEMPT)}):")
    for tid, reason in POISON_EXEMPT.items():
        print(f"  {tid}: {reason}")
    tests = {}                                                   # "<module>::<function>" -> FunctionDef
    for p in GPU_MODULES:
        mod = os.path.splitext(os.path.basename(p))[0]
        tree = _tree(p)
        for node in tree.body:
            if isinstance(node, ast.FunctionDef):
                tests[f"{mod}::{node.name}"] = node
                continue
            # poisoned_off outside a function (module level, a class body, a fixture's decorator) would exempt more than one test
            assert not _uses_poisoned_off(node) or (isinstance(node, ast.ImportFrom) and node.module == "common"), \
                f"{mod}: poisoned_off is used outside a test function (line {node.lineno})"
    for tid, reason in POISON_EXEMPT.items():
        assert "::" in tid and tid.split("::")[1].startswith("test_"), f"{tid}: an exemption names one test function, never a module"
        assert tid in tests, f"{tid}: no such test function"
        assert isinstance(reason, str) and len(reason) > 20, f"{tid}: an exemption states its reason"
        assert _uses_poisoned_off(tests[tid]), f"{tid} is listed but never leaves the fixture: drop the entry"
    for tid, fn in tests.items():
        if _uses_poisoned_off(fn):
            assert tid in POISON_EXEMPT and tid.split("::")[1].startswith("test_"), \
                f"{tid} leaves the fixture without a POISON_EXEMPT entry (helpers and fixtures may not leave it at all)"
    per_module = {}
    for tid in POISON_EXEMPT:
        per_module.setdefault(tid.split("::")[0], []).append(tid)
    for mod, ids in per_module.items():
        n_tests = sum(1 for t in tests if t.startswith(mod + "::test_"))
        assert len(ids) < n_tests, f"{mod}: every test is exempt - the module is exempt as a whole"


# ---------------------------------------------------------------------------------------------------------------------------------
# the buffer a kernel waits on
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_scratch_ring_comes_from_torch_zeros():
    """fdsa_fused_kernel's thread 0 spins until a slot flag at the head of the ring reads 0: a poisoned ring would never let it go.  The
    ring's only allocation is the torch.zeros of ops.fdsa_fused_tail, and no test allocates one."""
    from fdn_hip import ops
    src = inspect.getsource(ops.fdsa_fused_tail)
    fn = ast.parse(src).body[0]
    allocs = [n for n in ast.walk(fn) if isinstance(n, ast.Assign) and any(
        isinstance(t, ast.Subscript) and isinstance(t.value, ast.Name) and t.value.id == "_fdsa_scratch" for t in n.targets)]
    assert len(allocs) == 1, "one place fills _fdsa_scratch"
    call = allocs[0].value
    assert isinstance(call, ast.Call) and isinstance(call.func, ast.Attribute) and call.func.attr == "zeros" and call.func.value.id == "torch", \
        ast.unparse(allocs[0])
    passed = [n for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "_flat"
              and len(n.args) > 1 and isinstance(n.args[1], ast.Constant) and n.args[1].value == "scratch"]
    assert len(passed) == 1 and passed[0].args[0].id == "scr", "the ring handed to the library is that tensor"
    whole = open(inspect.getsourcefile(ops)).read()
    assert whole.count("_fdsa_scratch[") == 1 and whole.count("fdn_fdsa_fused_tail(") == 1, "a second writer or a second caller of the ring"
    for p in glob.glob(os.path.join(HERE, "*.py")):
        if os.path.basename(p) not in ("test_poison_cpu.py", "test_host_cpu.py"):      # (test_host_cpu.py passes null pointers: an argument check)
            assert "fdn_fdsa_fused_tail(" not in open(p).read(), f"{os.path.basename(p)} calls the C entry point with a ring of its own"
