"""TEST INFRASTRUCTURE ONLY -- poison what the allocator hands out uninitialised, so that a test can show that a result does not depend on
it (a helper module: no tests and no fixtures here; tests/test_scratch_poison_cpu.py shows that it is not blind, and
tests/test_scratch_independence_gpu.py uses it on the engines and wrappers).

`poisoned(monkeypatch, byte, devices=("cuda",))` wraps every initialisation-free allocation the package uses or could use --
torch.empty, torch.empty_like, torch.empty_strided, torch.empty_permuted, Tensor.new_empty, Tensor.new_empty_strided (and numpy.empty
for the host arrays, counted as device "cpu") -- and fills the result byte-wise with `byte` before the caller sees it.  A launch that
reads a byte nobody wrote then computes on `byte`, and two runs under two patterns differ.

THE LIMIT, on purpose: only floating dtypes and uint8 / int8 are filled.  Every other integer dtype and bool come back as the allocator
left them: such tensors are indices, counts and flags here, and a poisoned index could become a wild address on a machine that others
share.  A read of an unwritten int32 / int64 / bool element is therefore NOT found by this harness.

The three patterns (run FINITE before NAN: a finite difference is the easier one to trace):
  ZERO   0x00  0.0 everywhere
  FINITE 0x7B  finite in every format the kernels read: ~1.3e36 in f32 and bf16, 61280 in f16, 352 in e4m3, 2^-4 in E8M0 -- what a
               NaN-ignoring max / min / compare-and-select would hide under 0xFF shows here
  NAN    0xFF  a NaN in f32, bf16, f16, f64, e4m3 and E8M0
"""
import contextlib
import os
import sys

import torch

ZERO, FINITE, NAN = 0x00, 0x7B, 0xFF
PATTERNS = (ZERO, FINITE, NAN)                     # the order the GPU tests keep: 0x7B before 0xFF

TESTS_DIR = os.path.dirname(os.path.abspath(__file__))
PACKAGE_DIR = os.path.join(os.path.dirname(TESTS_DIR), "flexam_amd")
_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__))
_THIS = os.path.abspath(__file__)
_INLINE_SCOPES = ("<listcomp>", "<dictcomp>", "<setcomp>", "<genexpr>")       # not functions of their own in the census either

TORCH_FUNCTIONS = ("empty", "empty_like", "empty_strided", "empty_permuted")
TENSOR_METHODS = ("new_empty", "new_empty_strided")


def fillable(dtype) -> bool:
    """The dtypes this harness fills: floating ones and the byte types (which hold e4m3 / E8M0 data here)."""
    return dtype.is_floating_point or dtype in (torch.uint8, torch.int8)


def fill_bytes(t: torch.Tensor, byte: int) -> int:
    """Every byte of t := byte, in place (t of a fillable dtype).  Returns the bytes written."""
    if t.numel() == 0:
        return 0
    if t.dtype in (torch.uint8, torch.int8):
        t.fill_(byte if t.dtype == torch.uint8 or byte < 128 else byte - 256)
    else:
        try:
            t.view(torch.uint8).fill_(byte)
        except RuntimeError:                         # a dense but permuted layout: the same bit pattern, element by element
            one = torch.full((t.element_size(),), byte, dtype=torch.uint8, device=t.device).view(t.dtype)
            t.copy_(one.expand(1).reshape(()).expand_as(t))
    return t.numel() * t.element_size()


def _site():
    """(file name, function) of the innermost flexam_amd frame under the allocation; without one, of the innermost frame outside torch
    and this module (the test's own function)."""
    f = sys._getframe(2)
    first = None
    while f is not None:
        path = f.f_code.co_filename
        if f.f_code.co_name not in _INLINE_SCOPES and os.path.abspath(path) != _THIS:
            full = os.path.abspath(path)
            if full.startswith(PACKAGE_DIR + os.sep):
                return os.path.basename(full), _index(full).get((f.f_code.co_firstlineno, f.f_code.co_name), f.f_code.co_name), True
            if first is None and not full.startswith(_TORCH_DIR + os.sep):
                first = (os.path.basename(full), f.f_code.co_name, False)
        f = f.f_back
    return first or ("?", "?", False)


class Poison:
    """What one `poisoned` region did: calls = [(file, function)] per poisoned allocation; sites = those inside flexam_amd;
    allocations / bytes = running counts of what was filled; untouched = allocations left alone (other dtypes / devices);
    integer_sites = the flexam_amd sites of allocations on `devices` that were left alone for their dtype (seen, not poisoned)."""

    def __init__(self, byte, devices):
        self.byte, self.devices = int(byte), tuple(devices)
        self.calls, self.sites, self.integer_sites = [], set(), set()
        self.allocations = self.bytes = self.untouched = 0

    @property
    def files(self):
        return {f for f, _ in self.sites}

    def _take(self, t):
        if not isinstance(t, torch.Tensor) or t.device.type not in self.devices or not fillable(t.dtype) or t.is_sparse:
            self.untouched += 1
            if isinstance(t, torch.Tensor) and t.device.type in self.devices:
                name, func, inside = _site()
                if inside:
                    self.integer_sites.add((name, func))
            return t
        n = fill_bytes(t.detach(), self.byte)
        name, func, inside = _site()
        self.calls.append((name, func))
        if inside:
            self.sites.add((name, func))
        self.allocations += 1
        self.bytes += n
        return t

    def _take_numpy(self, a):
        import numpy as np
        if "cpu" not in self.devices or not (np.issubdtype(a.dtype, np.floating) or a.dtype in (np.uint8, np.int8)):
            self.untouched += 1
            return a
        if a.size:
            a.reshape(-1).view(np.uint8).fill(self.byte)
        name, func, inside = _site()
        self.calls.append((name, func))
        if inside:
            self.sites.add((name, func))
        self.allocations += 1
        self.bytes += a.nbytes
        return a


def _wrap(original, take):
    def wrapper(*args, **kwargs):
        return take(original(*args, **kwargs))
    wrapper.__wrapped__ = original
    wrapper.__name__ = getattr(original, "__name__", "empty")
    return wrapper


@contextlib.contextmanager
def poisoned(monkeypatch, byte, devices=("cuda",)):
    """with poisoned(monkeypatch, 0x7B) as p: ...  -- inside, the allocations named above come back filled with `byte` on `devices`
    (integers other than uint8 / int8, and bool, untouched: see the module's docstring).  p is the region's Poison record.  Regions
    nest (the inner one fills last, both record); leaving a region puts back exactly what it replaced."""
    import numpy as np
    record = Poison(byte, devices)
    with monkeypatch.context() as mp:
        for name in TORCH_FUNCTIONS:
            if hasattr(torch, name):
                mp.setattr(torch, name, _wrap(getattr(torch, name), record._take))
        for name in TENSOR_METHODS:
            if hasattr(torch.Tensor, name):
                mp.setattr(torch.Tensor, name, _wrap(getattr(torch.Tensor, name), record._take))
        mp.setattr(np, "empty", _wrap(np.empty, record._take_numpy))
        yield record


def poison_tensors(obj, byte, _seen=None):
    """Fills, in place, every tensor of a fillable dtype found in obj: a tensor, or dicts, lists, tuples and sets of such (nested), or an
    object, of which the attributes that ARE tensors are filled and no other attribute is entered (an exchange object of the workspace
    points back at its engine and the engine at its weights).  Other dtypes untouched, as above.  Used BETWEEN two steps on an engine's
    workspaces: whatever the next step reads there must be what the next step wrote.  Returns (tensors filled, bytes)."""
    seen = set() if _seen is None else _seen
    if id(obj) in seen:
        return 0, 0
    seen.add(id(obj))
    if isinstance(obj, torch.Tensor):
        if fillable(obj.dtype) and not obj.is_sparse:
            return 1, fill_bytes(obj.detach(), byte)
        return 0, 0
    if isinstance(obj, dict):
        children = list(obj.values())
    elif isinstance(obj, (list, tuple, set, frozenset)):
        children = list(obj)
    elif isinstance(obj, (str, bytes, int, float, bool, type(None), torch.nn.Module, type)) or callable(obj):
        return 0, 0
    else:
        held = list(getattr(obj, "__dict__", {}).values()) + [getattr(obj, s) for s in getattr(type(obj), "__slots__", ()) if hasattr(obj, s)]
        children = [c for c in held if isinstance(c, torch.Tensor)]
    count = size = 0
    for c in children:
        n, b = poison_tensors(c, byte, seen)
        count, size = count + n, size + b
    return count, size


# ----------------------------------------------------------------------------- the census: where the package allocates without initialising
CENSUS_NAMES = set(TORCH_FUNCTIONS) | set(TENSOR_METHODS)
_PARSED = {}


def _parse(path):
    """(index, sites) of one source file.  index: {(first line, name): qualified name} of every def and lambda, first line and name as a
    code object carries them (co_firstlineno, co_name), qualified by the enclosing classes and functions ("KVGather.__init__");
    sites: the qualified names of the scopes that call an initialisation-free torch allocation."""
    import ast
    if path not in _PARSED:
        try:
            with open(path) as fh:
                tree = ast.parse(fh.read(), path)
        except (OSError, SyntaxError):
            _PARSED[path] = ({}, set())
            return _PARSED[path]
        index, sites = {}, set()

        def walk(node, scope):
            for child in ast.iter_child_nodes(node):
                inner = scope
                if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)):
                    inner = (scope + "." if scope != "<module>" else "") + child.name
                    index[(min([child.lineno] + [d.lineno for d in child.decorator_list]), child.name)] = inner
                elif isinstance(child, ast.ClassDef):
                    inner = (scope + "." if scope != "<module>" else "") + child.name
                elif isinstance(child, ast.Lambda):
                    inner = (scope + "." if scope != "<module>" else "") + "<lambda>"
                    index[(child.lineno, "<lambda>")] = inner
                if isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute) and child.func.attr in CENSUS_NAMES:
                    base = child.func.value
                    if not (isinstance(base, ast.Name) and base.id in ("np", "numpy")):
                        sites.add(scope)
                walk(child, inner)
        walk(tree, "<module>")
        _PARSED[path] = (index, sites)
    return _PARSED[path]


def _index(path):
    return _parse(path)[0]


def census(package_dir=PACKAGE_DIR):
    """{(file name, qualified function)} of every call of an initialisation-free torch allocation in flexam_amd/*.py, found by an `ast`
    walk (GPU-free).  The function is the innermost enclosing def or lambda, named as a Poison record names the frame it finds, so the
    sites of a run can be compared with it."""
    import glob
    return {(os.path.basename(path), scope) for path in sorted(glob.glob(os.path.join(package_dir, "*.py"))) for scope in _parse(path)[1]}
