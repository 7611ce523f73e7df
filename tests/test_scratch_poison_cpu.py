"""CPU: the scratch-poisoning harness (tests/scratch_poison.py) is not blind -- a function that reads what it never wrote gives another
result under every pattern, one that writes everything gives the same bits, integers stay as they are, a poisoned allocation is traced
to its caller, and leaving a region restores torch.  And the GPU-free census of the package's initialisation-free allocation sites
that tests/test_scratch_independence_gpu.py holds its coverage against."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scratch_poison as SPZ  # noqa: E402
from scratch_poison import FINITE, NAN, PATTERNS, ZERO, poison_tensors, poisoned  # noqa: E402

CPU = ("cpu",)


def leaky_sum():
    buf = torch.empty(8)
    buf[:4] = torch.arange(4.0)
    return buf.sum()


def leaky_max():
    buf = torch.empty(8)
    buf[:4] = torch.arange(4.0)
    m = torch.tensor(-1.0)
    for v in buf:                                  # a NaN-ignoring maximum, as a kernel's `v > m ? v : m` is
        m = v if v > m else m
    return m


def tight_sum():
    buf = torch.empty(8)
    buf[:4] = torch.arange(4.0)
    buf[4:] = 1.0
    return buf.sum()


def _under(fn, monkeypatch):
    out = {}
    for byte in PATTERNS:
        with poisoned(monkeypatch, byte, devices=CPU):
            out[byte] = fn()
    return out


def _same(a, b):
    return torch.equal(a, b) or bool(torch.isnan(a).all() and torch.isnan(b).all())


def test_patterns_are_what_the_docstring_says():
    assert PATTERNS == (ZERO, FINITE, NAN) == (0x00, 0x7B, 0xFF)                  # 0x7B runs before 0xFF
    for dtype in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
        one = lambda byte: torch.full((dtype.itemsize,), byte, dtype=torch.uint8).view(dtype)
        assert torch.isnan(one(NAN)).all() and torch.isfinite(one(FINITE)).all() and float(one(ZERO)) == 0.0
    assert 1.2e36 < float(torch.full((4,), FINITE, dtype=torch.uint8).view(torch.float32)) < 1.4e36
    assert 1.2e36 < float(torch.full((2,), FINITE, dtype=torch.uint8).view(torch.bfloat16)) < 1.4e36
    if hasattr(torch, "float8_e4m3fn"):
        assert float(torch.full((1,), FINITE, dtype=torch.uint8).view(torch.float8_e4m3fn).float()) == 352.0
        assert torch.isnan(torch.full((1,), NAN, dtype=torch.uint8).view(torch.float8_e4m3fn).float()).all()
    assert 2.0 ** (FINITE - 127) == 2.0 ** -4                                      # E8M0: 2^(byte - 127); 0xFF is its NaN


def test_a_leaky_sum_differs_under_every_pattern(monkeypatch):
    out = _under(leaky_sum, monkeypatch)
    assert float(out[ZERO]) == 6.0 and torch.isnan(out[NAN]) and torch.isfinite(out[FINITE]) and float(out[FINITE]) > 1e36
    assert not _same(out[ZERO], out[FINITE]) and not _same(out[ZERO], out[NAN]) and not _same(out[FINITE], out[NAN])


def test_a_leaky_maximum_hides_the_nan_and_shows_the_finite_pattern(monkeypatch):
    """Why 0x7B exists: a compare-and-select maximum steps over NaN, so 0xFF equals 0x00; the huge finite value does not."""
    out = _under(leaky_max, monkeypatch)
    assert torch.equal(out[ZERO], out[NAN]) and float(out[ZERO]) == 3.0
    assert not torch.equal(out[ZERO], out[FINITE]) and float(out[FINITE]) > 1e36


def test_a_function_that_writes_everything_is_bit_equal(monkeypatch):
    out = _under(tight_sum, monkeypatch)
    assert torch.equal(out[ZERO], out[FINITE]) and torch.equal(out[ZERO], out[NAN]) and float(out[ZERO]) == 10.0


def test_every_wrapped_form_is_filled_and_integers_are_untouched(monkeypatch):
    like = torch.zeros(3, 5).t()                                                   # dense, not contiguous: empty_like keeps the layout
    with poisoned(monkeypatch, FINITE, devices=CPU) as p:
        made = [torch.empty(2, 3), torch.empty((4,), dtype=torch.bfloat16), torch.empty_like(like), torch.empty_strided((2, 3), (1, 2)),
                torch.zeros(1).new_empty(5), torch.zeros(1).new_empty_strided((2, 2), (2, 1)), torch.empty(6, dtype=torch.uint8),
                torch.empty(6, dtype=torch.int8), torch.empty(3, dtype=torch.float64), torch.empty(3, dtype=torch.float16)]
        if hasattr(torch, "empty_permuted"):
            made.append(torch.empty_permuted((2, 3), (1, 0)))
        host = np.empty((2, 3), dtype=np.float32)
        ints = [torch.full((4,), 7, dtype=dt) for dt in (torch.int32, torch.int64, torch.int16)]
        kept = [torch.empty(4, dtype=dt) for dt in (torch.int32, torch.int64, torch.int16, torch.bool)]
        elsewhere = torch.empty(3, device="meta")
    for t in made:
        raw = t.contiguous().view(torch.uint8)
        assert bool((raw == FINITE).all()), (t.dtype, t.stride())
    assert (host.view(np.uint8) == FINITE).all()
    assert p.allocations == len(made) + 1 and p.untouched == len(kept) + 1 and elsewhere.device.type == "meta"
    assert p.bytes == sum(t.numel() * t.element_size() for t in made) + host.nbytes
    # integer and bool tensors: poison_tensors leaves them as well, and fills the rest where it finds it
    class Holder:
        def __init__(self):
            self.w = torch.ones(3)
            self.index = ints[0]
            self.back = {"not": "entered", "t": torch.ones(2)}                     # an object's non-tensor attributes are not entered
    h = Holder()
    tree = {"a": torch.ones(4), "b": [torch.ones(2, dtype=torch.bfloat16), (ints[1], torch.ones(3, dtype=torch.uint8))], "o": h, "i": ints[2]}
    n, size = poison_tensors(tree, NAN)
    assert n == 4 and size == 16 + 4 + 3 + 12
    assert torch.isnan(tree["a"]).all() and torch.isnan(tree["b"][0].float()).all() and bool((tree["b"][1][1] == 0xFF).all()) and torch.isnan(h.w).all()
    assert all(bool((t == 7).all()) for t in ints) and bool((h.back["t"] == 1).all())


def test_the_record_names_the_file_and_function_of_the_call(monkeypatch):
    with poisoned(monkeypatch, ZERO, devices=CPU) as p:
        leaky_sum()
        [torch.empty(1) for _ in range(2)]                                         # a comprehension is not a function of its own
    assert p.calls == [("test_scratch_poison_cpu.py", "leaky_sum")] + [("test_scratch_poison_cpu.py", "test_the_record_names_the_file_and_function_of_the_call")] * 2
    assert p.sites == set() and p.files == set()                                   # (sites: flexam_amd's alone)
    # a frame of the package is preferred to the test's, and named with its class where it has one (a GPU-free allocation of flexam_amd)
    from flexam_amd.wan_text_encoder import _linear
    with poisoned(monkeypatch, FINITE, devices=CPU) as p:
        w = _linear(4, 3).weight
    assert p.calls == [("wan_text_encoder.py", "_linear")] and p.sites == {("wan_text_encoder.py", "_linear")} and p.files == {"wan_text_encoder.py"}
    assert p.sites <= SPZ.census() and bool((w.detach().view(torch.uint8) == FINITE).all())
    assert SPZ._index(os.path.join(SPZ.PACKAGE_DIR, "dit_sp.py"))[[k for k in SPZ._index(os.path.join(SPZ.PACKAGE_DIR, "dit_sp.py")) if k[1] == "_layout"][0]] == "KVHalo._layout"


def test_nesting_and_exit_restore_the_originals(monkeypatch):
    originals = {n: getattr(torch, n) for n in SPZ.TORCH_FUNCTIONS if hasattr(torch, n)}
    methods = {n: getattr(torch.Tensor, n) for n in SPZ.TENSOR_METHODS}
    np_empty = np.empty
    with poisoned(monkeypatch, ZERO, devices=CPU) as outer:
        assert torch.empty is not originals["empty"]
        with poisoned(monkeypatch, NAN, devices=CPU) as inner:
            assert torch.isnan(torch.empty(3)).all()                               # the inner region fills last
        assert inner.allocations == 1 and outer.allocations == 1
        assert bool((torch.empty(3) == 0).all()) and outer.allocations == 2 and inner.allocations == 1
        with pytest.raises(ZeroDivisionError):
            with poisoned(monkeypatch, FINITE, devices=CPU):
                1 / 0
        assert bool((torch.empty(3) == 0).all())                                   # an exception restores the enclosing region
    for n, f in originals.items():
        assert getattr(torch, n) is f
    for n, f in methods.items():
        assert getattr(torch.Tensor, n) is f
    assert np.empty is np_empty


# ----------------------------------------------------------------------------- the census
COVERED_MODULES = ("dit_engine.py", "dit_sp.py", "wan_vae3_8.py", "wan_text_encoder.py", "hip.py", "frames.py", "edit_masks.py", "implicit_conv.py")


def test_census_of_initialisation_free_allocations():
    """Every (file, function) of flexam_amd that allocates without initialising, by an ast walk: the modules the issue counted are there
    with about the counted number of calls, known sites are found under the names a stack frame carries, and numpy's host arrays and
    initialising calls are not listed."""
    sites = SPZ.census()
    files = {f for f, _ in sites}
    assert {"hip.py", "dit_engine.py", "wan_vae3_8.py", "dist.py", "dit_sp.py", "wan_text_encoder.py", "frames.py"} <= files
    for known in (("dit_engine.py", "DiTEngine._workspace"), ("dit_engine.py", "DiTEngine._k_mean_buffers"), ("dit_engine.py", "DiTEngine.run"),
                  ("dit_sp.py", "KVGather.__init__"), ("dit_sp.py", "KVHalo._layout"), ("hip.py", "_gemm_workspace.<lambda>"), ("hip.py", "gemm"),
                  ("hip.py", "k_mean"), ("wan_text_encoder.py", "_linear"), ("wan_vae3_8.py", "_ConvUp2x.run")):
        assert known in sites, known
    assert "conditioning_raster.py" not in files and not any(f == "<module>" for _, f in sites)        # (its one numpy.empty is a host array)
    assert 60 <= len(sites) <= 140, len(sites)
    print(f"{len(sites)} allocating functions in {len(files)} files; in the covered modules: {sum(f in COVERED_MODULES for f, _ in sites)}")
