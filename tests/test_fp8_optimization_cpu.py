"""CPU: the reference's qfloat8 helpers (FlexAM/utils/fp8_optimization.py) under flexam_amd's names -- which parameters
`convert_model_weight_to_float8` rounds to e4m3 (the reference's rule: every parameter whose name does not contain an excluded
keyword; nodes.py:327-343 excludes "modulation"), how it rounds them, and that `convert_weight_dtype_wrapper` records the compute
dtype without wrapping any forward.  Where the reference is mounted (oracle.ref_import.REF_ROOT), the selection is also compared
with the reference's own function run on this package's module tree."""
import importlib.util
import os

import pytest
import torch

from oracle import dit as O

F8 = torch.float8_e4m3fn


def tiny_model():
    from flexam_amd import Wan2_2Transformer3DModel_FlexAM
    kw = dict(O.DIT_TINY)
    kw.pop("eps")
    torch.manual_seed(0)
    m = Wan2_2Transformer3DModel_FlexAM(**kw)
    m.randomize_zero_init()
    return m.to(torch.bfloat16)


def test_selection_and_rounding_follow_the_reference_rule():
    from flexam_amd import convert_model_weight_to_float8
    m = tiny_model()
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    params = dict(m.named_parameters())
    convert_model_weight_to_float8(m, exclude_module_name=["modulation"], device="cpu")
    after = dict(m.named_parameters())
    assert list(after) == list(before)
    assert all(after[k] is params[k] for k in after)              # the same Parameter objects, new data
    n_f8 = 0
    for k, v in after.items():
        if "modulation" in k:
            assert v.dtype == torch.bfloat16 and torch.equal(v, before[k]), k
        else:
            assert v.dtype == F8, k
            assert torch.equal(v.view(torch.uint8), before[k].to(F8).view(torch.uint8)), k
            n_f8 += 1
    assert n_f8 > 0 and any("modulation" in k for k in after)
    assert set(m.state_dict()) == set(before)                      # the reference's keys
    # a second conversion changes nothing
    snap = {k: v.detach().clone() for k, v in m.named_parameters()}
    convert_model_weight_to_float8(m, exclude_module_name=["modulation"])
    assert all(torch.equal(v.view(torch.uint8) if v.dtype == F8 else v, snap[k].view(torch.uint8) if snap[k].dtype == F8 else snap[k])
               for k, v in m.named_parameters())


def test_wrapper_records_bf16_and_leaves_forward_alone():
    from flexam_amd import convert_model_weight_to_float8, convert_weight_dtype_wrapper
    m = tiny_model()
    convert_model_weight_to_float8(m, exclude_module_name=["modulation"])
    assert m.dtype == F8                                           # before the wrapper: the storage dtype
    forwards = {name: mod.__dict__.get("forward") for name, mod in m.named_modules()}
    convert_weight_dtype_wrapper(m, torch.bfloat16)
    assert m.dtype == torch.bfloat16
    for name, mod in m.named_modules():
        assert mod.__dict__.get("forward") is forwards[name], name
        assert not hasattr(mod, "original_forward"), name
    for bad in (torch.float16, torch.float32):
        with pytest.raises(NotImplementedError):
            convert_weight_dtype_wrapper(m, bad)


def test_replace_parameters_by_name_turns_parameters_into_tensors():
    from flexam_amd import replace_parameters_by_name
    m = tiny_model()
    replace_parameters_by_name(m, ["modulation"], device="cpu")
    assert not any("modulation" in k for k, _ in m.named_parameters())
    assert torch.is_tensor(m.blocks[0].modulation) and not isinstance(m.blocks[0].modulation, torch.nn.Parameter)


def test_autocast_model_forward_computes_in_origin_dtype_and_keeps_storage():
    from flexam_amd import autocast_model_forward
    torch.manual_seed(1)
    lin = torch.nn.Linear(64, 32)
    lin.weight.data = lin.weight.data.to(F8)
    lin.original_forward = lin.forward
    x = torch.randn(3, 64)
    y = autocast_model_forward(lin, torch.bfloat16, x)
    want = torch.nn.functional.linear(x.to(torch.bfloat16), lin.weight.to(torch.bfloat16), lin.bias.to(torch.bfloat16))
    assert y.dtype == torch.bfloat16 and torch.equal(y, want)
    assert lin.weight.dtype == F8 and lin.bias.dtype == torch.float32      # the stored parameters are untouched


def test_gemm_w8_width_rule_matches_the_kernel():
    """hip.gemm_w8_takes(N): the output widths the e4m3-weight GEMM has a plan for (it refuses the bf16 GEMM's 160-wide tile widths);
    block holders of other widths keep a bf16 copy instead."""
    from flexam_amd import hip
    for n in (192, 200, 256, 640, 1000, 3072, 6144, 9216, 14336):
        assert hip.gemm_w8_takes(n), n
    for n in (4, 64, 128, 160, 320, 480):
        assert not hip.gemm_w8_takes(n), n


def test_selection_equals_the_reference_function():
    from oracle.ref_import import REF_ROOT
    path = os.path.join(REF_ROOT, "FlexAM", "utils", "fp8_optimization.py")
    if not os.path.isfile(path):
        pytest.skip(f"the reference is not mounted at {REF_ROOT} (FLEXAM_REFERENCE_ROOT)")
    spec = importlib.util.spec_from_file_location("_ref_fp8_optimization", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    from flexam_amd import convert_model_weight_to_float8
    ours, theirs = tiny_model(), tiny_model()                        # same seed: the same weights
    convert_model_weight_to_float8(ours, exclude_module_name=["modulation"])
    ref.convert_model_weight_to_float8(theirs, exclude_module_name=["modulation"])
    a, b = dict(ours.named_parameters()), dict(theirs.named_parameters())
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype, k
        assert torch.equal(a[k].view(torch.uint8) if a[k].dtype == F8 else a[k], b[k].view(torch.uint8) if b[k].dtype == F8 else b[k]), k
