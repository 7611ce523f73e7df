"""The reference's qfloat8 weight storage (FlexAM/utils/fp8_optimization.py) under its own names and signatures, so that the
`model_full_load_and_qfloat8` / `model_cpu_offload_and_qfloat8` sequence of comfyui/wan2_2_fun_flexam/nodes.py:327-343

    convert_model_weight_to_float8(transformer, exclude_module_name=["modulation"], device=device)
    convert_weight_dtype_wrapper(transformer, weight_dtype)

runs unchanged on `flexam_amd.Wan2_2Transformer3DModel_FlexAM`.

Numerics are the reference's: every selected parameter is rounded to float8_e4m3fn once (`param.data.to(torch.float8_e4m3fn)`),
and every op computes in bf16 on the upcast values.  Unlike the reference, nothing is upcast per call: the DiT's block GEMMs
read the e4m3 parameters themselves (flexam_gemm_w8: e4m3 in HBM and LDS, widened to bf16 in registers -- exact), so the
mode stores the blocks in half the bytes of bf16 and computes bit-identically to the bf16 model on the rounded weights.
The few parameters outside the blocks (embeddings, head, norms, biases) are upcast once when the engine packs them.
"""
import torch
from torch import nn

F8 = torch.float8_e4m3fn


def replace_parameters_by_name(module, name_keywords, device):
    """Every parameter whose own name contains one of `name_keywords` stops being an nn.Parameter: it stays on its module under
    the same attribute name as a plain tensor on `device` (what `sequential_cpu_offload` wants for the modulation tables,
    nodes.py:320-324)."""
    for mod in module.modules():
        hits = [n for n in mod._parameters if mod._parameters[n] is not None and any(k in n for k in name_keywords)]
        for n in hits:
            value = mod._parameters.pop(n).detach().to(device=device)
            object.__setattr__(mod, n, value)


def convert_model_weight_to_float8(model, exclude_module_name=['embed_tokens'], device=None):
    """Round every parameter whose module path or name contains none of `exclude_module_name` to float8_e4m3fn, in place
    (`param.data`, so state-dict keys and Parameter objects stay).  `device` is accepted and unused, as in the reference."""
    for name, module in model.named_modules():
        if any(ex in name for ex in exclude_module_name):
            continue
        for param_name, param in module.named_parameters():
            if any(ex in param_name for ex in exclude_module_name):
                continue
            if param.dtype != F8:
                param.data = param.data.to(F8)


def autocast_model_forward(cls, origin_dtype, *inputs, **kwargs):
    """One call of `cls.original_forward` computed in `origin_dtype`: the inputs are cast, and the module runs on `origin_dtype`
    copies of its own parameters (torch.func.functional_call) while its stored parameters stay as they are.  For modules outside
    this package; convert_weight_dtype_wrapper does not install it on flexam_amd models, whose kernels read e4m3 directly."""
    from torch.func import functional_call
    upcast = {n: (p.to(origin_dtype) if p.is_floating_point() else p) for n, p in cls.named_parameters()}
    args = tuple(x.to(origin_dtype) if torch.is_tensor(x) and x.is_floating_point() else x for x in inputs)

    class _Call(nn.Module):                       # functional_call runs `forward`; this routes it to the saved one
        def __init__(self):
            super().__init__()
            self.m = cls

        def forward(self, *a, **k):
            return cls.original_forward(*a, **k)
    return functional_call(_Call(), {"m." + n: v for n, v in upcast.items()}, args, kwargs)


def convert_weight_dtype_wrapper(module, origin_dtype):
    """Record `origin_dtype` as the dtype `module` computes in (`module.dtype` reports it).  No forward is wrapped: the kernels
    read the e4m3 weights directly and compute in bf16, which is the only compute dtype they have."""
    if origin_dtype != torch.bfloat16:
        raise NotImplementedError(f"flexam_amd: qfloat8 weights compute in bfloat16 only, not {origin_dtype}")
    module._flexam_compute_dtype = origin_dtype
    engine = getattr(module, "invalidate_engine", None)
    if engine is not None:
        engine()
