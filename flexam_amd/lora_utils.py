"""The reference's LoRA merge (FlexAM/utils/lora_utils.py:371-490 `merge_lora`, :493-604 `unmerge_lora`) under its own names,
argument order and defaults, so that the sampler node's block (comfyui/wan2_2_fun_flexam/nodes.py:595-649) runs unchanged on a
`flexam_amd` pipeline:

    pipeline = merge_lora(pipeline, lora_path, multiplier, device=device, dtype=weight_dtype)
    ...
    pipeline = unmerge_lora(pipeline, lora_path, multiplier, device=device, dtype=weight_dtype)

Each layer is ONE launch of flexam_lora_merge on the stored weight, in place, whatever it is stored as (bf16, float32 or
float8_e4m3fn; a row range of a fused q|k|v buffer included):

    W <- round_to_W_dtype(float(W) + s * up @ down),        s = multiplier * (alpha / rank, or 1)

The factors are cast to `dtype` first, as the reference casts them (:472-473: under dtype=torch.bfloat16 their bf16 rounding is
reproduced); everything after that cast is fp32 arithmetic and one rounding.  The reference rounds the product, the scaled product
and the sum to `dtype` instead; fewer roundings is the deliberate difference (bounded in tests/test_lora_cpu.py).  Like the
reference's, an unmerge does not restore rounded weights bit for bit: each element ends within one storage ulp of where it began.

After the last layer `transformer.invalidate_engine()` drops everything the engine derived from the old weights (copied packs,
fused views, e4m3 operand copies, the per-clip cross K|V and text state): a kernel write bumps no version counter.
"""
import re
from collections import defaultdict

import torch

LORA_PREFIX_TRANSFORMER = "lora_unet"
LORA_PREFIX_TEXT_ENCODER = "lora_te"
# the closing part of a key -> the element name the merge reads: kohya's own, and PEFT's lora_A = down, lora_B = up under any
# adapter name (`lora_A.default.weight`, `lora_A.weight`)
_ELEM = re.compile(r"\.(lora_down\.weight|lora_up\.weight|alpha|lora_A\.(?:\w+\.)?weight|lora_B\.(?:\w+\.)?weight)$")
_STORED = (torch.bfloat16, torch.float32, torch.float8_e4m3fn)


def normalize_key(key: str):
    """One adapter key of any accepted style -> (flattened layer name, element), or (None, None) for a text-encoder key:
        kohya    lora_unet__blocks_0_self_attn_q.lora_down.weight
        ComfyUI  diffusion_model.blocks.0.self_attn.q.lora_down.weight
        PEFT     blocks.0.self_attn.q.lora_A.default.weight
    all give ("blocks_0_self_attn_q", "lora_down.weight"): the module's dotted name with `.` replaced by `_` (what the
    reference's rewriting at :379-395 and its split at `lora_unet_` amount to).  A key that closes in anything else (`diff_b`,
    `dora_scale`) keeps its last component as the element, so that messages name the real layer."""
    m = _ELEM.search(key)
    if m:
        layer, elem = key[:m.start()], m.group(1)
        if elem.startswith("lora_A"):
            elem = "lora_down.weight"
        elif elem.startswith("lora_B"):
            elem = "lora_up.weight"
    else:
        layer, _, elem = key.rpartition(".")
        if not layer:
            layer, elem = key, ""
    if LORA_PREFIX_TEXT_ENCODER in layer:
        return None, None
    if layer.startswith("diffusion_model."):
        layer = layer[len("diffusion_model."):]
    if layer.startswith(LORA_PREFIX_TRANSFORMER + "_"):
        layer = layer[len(LORA_PREFIX_TRANSFORMER) + 1:]
    return layer.replace(".", "_").lstrip("_"), elem


def group_updates(state_dict, transformer_only: bool = False):
    """{flattened layer name: {element: tensor}} in the adapter's own order (the reference's `updates`)."""
    updates = defaultdict(dict)
    for key, value in state_dict.items():
        layer, elem = normalize_key(key)
        if layer is None:
            if transformer_only:
                continue
            raise NotImplementedError(f"text-encoder LoRA ({key}) is not part of the FlexAM 5B path (SURVEY section 2): "
                                      "pass transformer_only=True to merge the transformer's layers only")
        updates[layer][elem] = value
    return updates


def _mergeable(weight) -> bool:
    return torch.is_tensor(weight) and (weight.dim() == 2 or (weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1)))


def target_table(transformer):
    """{flattened name: module} of every module with a 2-D or 1x1 4-D `weight` (dotted name of named_modules(), `.` -> `_`), and the
    set of flattened names whose weight has another form (the 5-D convolutions).  Two modules that flatten to one key raise here."""
    table, dotted, other = {}, {}, set()
    for name, mod in transformer.named_modules():
        w = getattr(mod, "weight", None)
        if not torch.is_tensor(w):
            continue
        flat = name.replace(".", "_")
        if not _mergeable(w):
            other.add(flat)
            continue
        if flat in table and table[flat] is not mod:
            raise ValueError(f"LoRA target table: modules '{dotted[flat]}' and '{name}' both flatten to '{flat}'")
        table[flat], dotted[flat] = mod, name
    return table, other


def layer_scale(elems, multiplier) -> float:
    """s = multiplier * (alpha / rank when the adapter carries an alpha, else 1), in Python floats."""
    if "alpha" in elems:
        a = elems["alpha"]
        return float(multiplier) * (float(a.item() if torch.is_tensor(a) else a) / elems["lora_up.weight"].shape[1])
    return float(multiplier) * 1.0


def resolve(transformer, state_dict, multiplier, transformer_only: bool = False, strict: bool = False):
    """[(module, up, down, s)] for every layer of the adapter that names a mergeable module, in the adapter's order; a layer that is
    not found, or whose weight is not a matrix, prints one line and is skipped (raises under strict)."""
    table, other = target_table(transformer)
    out = []
    for layer, elems in group_updates(state_dict, transformer_only).items():
        if layer not in table:
            why = "its weight is not a matrix or a 1x1 convolution" if layer in other else "no such module"
            if strict:
                raise KeyError(f"LoRA layer {layer}: {why}")
            print(f"Error loading layer: {layer} ({why}). Skipped.")
            continue
        if "lora_up.weight" not in elems or "lora_down.weight" not in elems:
            raise KeyError(f"LoRA layer {layer}: lora_up.weight / lora_down.weight missing; the adapter gives it {sorted(elems)}, "
                           "which this merge does not read")
        out.append((table[layer], elems["lora_up.weight"], elems["lora_down.weight"], layer_scale(elems, multiplier)))
    return out


def _factor(t, dtype, dev):
    """A factor as the kernel reads it: cast to `dtype` first (the reference's rounding of the factors), squeezed when it is a 1x1
    convolution's, on the merged module's device."""
    if dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise NotImplementedError(f"flexam_amd: LoRA factors are cast to float32, bfloat16 or float16, not {dtype}")
    t = t.to(dtype)
    if t.dim() == 4:
        if tuple(t.shape[2:]) != (1, 1):
            raise NotImplementedError(f"flexam_amd: LoRA factors of a {tuple(t.shape[2:])} convolution are not part of the FlexAM 5B path")
        t = t.squeeze(3).squeeze(2)
    if dtype == torch.float16:
        t = t.float()                                  # exact
    return t.to(dev).contiguous()


@torch.no_grad()
def _apply(pipeline, lora_path, multiplier, dtype, state_dict, transformer_only, sub_transformer_name, strict, sign):
    from . import hip
    if state_dict is None:
        from safetensors.torch import load_file
        state_dict = load_file(lora_path)
    transformer = getattr(pipeline, sub_transformer_name)
    todo = resolve(transformer, state_dict, multiplier, transformer_only, strict)
    try:
        for mod, up, down, s in todo:
            w = mod.weight.data
            if w.dtype not in _STORED:
                raise NotImplementedError(f"flexam_amd: LoRA merge into {w.dtype} weights is not implemented (bf16, float32, float8_e4m3fn)")
            if w.device.type != "cuda":
                raise RuntimeError(f"flexam_amd: LoRA merge runs only on a GPU through libflexam_hip.so (no CPU or eager fallback); the "
                                   f"weight is on {w.device}: move the model to cuda first")
            w2 = w.view(w.shape[0], w.shape[1]) if w.dim() == 4 else w
            hip.lora_merge(w2, _factor(up, dtype, w.device), _factor(down, dtype, w.device), sign * s)
    finally:
        invalidate = getattr(transformer, "invalidate_engine", None)
        if invalidate is not None and todo:
            invalidate()
    return pipeline


def merge_lora(pipeline, lora_path, multiplier, device='cpu', dtype=torch.float32, state_dict=None, transformer_only=False,
               sub_transformer_name="transformer", strict=False):
    """lora_utils.py:371-490.  `device` is accepted for the reference's signature; the factors always go to the merged module's own
    device (the kernel takes device pointers).  strict=True (this package's keyword) raises on a layer the reference would skip."""
    return _apply(pipeline, lora_path, multiplier, dtype, state_dict, transformer_only, sub_transformer_name, strict, 1.0)


def unmerge_lora(pipeline, lora_path, multiplier=1, device="cpu", dtype=torch.float32, sub_transformer_name="transformer", *,
                 state_dict=None, transformer_only=False, strict=False):
    """lora_utils.py:493-604: merge_lora with -multiplier.  The keyword-only arguments are this package's."""
    return _apply(pipeline, lora_path, multiplier, dtype, state_dict, transformer_only, sub_transformer_name, strict, -1.0)
