"""float64 restatement of the LoRA merge (flexam_amd/lora_utils.py, csrc/lora.hip) and the number formats it rounds to; shared by
tests/test_lora_cpu.py, tests/test_lora_gpu.py and tools/make_golden_lora.py.  Pure numpy / CPU torch.

    exact(W, U, D, s)            W + float32(s) * U @ D in float64 (the kernel takes s as fp32; products of bf16 / fp32 factors and
                                 sums of a few hundred of them carry ~1e-16 relative error in float64: "exact" at every storage ulp here)
    round_to(x, fmt)             x rounded ONCE to the format, to nearest even (e4m3: beyond 448 saturates), still as float64
    ulp(x, fmt)                  spacing of the format at |x|
    kernel_order(W, U, D, s)     fp32 restatement of the kernel: acc = fma(U[:, j], D[j], acc), j ascending, then fma(s, acc, W)
    reference_bound(...)         how far the REFERENCE's torch expression (`weight += multiplier * alpha * mm(up, down)` in `dtype`)
                                 may lie from the correctly rounded exact value
"""
import numpy as np
import torch

# significand bits (with the hidden one), smallest normal exponent, largest finite value
FORMATS = {"bf16": (8, -126, float(torch.finfo(torch.bfloat16).max)), "f32": (24, -126, float(torch.finfo(torch.float32).max)),
           "e4m3": (4, -6, 448.0)}
TORCH = {"bf16": torch.bfloat16, "f32": torch.float32, "e4m3": torch.float8_e4m3fn}
NAME = {v: k for k, v in TORCH.items()}


def f64(t):
    """A tensor of any storage type (or an array) as a float64 numpy array: exact."""
    if torch.is_tensor(t):
        return t.detach().cpu().to(torch.float32).double().numpy() if t.dtype != torch.float64 else t.detach().cpu().numpy()
    return np.asarray(t, np.float64)


def ulp(x, fmt):
    p, emin, _ = FORMATS[fmt]
    a = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.where(a > 0, np.maximum(e, emin), emin)
    return np.exp2(e - (p - 1))


def round_to(x, fmt):
    x = np.asarray(x, np.float64)
    u = ulp(x, fmt)
    y = np.rint(x / u) * u                      # x / u is exact (a power of two); rint rounds halves to even
    return np.clip(y, -FORMATS[fmt][2], FORMATS[fmt][2])


def exact(W, U, D, s):
    return f64(W) + float(np.float32(s)) * (f64(U) @ f64(D))


def merged(W, U, D, s, fmt=None):
    """The correctly rounded merge as a torch tensor of W's storage type."""
    fmt = fmt or NAME[W.dtype]
    return to_storage(round_to(exact(W, U, D, s), fmt), fmt)


def to_storage(x, fmt):
    """float64 values that the format holds exactly -> a tensor of that type."""
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.float32).to(TORCH[fmt])


def _fma32(x, y, z, doubt):
    """fp32 fma(x, y, z) of float64 arrays holding fp32 values: the product is exact in float64, the sum is rounded to float64 and
    then to fp32.  Where the float64 sum was itself inexact (its TwoSum error term is not zero) AND it lies within 2^-28 of an fp32
    ulp of a rounding tie, that first rounding (2^-29 of the ulp) could have decided: such elements are counted into doubt[0]."""
    p = x * y
    t = p + z
    r = t.astype(np.float32)
    if doubt is not None:
        zz = t - p
        err = (p - (t - zz)) + (z - zz)
        u = ulp(r.astype(np.float64), "f32")
        doubt[0] += int(((err != 0) & (np.abs(np.abs(t - r.astype(np.float64)) - 0.5 * u) < u * 2.0 ** -28)).sum())
    return r


def kernel_order(W, U, D, s, fmt=None, doubt=None):
    """The kernel's own arithmetic on the CPU, as a tensor of the storage type: acc = fma(U[:, j], D[j], acc) from 0 with j
    ascending, fma(s, acc, W), one conversion.  doubt = [0] collects the number of emulated fmas that are not certain (_fma32):
    with doubt[0] == 0 the result is the fmaf chain's, bit for bit."""
    fmt = fmt or NAME[W.dtype]
    w, u, d = f64(W), f64(U), f64(D)
    acc = np.zeros_like(w, dtype=np.float32)
    for j in range(u.shape[1]):
        acc = _fma32(u[:, j, None], d[j][None, :], acc.astype(np.float64), doubt)
    y = _fma32(np.float64(np.float32(s)), acc.astype(np.float64), w, doubt)
    if fmt == "e4m3":
        y = np.clip(y, -448.0, 448.0)
    return torch.from_numpy(y).to(TORCH[fmt])


def steps_apart(a, b, fmt):
    """|a - b| in units of the storage ulp at the larger magnitude (float64 arrays of representable values)."""
    a, b = f64(a), f64(b)
    return np.abs(a - b) / ulp(np.maximum(np.abs(a), np.abs(b)), fmt)


def reference_bound(W, U, D, s, dtype_fmt, fmt):
    """Per-element bound on |reference result - correctly rounded exact value| for a layer stored as `fmt`, merged by the reference
    with `dtype` = dtype_fmt ("f32" | "bf16").  U, D: the factors as stored in the adapter.
      dtype f32: one storage ulp (its arithmetic is fp32; the fixture's factors lie on a grid where it is exact up to the last add).
      dtype bf16: the factors are rounded to bf16 first -- that is part of the VALUE (lora_utils reproduces it) -- then half a bf16
        ulp of the product P, half a bf16 ulp of the scaled product sP, and one bf16 ulp of the larger of |W'| and |sP| for the sum
        and the storage rounding."""
    if dtype_fmt == "f32":
        x = exact(W, U, D, s)
        return x, ulp(round_to(x, fmt), fmt)
    u, d = round_to(f64(U), "bf16"), round_to(f64(D), "bf16")
    P = u @ d
    sP = float(np.float32(s)) * P
    x = f64(W) + sP
    return x, 0.5 * ulp(P, "bf16") + 0.5 * ulp(sP, "bf16") + ulp(np.maximum(np.abs(x), np.abs(sP)), "bf16")


def cast_factors(U, D, dtype_fmt):
    """The factors as merge_lora hands them to the kernel: cast to `dtype` first."""
    return (U.to(TORCH[dtype_fmt]), D.to(TORCH[dtype_fmt]))


# ----------------------------------------------------------------------------- the tiny module tree of the g16_lora_* fixtures
class Leaf(torch.nn.Module):
    """A parameter holder: `weight` of any rank under the module's name."""

    def __init__(self, weight):
        super().__init__()
        self.weight = torch.nn.Parameter(weight.clone(), requires_grad=False)


class Tree(torch.nn.Module):
    @property
    def device(self):
        return next(self.parameters()).device


def tree(weights):
    """{"blocks.0.self_attn.q": tensor, ...} -> nested modules under those dotted names (what named_modules() then reports)."""
    root = Tree()
    for name, w in weights.items():
        node, parts = root, name.split(".")
        for part in parts[:-1]:
            if part not in node._modules:
                node.add_module(part, torch.nn.Module())
            node = node._modules[part]
        node.add_module(parts[-1], Leaf(w))
    return root


class Pipe:
    def __init__(self, transformer):
        self.transformer = transformer


def tree_names(blocks=2):
    """The fixture tree: `blocks` blocks under the 5B key names, a text_embedding.0 and one 1x1 convolution; name -> weight shape."""
    shapes = {}
    for b in range(blocks):
        for attn in ("self_attn", "cross_attn"):
            for lin in "qkvo":
                shapes[f"blocks.{b}.{attn}.{lin}"] = (64, 64)
        shapes[f"blocks.{b}.ffn.0"] = (160, 64)
        shapes[f"blocks.{b}.ffn.2"] = (64, 160)
    shapes["text_embedding.0"] = (64, 96)
    shapes["conv_1x1"] = (64, 48, 1, 1)
    return shapes


def spell(layer, elem, style):
    """One adapter key in a style: layer = dotted module name, elem = "lora_down.weight" | "lora_up.weight" | "alpha"."""
    if style == "kohya":
        return "lora_unet__" + layer.replace(".", "_") + "." + elem
    if style == "comfy":
        return "diffusion_model." + layer + "." + elem
    if style == "peft":
        return layer + "." + {"lora_down.weight": "lora_A.default.weight", "lora_up.weight": "lora_B.default.weight"}.get(elem, elem)
    raise ValueError(style)


def load_case(path):
    """A g16_lora_* file -> dict(before, after, unmerged (or None), lora, multiplier, dtype_fmt, style)."""
    import json
    from safetensors import safe_open
    out = dict(before={}, after={}, unmerged={}, lora={})
    with safe_open(path, "pt") as f:
        meta = f.metadata()
        for k in f.keys():
            part, name = k.split("/", 1)
            out[part][name] = f.get_tensor(k)
    out.update(json.loads(meta["case"]))
    return out
