"""Writes tests/golden/g16_lora_*.safetensors: what the REFERENCE's merge_lora and unmerge_lora (FlexAM/utils/lora_utils.py:371-490,
:493-604) leave in the weights of a tiny module tree on the CPU -- two blocks with q/k/v/o, cross q/k/v/o and ffn.0/.2 under the 5B
key names (width 64, ffn 160), a text_embedding.0 and one 1x1 convolution -- next to the weights before and the adapter.

The two functions are cut out of the reference's lora_utils.py BY NAME with `ast` at run time and executed (the technique of
tools/make_golden_motion.py: the module's own top-level imports need diffusers and transformers); the reference's code runs, nothing
of it is stored here.  Needs the reference checkout (FLEXAM_REFERENCE_ROOT, as oracle/ref_raster.py reads it); never imported by flexam_amd, bench.py or the tests.

Cases (tests/lora_restatement.py reads them back):
    kohya_f32_bf16w    kohya keys, alpha, rank 4, dtype float32, bf16 weights; a layer the model does not have; a lora_te key under
                       transformer_only=True; text_embedding.0 and the 1x1 convolution (4-D factors)
    comfy_bf16_bf16w   ComfyUI keys, no alpha, rank 16, dtype bfloat16, bf16 weights; merge, then unmerge
    peft_f32_f32w      PEFT keys, no alpha, rank 16, dtype float32, fp32 weights; merge, then unmerge
    kohya_bf16_f32w    kohya keys, alpha, rank 4, dtype bfloat16, fp32 weights that hold bf16 values (the reference casts the whole
                       layer to `dtype`: fp32 weights with more bits would be rounded by the cast itself, which no merge can follow;
                       merge only: its unmerge leaves bf16 values again, a bf16 ulp from the start, not an fp32 one)
Under dtype float32 the factors lie on a coarse binary grid (5-bit integers times a power of two) and every scale is at most 1, so
the reference's fp32 products, sums and scaling are exact and its result is the exact value rounded as the bounds of
tests/lora_restatement.py name.  Under dtype bfloat16 the factors are plain fp32 normal draws that bf16 cannot hold: the cast to
`dtype` rounds them, in the reference and in flexam_amd.lora_utils alike, and a merge that skipped the cast would land ulps away.
Before anything is written the script asserts those bounds and the drift bound on the reference's own results.

    python tools/make_golden_lora.py
"""
import ast
import json
import os
import sys
from collections import defaultdict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lora_restatement as LR            # noqa: E402
from oracle import ref_raster            # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SOURCE = os.path.join(ref_raster.REF_ROOT, "FlexAM", "utils", "lora_utils.py")
CASES = [
    dict(name="kohya_f32_bf16w", style="kohya", alpha=2.0, rank=4, multiplier=0.75, dtype_fmt="f32", w_fmt="bf16", unmerge=False,
         layers=["blocks.0.self_attn.q", "blocks.0.self_attn.k", "blocks.1.cross_attn.v", "blocks.1.ffn.0", "text_embedding.0", "conv_1x1"],
         missing=True, text_encoder=True),
    dict(name="comfy_bf16_bf16w", style="comfy", alpha=None, rank=16, multiplier=0.5, dtype_fmt="bf16", w_fmt="bf16", unmerge=True,
         layers=["blocks.0.self_attn.v", "blocks.0.self_attn.o", "blocks.0.cross_attn.q", "blocks.1.cross_attn.k", "blocks.1.ffn.2"]),
    dict(name="peft_f32_f32w", style="peft", alpha=None, rank=16, multiplier=0.75, dtype_fmt="f32", w_fmt="f32", unmerge=True,
         layers=["blocks.0.self_attn.q", "blocks.0.cross_attn.o", "blocks.0.ffn.0", "blocks.1.self_attn.k", "blocks.1.ffn.2"]),
    dict(name="kohya_bf16_f32w", style="kohya", alpha=8.0, rank=4, multiplier=0.25, dtype_fmt="bf16", w_fmt="f32", unmerge=False,
         layers=["blocks.0.cross_attn.k", "blocks.1.self_attn.o", "blocks.1.ffn.0", "conv_1x1"], bf16_values=True),
]


def load_reference(load_file):
    tree = ast.parse(open(SOURCE).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("merge_lora", "unmerge_lora")]
    assert len(fns) == 2, [n.name for n in fns]
    mod = ast.Module(body=fns, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"torch": torch, "defaultdict": defaultdict, "load_file": load_file}
    exec(compile(mod, SOURCE, "exec"), ns)
    return ns["merge_lora"], ns["unmerge_lora"]


def make_case(c, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = LR.tree_names()
    before = {}
    for name, shape in shapes.items():
        w = torch.randn(shape, generator=g) * 0.05
        if c.get("bf16_values"):                      # fp32 storage, generic factors: keep |W| >= 0.03 above the delta (below), so
            w = torch.sign(w) * (0.03 + w.abs())      # that no sum cancels and fp32 arithmetic stays within one fp32 ulp
        if c["w_fmt"] == "bf16" or c.get("bf16_values"):
            w = w.to(torch.bfloat16)
        before[name] = w.to(LR.TORCH[c["w_fmt"]])
    lora, r = {}, c["rank"]
    for layer in c["layers"]:
        n, k = shapes[layer][:2]
        if c["dtype_fmt"] == "bf16":                  # plain fp32 draws: the cast to `dtype` rounds every one of them
            up, down = torch.randn(n, r, generator=g) * 0.5, torch.randn(r, k, generator=g) * (0.005 if c.get("bf16_values") else 0.02)
            assert not torch.equal(up, up.bfloat16().float()) and not torch.equal(down, down.bfloat16().float())
        else:
            up = torch.randint(-8, 9, (n, r), generator=g).float() / 8
            down = torch.randint(-8, 9, (r, k), generator=g).float() / 128
        if len(shapes[layer]) == 4:
            up, down = up[:, :, None, None], down[:, :, None, None]
        lora[LR.spell(layer, "lora_up.weight", c["style"])] = up.contiguous()
        lora[LR.spell(layer, "lora_down.weight", c["style"])] = down.contiguous()
        if c["alpha"] is not None:
            lora[LR.spell(layer, "alpha", c["style"])] = torch.tensor(c["alpha"])
    if c.get("missing"):
        lora[LR.spell("blocks.7.self_attn.q", "lora_up.weight", c["style"])] = torch.zeros(64, r)
        lora[LR.spell("blocks.7.self_attn.q", "lora_down.weight", c["style"])] = torch.zeros(r, 64)
    if c.get("text_encoder"):
        lora["lora_te_encoder_block_0_layer_0_q.lora_up.weight"] = torch.zeros(8, r)
        lora["lora_te_encoder_block_0_layer_0_q.lora_down.weight"] = torch.zeros(r, 8)
    return before, lora


def weights_of(tree, names):
    mods = dict(tree.named_modules())
    return {n: mods[n].weight.data.clone() for n in names}


def check(c, before, lora, after, unmerged):
    """The bounds of tests/test_lora_cpu.py on the reference's own results."""
    s = c["multiplier"] * (c["alpha"] / c["rank"] if c["alpha"] is not None else 1.0)
    assert s <= 1.0
    for layer in c["layers"]:
        up = lora[LR.spell(layer, "lora_up.weight", c["style"])].flatten(1)
        down = lora[LR.spell(layer, "lora_down.weight", c["style"])].flatten(1)
        w0, w1 = before[layer].flatten(1), after[layer].flatten(1)
        x, bound = LR.reference_bound(w0, up, down, s, c["dtype_fmt"], c["w_fmt"])
        err = np.abs(LR.f64(w1) - LR.round_to(x, c["w_fmt"]))
        assert (err <= bound).all(), (c["name"], layer, float((err / bound).max()))
        if unmerged is not None:
            w2 = unmerged[layer].flatten(1)
            lim = LR.ulp(np.maximum(np.abs(LR.f64(w0)), np.abs(LR.f64(w1))), c["w_fmt"])
            assert (np.abs(LR.f64(w2) - LR.f64(w0)) <= lim).all(), (c["name"], layer, "drift")
        print(f"  {layer}: reference within {float((err / bound).max()):.2f} of its bound; "
              f"{float((err > 0).mean()) * 100:.1f} % of elements differ from the correctly rounded value")


def main():
    from safetensors.torch import save_file
    for i, c in enumerate(CASES):
        before, lora = make_case(c, 1600 + i)
        merge, unmerge = load_reference(lambda path, _l=lora: dict(_l))
        tree = LR.tree(before)
        pipe = LR.Pipe(tree)
        dtype = LR.TORCH[c["dtype_fmt"]]
        merge(pipe, None, c["multiplier"], device="cpu", dtype=dtype, state_dict=dict(lora), transformer_only=True)
        after = weights_of(tree, c["layers"])
        untouched = [n for n in before if n not in c["layers"]]
        assert all(torch.equal(dict(tree.named_modules())[n].weight.data, before[n]) for n in untouched)
        assert all(dict(tree.named_modules())[n].weight.dtype == before[n].dtype for n in before)
        unmerged = None
        if c["unmerge"]:
            unmerge(pipe, "adapter", c["multiplier"], device="cpu", dtype=dtype)
            unmerged = weights_of(tree, c["layers"])
        print(c["name"])
        check(c, before, lora, after, unmerged)
        out = {"before/" + n: w.contiguous() for n, w in before.items()}
        out.update({"after/" + n: w.contiguous() for n, w in after.items()})
        out.update({"unmerged/" + n: w.contiguous() for n, w in (unmerged or {}).items()})
        out.update({"lora/" + k: v.contiguous() for k, v in lora.items()})
        meta = {k: c[k] for k in ("name", "style", "alpha", "rank", "multiplier", "dtype_fmt", "w_fmt", "layers")}
        meta["missing"] = ["blocks_7_self_attn_q"] if c.get("missing") else []
        path = os.path.join(GOLDEN, f"g16_lora_{c['name']}.safetensors")
        save_file(out, path, metadata={"case": json.dumps(meta)})
        print(f"  wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
