"""CPU: flexam_amd.lora_utils' key handling and target table, and the float64 restatement (tests/lora_restatement.py) against what the
REFERENCE's merge_lora / unmerge_lora left in the g16_lora_* fixtures (tools/make_golden_lora.py).  No kernel runs here; the GPU
half is tests/test_lora_gpu.py."""
import glob
import inspect
import os

import numpy as np
import pytest
import torch

import lora_restatement as LR
from conftest import GOLDEN

CASES = sorted(glob.glob(os.path.join(GOLDEN, "g16_lora_*.safetensors")))


def scale_of(c):
    return c["multiplier"] * (c["alpha"] / c["rank"] if c["alpha"] is not None else 1.0)


def test_fixtures_cover_the_cases():
    cs = [LR.load_case(p) for p in CASES]
    assert {c["style"] for c in cs} == {"kohya", "comfy", "peft"}
    assert {c["alpha"] is None for c in cs} == {True, False} and {c["rank"] for c in cs} == {4, 16}
    assert {(c["dtype_fmt"], c["w_fmt"]) for c in cs} >= {("f32", "bf16"), ("bf16", "bf16"), ("f32", "f32"), ("bf16", "f32")}
    assert any(c["missing"] for c in cs) and sum(bool(c["unmerged"]) for c in cs) >= 2
    assert any(v.dim() == 4 for c in cs for v in c["lora"].values())


def test_signatures_are_the_references():
    from flexam_amd import merge_lora, unmerge_lora
    m, u = inspect.signature(merge_lora).parameters, inspect.signature(unmerge_lora).parameters
    assert list(m)[:8] == ["pipeline", "lora_path", "multiplier", "device", "dtype", "state_dict", "transformer_only", "sub_transformer_name"]
    assert (m["device"].default, m["dtype"].default, m["state_dict"].default, m["transformer_only"].default,
            m["sub_transformer_name"].default, m["strict"].default) == ("cpu", torch.float32, None, False, "transformer", False)
    assert list(u)[:6] == ["pipeline", "lora_path", "multiplier", "device", "dtype", "sub_transformer_name"]
    assert (u["multiplier"].default, u["device"].default, u["dtype"].default, u["sub_transformer_name"].default,
            u["strict"].default) == (1, "cpu", torch.float32, "transformer", False)


def test_three_key_styles_resolve_to_one_list(capsys):
    """The three spellings of one adapter give the same (module, up, down, scale) list, in the same order."""
    from flexam_amd import lora_utils as L
    g = torch.Generator().manual_seed(3)
    shapes = LR.tree_names()
    model = LR.tree({n: torch.zeros(s) for n, s in shapes.items()})
    layers = ["blocks.0.self_attn.q", "blocks.1.cross_attn.k", "blocks.0.ffn.0", "blocks.1.ffn.2", "text_embedding.0", "conv_1x1"]
    factors = {n: (torch.randn(shapes[n][0], 4, generator=g), torch.randn(4, shapes[n][1], generator=g)) for n in layers}
    lists = []
    for style in ("kohya", "comfy", "peft"):
        sd = {}
        for n, (up, down) in factors.items():
            sd[LR.spell(n, "lora_down.weight", style)] = down
            sd[LR.spell(n, "lora_up.weight", style)] = up
            if style != "peft":
                sd[LR.spell(n, "alpha", style)] = torch.tensor(2.0)
        lists.append(L.resolve(model, sd, 0.5))
    mods = dict(model.named_modules())
    for got in lists:
        assert [m for m, *_ in got] == [mods[n] for n in layers]
        assert all(u is factors[n][0] and d is factors[n][1] for (_, u, d, _), n in zip(got, layers))
    assert [s for *_, s in lists[0]] == [0.5 * 2.0 / 4] * len(layers) == [s for *_, s in lists[1]]
    assert [s for *_, s in lists[2]] == [0.5] * len(layers)                       # no alpha: multiplier alone
    assert L.normalize_key("lora_unet__blocks_0_self_attn_q.lora_down.weight") == ("blocks_0_self_attn_q", "lora_down.weight")
    assert L.normalize_key("diffusion_model.blocks.0.self_attn.q.lora_down.weight") == ("blocks_0_self_attn_q", "lora_down.weight")
    assert L.normalize_key("blocks.0.self_attn.q.lora_A.default.weight") == ("blocks_0_self_attn_q", "lora_down.weight")
    assert L.normalize_key("blocks.0.ffn.2.lora_B.default.weight") == ("blocks_0_ffn_2", "lora_up.weight")
    assert L.normalize_key("lora_unet__blocks_0_self_attn_q.alpha") == ("blocks_0_self_attn_q", "alpha")
    # PEFT under another adapter name, or none; and tails the merge does not read keep the real layer's name
    assert L.normalize_key("blocks.0.ffn.2.lora_A.other.weight") == ("blocks_0_ffn_2", "lora_down.weight")
    assert L.normalize_key("blocks.0.ffn.2.lora_B.weight") == ("blocks_0_ffn_2", "lora_up.weight")
    assert L.normalize_key("diffusion_model.blocks.0.self_attn.q.diff_b") == ("blocks_0_self_attn_q", "diff_b")
    assert L.normalize_key("diffusion_model.text_embedding.0.lora_up.weight") == ("text_embedding_0", "lora_up.weight")
    with pytest.raises(KeyError, match="blocks_0_self_attn_q.*dora_scale"):
        L.resolve(model, {"blocks.0.self_attn.q.dora_scale": torch.zeros(1)}, 1.0)


def test_missing_unmergeable_and_text_encoder_layers(capsys):
    from flexam_amd import lora_utils as L
    model = LR.tree({"blocks.0.self_attn.q": torch.zeros(8, 8), "patch_embedding": torch.zeros(8, 4, 1, 2, 2)})
    up, down = torch.zeros(8, 2), torch.zeros(2, 8)
    sd = {"lora_unet__blocks_0_self_attn_q.lora_up.weight": up, "lora_unet__blocks_0_self_attn_q.lora_down.weight": down,
          "lora_unet__blocks_9_self_attn_q.lora_up.weight": up, "lora_unet__blocks_9_self_attn_q.lora_down.weight": down,
          "lora_unet__patch_embedding.lora_up.weight": up, "lora_unet__patch_embedding.lora_down.weight": down}
    got = L.resolve(model, sd, 1.0)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(got) == 1 and len(lines) == 2 and "blocks_9_self_attn_q" in lines[0] and "patch_embedding" in lines[1]
    with pytest.raises(KeyError, match="blocks_9_self_attn_q"):
        L.resolve(model, sd, 1.0, strict=True)
    te = dict(sd, **{"lora_te_encoder_block_0_q.lora_up.weight": up, "lora_te_encoder_block_0_q.lora_down.weight": down})
    assert len(L.resolve(model, te, 1.0, transformer_only=True)) == 1
    with pytest.raises(NotImplementedError, match="text-encoder LoRA"):
        L.resolve(model, te, 1.0)


def test_target_table_is_collision_free_for_the_5b_layout_and_raises_on_a_collision():
    from flexam_amd import Wan2_2Transformer3DModel_FlexAM
    from flexam_amd import lora_utils as L
    from oracle import dit as O
    kw = dict(O.DIT_5B)
    kw.pop("eps")
    with torch.device("meta"):
        model = Wan2_2Transformer3DModel_FlexAM(**kw)
    table, other = L.target_table(model)
    named = dict(model.named_modules())
    want = [n for n, m in named.items() if torch.is_tensor(getattr(m, "weight", None)) and L._mergeable(m.weight)]
    assert len(table) == len(want) == 30 * 10 + 9 and all(table[n.replace(".", "_")] is named[n] for n in want)
    assert {"patch_embedding", "cnn_conv5", "ref_conv"} <= other and not (other & set(table))
    for b in (0, 29):
        for n in ("self_attn_q", "self_attn_k", "self_attn_v", "self_attn_o", "cross_attn_q", "cross_attn_k", "cross_attn_v",
                  "cross_attn_o", "ffn_0", "ffn_2"):
            assert f"blocks_{b}_{n}" in table
    toy = LR.tree({"a.b_c": torch.zeros(2, 2), "a_b.c": torch.zeros(2, 2)})
    with pytest.raises(ValueError, match="both flatten to 'a_b_c'"):
        L.target_table(toy)


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[9:-12] for p in CASES])
def test_reference_results_within_the_stated_bounds_of_the_exact_merge(path):
    """dtype float32: the reference lies within one storage ulp of the correctly rounded exact value; dtype bfloat16: within half a
    bf16 ulp of the product + half a bf16 ulp of the scaled product + one bf16 ulp of the larger of |W'| and |sP| (float64
    quantities, factors rounded to bf16 first as both implementations do).  Layers the adapter does not name are untouched: the
    fixture stores them once."""
    c = LR.load_case(path)
    s = scale_of(c)
    assert sorted(c["after"]) == sorted(c["layers"])
    for layer in c["layers"]:
        up = c["lora"][LR.spell(layer, "lora_up.weight", c["style"])].flatten(1)
        down = c["lora"][LR.spell(layer, "lora_down.weight", c["style"])].flatten(1)
        w0, w1 = c["before"][layer].flatten(1), c["after"][layer].flatten(1)
        assert w1.dtype == w0.dtype == LR.TORCH[c["w_fmt"]] and not torch.equal(w0, w1)
        x, bound = LR.reference_bound(w0, up, down, s, c["dtype_fmt"], c["w_fmt"])
        err = np.abs(LR.f64(w1) - LR.round_to(x, c["w_fmt"]))
        print(f"{layer}: worst error / bound {float((err / bound).max()):.3f}; {float((err > 0).mean()) * 100:.2f} % of elements differ")
        assert (err <= bound).all(), layer


@pytest.mark.parametrize("path", [p for p in CASES if LR.load_case(p)["unmerged"]], ids=lambda p: os.path.basename(p)[9:-12])
def test_merge_then_unmerge_drifts_by_at_most_one_storage_ulp(path):
    """Reference results, and the restatement's own (each step rounded once): within one storage ulp at max(|W|, |W'|) of the start."""
    c = LR.load_case(path)
    s = scale_of(c)
    for layer in c["layers"]:
        w0, w1, w2 = (c[k][layer].flatten(1) for k in ("before", "after", "unmerged"))
        lim = LR.ulp(np.maximum(np.abs(LR.f64(w0)), np.abs(LR.f64(w1))), c["w_fmt"])
        assert (np.abs(LR.f64(w2) - LR.f64(w0)) <= lim).all(), layer
        up, down = LR.cast_factors(c["lora"][LR.spell(layer, "lora_up.weight", c["style"])].flatten(1),
                                   c["lora"][LR.spell(layer, "lora_down.weight", c["style"])].flatten(1), c["dtype_fmt"])
        m1 = LR.merged(w0, up, down, s)
        m2 = LR.merged(m1, up, down, -s)
        lim = LR.ulp(np.maximum(np.abs(LR.f64(w0)), np.abs(LR.f64(m1))), c["w_fmt"])
        assert (np.abs(LR.f64(m2) - LR.f64(w0)) <= lim).all(), layer


def test_rounding_restatement_agrees_with_torch_on_representable_and_tie_values():
    """round_to against torch's own conversions (single rounding from fp32), ties and subnormals included."""
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.randn(4000, generator=g) * 3, torch.randn(2000, generator=g) * 1e-3, torch.tensor([0.0, 448.0, 1.0078125, 1.0234375]),
                   torch.arange(-40, 40).float() / 1024, torch.arange(0, 64).float() * 0.0009765625])
    for fmt in ("bf16", "e4m3"):
        want = x.clamp(-448, 448).to(LR.TORCH[fmt]).float().double().numpy() if fmt == "e4m3" else x.to(LR.TORCH[fmt]).float().double().numpy()
        assert np.array_equal(LR.round_to(x.double().numpy(), fmt), want), fmt
    assert np.array_equal(LR.round_to(np.array([500.0, -1e4, 464.0, 463.9]), "e4m3"), np.array([448.0, -448.0, 448.0, 448.0]))
    assert LR.ulp(1.0, "bf16") == 2.0 ** -7 and LR.ulp(448.0, "e4m3") == 32.0 and LR.ulp(0.0, "e4m3") == 2.0 ** -9


def test_abi_declares_the_entry_point_and_the_table_follows():
    from flexam_amd import abi, gen_replay
    names = [n for n, _, _ in abi.PROTOTYPES]
    assert "flexam_lora_merge" in names and "flexam_lora_merge" in open(gen_replay.OUT).read()
    assert (abi.CONSTANTS["FLEXAM_LORA_BF16"], abi.CONSTANTS["FLEXAM_LORA_F32"], abi.CONSTANTS["FLEXAM_LORA_E4M3"]) == (0, 1, 2)
