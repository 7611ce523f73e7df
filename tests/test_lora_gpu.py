"""GPU: flexam_lora_merge (csrc/lora.hip) against the float64 restatement (tests/lora_restatement.py), flexam_amd.lora_utils against the
REFERENCE's results (tests/golden/g16_lora_*), and the engine's coherence after a merge: the next forward equals a model loaded from
the merged state dict, bit for bit.

Data of the kernel test.  "Within one storage ulp of the correctly rounded exact value, at most 1 % of elements different from it" is
a property of fp32 arithmetic only where the storage type is coarser than fp32 and the sum does not cancel: fp32 carries 2^-24 of
the TERMS, a storage ulp is 2^-7 (bf16) or 2^-3 (e4m3) of the RESULT.  e4m3: plain normal draws (a cancellation to 2^-20 of the terms
is a matter of the seed).  bf16: normal factors, but |W| >= 0.02 and a delta of standard deviation 0.003, so that no result is smaller
than 2^-15 of its terms -- among the 590 000 elements of the head's shape plain draws always hold a few that are.  For fp32 storage
any fp32 summation of r generic products misses the correctly rounded sum on most elements, so there
the factors lie on a coarse binary grid (5-bit integers times a power of two: every product and partial sum is exact in fp32) and the
one rounding left is the closing fma's -- which is the claim: one rounding.  Either way the fp32 restatement of the kernel's order is
held to the cap on the CPU before the GPU result is looked at; and on plain draws, for every storage type, the GPU result is held to
that restatement bit for bit (test_generic_data_follows_the_stated_order_bit_for_bit)."""
import glob
import os

import numpy as np
import pytest
import torch

import lora_restatement as LR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
BF, F32, F8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn
DEV = "cuda:0"
SHAPES = [(64, 64, 1), (130, 264, 5), (192, 3072, 16), (96, 160, 300)]
CASES = sorted(glob.glob(os.path.join(GOLDEN, "g16_lora_*.safetensors")))


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype == F8 else (t.contiguous().view(torch.int32) if t.dtype == F32 else t.contiguous().view(torch.int16))


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def fused(N, K, ld, w, g):
    """A fused buffer of N + 5 rows of stride ld whose rows 3 .. 3 + N hold w; everything else random."""
    buf = (torch.randn(N + 5, ld, generator=g) * 0.05).to(w.dtype)
    buf[3:3 + N, :K] = w
    return buf


def kernel_case(N, K, r, fmt, ffmt, seed):
    g = torch.Generator().manual_seed(seed)
    if fmt == "f32":
        U, D = torch.randint(-8, 9, (N, r), generator=g).float() / 8, torch.randint(-8, 9, (r, K), generator=g).float() / 128
        W = torch.randn(N, K, generator=g) * 0.05
    elif fmt == "bf16":
        # |W| >= 0.02 and s U D ~ N(0, 0.003^2): 3 to 25 bf16 ulps of W, and no sum cancels to within 2^-15 of its terms
        U, D = torch.randn(N, r, generator=g), torch.randn(r, K, generator=g) * (0.003 / (0.37 * r ** 0.5))
        W = torch.randn(N, K, generator=g)
        W = (torch.sign(W) * (0.02 + 0.05 * W.abs())).to(BF)
    else:
        U, D = torch.randn(N, r, generator=g), torch.randn(r, K, generator=g) * 0.05
        W = (torch.randn(N, K, generator=g) * 2.0).to(F8)
    return W, U.to(LR.TORCH[ffmt]), D.to(LR.TORCH[ffmt]), 0.37


@pytest.mark.parametrize("ffmt", ["f32", "bf16"])
@pytest.mark.parametrize("fmt", ["bf16", "f32", "e4m3"])
@pytest.mark.parametrize("N,K,r", SHAPES)
def test_kernel_against_the_restatement(N, K, r, fmt, ffmt):
    from flexam_amd import hip as H
    W, U, D, s = kernel_case(N, K, r, fmt, ffmt, 100 + N + r)
    want = LR.merged(W, U, D, s)
    # the condition: the kernel's own order in fp32, on the CPU, stays within the cap
    cpu = LR.steps_apart(LR.kernel_order(W, U, D, s), want, fmt)
    assert cpu.max() <= 1 and (cpu > 0).mean() <= 0.01, ("the test's data breaks its own condition", cpu.max(), (cpu > 0).mean())
    ld = K + (3 if (N, K, r) == SHAPES[0] else 8)          # + 3: rows aligned to nothing (the guarded path); + 8: the 4-element path
    g = torch.Generator().manual_seed(7)
    buf = fused(N, K, ld, W, g)
    dbuf = buf.to(DEV)
    # factors with row strides of their own
    Ud = torch.zeros(N, r + 3, dtype=U.dtype, device=DEV)[:, :r].copy_(U)
    Dd = torch.zeros(r, K + 5, dtype=D.dtype, device=DEV)[:, :K].copy_(D)
    H.lora_merge(dbuf[3:3 + N, :K], Ud, Dd, s)
    out = dbuf.cpu()
    steps = LR.steps_apart(out[3:3 + N, :K], want, fmt)
    print(f"N={N} K={K} r={r} {fmt} <- {ffmt}: worst {steps.max():.0f} ulp, {(steps > 0).mean() * 100:.3f} % differ (CPU fp32 order: {(cpu > 0).mean() * 100:.3f} %)")
    assert steps.max() <= 1 and (steps > 0).mean() <= 0.01
    mask = torch.ones(N + 5, ld, dtype=torch.bool)
    mask[3:3 + N, :K] = False
    assert torch.equal(bits(out)[mask], bits(buf)[mask]), "elements outside the row range changed"
    assert not same(out[3:3 + N, :K], W)


@pytest.mark.parametrize("ffmt", ["f32", "bf16"])
@pytest.mark.parametrize("fmt", ["f32", "bf16", "e4m3"])
@pytest.mark.parametrize("N,K,r", [(130, 264, 5), (96, 160, 300)])
def test_generic_data_follows_the_stated_order_bit_for_bit(N, K, r, fmt, ffmt):
    """Plain normal draws, where no fp32 sum is exact: the result is the header's chain -- acc = fma(U[n][j], D[j][k], acc) from 0
    with j ascending, fma(s, acc, W), one conversion to the storage type -- bit for bit (LR.kernel_order; the draws are such that
    none of its emulated fmas rounds close enough to a tie to be in doubt, which is checked first).  Another order of the sum, a
    separate multiply and add, or a second rounding would differ on a large part of the fp32 elements."""
    from flexam_amd import hip as H
    g = torch.Generator().manual_seed(300 + N + r)
    U, D = torch.randn(N, r, generator=g).to(LR.TORCH[ffmt]), (torch.randn(r, K, generator=g) * 0.05).to(LR.TORCH[ffmt])
    W = (torch.randn(N, K, generator=g) * (2.0 if fmt == "e4m3" else 0.05)).to(LR.TORCH[fmt])
    doubt = [0]
    want = LR.kernel_order(W, U, D, 0.37, doubt=doubt)
    assert doubt[0] == 0, "the test's draws leave an emulated fma in doubt"
    got = H.lora_merge(W.to(DEV), U.to(DEV), D.to(DEV), 0.37).cpu()
    differ = int((bits(got) != bits(want)).sum())
    print(f"N={N} K={K} r={r} {fmt} <- {ffmt}: {differ} of {N * K} elements differ from the stated order")
    assert differ == 0
    if fmt == "f32" and r == 300:                                     # the test can tell orders apart: descending j is another result
        assert not same(LR.kernel_order(W, U.flip(1), D.flip(0), 0.37), want)


@pytest.mark.parametrize("fmt", ["bf16", "f32", "e4m3"])
@pytest.mark.parametrize("N,K,r,s", [(130, 264, 5, 0.5), (96, 160, 300, 0.125)])
def test_integer_data_is_exact_in_any_order(N, K, r, s, fmt):
    """W in -4 .. 4, U and D in {-1, 0, 1}, s a power of two: every partial sum is exact in fp32, so the result is the exact sum
    rounded to the storage type once (at r = 5 the sum itself: representable in all three), bit for bit."""
    from flexam_amd import hip as H
    g = torch.Generator().manual_seed(N)
    W = torch.randint(-4, 5, (N, K), generator=g).float().to(LR.TORCH[fmt])
    U, D = torch.randint(-1, 2, (N, r), generator=g).float(), torch.randint(-1, 2, (r, K), generator=g).float()
    x = LR.exact(W, U, D, s)
    want = LR.to_storage(LR.round_to(x, fmt), fmt)
    if r == 5:
        assert np.array_equal(LR.f64(want), x)
    for ft in (F32, BF):
        got = H.lora_merge(W.to(DEV), U.to(DEV, ft), D.to(DEV, ft), s).cpu()
        assert same(got, want), (fmt, ft)
        back = H.lora_merge(got.to(DEV), U.to(DEV, ft), D.to(DEV, ft), -s).cpu()
        if r == 5:
            assert same(back, W), "unmerge of an exact merge"


def test_e4m3_results_beyond_448_saturate():
    from flexam_amd import hip as H
    W = torch.tensor([[400.0, -400.0, 448.0, 1.0]] * 2).to(F8).to(DEV)
    U, D = torch.ones(2, 1, device=DEV), torch.tensor([[100.0, -100.0, 64.0, 1e6]], device=DEV)
    got = H.lora_merge(W, U, D, 1.0).float().cpu()
    assert torch.equal(got, torch.tensor([[448.0, -448.0, 448.0, 448.0]] * 2))


# ----------------------------------------------------------------------------- the reference's results
def run_case(c, style=None, strict=False):
    from flexam_amd import merge_lora
    lora = c["lora"]
    if style is not None and style != c["style"]:                       # the same adapter under another style's names
        lora = {}
        for layer in c["layers"]:
            for elem in ("lora_up.weight", "lora_down.weight", "alpha"):
                k = LR.spell(layer, elem, c["style"])
                if k in c["lora"] and not (elem == "alpha" and style == "peft"):
                    lora[LR.spell(layer, elem, style)] = c["lora"][k]
    model = LR.tree(c["before"]).to(DEV)
    pipe = LR.Pipe(model)
    assert merge_lora(pipe, None, c["multiplier"], device="cpu", dtype=LR.TORCH[c["dtype_fmt"]], state_dict=lora, transformer_only=True,
                      strict=strict) is pipe
    return pipe, lora


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[9:-12] for p in CASES])
def test_merge_lora_matches_the_reference_within_its_bounds(path, capsys):
    from flexam_amd import unmerge_lora
    c = LR.load_case(path)
    s = c["multiplier"] * (c["alpha"] / c["rank"] if c["alpha"] is not None else 1.0)
    pipe, lora = run_case(c)
    printed = capsys.readouterr().out
    assert [m in printed for m in c["missing"]] == [True] * len(c["missing"]) and len(printed.strip().splitlines()) == len(c["missing"])
    got = {n: m.weight.data.cpu().clone() for n, m in pipe.transformer.named_modules() if hasattr(m, "weight")}
    for n, w0 in c["before"].items():
        if n not in c["layers"]:
            assert same(got[n], w0), f"{n} is not in the adapter"
    for layer in c["layers"]:
        up = c["lora"][LR.spell(layer, "lora_up.weight", c["style"])].flatten(1)
        down = c["lora"][LR.spell(layer, "lora_down.weight", c["style"])].flatten(1)
        w0, w1 = c["before"][layer].flatten(1), c["after"][layer].flatten(1)
        _, bound = LR.reference_bound(w0, up, down, s, c["dtype_fmt"], c["w_fmt"])
        err = np.abs(LR.f64(got[layer].flatten(1)) - LR.f64(w1))
        assert got[layer].dtype == w1.dtype and got[layer].shape == c["after"][layer].shape
        assert (err <= bound).all(), (layer, float((err / bound).max()))
        # and against the kernel's own contract: the factors cast to dtype, then one rounding
        u, d = LR.cast_factors(up, down, c["dtype_fmt"])
        assert LR.steps_apart(got[layer].flatten(1), LR.merged(w0, u, d, s), c["w_fmt"]).max() <= 1
    # the other two spellings of the same adapter: the same launches, so the same bits (alpha has no PEFT spelling)
    for style in ("kohya", "comfy", "peft"):
        if style != c["style"] and not (style == "peft" and c["alpha"] is not None):
            other, _ = run_case(c, style)
            assert all(same(m.weight.data.cpu(), got[n]) for n, m in other.transformer.named_modules() if hasattr(m, "weight")), style
    capsys.readouterr()
    if c["missing"]:
        with pytest.raises(KeyError, match=c["missing"][0]):
            run_case(c, strict=True)
    # unmerge: within one storage ulp, taken at max(|W|, |W'|), of the start (every case: the kernel never casts the layer)
    assert unmerge_lora(pipe, None, c["multiplier"], device="cpu", dtype=LR.TORCH[c["dtype_fmt"]], state_dict=lora,
                        transformer_only=True) is pipe
    for layer in c["layers"]:
        w0, w2 = c["before"][layer], dict(pipe.transformer.named_modules())[layer].weight.data.cpu()
        lim = LR.ulp(np.maximum(np.abs(LR.f64(w0)), np.abs(LR.f64(got[layer]))), c["w_fmt"])
        assert (np.abs(LR.f64(w2) - LR.f64(w0)) <= lim).all(), layer


def test_merge_lora_reads_the_adapter_file_and_refuses_what_it_does_not_do(tmp_path):
    from safetensors.torch import save_file
    from flexam_amd import merge_lora
    c = LR.load_case(os.path.join(GOLDEN, "g16_lora_kohya_f32_bf16w.safetensors"))          # the case with a lora_te key
    path = str(tmp_path / "adapter.safetensors")
    save_file({k: v.contiguous() for k, v in c["lora"].items()}, path)
    a = LR.Pipe(LR.tree(c["before"]).to(DEV))
    merge_lora(a, path, c["multiplier"], dtype=LR.TORCH[c["dtype_fmt"]], transformer_only=True)
    b, _ = run_case(c)
    assert all(same(x.data, y.data) for x, y in zip(a.transformer.parameters(), b.transformer.parameters()))
    with pytest.raises(NotImplementedError, match="text-encoder LoRA"):
        merge_lora(LR.Pipe(LR.tree(c["before"]).to(DEV)), path, 1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        merge_lora(LR.Pipe(LR.tree(c["before"])), path, 1.0, transformer_only=True)          # CPU weights: no eager fallback


# ----------------------------------------------------------------------------- coherence with the engine
TOUCHED = ["blocks.0.self_attn.q", "blocks.0.self_attn.k", "blocks.0.self_attn.v", "blocks.0.self_attn.o", "blocks.0.cross_attn.k",
           "blocks.0.cross_attn.v", "blocks.1.cross_attn.k", "blocks.1.cross_attn.v", "blocks.1.ffn.0", "blocks.1.ffn.2"]
RANK, SCALE = 4, 2.0 ** -8


def dit_model(mode, sd):
    from flexam_amd import Wan2_2Transformer3DModel_FlexAM, convert_model_weight_to_float8, convert_weight_dtype_wrapper
    from oracle import dit as O
    kw = dict(O.DIT_TINY)
    kw.pop("eps")
    m = Wan2_2Transformer3DModel_FlexAM(**kw)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    if mode != "fp32":
        m = m.to(BF)
    if mode == "fp8gemm":
        m.enable_fp8_gemm(True)
    if mode == "qfloat8":
        convert_model_weight_to_float8(m, exclude_module_name=["modulation"], device=DEV)
        convert_weight_dtype_wrapper(m, BF)
    return m


def dyadic_adapter(sd):
    """Integer factors in -2 .. 2 under kohya names; with s = 2^-8 every product, partial sum and the closing fma are exact in fp32."""
    g = torch.Generator().manual_seed(11)
    lora = {}
    for name in TOUCHED:
        n, k = sd[name + ".weight"].shape
        lora[LR.spell(name, "lora_up.weight", "kohya")] = torch.randint(-2, 3, (n, RANK), generator=g).float()
        lora[LR.spell(name, "lora_down.weight", "kohya")] = torch.randint(-2, 3, (RANK, k), generator=g).float()
    return lora


@pytest.fixture(scope="module")
def dit_inputs():
    from oracle import cases as C
    from oracle import dit as O
    cfg = dict(O.DIT_TINY)
    case = C.dit_case(cfg, 41)
    dcase = {k: ([u.to(DEV) for u in v] if isinstance(v, list) else (v.to(DEV) if torch.is_tensor(v) else v)) for k, v in case.items()}
    return C.dit_weights(cfg, 7), dcase


@pytest.mark.parametrize("mode", ["bf16", "fp32", "fp8gemm", "qfloat8"])
def test_forward_after_a_merge_equals_a_model_loaded_from_the_merged_weights(dit_inputs, mode):
    """bf16 parameters (packs share their storage), fp32 parameters (packs are copies), enable_fp8_gemm (e4m3 operand copies) and
    qfloat8 storage (e4m3 parameters).  Without merge_lora's closing invalidate_engine() the second forward serves the old per-clip
    cross K|V (every mode), the old copies (fp32) or the old e4m3 operands (fp8gemm)."""
    from flexam_amd import merge_lora
    sd, case = dit_inputs
    a = dit_model(mode, sd)
    before = {k: v.detach().cpu().clone() for k, v in a.state_dict().items()}
    lora = dyadic_adapter(before)
    want = dict(before)
    for name in TOUCHED:
        w = before[name + ".weight"]
        u, d = lora[LR.spell(name, "lora_up.weight", "kohya")], lora[LR.spell(name, "lora_down.weight", "kohya")]
        want[name + ".weight"] = LR.merged(w, u, d, SCALE)
        assert same(LR.kernel_order(w, u, d, SCALE), want[name + ".weight"]) and not same(w, want[name + ".weight"])
    y0 = a(**case).clone()
    merge_lora(LR.Pipe(a), None, SCALE, device=DEV, dtype=F32, state_dict=lora)
    y1 = a(**case).clone()
    b = dit_model(mode, sd)
    b.load_state_dict(want, strict=True)
    got, ref = a.state_dict(), b.state_dict()
    assert list(got) == list(ref)
    for k in ref:
        assert same(got[k].cpu(), ref[k].cpu()) and same(ref[k].cpu(), want[k]), k
    y2 = b(**case)
    assert bool(torch.isfinite(y2.float()).all()) and not torch.equal(y0, y2)
    assert same(y1, y2), f"{mode}: max |diff| {float((y1.float() - y2.float()).abs().max()):.3e}"


# ----------------------------------------------------------------------------- ABI errors
def test_lora_merge_argument_errors():
    """The C side returns its documented codes without launching (W keeps its bits); the host mirror raises on what C cannot see."""
    from flexam_amd import abi
    from flexam_amd import hip as H
    E_ARG, E_SHAPE = abi.CONSTANTS["FLEXAM_E_ARG"], abi.CONSTANTS["FLEXAM_E_SHAPE"]
    lib = H.load_library()
    w = torch.ones(8, 8, dtype=BF, device=DEV)
    u, d = torch.ones(8, 2, device=DEV), torch.ones(2, 8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    W, U, D = w.data_ptr(), u.data_ptr(), d.data_ptr()
    call = lambda *a: lib.flexam_lora_merge(*a, st)
    assert call(None, 0, 8, 8, 8, U, 1, 2, D, 1, 8, 2, 1.0) == E_ARG and b"null" in lib.flexam_last_error()
    assert call(W, 0, 8, 8, 8, None, 1, 2, D, 1, 8, 2, 1.0) == E_ARG
    assert call(W, 0, 8, 8, 8, U, 1, 2, None, 1, 8, 2, 1.0) == E_ARG
    assert call(W, 0, 8, 8, 8, U, 1, 2, D, 1, 8, 0, 1.0) == E_SHAPE                       # r = 0
    assert call(W, 0, 8, 0, 8, U, 1, 2, D, 1, 8, 2, 1.0) == E_SHAPE                       # N = 0
    assert call(W, 0, 4, 8, 8, U, 1, 2, D, 1, 8, 2, 1.0) == E_SHAPE                       # row stride shorter than the row
    assert call(W, 0, 8, 8, 8, U, 1, 2, D, 0, 8, 2, 1.0) == E_ARG and b"both" in lib.flexam_last_error()    # fp32 up, bf16 down
    assert call(W, 0, 8, 8, 8, U, 2, 2, D, 2, 8, 2, 1.0) == E_ARG                         # e4m3 factors
    assert call(W, 7, 8, 8, 8, U, 1, 2, D, 1, 8, 2, 1.0) == E_ARG and b"storage code" in lib.flexam_last_error()
    torch.cuda.synchronize()
    assert bool((w == 1).all())
    with pytest.raises(RuntimeError, match="both be float32 or both bf16"):
        H.lora_merge(w, u, d.to(BF), 1.0)
    with pytest.raises(RuntimeError, match="needs up"):
        H.lora_merge(w, torch.ones(4, 2, device=DEV), d, 1.0)
    with pytest.raises(RuntimeError, match="contiguous rows"):
        H.lora_merge(w.t(), u, d, 1.0)
    with pytest.raises(RuntimeError, match="2-D GPU tensor"):
        H.lora_merge(w.cpu(), u, d, 1.0)
    with pytest.raises(RuntimeError, match="stored as"):
        H.lora_merge(w.to(torch.float16), u, d, 1.0)
    assert bool((w == 1).all())
