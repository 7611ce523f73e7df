"""GPU: the reference's qfloat8 modes (comfyui/wan2_2_fun_flexam/nodes.py:327-343 -> flexam_amd.fp8_optimization) on a 3-layer model
at 5B width (d = 3072, 24 heads, ffn 14336).  Two copies of one seeded bf16 model:
  (a) `convert_model_weight_to_float8` and every e4m3 parameter upcast back to bf16 -- the bf16 path on the rounded weights;
  (b) the same conversion + `convert_weight_dtype_wrapper(model, bf16)` -- the block GEMMs read the e4m3 parameters themselves.
e4m3 -> bf16 is exact, so (b) must equal (a) bit for bit on every path (sampler, module seam, fp8 GEMM mode), while holding no bf16
copy of a block matrix."""
import types

import pytest
import torch

from oracle import cases as C
from oracle import dit as O

pytestmark = pytest.mark.gpu
BF, F8 = torch.bfloat16, torch.float8_e4m3fn
CFG = dict(O.DIT_5B, num_layers=3, text_len=64)     # 64 text rows: the per-clip cross K|V of 3 layers stays small next to the weights
NONBLOCK_PACKS = ("pe_w", "pe_b", "ref_w", "ref_b", "head_w", "head_b", "txt", "time", "dens", "hmod", "hmdens", "mod", "mdens", "cnn")
BLOCK_GEMMS = ("wqkv", "wo", "cwq", "cwkv", "cwo", "w1", "w2")


def make(seed, qfloat8):
    from flexam_amd import Wan2_2Transformer3DModel_FlexAM, convert_model_weight_to_float8, convert_weight_dtype_wrapper
    kw = dict(CFG)
    kw.pop("eps")
    torch.manual_seed(seed)
    with torch.device("cuda:0"):
        m = Wan2_2Transformer3DModel_FlexAM(**kw)
    m.randomize_zero_init(seed=seed)
    m = m.to(BF)
    convert_model_weight_to_float8(m, exclude_module_name=["modulation"], device="cuda:0")
    if qfloat8:
        convert_weight_dtype_wrapper(m, BF)
    else:
        for p in m.parameters():
            if p.dtype == F8:
                p.data = p.data.to(BF)
    return m


@pytest.fixture(scope="module")
def models():
    return make(0, False), make(0, True)


def case():
    return {k: ([u.cuda() for u in v] if isinstance(v, list) else (v.cuda() if torch.is_tensor(v) else v))
            for k, v in C.dit_case(CFG, 5, frames=2, h=8, w=8).items()}


def same(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def block_weight_bytes(m):
    return sum(p.numel() * p.element_size() for n, p in m.blocks.named_parameters() if n.endswith(".weight") and p.dim() == 2)


def _tensors(obj, out):
    if torch.is_tensor(obj):
        out.append(obj)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _tensors(v, out)
    elif isinstance(obj, dict):
        for v in obj.values():
            _tensors(v, out)
    elif hasattr(obj, "__dict__") and not isinstance(obj, torch.nn.Module):
        _tensors(vars(obj), out)
    return out


def test_qfloat8_storage_and_memory_of_the_first_forward(models):
    """Every block GEMM weight the engine uses is e4m3 and lies inside the parameters' own storage, and across the first forward
    (packing + run at a small L) torch.cuda.max_memory_allocated grows by less than 10 % of the e4m3 block-weight bytes once the
    engine's packs of the weights OUTSIDE the blocks (embeddings, head, conv taps, biases, norm and modulation rows: upcast once, DESIGN.md
    section 4) are set aside.  A bf16 copy of the blocks would be 200 % of them."""
    from flexam_amd import hip
    _, mb = models
    assert mb.dtype == BF and all(p.dtype == F8 for n, p in mb.blocks.named_parameters() if "modulation" not in n)
    wbytes = block_weight_bytes(mb)
    assert wbytes > 3 * 150e6
    d = case()
    hip.gemm(torch.zeros(64, 64, device="cuda:0", dtype=BF), torch.zeros(64, 64, device="cuda:0", dtype=BF))   # GEMM scratch exists already
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = mb(**d)
    torch.cuda.synchronize()
    peak, held = torch.cuda.max_memory_allocated() - base, torch.cuda.memory_allocated() - base
    print(f"e4m3 block weights {wbytes / 1e6:.0f} MB; first forward: peak +{peak / 1e6:.0f} MB, kept +{held / 1e6:.0f} MB")
    eng = mb.engine()
    assert eng.fused and len(eng.blocks) == 3
    storages = {p.untyped_storage().data_ptr() for p in mb.parameters()}
    for pk in eng.blocks:
        for name in BLOCK_GEMMS:
            assert pk[name].dtype == F8 and pk[name].untyped_storage().data_ptr() in storages, name
    kept_blocks = sum(t.numel() * t.element_size() for pk in eng.blocks for t in pk.values()
                      if torch.is_tensor(t) and t.is_cuda and t.untyped_storage().data_ptr() not in storages)
    assert kept_blocks < 0.02 * wbytes, kept_blocks               # biases / norm rows only
    seen, nonblock = set(), 0
    for t in _tensors([getattr(eng, a, None) for a in NONBLOCK_PACKS], []):
        ptr = t.untyped_storage().data_ptr()
        if t.is_cuda and ptr not in storages and ptr not in seen:
            seen.add(ptr)
            nonblock += t.untyped_storage().nbytes()
    print(f"non-block weight packs {nonblock / 1e6:.0f} MB; growth beyond them {(peak - nonblock) / 1e6:.0f} MB")
    assert nonblock < 0.6 * wbytes, nonblock                      # (3 layers: the non-block parameters are a third of the blocks' count)
    assert peak - nonblock < 0.10 * wbytes, (peak, nonblock, wbytes)
    assert peak - held < 0.10 * wbytes, (peak, held, wbytes)
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("replay", ["1", "0"])
def test_sampler_latents_bit_identical(models, monkeypatch, replay):
    """3 Euler steps with CFG, per-token timesteps and a foreground mask through Wan2_2FunControlPipeline_FlexAM, with recorded launch
    plans (FLEXAM_REPLAY=1, the default) and without."""
    from flexam_amd import Wan2_2FunControlPipeline_FlexAM
    from flexam_amd.pipeline_wan2_2_fun_control_FlexAM import LatentConditioning
    monkeypatch.setenv("FLEXAM_REPLAY", replay)
    sc = C.sampler_case(CFG)
    cond = LatentConditioning(sc["control_latents"], sc["additional_control"], sc["masked_video_latents"], sc["ref_latents"], sc["mask_pixels"])
    outs = []
    for m in models:
        pipe = Wan2_2FunControlPipeline_FlexAM(transformer=m)
        trace = []
        out = pipe(prompt_embeds=sc["context_cond"], negative_prompt_embeds=sc["context_uncond"], height=256, width=256, num_frames=9,
                   num_inference_steps=3, guidance_scale=6.0, density=0.1, latents=sc["latents"], conditioning=cond, output_type="latent",
                   callback_on_step_end=lambda p, i, t, kw: trace.append(kw["latents"].float().cpu().clone()))
        assert len(trace) == 3
        outs.append((out.videos.float().cpu(), trace))
    (va, ta), (vb, tb) = outs
    assert all(torch.equal(x, y) for x, y in zip(ta, tb)) and torch.equal(va, vb)
    assert bool(torch.isfinite(vb).all())


class _Wrap(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x, **kw):
        return self.inner(x, **kw)


def test_replaced_and_rebound_blocks_bit_identical(models):
    """The module path (a wrapped block, a re-bound self-attention forward: HipLinear / _Block / _SelfAttn called as modules)."""
    d = case()

    def delegating(self, x, seq_lens, grid_sizes, freqs, dtype=torch.bfloat16, t=0):
        return type(self).forward(self, x, seq_lens, grid_sizes, freqs, dtype, t=t)
    h = torch.randn(40, CFG["dim"], device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(9)).to(BF)
    outs = []
    for m in models:
        m.blocks[1] = _Wrap(m.blocks[1])
        m.blocks[2].self_attn.forward = types.MethodType(delegating, m.blocks[2].self_attn)
        try:
            assert not m.engine().fused
            outs.append(m(**d))
            # a block's projections called as modules
            outs.append(m.blocks[0].ffn[0](h))
            outs.append(m.blocks[0].cross_attn.o(h))
        finally:
            m.blocks[1] = m.blocks[1].inner
            del m.blocks[2].self_attn.forward
        assert m.engine().fused
    for what, x, y in zip(("model, wrapped + re-bound blocks", "ffn[0] as a module", "cross_attn.o as a module"), outs[:3], outs[3:]):
        assert same(x, y), what
    assert models[1].blocks[0].ffn[0].packed()[0].dtype == F8


def test_fp8_gemm_mode_and_state_dict_round_trip(models):
    """enable_fp8_gemm(True) on (b) equals it on (a) (weights upcast one matrix at a time for the per-channel quantisation); the state
    dict of (b) -- reference keys, e4m3 tensors, q|k|v aliased into one fused e4m3 buffer -- loads into another converted model, which
    keeps e4m3 storage and computes the same."""
    ma, mb = models
    d = case()
    outs = []
    for m in models:
        m.enable_fp8_gemm(True)
        try:
            outs.append(m(**d))
        finally:
            m.enable_fp8_gemm(False)
    assert same(outs[0], outs[1])
    ref = mb(**d)
    sd = mb.state_dict()
    assert list(sd) == list(ma.state_dict())
    assert all((v.dtype == BF) if "modulation" in k else (v.dtype == F8) for k, v in sd.items())
    q, k = mb.blocks[0].self_attn.q.weight, mb.blocks[0].self_attn.k.weight
    assert q.untyped_storage().data_ptr() == k.untyped_storage().data_ptr()        # aliased by the pack
    mc = make(1, True)
    mc(**d)                                                                          # packed (aliased) before the load
    mc.load_state_dict(sd, strict=True)
    assert all(p.dtype == F8 for n, p in mc.named_parameters() if "modulation" not in n)
    assert same(mc(**d), ref)
    eng = mc.engine()
    assert all(pk[name].dtype == F8 for pk in eng.blocks for name in BLOCK_GEMMS)
    del mc, eng


def test_narrow_e4m3_holder_called_as_module_falls_back_to_bf16():
    """A Linear holder whose width the e4m3 GEMM has no plan for (N = 64, e.g. a narrow head) keeps a bf16 copy when called as a
    module, as before qfloat8; a block-width holder reads its e4m3 weight."""
    from flexam_amd.wan_transformer3d_FlexAM import HipLinear
    g = torch.Generator(device="cuda:0").manual_seed(4)
    x = torch.randn(50, 256, device="cuda:0", generator=g).to(BF)
    for n, keeps_f8 in ((64, False), (160, False), (320, False), (3072, True)):
        lin8, lin16 = HipLinear(256, n).cuda(), HipLinear(256, n).cuda()
        w8 = (torch.randn(n, 256, device="cuda:0", generator=g) * 0.1).to(F8)
        lin8.weight.data, lin16.weight.data = w8, w8.to(BF)
        lin16.bias.data = lin8.bias.data.clone()
        assert (lin8.packed()[0].dtype == F8) == keeps_f8, n
        assert same(lin8(x), lin16(x)), n
