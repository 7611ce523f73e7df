"""GPU: no engine or wrapper result depends on bytes that no launch wrote.

The package allocates its activations, exchange buffers, rings and scratch with torch.empty and relies on every launch writing what a
later launch reads.  Here every workload runs four times with tests/scratch_poison.py around it -- under 0x00 twice (it must repeat
bit for bit at all), then under 0x7B (huge but finite in every format read here), then under 0xFF (NaN in every one) -- with models and
engines BUILT inside the patched region, and every documented output must be torch.equal to the 0x00 run.  Where an existing test holds
the workload to an oracle or a golden file, its check is applied to the 0x00 run, so "equal" is not "equally wrong".  Between two steps
of one DiT engine the workspaces are poisoned again in place (poison_tensors): the replayed step must give the first step's bits.

Integer index buffers are never poisoned (scratch_poison's stated limit).  Nothing is asserted about timing.  The last test holds the
union of the package's allocation sites poisoned in this module's runs against the GPU-free census (NOT_REACHED lists the exceptions).

Allocations / bytes poisoned per workload and pattern run, as measured on an MI355X (recorded, not asserted; `pytest -s` prints them):
  workload                                  allocations    bytes      workload                          allocations    bytes
  dit bf16 / qfloat8 / window / window-sage          53    76.2 MB    sampler (4 steps)                          45    72.8 MB
  dit fp8gemm                                        81    78.0 MB    emulated cfg-parallel rank                 50    75.3 MB
  dit ragged (105 tokens)                            53    70.9 MB    history (5x16x24, then 3x16x16)            95    96.4 MB
  dit sage-smooth (256 tokens)                       57    76.3 MB    vae decode (twice)                        127   110.5 MB
  dit sage-ragged                                    57    70.9 MB    vae decode, 9 frames                      165    88.6 MB
  3 ranks: K|V gather, waited / overlapped           58    77.5 MB    vae tiled decode, world 2                 189   132.8 MB
  3 ranks: one piece; + frame window                 58    78.0 MB    vae parallel decode, 3 ranks               69    87.9 MB
  3 ranks: record gather (SAGE)                      55    78.1 MB    vae encode                                 73    68.7 MB
  3 ranks: all-to-all over heads (3 heads)           74    84.4 MB    text encoder                               18    68.2 MB
  3 ranks: halo exchange, frames / tokens            60    80.9 MB    wrappers: attention                        15     7.9 MB
  lora merge / unmerge                              127    92.6 MB    wrappers: GEMMs and row kernels            18    85.9 MB
  raster + colour tables                             18     0.7 MB    motion (MoGe + VGGT routes)                30     2.3 MB
  edit masks                                          3    0.06 MB    frames                                      4     1.2 MB
(FLEXAM_REPLAY=0 and 1 allocate alike; each count includes the 64 MiB tail split-K scratch where a GEMM runs.)  52 of the 56
allocation sites of the covered modules are poisoned, three are integer-only and one is CPU parameter construction; nothing differed.
"""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scratch_poison as SPZ  # noqa: E402
import test_sp_gpu as SP  # noqa: E402
import test_sp_window_gpu as W  # noqa: E402
from scratch_poison import FINITE, NAN, ZERO, poison_tensors, poisoned  # noqa: E402
from oracle import cases as C  # noqa: E402
from oracle import dit as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
ORDER = (ZERO, ZERO, FINITE, NAN)                   # repeatable at all, then 0x7B BEFORE 0xFF

_SITES = set()                                      # (file, function) of every package allocation poisoned by this module's runs
_INTEGER_SITES = set()                              # ... and of those seen on the GPU and left alone for their integer dtype
_STATS = {}                                         # workload -> (allocations, bytes) of one pattern run
_RAN = set()


def _to_dev(case):
    return {k: ([u.to(DEV) for u in v] if isinstance(v, list) else (v.to(DEV) if torch.is_tensor(v) else v)) for k, v in case.items()}


def _fresh_scratch():
    """The wrappers' per-(device, stream) scratch (tail split-K slabs, split-KV partials) is cached for the process: dropped here, so
    that every pattern run allocates -- and poisons -- its own."""
    from flexam_amd import hip
    torch.cuda.synchronize()
    hip._GEMM_WS.clear()
    hip._ATTN_WS.clear()


def _describe(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape / dtype {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
    af, bf = a.double(), b.double()
    bad = ~((af == bf) | (torch.isnan(af) & torch.isnan(bf)))
    first = bad.flatten().nonzero()[:4].flatten().tolist()
    return (f"{int(bad.sum())} of {a.numel()} elements differ (first flat indices {first}); NaN {int(torch.isnan(af).sum())} vs "
            f"{int(torch.isnan(bf).sum())}; max |a| {float(af[~torch.isnan(af)].abs().max()) if (~torch.isnan(af)).any() else float('nan'):.4g}")


def independent(name, work, aimed, monkeypatch, check=None):
    """work(byte) -> {label: CPU tensor}, everything it builds built inside.  Runs it under ORDER, asserts what the module's docstring
    says, records sites and counts.  aimed: package files that must have allocated (a run that poisoned nothing proves nothing).
    check(outputs of the first 0x00 run): the existing test's oracle / golden comparison."""
    base = None
    for i, byte in enumerate(ORDER):
        _fresh_scratch()
        with poisoned(monkeypatch, byte) as p:
            out = work(byte)
            torch.cuda.synchronize()
        _SITES.update(p.sites)
        _INTEGER_SITES.update(p.integer_sites)
        assert set(aimed) <= p.files, f"{name}: under 0x{byte:02X} only {sorted(p.files)} allocated, aimed at {sorted(aimed)}"
        assert p.allocations > 0 and p.bytes > 0
        if base is None:
            base = out
            _STATS[name] = (p.allocations, p.bytes)
            print(f"{name}: {p.allocations} allocations, {p.bytes} bytes poisoned per run, {len(p.sites)} sites in {sorted(p.files)}")
            for k, v in out.items():
                assert v.device.type == "cpu" and (not v.dtype.is_floating_point or bool(torch.isfinite(v.float()).all())), f"{name}: {k} is not finite under 0x00"
            if check is not None:
                check(out)
            continue
        assert list(out) == list(base), name
        for k in base:
            what = "the second 0x00 run (not repeatable at all)" if i == 1 else f"0x{byte:02X}"
            assert torch.equal(out[k], base[k]), f"{name}: {k} under {what} differs from 0x00: {_describe(out[k], base[k])}"
    _RAN.add(name)
    return base


def test_the_harness_sees_a_leak_on_the_gpu(monkeypatch):
    """Not blind here either: a torch-level leak on the GPU, and a launch of the package made to read what nothing wrote -- attn_merge
    told to merge eight slots of a workspace of which seven were written (in bounds: the eighth slot is allocated, and poisoned)."""
    from flexam_amd import hip
    g = torch.Generator().manual_seed(3)
    q, k, v = _randn(g, 1, 300, 2, 128), _randn(g, 1, 1111, 2, 128), _randn(g, 1, 1111, 2, 128)
    sums, merged = {}, {}
    for byte in (ZERO, FINITE, NAN):
        with poisoned(monkeypatch, byte) as p:
            buf = torch.empty(8, device=DEV)
            buf[:4] = 1.0
            sums[byte] = buf.sum().cpu()
            ws = hip.attn_partial_workspace(1, 2, 300, 8, q.device)
            n = 0
            for lo, hi, splits in ((0, 400, 3), (400, 1000, 3), (1000, 1111, 1)):
                n += hip.attn_fwd_partial(q, k[:, lo:hi], v[:, lo:hi], ws, n, splits)
            assert n == 7
            right = hip.attn_merge(torch.empty(1, 300, 2, 128, device=DEV, dtype=BF), ws, 7).float().cpu()
            merged[byte] = (right, hip.attn_merge(torch.empty(1, 300, 2, 128, device=DEV, dtype=BF), ws, 8).float().cpu())
        assert p.sites == {("hip.py", "_partials")} and p.allocations == 5
    assert float(sums[ZERO]) == 4.0 and float(sums[FINITE]) > 1e36 and bool(torch.isnan(sums[NAN]))
    assert torch.equal(merged[FINITE][0], merged[ZERO][0]) and torch.equal(merged[NAN][0], merged[ZERO][0])          # seven slots: independent
    assert not torch.equal(merged[FINITE][1], merged[ZERO][1]) or not torch.equal(merged[NAN][1], merged[ZERO][1])    # eight: the leak shows


# ----------------------------------------------------------------------------- DiT forward
_WEIGHTS = {}


def _dit_weights(cfg, seed, peaked=False):
    key = (tuple(sorted((k, str(v)) for k, v in cfg.items())), seed, peaked)
    if key not in _WEIGHTS:
        sd = C.dit_weights(cfg, seed)
        if peaked:
            C.scale_self_attention_logits(sd, W.LOGIT_STD)
        _WEIGHTS[key] = sd
    return _WEIGHTS[key]


def _dit(cfg, sd, **model_kw):
    from flexam_amd import Wan2_2Transformer3DModel_FlexAM
    kw = dict(cfg)
    kw.pop("eps")
    m = Wan2_2Transformer3DModel_FlexAM(**kw, **model_kw)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


SAGE = {"VIDEOX_ATTENTION_TYPE": "SAGE_ATTENTION"}
# variant -> (environment, model keywords, set-up, weights with peaked logits, case).  "ragged": tests/test_dit_gpu.py's
# test_dit_ragged_tokens_and_cfg_skip (105 tokens: row and key tails everywhere); every other one the 256-token case of seed 41
DIT_VARIANTS = {
    "bf16": ({}, {}, None, False),
    "ragged": ({}, {}, None, False),
    "fp8gemm": ({}, {}, "fp8gemm", False),
    "qfloat8": ({}, {}, "qfloat8", False),
    "sage-smooth": (dict(SAGE, FLEXAM_SAGE_SMOOTH_K="1", FLEXAM_SAGE_SMOOTH_V="1"), {}, None, False),
    "sage-ragged": (dict(SAGE, FLEXAM_SAGE_SMOOTH_K="1", FLEXAM_SAGE_SMOOTH_V="1"), {}, None, False),
    "window": ({}, dict(window_frames=(1, 0), window_sink=64), None, True),
    "window-sage": (dict(SAGE, FLEXAM_SAGE_WINDOW="1"), dict(window_frames=(1, 0), window_sink=64), None, True),
}
DIT_ENV = ("VIDEOX_ATTENTION_TYPE", "FLEXAM_SAGE_SMOOTH_K", "FLEXAM_SAGE_SMOOTH_V", "FLEXAM_SAGE_WINDOW", "FLEXAM_REPLAY", "FLEXAM_SP_WINDOW",
           "FLEXAM_SP_HALO", "FLEXAM_CROSS_DEDUP")
_ORACLE = {}


def _dit_oracle(variant):
    """The fp32 oracle of a variant that an existing test holds to it with test_dit_gpu.check (the same tolerance), once."""
    if variant not in _ORACLE:
        cfg = dict(O.DIT_TINY)
        if variant == "bf16":
            _ORACLE[variant] = O.dit_forward(_dit_weights(cfg, 7), cfg, **C.dit_case(cfg, 41))
        elif variant == "ragged":
            _ORACLE[variant] = O.dit_forward(_dit_weights(cfg, 23), cfg, **C.dit_case(cfg, 9, frames=2, h=10, w=14, batch=2, text_lens=(16, 1)))
        elif variant == "window":
            _ORACLE[variant] = W._want(False, "frames")
    return _ORACLE[variant]


@pytest.mark.parametrize("replay", ["1", "0"])
@pytest.mark.parametrize("variant", list(DIT_VARIANTS))
def test_dit_forward(variant, replay, monkeypatch):
    """Three forwards of one model: the second is a replay of the recorded plan (FLEXAM_REPLAY=1) or launch by launch again (0); before
    the third the engine's workspaces are poisoned in place.  All three the same bits, under every pattern."""
    import test_dit_gpu as TD
    from flexam_amd.dit_engine import DiTEngine
    env, model_kw, setup, peaked = DIT_VARIANTS[variant]
    for k in DIT_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("FLEXAM_REPLAY", replay)
    monkeypatch.setattr(DiTEngine, "_sage_window_warned", True)
    cfg = dict(O.DIT_TINY)
    ragged = variant.endswith("ragged")
    sd = _dit_weights(cfg, 23 if ragged else 7, peaked)
    case = C.dit_case(cfg, 9, frames=2, h=10, w=14, batch=2, text_lens=(16, 1)) if ragged else C.dit_case(cfg, 41)

    def work(byte):
        m = _dit(cfg, sd, **model_kw)
        if setup is not None:
            m = m.to(BF)
        if setup == "fp8gemm":
            m.enable_fp8_gemm(True)
        if setup == "qfloat8":
            from flexam_amd import convert_model_weight_to_float8, convert_weight_dtype_wrapper
            convert_model_weight_to_float8(m, exclude_module_name=["modulation"], device=DEV)
            convert_weight_dtype_wrapper(m, BF)
        d = _to_dev(case)
        first = m(**d).float().cpu()
        eng = m.engine()
        assert eng.fused and not eng.replay_taken and bool(eng.sage_taken) == ("sage" in variant)
        if variant.startswith("sage"):
            assert eng.sage_smooth_taken and eng.sage_smooth_v_taken
        second = m(**d).float().cpu()
        assert bool(eng.replay_taken) == (replay == "1")
        # Between steps.  What each holds (read in dit_engine.py): _ws -- the activations x / h / qkv / ao / ffn / head, the fp8 operand
        # rows and scales, the AdaLN tables (rewritten by mod_table in front of the plan) and the int32 row index (an integer: left
        # alone); _kmean / _vmean -- (mean, per-part scratch) of smooth-K / smooth-V, written by k_mean before the attention reads them.
        # None of it is meant to survive a forward.  _attn8, the MXFP8 operand buffers, DOES hold state when the token count is no
        # multiple of 256: the query rows and key records past L are allocated as ZEROS (hip.attn_fp8_buffers) and never written
        # again, which the kernels rely on (hip._check_fp8_bufs) -- so it is poisoned only where there is no such padding.
        held = [eng._ws, eng._kmean, eng._vmean]
        if eng.cond["L"] % 256 == 0:
            held.append(eng._attn8)
        n, size = poison_tensors(held, byte)
        assert n >= 6 and size > 0
        third = m(**d).float().cpu()
        assert bool(eng.replay_taken) == (replay == "1")
        assert torch.equal(second, first), f"second forward differs from the first: {_describe(second, first)}"
        assert torch.equal(third, first), f"forward after poisoning the workspaces differs from the first: {_describe(third, first)}"
        return dict(out=first)

    def check(out):
        if variant in ("bf16", "ragged", "window"):
            TD.check(out["out"], _dit_oracle(variant), f"dit {variant} under 0x00")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        independent(f"dit-{variant}-replay{replay}", work, {"dit_engine.py", "hip.py", "wan_transformer3d_FlexAM.py"}, monkeypatch, check)


# ----------------------------------------------------------------------------- sampler, history
def test_sampler_steps(monkeypatch):
    """tests/test_replay_gpu.py's four sampler steps of the CFG pair (three layers, block 0's self-attention half shared), the latents
    after every step."""
    from flexam_amd import Wan2_2FunControlPipeline_FlexAM
    from flexam_amd.pipeline_wan2_2_fun_control_FlexAM import LatentConditioning
    for k in DIT_ENV:
        monkeypatch.delenv(k, raising=False)
    cfg = dict(O.DIT_TINY, num_layers=3)
    sd = _dit_weights(cfg, 7)
    sc = C.sampler_case(cfg)

    def work(byte):
        m = _dit(cfg, sd)
        pipe = Wan2_2FunControlPipeline_FlexAM(transformer=m)
        cond = LatentConditioning(sc["control_latents"], sc["additional_control"], sc["masked_video_latents"], sc["ref_latents"], sc["mask_pixels"])
        steps, taken = {}, []

        def cb(p, i, t, k):
            steps[f"latents after step {i}"] = k["latents"].float().cpu().clone()
            taken.append((bool(m.engine().replay_taken), bool(m.engine().share0_taken)))
        pipe(prompt_embeds=sc["context_cond"], negative_prompt_embeds=sc["context_uncond"], height=256, width=256, num_frames=9,
             num_inference_steps=4, guidance_scale=6.0, density=0.1, latents=sc["latents"], conditioning=cond, output_type="latent",
             callback_on_step_end=cb)
        assert len(steps) == 4 and [t for t, _ in taken][1:] == [True] * 3 and all(s for _, s in taken)
        return steps

    def check(out):                                 # smoke()'s comparison of the same loop, on four steps
        from oracle import sampler as S
        ml, mask, pinned = S.prepare_masks(sc["mask_pixels"], sc["latents"])
        ref = S.denoise_loop(lambda **k: O.dit_forward(sd, cfg, **k), S.FlowMatchEulerSchedule(1000, 5.0), 4, sc["latents"], sc["context_uncond"],
                             sc["context_cond"], sc["control_latents"], sc["additional_control"], ml, sc["masked_video_latents"],
                             sc["ref_latents"], mask, pinned, 0.1, 6.0)
        p = C.psnr(out["latents after step 3"], ref)
        print(f"sampler, four steps against the fp32 oracle: {p:.1f} dB")
        assert p >= 40.0
    independent("sampler", work, {"dit_engine.py", "hip.py"}, monkeypatch, check)


def test_emulated_cfg_parallel_rank(monkeypatch):
    """tests/test_replay_gpu.py's emulated rank 1 of four, CFG-parallel (two CFG rows x two token chunks; LoopbackGroup: every collective
    a device copy of the real size on a side stream): the overlapped K|V gather in two head-group pieces with its partial softmaxes and
    merge, and the engine's gather of the head output over the world group.  Three sampler steps, the last two replayed."""
    from benchlib.emulate import set_emulated_layout
    from flexam_amd import Wan2_2FunControlPipeline_FlexAM
    from flexam_amd.pipeline_wan2_2_fun_control_FlexAM import LatentConditioning
    for k in DIT_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(FLEXAM_SP_MODE="allgather", FLEXAM_SP_OVERLAP="1", FLEXAM_SP_PIECES="2", FLEXAM_REPLAY="1").items():
        monkeypatch.setenv(k, v)
    cfg = dict(O.DIT_TINY, dim=512, num_heads=4, num_layers=2)
    sd = _dit_weights(cfg, 7)
    sc = C.sampler_case(cfg)

    def work(byte):
        m = _dit(cfg, sd)
        set_emulated_layout(m, 4, True, 1)
        pipe = Wan2_2FunControlPipeline_FlexAM(transformer=m)
        cond = LatentConditioning(sc["control_latents"], sc["additional_control"], sc["masked_video_latents"], sc["ref_latents"], sc["mask_pixels"])
        pipe.prepare(sc["latents"], cond, sc["context_cond"], sc["context_uncond"], density=0.1, guidance_scale=6.0, num_inference_steps=4)
        steps, taken = {}, []
        for i in range(3):
            pipe.denoise_step(i)
            torch.cuda.synchronize()
            steps[f"latents after step {i}"] = pipe._state["latents"].float().cpu().clone()
            taken.append(bool(m.engine().replay_taken))
        assert taken == [False, True, True] and m.engine().cfg_size == 2 and m.engine().sp_size == 2
        return steps
    independent("emulated-cfg-parallel", work, {"dit_engine.py", "dit_sp.py", "hip.py"}, monkeypatch)


def test_history_of_a_larger_clip_does_not_reach_the_next(monkeypatch):
    """One engine runs the (5, 16, 24) clip and then the (3, 16, 16) clip under 0xFF: its workspaces are dropped and re-made for the new
    shape, its caches hold the other clip's leftovers.  The second result must be a fresh engine's under 0x00."""
    for k in DIT_ENV:
        monkeypatch.delenv(k, raising=False)
    cfg = dict(O.DIT_TINY)
    sd = _dit_weights(cfg, 7)
    big, small = C.dit_case(cfg, 47, frames=5, h=16, w=24), C.dit_case(cfg, 41)
    for env in ({}, SAGE):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _fresh_scratch()
        with poisoned(monkeypatch, ZERO) as p0:
            want = _dit(cfg, sd)(**_to_dev(small)).float().cpu()
        _SITES.update(p0.sites)
        for byte in (FINITE, NAN):
            _fresh_scratch()
            with poisoned(monkeypatch, byte) as p:
                m = _dit(cfg, sd)
                other = m(**_to_dev(big)).float().cpu()
                m(**_to_dev(big))
                got = m(**_to_dev(small)).float().cpu()
                again = m(**_to_dev(small)).float().cpu()
                torch.cuda.synchronize()
            _SITES.update(p.sites)
            assert {"dit_engine.py", "hip.py"} <= p.files and bool(torch.isfinite(other).all())
            assert torch.equal(got, want), f"0x{byte:02X} {env}: after another clip {_describe(got, want)}"
            assert torch.equal(again, want) and m.engine().replay_taken and bool(m.engine().sage_taken) == bool(env)
    _STATS["history"] = (p.allocations, p.bytes)
    _RAN.add("history")


# ----------------------------------------------------------------------------- sequence parallelism: one world of three ranks over gloo
SW = {"FLEXAM_SP_WINDOW": "1"}
HALO = dict(SW, FLEXAM_SP_HALO="1")
# (heads or False = DIT_TINY, mask, mode as test_sp_gpu.set_mode_env spells it, switches).  256 tokens over 3 ranks: 258 padded rows,
# the last rank holds two pad rows (the record gather pads to whole key tiles: 384 rows, the last rank pads only)
SP_CASES = [
    (False, None, "allgather-wait", {}), (False, None, "allgather-wait-p1", {}), (False, None, "allgather", {}),
    (False, None, "allgather-wait-p1-sage", {}),
    (3, None, "ulysses-ov0", {}), (3, None, "ulysses-ov1", {}),
    (False, "frames", "allgather-wait-p1", SW), (3, "tokens", "ulysses-ov0", SW),
    (False, "frames", "allgather-wait-p1", HALO), (False, "tokens", "allgather-wait", HALO),
]
SP_SWITCHES = W.SWITCHES + ("FLEXAM_SP_HALO", "FLEXAM_SAGE_SMOOTH_K", "FLEXAM_SAGE_SMOOTH_V")


def _sp_key(case):
    heads, mask, mode, env = case
    return (heads, mask, mode, tuple(sorted(env.items())))


def _worker(rank, world, port, ret, cases, wide=False, backend="gloo"):
    """One rank: every case under every pattern, the patch applied inside the rank, models built inside it.
    ret[rank] = {key: [(byte, first output, facts) per pattern run] | error text}, plus "sites" and "stats"."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    mp = pytest.MonkeyPatch()
    try:
        from flexam_amd.dit_engine import DiTEngine
        results, sites, integer_sites, stats = {}, set(), set(), {}
        for case in cases:
            heads, mask, mode, env = case
            try:
                for name in SP_SWITCHES:
                    os.environ.pop(name, None)
                SP.set_mode_env(mode)
                os.environ.update(env)
                cfg = W._cfg(heads)
                sd = W._weights(cfg)
                runs = []
                for byte in ORDER:
                    _fresh_scratch()
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore", RuntimeWarning)
                        with poisoned(mp, byte) as p:
                            m = _dit(cfg, sd, **(W.MASKS[mask] if mask else {}))
                            m.enable_multi_gpus_inference(cfg_parallel=False)
                            d = W._inputs(cfg)
                            first = m(**d).float().cpu()
                            eng = m.engine()
                            facts = dict(sp=eng.sp_size, sp_mode=eng.sp_mode, fused=eng.fused, sage=bool(eng.sage_taken), halo_rows=eng.halo_rows,
                                         replayed_first=bool(eng.replay_taken))
                            second = m(**d).float().cpu()
                            facts.update(replayed_second=bool(eng.replay_taken), second_equal=bool(torch.equal(first, second)),
                                         files=sorted(p.files))
                            torch.cuda.synchronize()
                            del m, eng
                    runs.append((byte, first, facts))
                    sites |= p.sites
                    integer_sites |= p.integer_sites
                    stats[_sp_key(case)] = (p.allocations, p.bytes)
                results[_sp_key(case)] = runs
            except Exception as e:                             # noqa: BLE001  raised on every rank alike: the next case still runs
                import traceback
                results[_sp_key(case)] = f"{type(e).__name__}: {e}\n{traceback.format_exc()}"
        # the VAE's parallel decode over the same ranks: every rank decodes its tile, one all-gather assembles the clip
        try:
            import test_vae_gpu as TV
            z = C.vae_case(seed=56, frames=3, h=6, w=4)
            runs = []
            for byte in ORDER:
                _fresh_scratch()
                with poisoned(mp, byte) as p:
                    vae, _ = TV.build(seed=55)
                    vae.enable_parallel_decode()
                    video = vae.decode(z.to(DEV)).sample.float().cpu()
                    torch.cuda.synchronize()
                    del vae
                runs.append((byte, video, dict(files=sorted(p.files))))
                sites |= p.sites
                integer_sites |= p.integer_sites
                stats["vae-parallel"] = (p.allocations, p.bytes)
            results["vae-parallel"] = runs
        except Exception as e:                                 # noqa: BLE001
            import traceback
            results["vae-parallel"] = f"{type(e).__name__}: {e}\n{traceback.format_exc()}"
        results["sites"], results["integer_sites"], results["stats"] = sorted(sites), sorted(integer_sites), stats
        ret[rank] = results
    finally:
        mp.undo()
        dist.destroy_process_group()


_WORLD = []


def _world():
    """The one world of three ranks, spawned once per session (three processes in all)."""
    if not _WORLD:
        saved, SP._worker = SP._worker, _worker                  # run_world spawns test_sp_gpu._worker: this module's, for the call
        try:
            _WORLD.append(SP.run_world(3, SP_CASES))
        finally:
            SP._worker = saved
        for r in _WORLD[0]:
            _SITES.update(tuple(s) for s in r["sites"])
            _INTEGER_SITES.update(tuple(s) for s in r["integer_sites"])
    return _WORLD[0]


@pytest.mark.parametrize("case", SP_CASES, ids=[f"h{c[0] or 2}-{c[1]}-{c[2]}" + "".join("+" + k.split("_", 1)[1].lower() for k in sorted(c[3])) for c in SP_CASES])
def test_sequence_parallel_forward(case):
    heads, mask, mode, env = case
    per_rank = [r[_sp_key(case)] for r in _world()]
    for r in per_rank:
        assert not isinstance(r, str), r
    name = f"sp3-{mode}" + (f"-{mask}" if mask else "") + ("-halo" if "FLEXAM_SP_HALO" in env else "")
    for rank, runs in enumerate(per_rank):
        (_, base, facts0) = runs[0]
        assert bool(torch.isfinite(base).all())
        for i, (byte, out, facts) in enumerate(runs):
            assert facts["sp"] == 3 and facts["fused"] and facts["sp_mode"] == mode.split("-")[0]
            assert facts["second_equal"] and not facts["replayed_first"] and facts["replayed_second"], (rank, byte, facts)
            assert {"dit_engine.py", "dit_sp.py", "hip.py"} <= set(facts["files"]), facts["files"]
            assert ("FLEXAM_SP_HALO" in env) == (facts["halo_rows"] is not None)
            if i:
                what = "the second 0x00 run (not repeatable at all)" if i == 1 else f"0x{byte:02X}"
                assert torch.equal(out, base), f"{name}, rank {rank}: under {what} {_describe(out, base)}"
        assert torch.equal(base, per_rank[0][0][1])             # every rank returns the whole output, the same bits
    if "-sage" not in mode:                                      # the existing tests' oracle for the bf16 forms (test_sp_window_gpu / test_sp_gpu)
        import test_dit_gpu as TD
        cfg = W._cfg(heads)
        if not mask and ("sp", heads) not in _ORACLE:
            _ORACLE["sp", heads] = O.dit_forward(W._weights(cfg), cfg, **C.dit_case(cfg, 41))
        want = W._want(heads, mask) if mask else _ORACLE["sp", heads]
        TD.check(per_rank[0][0][1], want, name)
    _STATS[name] = _world()[0]["stats"][_sp_key(case)]
    _RAN.add(name)


def test_vae_parallel_decode_over_the_ranks():
    """AutoencoderKLWan3_8.enable_parallel_decode in the world above: three row bands of a [6, 4] latent, gathered into buffers the
    decode allocates without initialising."""
    import test_vae_gpu as TV
    from oracle import vae as OV
    per_rank = [r["vae-parallel"] for r in _world()]
    for r in per_rank:
        assert not isinstance(r, str), r
    for rank, runs in enumerate(per_rank):
        base = runs[0][1]
        for i, (byte, video, facts) in enumerate(runs):
            assert {"wan_vae3_8.py", "hip.py"} <= set(facts["files"])
            assert torch.equal(video, base), f"vae parallel decode, rank {rank}, run {i} under 0x{byte:02X}: {_describe(video, base)}"
        assert torch.equal(base, per_rank[0][0][1])
    z = C.vae_case(seed=56, frames=3, h=6, w=4)
    want = OV.vae_decode(C.vae_weights(C.VAE_SMALL, seed=55, prefix="model."), z, C.VAE_SMALL["temporal_up"], OV.LATENT_MEAN, OV.LATENT_STD)
    TV.check(per_rank[0][0][1], want, "vae parallel decode, three ranks, under 0x00")
    _STATS["vae-parallel-3"] = _world()[0]["stats"]["vae-parallel"]
    _RAN.add("vae-parallel-3")


# ----------------------------------------------------------------------------- VAE
def test_vae_decode(golden, monkeypatch):
    """tests/test_vae_gpu.py's golden decode ([1, 48, 3, 4, 6] -> 9 x 64 x 96), twice on one engine: the rings and guarded images keep
    their zeros and their history between the two calls and are not touched here."""
    import test_vae_gpu as TV
    z = C.vae_case(h=4, w=6)

    def work(byte):
        vae, _ = TV.build()
        first = vae.decode(z.to(DEV)).sample.float().cpu()
        again = vae.decode(z.to(DEV)).sample.float().cpu()
        assert torch.equal(first, again)
        return dict(video=first)
    independent("vae-decode", work, {"wan_vae3_8.py", "hip.py"}, monkeypatch, lambda out: TV.check(out["video"], golden("g7_vae_decode")["out"], "vae decode g7 under 0x00"))


def test_vae_decode_nine_frames_ring_wraps(monkeypatch):
    import test_vae_gpu as TV
    from oracle import vae as OV
    z = C.vae_case(seed=84, frames=9, h=2, w=4)

    def work(byte):
        vae, _ = TV.build(seed=83)
        return dict(video=vae.decode(z.to(DEV)).sample.float().cpu())

    def check(out):
        want = OV.vae_decode(C.vae_weights(C.VAE_SMALL, seed=83, prefix="model."), z, C.VAE_SMALL["temporal_up"], OV.LATENT_MEAN, OV.LATENT_STD)
        TV.check(out["video"], want, "vae decode 9 chunks under 0x00")
        TV.check(out["video"][:, :, -8:], want[:, :, -8:], "last two chunks")
    independent("vae-decode-9", work, {"wan_vae3_8.py", "hip.py"}, monkeypatch, check)


def test_vae_tiled_decode(monkeypatch):
    """One tiled decode, world = 2: both tiles of tests/test_vae_gpu.py's (2, 8, 4) case and what they assemble to -- the full decode."""
    import test_vae_gpu as TV
    z = C.vae_case(seed=56, frames=3, h=8, w=4)

    def work(byte):
        vae, _ = TV.build(seed=55)
        full = vae.decode(z.to(DEV)).sample[0]
        eng = vae.engine()
        tiles = [eng.decode(z[0].to(DEV), stripe=(r, 2)) for r in range(2)]
        whole = eng.assemble_tiles(tiles, eng.band_grid(8, 4, 2))
        assert torch.equal(whole, full)
        return dict(tile0=tiles[0].float().cpu(), tile1=tiles[1].float().cpu(), whole=whole.float().cpu())
    independent("vae-tiled-2", work, {"wan_vae3_8.py", "hip.py"}, monkeypatch)


def test_vae_encode(golden, monkeypatch):
    import test_vae_gpu as TV
    xv, xi = C.vae_enc_case(), C.vae_enc_case(seed=43, frames=1, h=32, w=32)

    def work(byte):
        vae, _ = TV.build_encoder()
        post = vae.encode(xv.to(DEV)).latent_dist
        return dict(mu_video=post.mode().float().cpu(), parameters=post.parameters.float().cpu(), mu_image=vae.encode(xi.to(DEV))[0].mode().float().cpu())

    def check(out):
        fx = golden("g8_vae_encode")
        TV.check_latent(out["mu_video"], fx["mu_video"], "vae encode g8 video under 0x00")
        TV.check_latent(out["mu_image"], fx["mu_image"], "vae encode g8 image under 0x00")
    independent("vae-encode", work, {"wan_vae3_8.py", "hip.py"}, monkeypatch, check)


# ----------------------------------------------------------------------------- text encoder
def test_text_encoder(monkeypatch):
    """The tiny umT5 of tests/test_text_encoder_gpu.py at 40 tokens: the P.V GEMMs' K is padded to lp = 64 > l, behind the zero fill of the
    softmax kernel; prompts of 33 and 40 tokens under an attention mask.  Compared over the valid rows, which the pipeline slices."""
    import test_text_encoder_gpu as TT
    from oracle import t5 as OT
    cfg = dict(OT.T5_TINY, shared_pos=True, num_heads=4, dim=256, dim_attn=256, dim_ffn=384, num_layers=3)
    ids, mask = OT.t5_case(cfg, seed=78, batch=2, length=40, lens=(33, 40))

    def work(byte):
        m, _ = TT.build(cfg, seed=9)
        out = m(ids.to(DEV), mask.to(DEV))[0]
        return {f"prompt {b}": out[b, :n].float().cpu() for b, n in enumerate((33, 40))}

    def check(out):
        want = OT.t5_encode(OT.seeded_t5_weights(cfg, 9), cfg, ids, mask)
        for b, n in enumerate((33, 40)):
            TT.check(out[f"prompt {b}"], want[b, :n], f"t5 prompt {b} under 0x00")
    independent("text-encoder", work, {"wan_text_encoder.py", "hip.py"}, monkeypatch, check)


# ----------------------------------------------------------------------------- wrappers with scratch of their own
def _randn(g, *shape, dtype=BF, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(DEV, dtype)


def test_wrappers_attention(monkeypatch):
    from flexam_amd import hip
    g = torch.Generator().manual_seed(3)
    q, k, v = _randn(g, 1, 300, 2, 128), _randn(g, 1, 1111, 2, 128), _randn(g, 1, 1111, 2, 128)
    q70, k70, v70 = (_randn(g, 2, 70, 2, 128) for _ in range(3))
    q100, k100, v100 = (_randn(g, 1, 100, 2, 128) for _ in range(3))

    def work(byte):
        out = {}
        out["attn_fwd kv_splits=3"] = hip.attn_fwd(q, k, v, kv_splits=3)
        out["attn_fwd planned"] = hip.attn_fwd(q, k, v)
        out["attn_fwd_lastkey"] = hip.attn_fwd_lastkey(q, k[:, :12], v[:, :12], 5.0)
        out["attn_fwd_window"] = hip.attn_fwd_window(q70, k70, v70, (20, 7), sink=3)
        # three key sets into an 8-slot workspace, 3 + 3 + 1 slots used: the merge reads the slots it is told, never the eighth
        ws = hip.attn_partial_workspace(1, 2, 300, 8, q.device)
        n = 0
        for lo, hi, splits in ((0, 400, 3), (400, 1000, 3), (1000, 1111, 1)):
            n += hip.attn_fwd_partial(q, k[:, lo:hi], v[:, lo:hi], ws, n, splits)
        assert n <= 7
        out["attn_fwd_partial + attn_merge"] = hip.attn_merge(torch.empty(1, 300, 2, 128, device=DEV, dtype=BF), ws, n)
        # MXFP8: L = 70 -- query rows padded to 256, the second key record ragged (6 of 64 keys)
        bufs = hip.attn_fp8_pack(q70, k70, v70)
        out["attn_fwd_fp8 L=70"] = hip.attn_fwd_fp8(bufs, 70)
        out["attn_fwd_fp8 split"] = hip.attn_fwd_fp8(bufs, 70, kv_splits=2)
        # the records of 100 keys as two gathered chunks of one tile each (the last one ragged), as the record gather hands them over
        q8, qs, kv8 = hip.attn_fp8_pack(q100, k100, v100)
        out["attn_fwd_fp8_chunked"] = hip.attn_fwd_fp8_chunked(q8, qs, kv8.permute(2, 0, 1, 3).unsqueeze(3).contiguous(), 100, 100)
        out["attn_fwd_fp8 L=100"] = hip.attn_fwd_fp8((q8, qs, kv8), 100)
        return {k_: v_.float().cpu() for k_, v_ in out.items()}

    def check(out):
        def sdpa(q_, k_, v_):
            qt, kt, vt = (u.float().cpu().transpose(1, 2) for u in (q_, k_, v_))
            return ((qt @ kt.transpose(-1, -2) / 128 ** 0.5).softmax(-1) @ vt).transpose(1, 2)
        want = sdpa(q, k, v)
        for name in ("attn_fwd kv_splits=3", "attn_fwd planned", "attn_fwd_partial + attn_merge"):
            assert float((out[name] - want).abs().max()) <= 2e-2, name          # bf16 output of O(1) values: 2^-8 relative, with room
        # the same records in one piece and in chunks: the same keys, tile by tile (bf16 output: one ulp of O(1) values, with room)
        assert float((out["attn_fwd_fp8_chunked"] - out["attn_fwd_fp8 L=100"]).abs().max()) <= 2e-2
    independent("wrappers-attention", work, {"hip.py"}, monkeypatch, check)


def test_wrappers_gemm_and_rows(monkeypatch):
    from flexam_amd import hip
    from flexam_amd.rope import rope_tables
    g = torch.Generator().manual_seed(1)
    m, k, n = 2912, 512, 768                                  # 39 tiles of 224 x 256: a tail split-K launch + finish ride along (test_replay_gpu)
    a, w, b = _randn(g, m, k), _randn(g, n, k, scale=k ** -0.5), _randn(g, n, dtype=F32)
    x = _randn(g, m, n, dtype=F32)
    kk = _randn(g, 2 * 300, 256)
    wk = (1 + 0.1 * torch.randn(256, generator=g)).to(DEV)
    cos, sin = (t.to(DEV) for t in rope_tables((5, 6, 10), 300, 128))
    B, L, c, sp = 2, 48, 256, 2
    qkv = _randn(g, B * L, 3 * c)
    wq = (1 + 0.1 * torch.randn(c, generator=g)).to(DEV)
    t_rows = torch.tensor([0.0, 731.5, 999.0], device=DEV)
    wl = _randn(g, 96, 256, scale=1 / 16)

    def work(byte):
        out = {}
        out["gemm 2912x512x768"] = hip.gemm(a, w, b, epilogue=hip.EPI_GELU_TANH)
        out["gemm f32"] = hip.gemm(a[:100], w, None, out_dtype=F32)
        (a8, sa), (w8, sw) = hip.quantize_rows_fp8(a), hip.quantize_rows_fp8(w)
        out["quantize_rows_fp8 q"], out["quantize_rows_fp8 scale"] = a8, sa
        out["gemm_fp8"] = hip.gemm_fp8(a8, sa, w8, sw, b)
        out["ln_modulate"] = hip.ln_modulate(x)
        out["mul_bf16"] = hip.mul_bf16(a, a)
        out["k_mean plain"] = hip.k_mean(kk, None, None, None, 300)
        out["k_mean norm+rope"] = hip.k_mean(kk, wk, cos, sin, 300)
        s = hip.sinusoid_embed(t_rows, 256)
        out["sinusoid_embed"] = s
        out["small_linear"] = hip.small_linear(s, wl, None, silu_in=True)
        out["unpatchify"] = hip.unpatchify(x[:12, :16].contiguous(), 0, 4, 2, 4, 6)
        # the all-to-all send layout [B, sp, lc, 3G]: every cell is named by q, k or v (tests/test_dit_row_kernels_gpu.py)
        G = c // sp
        dst = torch.empty(B * sp * L * 3 * G, device=DEV, dtype=BF)
        hip.rmsnorm_rope_scatter(qkv[:, :c], wq, qkv[:, c:2 * c], wk, qkv[:, 2 * c:], dst, dst[G:], dst[2 * G:], ld_out=3 * G, out_bs=sp * L * 3 * G,
                                 col_block=G, block_stride=L * 3 * G, rope_cos=cos, rope_sin=sin, tokens_per_batch=L, token_offset=0, head_dim=128)
        out["rmsnorm_rope_scatter"] = dst
        return {k_: v_.float().cpu() for k_, v_ in out.items()}

    def check(out):
        want = torch.nn.functional.gelu(a.float().cpu() @ w.float().cpu().t() + b.cpu(), approximate="tanh")
        assert float((out["gemm 2912x512x768"] - want).abs().max()) <= 2 ** -7 * float(want.abs().max())
        assert float((out["gemm_fp8"] - (a.float().cpu() @ w.float().cpu().t() + b.cpu())).abs().max()) <= 0.5       # e4m3 operands: 2^-4 relative per product, K = 512
        assert float((out["k_mean plain"] - kk.float().cpu().view(2, 300, 256).mean(1)).abs().max()) <= 1e-5
    independent("wrappers-gemm-rows", work, {"hip.py"}, monkeypatch, check)


# ----------------------------------------------------------------------------- one case each of the steps around the sampler
def test_conditioning_raster_and_colour_tables(golden, monkeypatch):
    """tests/test_raster_colors_gpu.py's "plain" clip from device tracks: percentile selection, colour tables, rasteriser."""
    from flexam_amd import conditioning_raster as P
    from oracle import make_golden_raster as G
    pts, vis, mask, gen, pw = G.case("plain")
    pts = np.ascontiguousarray(pts, dtype=np.float32)

    def work(byte):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            tr, cos, dep = P.visualize_tracking_DELTA(torch.from_numpy(pts).to(DEV), torch.from_numpy(np.asarray(vis)), False, pw, G.H, G.W, 4, gen, mask_video=mask)
        return dict(tracking=tr.cpu(), depth=dep.cpu(), **{f"cos{i}": cos[i].cpu() for i in range(4)})

    def check(out):
        by = lambda v: (v[0].permute(1, 2, 3, 0) * 255).round().to(torch.uint8).numpy()
        fx = golden("g13_raster_plain")
        assert np.array_equal(by(out["tracking"]), fx["tracking"].numpy()) and np.array_equal(by(out["depth"]), fx["depth"].numpy())
        assert all(np.array_equal(by(out[f"cos{i}"]), fx[f"cos{i}"].numpy()) for i in range(4))
    independent("raster-colours", work, {"hip.py"}, monkeypatch, check)


def test_motion_edit_to_videos(golden, monkeypatch):
    """tests/test_motion_gpu.py's end-to-end MoGe route: camera and object motion of a point map, then the six conditioning videos."""
    import test_motion_gpu as TM
    from flexam_amd import CameraMotionGenerator, moge_tracks
    fx, gv = golden("g15_motion_moge"), golden("g15_motion_vggt")

    def work(byte):
        cam = CameraMotionGenerator("rot y 14; trans 0.05 -0.02 -0.3", frame_num=TM.T, H=TM.MH, W=TM.MW, device=TM.dev())
        cam.set_intr(fx["intr"])
        tracks, vis = moge_tracks(fx["point_map"], fx["valid_mask_e2e"], cam, cam.get_default_motion(), TM.MH, TM.MW, object_mask=fx["object_mask"],
                                  object_motion="rot", distance=50)
        videos = TM._videos(tracks, vis, 2)
        # the VGGT route: unproject with the estimated cameras, project with the edited ones
        cam2 = CameraMotionGenerator("rot y 8; trans 0.05 0 0.1", frame_num=TM.T, H=TM.MH, W=TM.MW, device=TM.dev())
        src = gv["tracks64"][:, gv["e2e_keep"]]
        moved = cam2.w2s_vggt(cam2.s2w_vggt(src, gv["extrinsics"], gv["intrinsics"]), gv["extrinsics"], gv["intrinsics"], cam2.get_default_motion(),
                              override_extrinsics=False)
        videos2 = TM._videos(moved, gv["e2e_vis"].numpy(), 4)
        return dict(tracks=tracks.float().cpu(), vggt_tracks=moved.double().cpu(), **{f"video {i}": v.cpu() for i, v in enumerate(videos)},
                    **{f"vggt video {i}": v.cpu() for i, v in enumerate(videos2)})

    def check(out):
        TM._assert_videos([out[f"video {i}"] for i in range(6)], fx["videos_e2e"])
        TM._assert_videos([out[f"vggt video {i}"] for i in range(6)], gv["videos_e2e"])
    independent("motion", work, {"hip.py"}, monkeypatch, check)


def test_edit_masks(monkeypatch):
    """tests/test_edit_masks_gpu.py's small case: blur, convex hulls (runs, union-find), dilation."""
    import edit_mask_restatement as R
    from flexam_amd import generate_mask_bg_tracking_for_validation as bg
    from flexam_amd import generate_mask_fg_tracking_for_validation as fg
    rng = np.random.default_rng(9)
    planes = [(rng.random((48, 64)) < 0.004) for _ in range(3)]
    for p in planes:
        p[10:30, 20:40] = True
    one = torch.from_numpy(np.stack([np.zeros_like(planes[0])] + planes).astype(np.float32)[:, None])

    def work(byte):
        from flexam_amd import edit_masks as E
        from flexam_amd import hip
        binary = (one[1:, 0] > 0.5).to(torch.uint8).to(DEV).contiguous()
        runs, nruns = hip.edit_mask_hull(binary)                   # the wrappers' own outputs (the module hands them its buffers)
        dilated = hip.edit_mask_dilate(runs, nruns, 64, E._table("ellipse", 5, torch.device(DEV)))
        out = dict(foreground=fg(one.to(DEV), dilation_pixels=5).cpu(), background=bg(one.repeat(1, 3, 1, 1) * 255.0).cpu(), dilated=dilated.cpu())
        assert torch.equal(out["dilated"], fg(one.to(DEV), blur_radius=0, dilation_pixels=5)[1:, 0].cpu())
        return out

    def check(out):
        for f, p in enumerate(planes, start=1):
            assert np.array_equal(out["foreground"][f, 0].numpy(), R.refine_frame(p.astype(np.float32), dilation_pixels=5))
    independent("edit-masks", work, {"hip.py"}, monkeypatch, check)


def test_frames(monkeypatch):
    """tests/test_frames_gpu.py: the mask video's antialiased resize (frame count rule: the last frame repeated), the video branch, bytes out."""
    import frames_restatement as R
    import torch.nn.functional as F
    from flexam_amd import frames_to_bytes, get_maskvideo_to_video_latent, get_video_to_video_latent
    video = R.blob_mask_video(9, 135, 240)
    (h, w), size = R.SHAPES[2]
    clip = torch.from_numpy(R.case(h, w, "f32", 7).copy())

    def work(byte):
        dev = get_maskvideo_to_video_latent(video, 9, (64, 112))
        short = get_maskvideo_to_video_latent(video[4:7], 5, (64, 112))
        got, mask, _, _ = get_video_to_video_latent(clip, 5, size)
        return dict(mask_frames=dev.cpu(), short=short.cpu(), video=got.cpu(), mask=mask.cpu(), bytes=frames_to_bytes(got[0].contiguous(), signed=False).cpu())

    def check(out):
        import test_frames_gpu as TF
        host = F.interpolate(torch.from_numpy(video).permute(0, 3, 1, 2).float(), size=(64, 112), mode="bilinear", align_corners=False, antialias=True)
        TF._check(out["mask_frames"].to(DEV), host.numpy(), R.tolerance(135, 240, 64, 112, True), "mask frames under 0x00")
    independent("frames", work, {"frames.py", "hip.py"}, monkeypatch, check)


def test_lora_merge_and_unmerge(monkeypatch):
    """tests/test_lora_gpu.py's dyadic adapter on the tiny DiT (bf16 parameters): forward, merge, forward, unmerge, forward -- the merged
    weights are the restatement's (bf16 storage rounds once per merge, so the unmerged weights are compared across the patterns only)."""
    import lora_restatement as LR
    import test_lora_gpu as TL
    from flexam_amd import merge_lora, unmerge_lora
    cfg = dict(O.DIT_TINY)
    sd = _dit_weights(cfg, 7)
    case = C.dit_case(cfg, 41)

    def work(byte):
        m = TL.dit_model("bf16", sd)
        before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        lora = TL.dyadic_adapter(before)
        d = _to_dev(case)
        y0 = m(**d).float().cpu()
        merge_lora(LR.Pipe(m), None, TL.SCALE, device=DEV, dtype=F32, state_dict=lora)
        merged = {name: m.state_dict()[name + ".weight"].float().cpu() for name in TL.TOUCHED}
        y1 = m(**d).float().cpu()
        unmerge_lora(LR.Pipe(m), None, TL.SCALE, device=DEV, dtype=F32, state_dict=lora)
        y2 = m(**d).float().cpu()
        unmerged = {name: m.state_dict()[name + ".weight"].float().cpu() for name in TL.TOUCHED}
        assert not torch.equal(y1, y0) and not torch.equal(y2, y1)
        return dict(y0=y0, y1=y1, y2=y2, **{"merged " + k: v for k, v in merged.items()}, **{"unmerged " + k: v for k, v in unmerged.items()})

    def check(out):
        before = {k: v.to(BF) for k, v in sd.items()}
        lora = TL.dyadic_adapter(before)
        for name in TL.TOUCHED:
            u, dn = lora[LR.spell(name, "lora_up.weight", "kohya")], lora[LR.spell(name, "lora_down.weight", "kohya")]
            assert torch.equal(out["merged " + name], LR.merged(before[name + ".weight"], u, dn, TL.SCALE).float()), name
    independent("lora", work, {"dit_engine.py", "hip.py"}, monkeypatch, check)


# ----------------------------------------------------------------------------- coverage: a cap, not a measurement
COVERED_MODULES = ("dit_engine.py", "dit_sp.py", "wan_vae3_8.py", "wan_text_encoder.py", "hip.py", "frames.py", "edit_masks.py", "implicit_conv.py")
# Sites of the covered modules that a one-GPU run of this module cannot reach, each with its reason.
NOT_REACHED = {
    ("wan_text_encoder.py", "_linear"): "parameter construction on the CPU (torch.empty inside nn.Parameter), loaded over by load_state_dict before the model moves to the GPU",
}
# Sites whose every allocation is an integer buffer (runs, counts, indices, keys): seen by the harness and left alone on purpose --
# scratch_poison's limit.  Held here so that the list cannot grow silently: each must have been SEEN, and none poisoned.
INTEGER_ONLY = {
    ("hip.py", "edit_mask_hull"): "runs / nruns int32 and the union-find scratch (int32)",
    ("hip.py", "motion_compact"): "index, count and the scan scratch, int32",
    ("hip.py", "raster_keys"): "the int64 depth | point keys",
}
WORKLOADS = 2 * len(DIT_VARIANTS) + 3 + len(SP_CASES) + 1 + 4 + 1 + 2 + 5   # DiT, sampler + emulated rank + history, ranks (+ VAE), VAE, text, wrappers, the steps around


def test_every_allocation_site_of_the_covered_modules_was_poisoned():
    """The union of the sites poisoned above (the spawned ranks' came back with their results) against the census of
    tests/test_scratch_poison_cpu.py: every initialisation-free allocation site of the covered modules was reached, NOT_REACHED apart."""
    assert len(_RAN) == WORKLOADS, f"only {len(_RAN)} of {WORKLOADS} workloads of this module ran and passed: the coverage is that of the whole module"
    census = {s for s in SPZ.census() if s[0] in COVERED_MODULES}
    assert len(census) >= 45
    assert set(NOT_REACHED) <= census, sorted(set(NOT_REACHED) - census)
    reached = {s for s in _SITES if s[0] in COVERED_MODULES}
    print(f"{len(reached)} of {len(census)} sites of the covered modules poisoned; workloads: {len(_STATS)}")
    for name in sorted(_STATS):
        print(f"  {name:44s} {_STATS[name][0]:6d} allocations {_STATS[name][1]:12d} bytes")
    assert not (reached & set(NOT_REACHED)), f"reached after all, take them off NOT_REACHED: {sorted(reached & set(NOT_REACHED))}"
    assert set(INTEGER_ONLY) <= census and set(INTEGER_ONLY) <= _INTEGER_SITES and not (reached & set(INTEGER_ONLY)), \
        f"INTEGER_ONLY: not seen {sorted(set(INTEGER_ONLY) - _INTEGER_SITES)}, poisoned after all {sorted(reached & set(INTEGER_ONLY))}"
    missing = census - reached - set(NOT_REACHED) - set(INTEGER_ONLY)
    assert not missing, f"allocation sites no workload of this module poisoned: {sorted(missing)}"
