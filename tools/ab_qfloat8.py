"""Dev tool: the qfloat8 weight storage (flexam_amd.fp8_optimization, flexam_gemm_w8) against the bf16 model, in ONE process with
alternating arms.
  1. per-shape GEMM time of the block GEMMs at M = 23296 (the single-GPU CFG pair at 97x512x896) and M = 2912 (a rank of eight):
     flexam_gemm_w8* against flexam_gemm_bf16* on the same A / upcast W, interleaved launches, HIP events, median;
  2. ms per denoise step of bench.py's pipeline (97x512x896, 30 layers, CFG pair) on (a) the bf16 model and (b) its qfloat8 conversion
     (nodes.py:327-343: convert_model_weight_to_float8 + convert_weight_dtype_wrapper), groups of steps alternating between the arms;
  3. weight memory of each model (torch.cuda.memory_allocated deltas) and torch.cuda.max_memory_allocated over each arm's steps.
usage: ab_qfloat8.py [--steps=3] [--rounds=5] [--reps=20]"""
import os
import statistics
import sys
import time

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch

import bench
from flexam_amd import Wan2_2FunControlPipeline_FlexAM, convert_model_weight_to_float8, convert_weight_dtype_wrapper
from flexam_amd import hip as H
from flexam_amd.configs import WAN22_FUN_5B_FLEXAM
from flexam_amd.pipeline_wan2_2_fun_control_FlexAM import LatentConditioning

opt = {a.split("=")[0][2:]: int(a.split("=")[1]) for a in sys.argv[1:] if a.startswith("--")}
steps, rounds, reps = opt.get("steps", 3), opt.get("rounds", 5), opt.get("reps", 20)
dev = torch.device("cuda:0")
torch.cuda.set_device(0)
BF, F8 = torch.bfloat16, torch.float8_e4m3fn
GB = 1e9

# ---------------------------------------------------------------- 1. GEMM shapes
d, ffn = WAN22_FUN_5B_FLEXAM["dim"], WAN22_FUN_5B_FLEXAM["ffn_dim"]
shapes = [("qkv", 3 * d, d, "plain"), ("o-proj +res", d, d, "res"), ("cross-q", d, d, "plain"), ("ffn1 +gelu", ffn, d, "gelu"),
          ("ffn2 +res", d, ffn, "res")]
print(f"{'shape':14s} {'M':>6s} {'N':>6s} {'K':>6s}   {'bf16 ms':>8s} {'w8 ms':>8s}  {'w8/bf16':>8s}", flush=True)
g = torch.Generator(device=dev).manual_seed(0)
for M in (23296, 2912):
    for name, N, K, kind in shapes:
        a = torch.randn(M, K, device=dev, generator=g).to(BF)
        w8 = (torch.randn(N, K, device=dev, generator=g) * 0.02).to(F8)
        wb = w8.to(BF)
        bias = torch.randn(N, device=dev, generator=g)
        x = torch.zeros(M, N, device=dev) if kind == "res" else None
        out = None if kind == "res" else torch.empty(M, N, device=dev, dtype=BF)
        gate = torch.randn(2, N, device=dev, generator=g) if kind == "res" else None

        def run(w):
            if kind == "res":
                H.gemm_gate_residual(a, w, bias, x, gate=gate, rows_per_batch=(M + 1) // 2)
            else:
                H.gemm(a, w, bias, out=out, epilogue=H.EPI_GELU_TANH if kind == "gelu" else H.EPI_NONE)
        t = {"bf16": [], "w8": []}
        for i in range(reps + 2):
            for arm, w in (("bf16", wb), ("w8", w8)) if i % 2 == 0 else (("w8", w8), ("bf16", wb)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(w)
                e1.record()
                e1.synchronize()
                if i >= 2:
                    t[arm].append(e0.elapsed_time(e1))
        mb_, m8 = statistics.median(t["bf16"]), statistics.median(t["w8"])
        print(f"{name:14s} {M:6d} {N:6d} {K:6d}   {mb_:8.3f} {m8:8.3f}  {m8 / mb_:8.3f}", flush=True)
        del a, w8, wb, bias, x, out, gate
torch.cuda.empty_cache()

# ---------------------------------------------------------------- 2./3. models and steps
cfg = dict(WAN22_FUN_5B_FLEXAM)
i = bench.synthetic_inputs(97, 512, 896, cfg["text_dim"], "motion")
cond = LatentConditioning(control_latents=i["control"], additional_control=i["additional"], masked_video_latents=i["masked"],
                          ref_latents=i["ref"], mask_latents=i["mask_latents"], mask=i["mask"], mask_pixels=i["mask_pixels"])


def block_bytes(m):
    return sum(p.numel() * p.element_size() for n, p in m.blocks.named_parameters() if n.endswith(".weight") and p.dim() == 2)


torch.cuda.synchronize()
m0 = torch.cuda.memory_allocated()
model_a = bench.build_model(cfg, dev)
torch.cuda.synchronize()
m1 = torch.cuda.memory_allocated()
model_b = bench.build_model(cfg, dev)
convert_model_weight_to_float8(model_b, exclude_module_name=["modulation"], device=dev)
convert_weight_dtype_wrapper(model_b, BF)
torch.cuda.synchronize()
m2 = torch.cuda.memory_allocated()
print(f"\nparameters: bf16 model {(m1 - m0) / GB:.2f} GB (block matrices {block_bytes(model_a) / GB:.2f} GB); "
      f"qfloat8 model {(m2 - m1) / GB:.2f} GB (block matrices {block_bytes(model_b) / GB:.2f} GB)", flush=True)
arms = {}
for name, m in (("bf16", model_a), ("qfloat8", model_b)):
    pipe = Wan2_2FunControlPipeline_FlexAM(transformer=m)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    pipe.prepare(i["latents"], cond, i["ctx_c"], i["ctx_u"], density=0.1, guidance_scale=6.0, num_inference_steps=50)
    pipe.denoise_step(0)
    torch.cuda.synchronize()
    print(f"{name}: engine packs + activation buffers + recorded plans after the first step: +{(torch.cuda.memory_allocated() - before) / GB:.2f} GB",
          flush=True)
    arms[name] = pipe
res = {a: [] for a in arms}
peak = {a: [] for a in arms}
n = 1
for r in range(rounds + 1):                       # round 0 = warm-up, dropped
    for a in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
        pipe = arms[a]
        pipe.denoise_step(n % 50)
        n += 1
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(steps):
            pipe.denoise_step(n % 50)
            n += 1
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if r:
            res[a].append(el / steps * 1e3)
            peak[a].append(torch.cuda.max_memory_allocated() - base)
b = statistics.median(res["bf16"])
for a in arms:
    m = statistics.median(res[a])
    print(f"{a:8s} {m:8.2f} ms/step ({100 * (m / b - 1):+.2f} %)  min {min(res[a]):.2f} max {max(res[a]):.2f}   "
          f"step peak above resident {max(peak[a]) / GB:.3f} GB", flush=True)
print(f"max_memory_allocated over the run (both models resident): {torch.cuda.max_memory_allocated() / GB:.2f} GB")
