"""Times a LoRA merge at the 5B model's width: a rank-64 adapter over the ten linears (self q/k/v/o, cross q/k/v/o, ffn.0, ffn.2) of
all 30 blocks (d = 3072, ffn 14336; 9.8 GB of bf16 weights), adapter and weights already on the GPU, two ways on the same device:

    flexam_amd.merge_lora         one flexam_lora_merge launch per layer (fp32 arithmetic, one rounding)
    the reference's expression    `weight.data += multiplier * alpha * torch.mm(up, down)` per layer in `dtype`
                                  (FlexAM/utils/lora_utils.py:485, as the sampler node calls it: device="cuda", dtype=bf16)

and a plain device copy of a 2 GiB buffer for the bandwidth a pass over the weights could reach: a merge reads and writes every
weight once, so its traffic is twice the weights' bytes (the factors are 1 % of that).  Merges alternate with unmerges so the values
stay bounded.  Warm-up first; each timing ends in a device synchronise; best of N.

    python tools/lora_bench.py [--repeats 3] [--layers 30] [--out profiles/lora_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM, FFN, RANK = 3072, 14336, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--layers", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from torch import nn
    from flexam_amd import merge_lora, unmerge_lora
    if not torch.cuda.is_available():
        raise SystemExit("lora_bench: no GPU (this measures the GPU path; there is nothing to fall back to)")
    dev, bf = torch.device("cuda:0"), torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)

    def holder(n, k):
        m = nn.Module()
        m.weight = nn.Parameter((torch.randn(n, k, device=dev, generator=g) * 0.02).to(bf), requires_grad=False)
        return m

    def attn():
        m = nn.Module()
        for name in "qkvo":
            m.add_module(name, holder(DIM, DIM))
        return m

    model = nn.Module()
    model.blocks = nn.ModuleList()
    for _ in range(args.layers):
        b = nn.Module()
        b.self_attn, b.cross_attn = attn(), attn()
        b.ffn = nn.Sequential(holder(FFN, DIM), nn.Identity(), holder(DIM, FFN))
        model.blocks.append(b)

    class Pipe:
        transformer = model
    targets = [(n, m) for n, m in model.named_modules() if hasattr(m, "weight")]
    sd = {}
    for n, m in targets:
        N, K = m.weight.shape
        sd[f"diffusion_model.{n}.lora_up.weight"] = (torch.randn(N, RANK, device=dev, generator=g) * 0.02).to(bf)
        sd[f"diffusion_model.{n}.lora_down.weight"] = (torch.randn(RANK, K, device=dev, generator=g) * 0.02).to(bf)
    wbytes = sum(m.weight.numel() * 2 for _, m in targets)

    def ours(sign):
        (merge_lora if sign > 0 else unmerge_lora)(Pipe, None, 1.0, device="cuda", dtype=bf, state_dict=sd)

    def reference(sign):
        for n, m in targets:
            up, down = sd[f"diffusion_model.{n}.lora_up.weight"], sd[f"diffusion_model.{n}.lora_down.weight"]
            if sign > 0:
                m.weight.data += 1.0 * 1.0 * torch.mm(up, down)
            else:
                m.weight.data -= 1.0 * 1.0 * torch.mm(up, down)

    def best(fn):
        fn(1.0), fn(-1.0)
        torch.cuda.synchronize()
        times = []
        for i in range(2 * args.repeats):
            t0 = time.perf_counter()
            fn(1.0 if i % 2 == 0 else -1.0)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return min(times)

    src = torch.empty(1 << 30, dtype=bf, device=dev).normal_()
    dst = torch.empty_like(src)
    copy_s = best(lambda _s: dst.copy_(src))
    copy_bw = 2 * src.numel() * 2 / copy_s
    del src, dst
    t_ours, t_ref = best(ours), best(reference)
    rec = {"device": torch.cuda.get_device_name(0), "layers": args.layers, "linears": len(targets), "rank": RANK, "weights": "bf16",
           "factors": "bf16", "weight_gb": round(wbytes / 1e9, 2), "merge_lora_ms": round(1e3 * t_ours, 2),
           "reference_expression_ms": round(1e3 * t_ref, 2), "copy_gb_per_s": round(copy_bw / 1e9, 1),
           "merge_lora_gb_per_s": round(2 * wbytes / t_ours / 1e9, 1), "fraction_of_copy_bandwidth": round(2 * wbytes / t_ours / copy_bw, 3),
           "repeats": args.repeats}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
