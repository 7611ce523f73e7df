"""Dev tool: what the smooth-K and smooth-V passes cost per block at the bench shape (CFG pair, L = 11648, 24 heads; k and v column views of
the [M, 9216] q|k|v buffer, as the engine calls them).  Times hip.k_mean in both forms and the fused producer with and without a shift;
for smooth-V the mean of the V columns, the V-only pack with and without v_shift and the attention with and without o_shift; with device
events over `--iters` back-to-back calls after a warm-up, and prints the mean kernel's GB/s: the bytes are those the algorithm needs
(K once, the parts written and read once, the mean).  usage: k_mean_bench.py [--iters=200] [--parts=512,256,1024]"""
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402
from flexam_amd import hip as H  # noqa: E402

opt = {a.split("=")[0][2:]: a.split("=")[1] for a in sys.argv[1:] if a.startswith("--")}
iters = int(opt.get("iters", 200))
B, L, heads, D = 2, 11648, 24, 128
C, M = heads * D, 2 * 11648
parts_list = [int(p) for p in opt.get("parts", str(H.k_mean_parts(L))).split(",")]
g = torch.Generator().manual_seed(0)
qkv = (torch.randn(M, 3 * C, generator=g) * 1.5).to(torch.bfloat16).cuda()
q, k = qkv[:, :C], qkv[:, C:2 * C]
wq, wk = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.rand(C, generator=g) + 0.5).cuda()
ang = torch.rand(L, D // 2, generator=g) * 6.28
cos, sin = ang.cos().cuda(), ang.sin().cuda()
bufs = H.attn_fp8_buffers(B, heads, L, "cuda")
mean = torch.empty(B, C, device="cuda")


def timed(fn, group=20):
    """us per call: `group` calls recorded into a launch plan and replayed from C (the wrappers' 20-30 us of Python per call would
    otherwise be what is timed), iters / group replays between two device events."""
    with H.record() as plan:
        for _ in range(group):
            fn()
    plan.run()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = max(1, iters // group)
    a.record()
    for _ in range(n):
        plan.run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / (n * group) * 1e3


print(f"B={B} L={L} C={C}, k rows of pitch {k.stride(0)}; {iters} calls per figure; wrapper's parts = {H.k_mean_parts(L)}")
for parts in parts_list:
    scratch = torch.empty(B, parts, C, device="cuda")
    nbytes = M * C * 2 + 2 * scratch.numel() * 4 + mean.numel() * 4
    for what, fn in (("norm+rope", lambda: H.k_mean(k, wk, cos, sin, L, out=mean, scratch=scratch)),
                     ("as given ", lambda: H.k_mean(k, None, None, None, L, out=mean, scratch=scratch))):
        us = timed(fn)
        print(f"k_mean {what} parts={parts:5d}: {us:7.1f} us per call (both launches)  {nbytes / us * 1e-3:7.1f} GB/s  ({nbytes / 1e6:.1f} MB)")
us0 = timed(lambda: H.rmsnorm_rope_mx(q, wq, k, wk, bufs, cos, sin, L))
us1 = timed(lambda: H.rmsnorm_rope_mx(q, wq, k, wk, bufs, cos, sin, L, k_shift=mean))
print(f"rmsnorm_rope_mx: {us0:.1f} us per call; with k_shift (two launches): {us1:.1f} us")
# smooth-V: the mean of the V columns (as given), the V-only pack the fused producer is followed by, the attention that adds the mean back
v, v4 = qkv[:, 2 * C:], qkv.view(B, L, 3, heads, D)[:, :, 2]
v_mean, v_scratch = torch.empty(B, C, device="cuda"), torch.empty(B, H.k_mean_parts(L), C, device="cuda")
us = timed(lambda: H.k_mean(v, None, None, None, L, out=v_mean, scratch=v_scratch))
print(f"k_mean of the V columns (as given, parts={v_scratch.shape[1]}): {us:.1f} us per call (both launches)")
us0 = timed(lambda: H.attn_fp8_pack(None, None, v4, bufs))
us1 = timed(lambda: H.attn_fp8_pack(None, None, v4, bufs, v_shift=v_mean))
print(f"attn_fp8_pack, V only: {us0:.1f} us per call; with v_shift: {us1:.1f} us")
out = torch.empty(B, L, heads, D, dtype=torch.bfloat16, device="cuda")
H.rmsnorm_rope_mx(q, wq, k, wk, bufs, cos, sin, L)
us0 = timed(lambda: H.attn_fwd_fp8(bufs, L, out=out), group=4)
us1 = timed(lambda: H.attn_fwd_fp8(bufs, L, out=out, o_shift=v_mean), group=4)
print(f"attn_fwd_fp8: {us0:.1f} us per call; with o_shift: {us1:.1f} us")
