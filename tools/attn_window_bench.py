"""Dev tool: what a sliding window saves per self-attention launch at the bench shape (B = 2, H = 24, L = 11648 = 26 frames of 448
tokens, pre-scaled q) -> profiles/attn_window_bench.json.

Arms: full attention through hip.attn_fwd (the yardstick: the launch the engine makes without a window, tail split and merge included)
against hip.attn_fwd_window with windows of +-k latent frames ((448 k, 448 k), k = 2, 5, 12) and causal.  All arms run in ONE process on
the same buffers, alternating: `--rounds` rounds, each timing every arm once with device events around `--iters` back-to-back launches;
the figure of an arm is the median over the rounds.  Per arm the record holds the time, the share of (query block, key tile) pairs the
kernel visits (hip.attn_window_tiles, the planner the kernel's own rule is tested against), the time relative to the full call's and
the time per visited tile relative to the full call's -- 1.0 would be a window that costs nothing but the tiles it visits.

Condition (asserted, exit status 1): a window that visits at most half the tiles takes less time than the full call of the same run.

usage: attn_window_bench.py [--iters=10] [--rounds=7] [--out=profiles/attn_window_bench.json]"""
import json
import os
import statistics
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402
from flexam_amd import hip as H  # noqa: E402

opt = {a.split("=")[0][2:]: a.split("=")[1] for a in sys.argv[1:] if a.startswith("--")}
iters, rounds = int(opt.get("iters", 10)), int(opt.get("rounds", 7))
out_path = os.path.join(root, opt.get("out", "profiles/attn_window_bench.json"))
B, heads, L, D = 2, 24, 11648, 128
FRAME = 448
g = torch.Generator().manual_seed(0)
q, k, v = ((torch.randn(B, L, heads, D, generator=g) * s).to(torch.bfloat16).cuda() for s in (0.35, 1.0, 1.0))      # q in exp2 units: logits of std ~4
o = torch.empty_like(q)

ARMS = [("full", None)] + [(f"window_{n}_frames", (FRAME * n, FRAME * n)) for n in (2, 5, 12)] + [("causal", (-1, 0))]


def launch(window):
    if window is None:
        H.attn_fwd(q, k, v, out=o, prescaled=True)
    else:
        H.attn_fwd_window(q, k, v, window, out=o, prescaled=True)


def share(window):
    visited = sum(b - a + 1 for a, b in H.attn_window_tiles(L, window if window is not None else (-1, -1)))
    return visited / (H.attn_units(1, L) * H.attn_kv_tiles(L))


def timed(window):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        launch(window)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


for _, w in ARMS:                                  # warm-up: every instance once (LDS attribute, code load), then the clock
    launch(w)
for _ in range(3):
    launch(None)
torch.cuda.synchronize()
ms = {name: [] for name, _ in ARMS}
for _ in range(rounds):
    for name, w in ARMS:
        ms[name].append(timed(w))
full = statistics.median(ms["full"])
arms, ok = {}, True
for name, w in ARMS:
    t, s = statistics.median(ms[name]), share(w)
    arms[name] = dict(window=list(w) if w else None, ms=round(t, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                      tile_share=round(s, 4), time_ratio=round(t / full, 4), time_per_tile_ratio=round(t / full / s, 3))
    if w is not None and s <= 0.5 and not t < full:
        ok = False
    print(f"{name:18s} {t:8.3f} ms (min {min(ms[name]):.3f}, max {max(ms[name]):.3f})  tiles {s:6.3f}  time {t / full:6.3f}  per tile {t / full / s:5.2f}")
rec = dict(shape=dict(B=B, H=heads, L=L, head_dim=D, prescaled=True), iters=iters, rounds=rounds, device=torch.cuda.get_device_name(0),
           method="one process, arms alternating per round, device events around `iters` back-to-back launches, median over the rounds",
           arms=arms, condition="every window that visits at most half the tiles is faster than the full call of the same run",
           condition_met=ok)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print("wrote", out_path, "condition met" if ok else "CONDITION NOT MET")
sys.exit(0 if ok else 1)
