"""Dev tool: what a sliding window saves per self-attention launch at the bench shape (B = 2, H = 24, L = 11648 = 26 frames of 448
tokens, pre-scaled q) -> profiles/attn_window_bench.json; with --sink, what keeping the first keys visible costs on top of it
-> profiles/attn_window_sink_bench.json.

Arms: full attention through hip.attn_fwd (the yardstick: the launch the engine makes without a window, tail split and merge included)
against hip.attn_fwd_window with windows of +-k latent frames ((448 k, 448 k), k = 2, 5, 12) and causal.  All arms run in ONE process on
the same buffers, alternating: `--rounds` rounds, each timing every arm once with device events around `--iters` back-to-back launches;
the figure of an arm is the median over the rounds.  Per arm the record holds the time, the share of (query block, key tile) pairs the
kernel visits (hip.attn_window_tiles, the planner the kernel's own rule is tested against), the time relative to the full call's and
the time per visited tile relative to the full call's -- 1.0 would be a window that costs nothing but the tiles it visits.

Condition (asserted, exit status 1): a window that visits at most half the tiles takes less time than the full call of the same run.

--sink=a,b,...: the arms are the full call and every window of +-2, +-5, +-12 frames with every sink of the list (tile shares from
hip.attn_window_sink_tiles; no causal arm: a sink lies to the left of the window).  With --base=<a parent build of libflexam_hip.so> the
same call also times the sink = 0 launches of the in-tree library against that build, each window three times per round -- base,
in-tree, base again, the order rotating -- and checks that both give the same bytes: `margin` is the spread of the base build against
itself (its two arms' medians), `new_over_base` the in-tree median over the pooled base median, `slower_beyond_margin` says whether it
exceeds 1 + margin.

usage: attn_window_bench.py [--iters=10] [--rounds=7] [--out=profiles/attn_window_bench.json]
       attn_window_bench.py --sink=0,448,896 [--base=path/to/parent/libflexam_hip.so] [--out=profiles/attn_window_sink_bench.json]"""
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
sinks = [int(s) for s in opt["sink"].split(",")] if "sink" in opt else None
out_path = os.path.join(root, opt.get("out", "profiles/attn_window_bench.json" if sinks is None else "profiles/attn_window_sink_bench.json"))
B, heads, L, D = 2, 24, 11648, 128
FRAME = 448
g = torch.Generator().manual_seed(0)
q, k, v = ((torch.randn(B, L, heads, D, generator=g) * s).to(torch.bfloat16).cuda() for s in (0.35, 1.0, 1.0))      # q in exp2 units: logits of std ~4
o = torch.empty_like(q)

WINDOWS = [(f"window_{n}_frames", (FRAME * n, FRAME * n)) for n in (2, 5, 12)]
if sinks is None:
    ARMS = [("full", None, 0)] + [(name, w, 0) for name, w in WINDOWS] + [("causal", (-1, 0), 0)]
else:
    ARMS = [("full", None, 0)] + [(f"{name}_sink_{s}", w, s) for name, w in WINDOWS for s in sinks]


def launch(window, sink=0, out=o):
    if window is None:
        H.attn_fwd(q, k, v, out=out, prescaled=True)
    elif sink:
        H.attn_fwd_window(q, k, v, window, out=out, prescaled=True, sink=sink)
    else:
        H.attn_fwd_window(q, k, v, window, out=out, prescaled=True)


def share(window, sink=0):
    runs = H.attn_window_sink_tiles(L, window if window is not None else (-1, -1), sink)
    return sum(b - a + 1 for r in runs for a, b in r) / (H.attn_units(1, L) * H.attn_kv_tiles(L))


def timed(window, sink=0):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        launch(window, sink)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


for _, w, s in ARMS:                               # warm-up: every instance once (LDS attribute, code load), then the clock
    launch(w, s)
for _ in range(3):
    launch(None)
torch.cuda.synchronize()
ms = {name: [] for name, _, _ in ARMS}
for _ in range(rounds):
    for name, w, s in ARMS:
        ms[name].append(timed(w, s))
full = statistics.median(ms["full"])
arms, ok = {}, True
for name, w, s in ARMS:
    t, sh = statistics.median(ms[name]), share(w, s)
    arms[name] = dict(window=list(w) if w else None, ms=round(t, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                      tile_share=round(sh, 4), time_ratio=round(t / full, 4), time_per_tile_ratio=round(t / full / sh, 3))
    if sinks is not None and w is not None:
        arms[name]["sink"] = s
    if w is not None and sh <= 0.5 and not t < full:
        ok = False
    print(f"{name:28s} {t:8.3f} ms (min {min(ms[name]):.3f}, max {max(ms[name]):.3f})  tiles {sh:6.4f}  time {t / full:6.3f}  per tile {t / full / sh:5.2f}")
rec = dict(shape=dict(B=B, H=heads, L=L, head_dim=D, prescaled=True), iters=iters, rounds=rounds, device=torch.cuda.get_device_name(0),
           method="one process, arms alternating per round, device events around `iters` back-to-back launches, median over the rounds",
           arms=arms, condition="every window that visits at most half the tiles is faster than the full call of the same run",
           condition_met=ok)

if sinks is not None and "base" in opt:
    # sink = 0 against a parent build: base, in-tree, base again per window and round, rotating; hip._lib switches the build
    import ctypes

    def build_of(path):
        """A build of the library with the entry points it has declared (a parent build lacks the ones added since)."""
        lib = ctypes.CDLL(path)
        for fn_name, (argtypes, restype) in H._SIGNATURES.items():
            fn = getattr(lib, fn_name, None)
            if fn is not None:
                fn.argtypes, fn.restype = argtypes, restype
        return lib

    base_lib, new_lib = build_of(os.path.abspath(opt["base"])), H.load_library(H.LIB_PATH)
    libs = {"base_a": base_lib, "new": new_lib, "base_b": base_lib}
    outs = {tag: torch.empty_like(q) for tag in ("base_a", "new")}
    for tag in outs:                               # warm-up of both builds, and the bytes they give
        H._lib = libs[tag]
        for _, w in WINDOWS:
            launch(w, 0, outs[tag])
    torch.cuda.synchronize()
    ab = {name: {tag: [] for tag in libs} for name, _ in WINDOWS}
    same = {}
    for name, w in WINDOWS:
        for tag in outs:
            H._lib = libs[tag]
            launch(w, 0, outs[tag])
        torch.cuda.synchronize()
        same[name] = bool(torch.equal(outs["base_a"], outs["new"]))
    order = list(libs)
    for r in range(rounds):
        for name, w in WINDOWS:
            for tag in order[r % 3:] + order[:r % 3]:
                H._lib = libs[tag]
                ab[name][tag].append(timed(w, 0))
    H._lib = new_lib
    rec["sink_0_against_base"] = dict(method="sink = 0 launches (hip.attn_fwd_window) of the base build and of the in-tree build in this process: per window "
                                             "and round base, in-tree, base again in rotating order; margin = the base build against itself",
                                      windows={})
    for name, w in WINDOWS:
        a, n, b = (statistics.median(ab[name][tag]) for tag in libs)
        base = statistics.median(ab[name]["base_a"] + ab[name]["base_b"])
        margin = abs(a - b) / base
        rec["sink_0_against_base"]["windows"][name] = dict(window=list(w), base_a_ms=round(a, 4), base_b_ms=round(b, 4), new_ms=round(n, 4),
                                                           margin=round(margin, 4), new_over_base=round(n / base, 4),
                                                           slower_beyond_margin=bool(n / base > 1 + margin), same_bytes=same[name])
        print(f"sink 0, {name:18s} base {a:7.3f} / {b:7.3f} ms  in-tree {n:7.3f} ms  new / base {n / base:6.4f}  margin {margin:6.4f}  same bytes {same[name]}")

with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print("wrote", out_path, "condition met" if ok else "CONDITION NOT MET")
sys.exit(0 if ok else 1)
