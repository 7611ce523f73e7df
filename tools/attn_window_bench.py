"""Dev tool: what a sliding window saves per self-attention launch at the bench shape (B = 2, H = 24, L = 11648 = 26 frames of 448
tokens, pre-scaled q) -> profiles/attn_window_bench.json; with --sink, what keeping the first keys visible costs on top of it
-> profiles/attn_window_sink_bench.json; with --frames, the window counted in frames (hip.attn_fwd_window(..., frame_tokens=448))
-> profiles/attn_window_frames_bench.json.

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

--frames[=2,5,12] [--sink=0,448]: the arms are the full call and the frame windows +-k frames of the list, frame-block-causal (-1, 0) and
per-frame (0, 0), each with every sink of the list (tile shares from hip.attn_window_frames_tiles), and beside every +-k arm the token
window of the same span, (448 k, 448 k) with the same sink: the frame form visits more tiles and masks none of them at this shape (448
tokens are 7 key tiles), `faster_per_visited_tile` records which of the two takes less time per tile it visits.  With --base the same
call times the token-window launches (frame_tokens = 0, every sink of the list) of the in-tree library against that build, as above.

--sage [--base=...]: the windows under the MXFP8 kernel (hip.attn_fwd_fp8 with a window: FLEXAM_SAGE_WINDOW=1's launch) -> profiles/
attn_window_sage_bench.json.  Arms: the full MXFP8 launch (hip.attn_fwd_fp8, the engine's call: tail split and merge included), the
token windows of +-2 / +-5 / +-12 frames and the frame windows +-2 / +-5 / +-12, (-1, 0) and (0, 0), each with sink 0 and 448.  Per
arm: the time, its share of the full MXFP8 launch, the share of tiles visited, and the time of the bf16 windowed launch of the SAME mask
taken in the same call (the two alternate inside every round), `mxfp8_over_bf16` their ratio.  With --base the unwindowed MXFP8
launch and the full bf16 launch of the in-tree library are timed against that build as above (base, in-tree, base).  No condition.

--rank-of=N (N = 8): the windows at a rank's shape under sequence parallelism (FLEXAM_SP_WINDOW=1's launch, hip.attn_fwd_window(...,
q_offset=)) -> profiles/attn_window_sp_bench.json.  Lk = 11648 keys, Lq = ceil(11648 / N) queries at the offsets of ranks 0, N / 2 and
N - 1; per rank the unmasked launch a rank runs today (hip.attn_fwd on (Lq, Lk), tail split and merge included) and the masks --sage
walks (token and frame windows of +-2 / +-5 / +-12 frames, frame-block-causal, per-frame, sink 0 and 448), alternating inside every
round.  Per arm: the time, its share of the rank's unmasked launch, the share of (query block, key tile) pairs visited
(hip.attn_window_at_tiles), and the number of work units.  No condition.

--rank-of=N --halo: the same masks and ranks on a COMPACT key buffer (FLEXAM_SP_HALO=1's launch, hip.attn_fwd_window(..., q_offset=,
key_gap_tiles=, Lk=)) -> profiles/attn_window_halo_bench.json.  K and V are packed by dit_layout.halo_plan; per mask and rank the halo
launch is timed beside the q_offset launch on the full keys, three arms per round -- full keys, halo, full keys again, the order rotating
--, and both must give the same bytes: `margin` is the spread of the full-key launch against itself (its two arms' medians),
`halo_over_at` the halo median over the pooled full-key median, `slower_beyond_margin` says whether it exceeds 1 + margin.  Beside
them the planned rows: the buffer's, the remote rows a rank receives, and the Lk - Lq the gather moves.  No condition.

--rank-of=N --sage: the frame windows +-2 / +-5 / +-12 (sink 0 and 448) under the MXFP8 kernel at a rank's shape under the record gather
(FLEXAM_SP_SAGE_WINDOW=1's launch, hip.attn_fwd_fp8_chunked(..., window=, q_offset=)) -> profiles/attn_window_sp_sage_bench.json.
Lq = 64 ceil(11648 / (64 N)) rows a rank (1472 at N = 8: the record padding, not the bf16 gather's 1456), the records of every rank's
chunk stacked rank-major, ranks 0, N / 2 and N - 1.  Per rank the unmasked MXFP8 launch a rank runs today (hip.attn_fwd_fp8_chunked)
and, per mask, the windowed MXFP8 launch beside the windowed bf16 launch of the same mask on the same rows (hip.attn_fwd_window(...,
q_offset=)), alternating inside every round; per arm its spread against itself.  No condition.

usage: attn_window_bench.py [--iters=10] [--rounds=7] [--out=profiles/attn_window_bench.json]
       attn_window_bench.py --rank-of=8 [--out=profiles/attn_window_sp_bench.json]
       attn_window_bench.py --rank-of=8 --sage [--out=profiles/attn_window_sp_sage_bench.json]
       attn_window_bench.py --rank-of=8 --halo [--out=profiles/attn_window_halo_bench.json]
       attn_window_bench.py --sage [--base=path/to/parent/libflexam_hip.so] [--out=profiles/attn_window_sage_bench.json]
       attn_window_bench.py --sink=0,448,896 [--base=path/to/parent/libflexam_hip.so] [--out=profiles/attn_window_sink_bench.json]
       attn_window_bench.py --frames[=2,5,12] [--sink=0,448] [--base=path/to/parent/libflexam_hip.so] [--out=profiles/attn_window_frames_bench.json]"""
import json
import os
import statistics
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402
from flexam_amd import hip as H  # noqa: E402

opt = {a.split("=")[0][2:]: a.partition("=")[2] for a in sys.argv[1:] if a.startswith("--")}
iters, rounds = int(opt.get("iters", 10)), int(opt.get("rounds", 7))
frames = [int(n) for n in (opt["frames"] or "2,5,12").split(",")] if "frames" in opt else None
sinks = [int(s) for s in opt["sink"].split(",")] if "sink" in opt else [0, 448] if frames is not None else None
out_path = os.path.join(root, opt.get("out", "profiles/attn_window_frames_bench.json" if frames is not None else
                                      "profiles/attn_window_bench.json" if sinks is None else "profiles/attn_window_sink_bench.json"))
B, heads, L, D = 2, 24, 11648, 128
FRAME = 448
g = torch.Generator().manual_seed(0)
q, k, v = ((torch.randn(B, L, heads, D, generator=g) * s).to(torch.bfloat16).cuda() for s in (0.35, 1.0, 1.0))      # q in exp2 units: logits of std ~4
o = torch.empty_like(q)

WINDOWS = [(f"window_{n}_frames", (FRAME * n, FRAME * n)) for n in (frames or (2, 5, 12))]
# an arm: (name, window, sink, frame_tokens); frame_tokens = 0: the window counts tokens
if frames is not None:
    FRAME_WINDOWS = [(f"frames_{n}_{n}", (n, n)) for n in frames] + [("frames_block_causal", (-1, 0)), ("frames_per_frame", (0, 0))]
    ARMS = [("full", None, 0, 0)] + [(f"{name}_sink_{s}", w, s, FRAME) for name, w in FRAME_WINDOWS for s in sinks]
    ARMS += [(f"tokens_{n}_{n}_sink_{s}", (FRAME * n, FRAME * n), s, 0) for n in frames for s in sinks]      # the token window of the same span
elif sinks is None:
    ARMS = [("full", None, 0, 0)] + [(name, w, 0, 0) for name, w in WINDOWS] + [("causal", (-1, 0), 0, 0)]
else:
    ARMS = [("full", None, 0, 0)] + [(f"{name}_sink_{s}", w, s, 0) for name, w in WINDOWS for s in sinks]


def launch(window, sink=0, frame_tokens=0, out=o):
    if window is None:
        H.attn_fwd(q, k, v, out=out, prescaled=True)
    elif frame_tokens:
        H.attn_fwd_window(q, k, v, window, out=out, prescaled=True, sink=sink, frame_tokens=frame_tokens)
    elif sink:
        H.attn_fwd_window(q, k, v, window, out=out, prescaled=True, sink=sink)
    else:
        H.attn_fwd_window(q, k, v, window, out=out, prescaled=True)


def share(window, sink=0, frame_tokens=0):
    window = window if window is not None else (-1, -1)
    runs = H.attn_window_frames_tiles(L, window, frame_tokens, sink) if frame_tokens else H.attn_window_sink_tiles(L, window, sink)
    return sum(b - a + 1 for r in runs for a, b in r) / (H.attn_units(1, L) * H.attn_kv_tiles(L))


def timed(window, sink=0, frame_tokens=0):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        launch(window, sink, frame_tokens)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def timed_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def sage_bench():
    """--sage: see the module docstring."""
    bufs = H.attn_fp8_pack(q, k, v)
    masks = [(f"tokens_{n}_{n}_sink_{s}", (FRAME * n, FRAME * n), s, 0) for n in (2, 5, 12) for s in (0, FRAME)]
    masks += [(f"{name}_sink_{s}", w, s, FRAME) for name, w in [(f"frames_{n}_{n}", (n, n)) for n in (2, 5, 12)] +
              [("frames_block_causal", (-1, 0)), ("frames_per_frame", (0, 0))] for s in (0, FRAME)]
    calls = {"full": lambda: H.attn_fwd_fp8(bufs, L, out=o), "full_bf16": lambda: launch(None)}
    for name, w, s, ft in masks:
        calls[name] = lambda w=w, s=s, ft=ft: H.attn_fwd_fp8(bufs, L, out=o, window=w, sink=s, frame_tokens=ft)
        calls[name + "/bf16"] = lambda w=w, s=s, ft=ft: launch(w, s, ft)
    for fn in calls.values():                      # warm-up: every instance once
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            ms[name].append(timed_call(fn))
    med = {name: statistics.median(x) for name, x in ms.items()}
    arms = dict(full=dict(ms=round(med["full"], 4), ms_min=round(min(ms["full"]), 4), ms_max=round(max(ms["full"]), 4), bf16_ms=round(med["full_bf16"], 4),
                          mxfp8_over_bf16=round(med["full"] / med["full_bf16"], 4)))
    print(f"{'full':32s} {med['full']:8.3f} ms  bf16 {med['full_bf16']:8.3f} ms  mxfp8 / bf16 {med['full'] / med['full_bf16']:6.3f}")
    for name, w, s, ft in masks:
        t, tb, sh = med[name], med[name + "/bf16"], share(w, 0 if w[0] < 0 else s, ft)
        arms[name] = dict(window=list(w), sink=s, frame_tokens=ft, ms=round(t, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                          tile_share=round(sh, 4), time_ratio=round(t / med["full"], 4), time_per_tile_ratio=round(t / med["full"] / sh, 3),
                          bf16_ms=round(tb, 4), bf16_time_ratio=round(tb / med["full_bf16"], 4), mxfp8_over_bf16=round(t / tb, 4))
        print(f"{name:32s} {t:8.3f} ms  tiles {sh:6.4f}  of full mxfp8 {t / med['full']:6.3f}  bf16 same mask {tb:8.3f} ms  mxfp8 / bf16 {t / tb:6.3f}")
    rec = dict(shape=dict(B=B, H=heads, L=L, head_dim=D, frame_tokens=FRAME), iters=iters, rounds=rounds, device=torch.cuda.get_device_name(0),
               method="one process, every MXFP8 arm and the bf16 windowed launch of the same mask alternating per round, device events around "
                      "`iters` back-to-back launches, median over the rounds; time_ratio: of the full MXFP8 launch (hip.attn_fwd_fp8)",
               arms=arms, windowed_mxfp8_faster_than_windowed_bf16={name: bool(med[name] < med[name + "/bf16"]) for name, *_ in masks})
    if opt.get("base"):
        import ctypes
        base_lib, new_lib = ctypes.CDLL(os.path.abspath(opt["base"])), H.load_library(H.LIB_PATH)
        for fn_name, (argtypes, restype) in H._SIGNATURES.items():
            fn = getattr(base_lib, fn_name, None)
            if fn is not None:
                fn.argtypes, fn.restype = argtypes, restype
        libs = {"base_a": base_lib, "new": new_lib, "base_b": base_lib}
        outs = {tag: torch.empty_like(q) for tag in ("base_a", "new")}
        both = {"mxfp8_full": lambda out=o: H.attn_fwd_fp8(bufs, L, out=out), "bf16_full": lambda out=o: launch(None, out=out)}
        same, ab = {}, {name: {tag: [] for tag in libs} for name in both}
        for name, fn in both.items():              # warm-up of both builds, and the bytes they give
            for tag in outs:
                H._lib = libs[tag]
                fn(outs[tag])
            torch.cuda.synchronize()
            same[name] = bool(torch.equal(outs["base_a"], outs["new"]))
        order = list(libs)
        for r in range(rounds):
            for name, fn in both.items():
                for tag in order[r % 3:] + order[:r % 3]:
                    H._lib = libs[tag]
                    ab[name][tag].append(timed_call(fn))
        H._lib = new_lib
        rec["unwindowed_against_base"] = dict(method="the unwindowed MXFP8 launch (hip.attn_fwd_fp8) and the full bf16 launch (hip.attn_fwd) of the base build "
                                              "and of the in-tree build in this process: per round base, in-tree, base again in rotating order; margin = the "
                                              "base build against itself", launches={})
        for name in both:
            a, n, b = (statistics.median(ab[name][tag]) for tag in libs)
            base = statistics.median(ab[name]["base_a"] + ab[name]["base_b"])
            margin = abs(a - b) / base
            rec["unwindowed_against_base"]["launches"][name] = dict(base_a_ms=round(a, 4), base_b_ms=round(b, 4), new_ms=round(n, 4), margin=round(margin, 4),
                                                                    new_over_base=round(n / base, 4), slower_beyond_margin=bool(n / base > 1 + margin),
                                                                    same_bytes=same[name])
            print(f"{name:12s} base {a:7.3f} / {b:7.3f} ms  in-tree {n:7.3f} ms  new / base {n / base:6.4f}  margin {margin:6.4f}  same bytes {same[name]}")
    path = os.path.join(root, opt.get("out", "profiles/attn_window_sage_bench.json"))
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", path)


def rank_bench(N):
    """--rank-of=N: see the module docstring."""
    Lq, n_tiles = -(-L // N), H.attn_kv_tiles(L)
    q_pad = torch.zeros(B, N * Lq, heads, D, dtype=torch.bfloat16, device="cuda")       # the sequence padded over the ranks, zero pad rows
    q_pad[:, :L] = q
    out = torch.empty(B, Lq, heads, D, dtype=torch.bfloat16, device="cuda")
    masks = [(f"tokens_{n}_{n}_sink_{s}", (FRAME * n, FRAME * n), s, 0) for n in (2, 5, 12) for s in (0, FRAME)]
    masks += [(f"{name}_sink_{s}", w, s, FRAME) for name, w in [(f"frames_{n}_{n}", (n, n)) for n in (2, 5, 12)] +
              [("frames_block_causal", (-1, 0)), ("frames_per_frame", (0, 0))] for s in (0, FRAME)]
    units = H.attn_units(B * heads, Lq)
    rec = dict(shape=dict(B=B, H=heads, Lk=L, Lq=Lq, ranks=N, head_dim=D, frame_tokens=FRAME, prescaled=True), work_units=units, iters=iters, rounds=rounds,
               device=torch.cuda.get_device_name(0),
               method="one process, per rank the unmasked launch (hip.attn_fwd on (Lq, Lk): the launch a rank runs today, tail split and merge "
                      "included) and every windowed launch at the rank's offset (hip.attn_fwd_window(..., q_offset=)) alternating per round, device "
                      "events around `iters` back-to-back launches, median over the rounds; time_ratio: of the unmasked launch of the same rank; "
                      "tile_share: hip.attn_window_at_tiles over (query blocks x key tiles)", ranks={})
    for rank in sorted({0, N // 2, N - 1}):
        off = rank * Lq
        qr = q_pad[:, off:off + Lq]
        calls = {"full": lambda: H.attn_fwd(qr, k, v, out=out, prescaled=True)}
        for name, w, s, ft in masks:
            calls[name] = lambda w=w, s=s, ft=ft: H.attn_fwd_window(qr, k, v, w, out=out, prescaled=True, sink=s, frame_tokens=ft, q_offset=off)
        for fn in calls.values():                      # warm-up: every instance once
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in calls}
        for _ in range(rounds):
            for name, fn in calls.items():
                ms[name].append(timed_call(fn))
        med = {name: statistics.median(x) for name, x in ms.items()}
        arms = dict(full=dict(ms=round(med["full"], 4), ms_min=round(min(ms["full"]), 4), ms_max=round(max(ms["full"]), 4)))
        print(f"rank {rank} of {N} (rows {off} .. {off + Lq - 1}), {units} work units: unmasked {med['full']:.3f} ms")
        for name, w, s, ft in masks:
            runs = H.attn_window_at_tiles(Lq, L, off, w, s, ft)
            sh = sum(b - a + 1 for r in runs for a, b in r) / (len(runs) * n_tiles)
            t = med[name]
            arms[name] = dict(window=list(w), sink=s, frame_tokens=ft, ms=round(t, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                              tile_share=round(sh, 4), time_ratio=round(t / med["full"], 4), time_per_tile_ratio=round(t / med["full"] / sh, 3))
            print(f"  {name:30s} {t:8.3f} ms  tiles {sh:6.4f}  time {t / med['full']:6.3f}  per tile {t / med['full'] / sh:5.2f}")
        rec["ranks"][str(rank)] = dict(q_offset=off, arms=arms)
    path = os.path.join(root, opt.get("out", "profiles/attn_window_sp_bench.json"))
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", path)


def halo_bench(N):
    """--rank-of=N --halo: see the module docstring."""
    from flexam_amd.dit_layout import halo_plan
    Lq = -(-L // N)
    q_pad = torch.zeros(B, N * Lq, heads, D, dtype=torch.bfloat16, device="cuda")
    q_pad[:, :L] = q
    outs = [torch.empty(B, Lq, heads, D, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    masks = [(f"tokens_{n}_{n}_sink_{s}", (FRAME * n, FRAME * n), s, 0) for n in (2, 5, 12) for s in (0, FRAME)]
    masks += [(f"{name}_sink_{s}", w, s, FRAME) for name, w in [(f"frames_{n}_{n}", (n, n)) for n in (2, 5, 12)] +
              [("frames_block_causal", (-1, 0)), ("frames_per_frame", (0, 0))] for s in (0, FRAME)]
    rec = dict(shape=dict(B=B, H=heads, Lk=L, Lq=Lq, ranks=N, head_dim=D, frame_tokens=FRAME, prescaled=True), iters=iters, rounds=rounds,
               device=torch.cuda.get_device_name(0), gather_remote_rows=L - Lq,
               method="one process; per rank and mask the launch on the full keys (hip.attn_fwd_window(..., q_offset=)) and the launch on the "
                      "compact buffer dit_layout.halo_plan lays out (..., key_gap_tiles=, Lk=), three arms per round -- full keys, halo, full keys, "
                      "the order rotating --, device events around `iters` back-to-back launches, median over the rounds; the two launches "
                      "must give the same bytes; margin: the full-key launch against itself; remote_rows: what the rank receives, of "
                      "gather_remote_rows under the K|V gather", ranks={})
    for rank in sorted({0, N // 2, N - 1}):
        off = rank * Lq
        qr = q_pad[:, off:off + Lq]
        arms = {}
        print(f"rank {rank} of {N} (rows {off} .. {off + Lq - 1})")
        for name, w, s, ft in masks:
            plan = halo_plan(L, N, rank, w, s, ft)
            s_n = -(-min(s, L) // H.ATTN_KV_TILE) if w[0] >= 0 else 0
            rows = torch.arange(plan.rows, device="cuda")
            rows = torch.where(rows < s_n * H.ATTN_KV_TILE, rows, rows + plan.gap * H.ATTN_KV_TILE)
            kc, vc = k[:, rows].contiguous(), v[:, rows].contiguous()
            at = lambda out: H.attn_fwd_window(qr, k, v, w, out=out, prescaled=True, sink=s, frame_tokens=ft, q_offset=off)
            halo = lambda out: H.attn_fwd_window(qr, kc, vc, w, out=out, prescaled=True, sink=s, frame_tokens=ft, q_offset=off,
                                                 key_gap_tiles=plan.gap, Lk=L)
            at(outs[0])
            halo(outs[1])
            torch.cuda.synchronize()
            same = bool(torch.equal(outs[0], outs[1]))
            calls = [("at_a", lambda: at(outs[0])), ("halo", lambda: halo(outs[1])), ("at_b", lambda: at(outs[0]))]
            ms = {n: [] for n, _ in calls}
            for r in range(rounds):
                for n, fn in calls[r % 3:] + calls[:r % 3]:
                    ms[n].append(timed_call(fn))
            med = {n: statistics.median(x) for n, x in ms.items()}
            pooled = statistics.median(ms["at_a"] + ms["at_b"])
            margin = abs(med["at_a"] - med["at_b"]) / pooled
            ratio = med["halo"] / pooled
            remote = sum(n for *_, n in plan.recvs)
            arms[name] = dict(window=list(w), sink=s, frame_tokens=ft, key_gap_tiles=plan.gap, buffer_rows=plan.rows, remote_rows=remote,
                              remote_share=round(remote / (L - Lq), 4), whole_sequence=plan.gap == 0 and plan.rows == L, same_bytes=same,
                              at_ms=round(pooled, 4), at_a_ms=round(med["at_a"], 4), at_b_ms=round(med["at_b"], 4), halo_ms=round(med["halo"], 4),
                              halo_ms_min=round(min(ms["halo"]), 4), halo_ms_max=round(max(ms["halo"]), 4), margin=round(margin, 4),
                              halo_over_at=round(ratio, 4), slower_beyond_margin=bool(ratio > 1 + margin))
            print(f"  {name:30s} at {pooled:7.3f} ms  halo {med['halo']:7.3f} ms  ratio {ratio:6.4f} (margin {margin:6.4f})  rows {plan.rows:6d} "
                  f"remote {remote:6d} of {L - Lq}  same bytes {same}")
        rec["ranks"][str(rank)] = dict(q_offset=off, arms=arms)
    path = os.path.join(root, opt.get("out", "profiles/attn_window_halo_bench.json"))
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", path)


def rank_sage_bench(N):
    """--rank-of=N --sage: see the module docstring."""
    tile = H.ATTN_KV_TILE
    lc = tile * -(-L // (tile * N))                    # resolve_mode pads the record gather to 64 x ranks
    pad = lambda t: torch.cat([t, torch.zeros(B, N * lc - L, heads, D, dtype=t.dtype, device=t.device)], dim=1)
    q_pad, k_pad, v_pad = pad(q), pad(k), pad(v)
    packed = [H.attn_fp8_pack(*(t[:, r * lc:(r + 1) * lc] for t in (q_pad, k_pad, v_pad))) for r in range(N)]
    recs = torch.stack([p[2] for p in packed]).contiguous()      # [N][B][H][lc / 64] records, rank-major: what the all-gather leaves
    out = torch.empty(B, lc, heads, D, dtype=torch.bfloat16, device="cuda")
    masks = [(f"frames_{n}_{n}_sink_{s}", (n, n), s, FRAME) for n in (2, 5, 12) for s in (0, FRAME)]
    units, n_tiles = H.attn_units(B * heads, lc), H.attn_kv_tiles(L)
    rec = dict(shape=dict(B=B, H=heads, Lk=L, Lq=lc, ranks=N, chunk_tiles=lc // tile, head_dim=D, frame_tokens=FRAME), work_units=units, iters=iters,
               rounds=rounds, device=torch.cuda.get_device_name(0),
               note=f"Lq = {lc} rows a rank: the record gather pads the sequence to 64 x ranks; the bf16 K|V gather's chunk is {-(-L // N)} rows "
                    f"(profiles/attn_window_sp_bench.json).  The bf16 arm here runs on the same {lc} rows at the same offset, so the two windowed "
                    "launches of a mask do the same work",
               bytes_per_key_and_head=dict(mxfp8_records=288, bf16_rows=512, note="whole chunks travel either way"),
               method="one process, per rank the unmasked MXFP8 launch on the gathered records (hip.attn_fwd_fp8_chunked: the launch a rank runs "
                      "today, tail split and merge included) and, per mask, the windowed MXFP8 launch at the rank's offset "
                      "(hip.attn_fwd_fp8_chunked(..., window=, q_offset=)) and the windowed bf16 launch of the same mask and rows "
                      "(hip.attn_fwd_window(..., q_offset=)) alternating per round, device events around `iters` back-to-back launches, median "
                      "over the rounds; ms_min / ms_max: the arm's spread against itself; tile_share: hip.attn_window_at_tiles over (query "
                      "blocks x key tiles)",
               not_measured=["no multi-GPU run", "no link time", "no in-step figure", "no quality figure on a real checkpoint"], ranks={})
    for rank in sorted({0, N // 2, N - 1}):
        off = rank * lc
        q8, qs = packed[rank][0], packed[rank][1]
        qr = q_pad[:, off:off + lc]
        calls = {"full": lambda: H.attn_fwd_fp8_chunked(q8, qs, recs, lc, L, out=out)}
        for name, w, s, ft in masks:
            calls[name] = lambda w=w, s=s, ft=ft: H.attn_fwd_fp8_chunked(q8, qs, recs, lc, L, out=out, window=w, sink=s, frame_tokens=ft, q_offset=off)
            calls[name + "/bf16"] = lambda w=w, s=s, ft=ft: H.attn_fwd_window(qr, k, v, w, out=out, prescaled=True, sink=s, frame_tokens=ft, q_offset=off)
        for fn in calls.values():                      # warm-up: every instance once
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in calls}
        for _ in range(rounds):
            for name, fn in calls.items():
                ms[name].append(timed_call(fn))
        med = {name: statistics.median(x) for name, x in ms.items()}
        arms = dict(full=dict(ms=round(med["full"], 4), ms_min=round(min(ms["full"]), 4), ms_max=round(max(ms["full"]), 4)))
        print(f"rank {rank} of {N} (rows {off} .. {off + lc - 1}), {units} work units: unmasked MXFP8 {med['full']:.3f} ms")
        for name, w, s, ft in masks:
            runs = H.attn_window_at_tiles(lc, L, off, w, s, ft)
            sh = sum(b - a + 1 for r in runs for a, b in r) / (len(runs) * n_tiles)
            t, tb = med[name], med[name + "/bf16"]
            arms[name] = dict(window=list(w), sink=s, frame_tokens=ft, ms=round(t, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                              tile_share=round(sh, 4), time_ratio=round(t / med["full"], 4), bf16_ms=round(tb, 4), bf16_ms_min=round(min(ms[name + "/bf16"]), 4),
                              bf16_ms_max=round(max(ms[name + "/bf16"]), 4), mxfp8_over_bf16=round(t / tb, 4),
                              slower_than_unmasked=bool(t > med["full"]))
            print(f"  {name:24s} {t:8.3f} ms (min {min(ms[name]):.3f}, max {max(ms[name]):.3f})  tiles {sh:6.4f}  of unmasked {t / med['full']:6.3f}  "
                  f"bf16 same mask {tb:8.3f} ms  mxfp8 / bf16 {t / tb:6.3f}")
        rec["ranks"][str(rank)] = dict(q_offset=off, arms=arms)
    path = os.path.join(root, opt.get("out", "profiles/attn_window_sp_sage_bench.json"))
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", path)


if "rank-of" in opt and "sage" in opt:
    rank_sage_bench(int(opt["rank-of"] or 8))
    sys.exit(0)
if "sage" in opt:
    sage_bench()
    sys.exit(0)
if "rank-of" in opt and "halo" in opt:
    halo_bench(int(opt["rank-of"] or 8))
    sys.exit(0)
if "rank-of" in opt:
    rank_bench(int(opt["rank-of"] or 8))
    sys.exit(0)

for _, w, s, ft in ARMS:                           # warm-up: every instance once (LDS attribute, code load), then the clock
    launch(w, s, ft)
for _ in range(3):
    launch(None)
torch.cuda.synchronize()
ms = {name: [] for name, _, _, _ in ARMS}
for _ in range(rounds):
    for name, w, s, ft in ARMS:
        ms[name].append(timed(w, s, ft))
full = statistics.median(ms["full"])
arms, ok = {}, True
for name, w, s, ft in ARMS:
    t, sh = statistics.median(ms[name]), share(w, s, ft)
    arms[name] = dict(window=list(w) if w else None, ms=round(t, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                      tile_share=round(sh, 4), time_ratio=round(t / full, 4), time_per_tile_ratio=round(t / full / sh, 3))
    if sinks is not None and w is not None:
        arms[name]["sink"] = s
    if frames is not None and w is not None:
        arms[name]["frame_tokens"] = ft
    if w is not None and sh <= 0.5 and not t < full:
        ok = False
    print(f"{name:28s} {t:8.3f} ms (min {min(ms[name]):.3f}, max {max(ms[name]):.3f})  tiles {sh:6.4f}  time {t / full:6.3f}  per tile {t / full / sh:5.2f}")
if frames is not None:                             # beside each +-k frame arm: the token window of the same span
    for n in frames:
        for s in sinks:
            fr, tk = arms[f"frames_{n}_{n}_sink_{s}"], arms[f"tokens_{n}_{n}_sink_{s}"]
            fr["token_window_same_span"] = f"tokens_{n}_{n}_sink_{s}"
            fr["time_over_token_window"] = round(fr["ms"] / tk["ms"], 4)
            fr["faster_per_visited_tile"] = "frames" if fr["ms"] / fr["tile_share"] < tk["ms"] / tk["tile_share"] else "tokens"
            print(f"+-{n} frames, sink {s}: frames / tokens time {fr['ms'] / tk['ms']:6.3f}, per visited tile {fr['time_per_tile_ratio']:5.3f} / "
                  f"{tk['time_per_tile_ratio']:5.3f} of the full call's: {fr['faster_per_visited_tile']} faster per tile")
rec = dict(shape=dict(B=B, H=heads, L=L, head_dim=D, prescaled=True), iters=iters, rounds=rounds, device=torch.cuda.get_device_name(0),
           method="one process, arms alternating per round, device events around `iters` back-to-back launches, median over the rounds",
           arms=arms, condition="every window that visits at most half the tiles is faster than the full call of the same run",
           condition_met=ok)

if sinks is not None and opt.get("base"):
    # sink = 0 (--frames: the token windows) against a parent build: base, in-tree, base again per window and round, rotating; hip._lib switches the build
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
    # the launches both builds have: sink = 0 (--sink), or the token windows (frame_tokens = 0) with every sink of the list (--frames)
    AB = [(name, w, 0) for name, w in WINDOWS] if frames is None else [(f"{name}_sink_{s}", w, s) for name, w in WINDOWS for s in sinks]
    for tag in outs:                               # warm-up of both builds, and the bytes they give
        H._lib = libs[tag]
        for _, w, s in AB:
            launch(w, s, 0, outs[tag])
    torch.cuda.synchronize()
    ab = {name: {tag: [] for tag in libs} for name, _, _ in AB}
    same = {}
    for name, w, s in AB:
        for tag in outs:
            H._lib = libs[tag]
            launch(w, s, 0, outs[tag])
        torch.cuda.synchronize()
        same[name] = bool(torch.equal(outs["base_a"], outs["new"]))
    order = list(libs)
    for r in range(rounds):
        for name, w, s in AB:
            for tag in order[r % 3:] + order[:r % 3]:
                H._lib = libs[tag]
                ab[name][tag].append(timed(w, s))
    H._lib = new_lib
    key = "sink_0_against_base" if frames is None else "token_windows_against_base"
    rec[key] = dict(method=("sink = 0 launches" if frames is None else "token-window launches (frame_tokens = 0)") + " (hip.attn_fwd_window) of the base build "
                    "and of the in-tree build in this process: per window and round base, in-tree, base again in rotating order; margin = the base "
                    "build against itself", windows={})
    for name, w, s in AB:
        a, n, b = (statistics.median(ab[name][tag]) for tag in libs)
        base = statistics.median(ab[name]["base_a"] + ab[name]["base_b"])
        margin = abs(a - b) / base
        rec[key]["windows"][name] = dict(window=list(w), sink=s, base_a_ms=round(a, 4), base_b_ms=round(b, 4), new_ms=round(n, 4),
                                         margin=round(margin, 4), new_over_base=round(n / base, 4),
                                         slower_beyond_margin=bool(n / base > 1 + margin), same_bytes=same[name])
        print(f"sink {s}, {name:26s} base {a:7.3f} / {b:7.3f} ms  in-tree {n:7.3f} ms  new / base {n / base:6.4f}  margin {margin:6.4f}  same bytes {same[name]}")

with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print("wrote", out_path, "condition met" if ok else "CONDITION NOT MET")
sys.exit(0 if ok else 1)
