"""What a forward of the DiT engine decides before it launches anything, as functions of plain values: the token layout of a
sequence-parallel rank, the key ranges and partial-softmax slots of the overlapped K|V gather, the o-projection's A offsets behind
the all-to-all over heads, and the resolution of the environment switches into a parallel layout (DiTEngine.set_parallel) and a
forward mode (DiTEngine._mode).  No tensors and no GPU: tests/test_dit_layout_cpu.py pins every one of them on a CPU host."""
from collections import namedtuple

from . import hip
from .dist import chunk_bounds, padded_len, real_tokens

# What the block and head launches of one forward depend on apart from buffer contents and addresses, resolved once at the start of
# DiTEngine.run (resolve_mode): the stages read it, and a recorded launch plan is keyed on it
_Mode = namedtuple("_Mode", "B Lp lc tok0 R rows_per_batch only_row "                                 # sizes (Lp: padded sequence)
                   "per_layer share0 sage sage_gather sage_fused fp8 fp8_oproj ffn_apriori "        # switches
                   "sp rank sp_mode sp_pieces sp_overlap_level sp_fused_qkv use_plan")              # layout

Parallel = namedtuple("Parallel", "sp_mode sp_overlap_level sp_pieces sp_fused_qkv")
SINGLE_RANK = Parallel(sp_mode=None, sp_overlap_level=0, sp_pieces=1, sp_fused_qkv=True)            # before any set_parallel

# sizes of the key ranges (local, before, after) of a rank, the splits requested for each (0: empty range), the partial-softmax slots
# they really take, and the slots of all three: what sizes the merge workspace
KeyRanges = namedtuple("KeyRanges", "sizes splits slots total")


def token_layout(L: int, sp: int, rank: int, unit: int = None):
    """(Lp, lc, tok0): the sequence padded to a multiple of `unit` (sp, or sp * ATTN_KV_TILE when MXFP8 records are gathered: every
    chunk is then a whole number of key tiles), the rows of a rank's chunk and the global index of its first token.
    A sequence that does not divide over the ranks is padded with zero tokens at its end, as the reference does (FX.py:919-925);
    they are rows like any other in every token-local op, never keys of self-attention (the key ranges end at L), and the head
    gather drops them."""
    Lp = padded_len(L, sp if unit is None else unit)
    tok0, end = chunk_bounds(Lp, rank, sp)
    return Lp, end - tok0, tok0


def key_range_sizes(L: int, sp: int, rank: int):
    """The overlapped K|V gather attends in up to three partial calls: to the LOCAL chunk's real tokens (straight from the send
    buffer), then to the real tokens BEFORE and AFTER it in the gathered buffer; pad rows are in none of them."""
    start, end = chunk_bounds(L, rank, sp)
    return real_tokens(L, rank, sp), min(start, L), max(0, L - end)


def gather_key_ranges(L: int, sp: int, rank: int, batch_heads: int) -> KeyRanges:
    """key_range_sizes with the splits planned for them.  batch_heads: (samples x heads) of one call, the heads of piece 0."""
    sizes = key_range_sizes(L, sp, rank)
    start, end = chunk_bounds(L, rank, sp)
    units = hip.attn_units(batch_heads, end - start)
    # no CU count passed: these ranges are planned for the planner's default of 256 CUs, whatever FLEXAM_CU_BUDGET says
    splits = tuple(hip.attn_partial_splits(units, hip.attn_kv_tiles(n)) if n else 0 for n in sizes)
    slots = tuple(hip.attn_effective_splits(n, s) if n else 0 for n, s in zip(sizes, splits))
    return KeyRanges(sizes, splits, slots, sum(slots))


def a2a_koff(d: int, G: int, rows: int):
    """Element offset of every 64-wide K block of the o-projection's A operand behind the all-to-all over heads: the attention
    output returns as one [rows, G] block per rank, so column c of the [rows, d] matrix lies in block c // G at column c % G."""
    return [(kb * 64 // G) * (rows * G) + (kb * 64) % G for kb in range(d // 64)]


def resolve_parallel(env, nh: int, sp_size: int) -> Parallel:
    """FLEXAM_SP_MODE / FLEXAM_SP_OVERLAP / FLEXAM_SP_PIECES / FLEXAM_SP_FUSED_QKV for `sp_size` ranks and `nh` heads."""
    mode = env.get("FLEXAM_SP_MODE", "allgather")
    if mode not in ("ulysses", "allgather"):
        raise ValueError(f"FLEXAM_SP_MODE={mode!r}: expected 'ulysses' or 'allgather'")
    if nh % max(sp_size, 1):
        mode = "allgather"                      # (the all-to-all needs the heads to divide over the ranks)
    # FLEXAM_SP_OVERLAP.  K|V all-gather: 0 (default since r6) = ONE gather per block and CFG row, waited for, then ONE ordinary
    # attention call; 1 = head-group pieces with local-chunk-first partial attention + merge underneath them.  r5 measured the
    # overlap machinery at 6.7 ms of a 48 ms rank step at 8 GPUs (three partial calls parking 17 fp32 slots for a merge: 605 us of
    # attention per block against 342 for the one call; profiles/r5o_*): it pays only on links slow enough that hiding ~0.3 ms of
    # a block's gather is worth 0.22 ms of compute, which bench.py's layout probe measures per node -- the default is the form
    # that is fastest on compute.  All-to-all over heads: 1 (default) = a sample's blocks leave under the other sample's projection,
    # 2 = attention per sample as well, 0 = one exchange for the pair.
    ov = env.get("FLEXAM_SP_OVERLAP")
    ov = ("1" if mode == "ulysses" else "0") if ov is None else ov.strip().lower()
    level = 0 if ov in ("0", "off", "false", "no", "") else (2 if ov == "2" else 1)      # anything else: on (1)
    # with the overlap on, the K|V gather is cut into `sp_pieces` groups of heads, one collective each: the attention of a group starts
    # when ITS piece has landed, the later pieces travel underneath it.  Default: 2 pieces from 4 chunks on (3+ peers: the gather
    # outlasts the local-chunk attention it hides under), 1 below and whenever the gather is waited for (two attention calls on half
    # the heads each fill 256 CUs worse than one: 44.2 against 41.4 ms per rank step, profiles/r5o_*)
    pieces = env.get("FLEXAM_SP_PIECES")
    pieces = int(pieces) if pieces is not None else (2 if (sp_size >= 4 and nh % 2 == 0 and level and mode == "allgather") else 1)
    if mode != "allgather":
        pieces = 1                              # (head-group pieces belong to the gather)
    if pieces < 1 or nh % pieces:
        raise ValueError(f"FLEXAM_SP_PIECES={pieces}: must divide the {nh} heads")
    return Parallel(mode, level, pieces if sp_size > 1 else 1, env.get("FLEXAM_SP_FUSED_QKV", "1") != "0")


def sage_asked(env) -> bool:
    """The reference reads the switch at every attention call (attention_utils.py:195)."""
    return env.get("VIDEOX_ATTENTION_TYPE", "FLASH_ATTENTION") == "SAGE_ATTENTION"


def smooth_k_asked(env) -> bool:
    """FLEXAM_SAGE_SMOOTH_K=1 (default 0): quantise K - mean_tokens(K) in the MXFP8 self-attention.  Not a field of _Mode: DiTEngine._mode
    keeps it beside the mode (it holds for `sage and sp == 1` only) and keys its launch plans on it."""
    return env.get("FLEXAM_SAGE_SMOOTH_K", "0") == "1"


def smooth_v_asked(env) -> bool:
    """FLEXAM_SAGE_SMOOTH_V=1 (default 0): quantise V - mean_tokens(V) in the MXFP8 self-attention and add the mean back to its output
    in fp32.  Independent of smooth-K and kept like it: beside the mode in DiTEngine._mode (`sage and sp == 1` only), in the plan key."""
    return env.get("FLEXAM_SAGE_SMOOTH_V", "0") == "1"


def sage_window_asked(env) -> bool:
    """FLEXAM_SAGE_WINDOW=1 (default 0): a windowed self-attention (window_size / window_frames, with window_sink) under SAGE_ATTENTION
    runs the windowed MXFP8 kernel instead of falling back to the windowed bf16 one.  Not a field of _Mode: with it the mode keeps
    `sage`, without it DiTEngine._mode clears it, so the two forwards already differ in their mode and their launch plans."""
    return env.get("FLEXAM_SAGE_WINDOW", "0") == "1"


def sp_window_asked(env) -> bool:
    """FLEXAM_SP_WINDOW=1 (default 0): a windowed self-attention (window_size / window_frames, with window_sink) under sequence
    parallelism runs the windowed bf16 kernel at each rank's query offset (flexam_attn_fwd_window_at) instead of being refused: one call
    per head-group piece of the K|V gather on the gathered keys, or on the rank's heads behind the all-to-all.  Not a field of _Mode:
    without it DiTEngine._mode and _SelfAttn.forward raise before any mode exists."""
    return env.get("FLEXAM_SP_WINDOW", "0") == "1"


def sp_sage_window_asked(env) -> bool:
    """FLEXAM_SP_SAGE_WINDOW=1 (default 0): on top of FLEXAM_SP_WINDOW=1, SAGE_ATTENTION and FLEXAM_SAGE_WINDOW=1 -- it acts with all
    three only -- a windowed self-attention under the K|V gather exchanges the MXFP8 records as an unmasked model does and runs the
    windowed MXFP8 kernel at each rank's query offset on them (flexam_attn_fwd_fp8_window_at; dit_sp.RecordGather) instead of gathering
    bf16 K|V for the windowed bf16 kernel.  Not a field of _Mode: with it the mode keeps `sage` / `sage_gather`, without it
    DiTEngine._mode never asks resolve_mode for the record gather, so the two forwards differ in their mode and their launch plans."""
    return (env.get("FLEXAM_SP_SAGE_WINDOW", "0") == "1" and sp_window_asked(env) and sage_asked(env) and sage_window_asked(env))


def sp_halo_asked(env) -> bool:
    """FLEXAM_SP_HALO=1 (default 0): under FLEXAM_SP_WINDOW=1, the K|V gather and the bf16 kernel, a rank receives only the key rows its
    windowed call visits (halo_plan) into a compact buffer and runs flexam_attn_fwd_window_halo on it (dit_sp.KVHalo).  Not a field of
    _Mode: DiTEngine._mode keeps it beside the mode and keys its launch plans on it."""
    return env.get("FLEXAM_SP_HALO", "0") == "1"


# What a rank's windowed call reads of the sequence's keys, and who holds it (halo_plan).  gap: whole key tiles left out between the sink
# tiles and the window tiles; rows: rows of the compact buffer; local: the rank's own rows in it, [(src_row0, dst_row0, n), ...];
# recvs / sends: [(peer, src_row0, dst_row0, n), ...] -- src in rows of the SENDER's chunk, dst in rows of the RECEIVER's buffer --
# sorted by peer and row, so that the k-th range a rank sends a peer is the k-th that peer receives from it
HaloPlan = namedtuple("HaloPlan", "gap rows local recvs sends")


def _halo_segments(L, sp, rank, window, sink, frame_tokens):
    """(gap, rows, [(key0, key1, buffer_row0), ...]): the key ranges [key0, key1) the compact buffer of `rank` holds, at most two.  From
    the runs hip.attn_window_at_tiles plans for the rank's query blocks, pad rows included (they are queries, and the kernel walks their
    tiles): the sink tiles [0, s_n) are every block's first run; the window runs are non-decreasing in the block, so their union is one
    run from the first block's first window tile to the last window tile of any block, and the first block's gap is the smallest."""
    tile = hip.ATTN_KV_TILE
    _, lc, tok0 = token_layout(L, sp, rank)
    runs = hip.attn_window_at_tiles(lc, L, tok0, window, sink, frame_tokens)
    s_n = -(-min(int(sink), L) // tile) if hip.attn_window(window)[0] >= 0 else 0
    first = runs[0] if runs else []
    gap = first[1][0] - s_n if len(first) == 2 else first[0][0] if first and not s_n else 0
    end = max([r[-1][1] for r in runs if r], default=-1) + 1              # tiles: one behind the last any block visits
    segs = [(0, min(s_n * tile, L), 0)] if s_n else []
    if end > s_n + gap:
        segs.append(((s_n + gap) * tile, min(end * tile, L), s_n * tile))
    if len(segs) == 2 and gap == 0:                                       # the two runs touch: one range
        segs = [(0, segs[1][1], 0)]
    return gap, (segs[-1][1] - segs[-1][0] + segs[-1][2] if segs else 0), segs


def halo_plan(L: int, sp: int, rank: int, window, sink: int = 0, frame_tokens: int = 0) -> HaloPlan:
    """Which key rows travel to `rank` of `sp` for its windowed self-attention call (flexam_attn_fwd_window_halo), and which it sends.
    The compact buffer is tile-aligned: the sink tiles, then the window tiles from global tile s_n + gap on, a last tile cut at L; every
    row of it is a planned row (the rank's own, or one peer's), so no tile a unit can visit holds a row nobody wrote.  Pad rows (global
    tokens from L on) are never keys.  Remote rows are at most the rows some query of the rank sees plus 3 x (ATTN_KV_TILE - 1): tile
    alignment at the end of the sink run and at both ends of the window run.  gap = 0 and rows = L is the whole sequence: the call of
    flexam_attn_fwd_window_at.  GPU-free; every rank can state every other rank's plan, which is how the sends are derived."""
    lc = token_layout(L, sp, rank)[1]
    chunk = lambda r: (r * lc, max(r * lc, min((r + 1) * lc, L)))         # the real rows of rank r
    gap, rows, segs = _halo_segments(L, sp, rank, window, sink, frame_tokens)

    def pieces(segments, holder):                                         # (src_row0, dst_row0, n) of `segments` held by `holder`
        h0, h1 = chunk(holder)
        out = []
        for k0, k1, d0 in segments:
            a, b = max(k0, h0), min(k1, h1)
            if a < b:
                out.append((a - h0, d0 + a - k0, b - a))
        return out

    recvs = [(p, *x) for p in range(sp) if p != rank for x in pieces(segs, p)]
    sends = [(p, *x) for p in range(sp) if p != rank for x in pieces(_halo_segments(L, sp, p, window, sink, frame_tokens)[2], rank)]
    return HaloPlan(gap, rows, pieces(segs, rank), recvs, sends)


def resolve_mode(env, *, fused, nl, nh, hd, dim, table_limit, fp8, sp, rank, parallel: Parallel, B, L, dens_same,
                 bx, R, rows_per_batch, only_row, rows_shared, teacache: bool, record_gather: bool = True) -> _Mode:
    """The mode of one forward.  env: the environment mapping; fused .. parallel: the engine (all blocks native, layers, heads, head
    width, model width, byte limit of the all-layer AdaLN table, enable_fp8, ranks, this rank, set_parallel's resolution); B, L,
    dens_same: the clip (samples, real tokens, all samples carry one density); the rest: the call (samples of the latent, table rows,
    DiTEngine.run's arguments, whether a TeaCache is attached)."""
    sp_mode, overlap, pieces, fused_qkv = parallel
    B = B if only_row is None else 1
    # VIDEOX_ATTENTION_TYPE=SAGE_ATTENTION under the K|V gather (one gather, waited for): the ranks exchange their MXFP8 key / value
    # RECORDS (one per 64 keys) instead of bf16 rows, so every chunk is a whole number of 64-key tiles: the padding unit is 64 x ranks
    asked = sage_asked(env)
    # (record_gather = False: the caller does not use the gathered records -- a windowed model without FLEXAM_SP_SAGE_WINDOW=1, whose mask
    #  flexam_attn_fwd_fp8_chunked does not take -- and the bf16 K|V gather runs, padded to the ranks alone)
    sage_gather = asked and fused and sp > 1 and sp_mode == "allgather" and overlap == 0 and pieces == 1 and record_gather
    Lp, lc, tok0 = token_layout(L, sp, rank, sp * hip.ATTN_KV_TILE if sage_gather else sp)
    # quantised self-attention on one rank: MXFP8 operands of the rank's tokens.  Sequence parallel with the all-to-all over heads:
    # every rank ends up with ALL tokens of its heads in bf16, packs them and runs the MXFP8 kernel on them.  K|V all-gather in its
    # default form (one gather, waited for): each rank quantises ITS keys / values and the MXFP8 records are what is gathered
    # (sage_gather, above).  The overlapped gather forms (head-group pieces, partial softmaxes) keep the bf16 kernel
    sage = asked and fused and (sp == 1 or (sp_mode == "ulysses" and Lp == L) or sage_gather)
    # CFG pair on one latent (PIPE.py:846-848 feeds `torch.cat([latents] * 2)`): until the first cross-attention the two samples
    # are the same tensor -- same tokens, same timestep rows, same density -- so block 0 runs LayerNorm, q|k|v, RoPE, self-
    # attention and the output projection ONCE and the second sample's residual stream is a copy (half of 1/30 of the
    # attention and projection work of a step; every later operation sees the text and runs per sample)
    share0 = (fused and B == 2 and bx == 1 and sp == 1 and rows_shared and dens_same and not teacache
              and env.get("FLEXAM_SHARE_BLOCK0", "1") != "0")
    per_layer = (not fused) or nl * R * 6 * dim * 4 > table_limit
    return _Mode(B=B, Lp=Lp, lc=lc, tok0=tok0, R=R, rows_per_batch=rows_per_batch, only_row=only_row,
                 per_layer=per_layer, share0=bool(share0), sage=bool(sage), sage_gather=bool(sage_gather),
                 sage_fused=bool(sage) and nh == 24 and hd == hip.ATTN_HEAD_DIM,
                 fp8=fp8, fp8_oproj=fp8 and env.get("FLEXAM_FP8_OPROJ", "0") == "1",
                 ffn_apriori=env.get("FLEXAM_FP8_FFN_APRIORI", "1") != "0",
                 sp=sp, rank=rank, sp_mode=sp_mode, sp_pieces=pieces, sp_overlap_level=overlap, sp_fused_qkv=fused_qkv,
                 use_plan=fused and not teacache and not per_layer and env.get("FLEXAM_REPLAY", "1") != "0")
