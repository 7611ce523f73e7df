"""CPU, world_size 2 under gloo: the sequence-parallel plumbing of flexam_amd/dist.py (same code
path RCCL runs on GPUs).  Compute in these tests is the fp32 oracle; what is under test is the
sharding: contiguous token chunks, K/V all-gather layout, global-token RoPE offsets, row-index
sharding and the final token all-gather must reproduce the single-process result."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import dit as O


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, fn, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ret[rank] = fn(rank, world)
    finally:
        dist.destroy_process_group()


def run_world(fn, world=2):
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_worker, args=(r, world, _free_port.port, fn, ret)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0, f"rank exited with {p.exitcode}"
    return [ret[r] for r in range(world)]


@pytest.fixture(autouse=True)
def _port():
    _free_port.port = _free_port()


def _gather_layout(rank, world):
    from flexam_amd.dist import all_gather_seq, chunk_bounds, shard_rows
    b, l, x = 2, 12, 5
    full = torch.arange(b * l * x, dtype=torch.float32).view(b, l, x)
    s, e = chunk_bounds(l, rank, world)
    out = all_gather_seq(full[:, s:e].clone())
    idx = torch.arange(b * l, dtype=torch.int32)
    return bool(torch.equal(out, full)), shard_rows(idx, b, l, rank, world).tolist(), (s, e)


def test_all_gather_seq_layout_and_row_sharding():
    res = run_world(_gather_layout)
    assert all(r[0] for r in res)
    assert res[0][1] == list(range(0, 6)) + list(range(12, 18)) and res[1][1] == list(range(6, 12)) + list(range(18, 24))
    assert res[0][2] == (0, 6) and res[1][2] == (6, 12)


def _sp_self_attention(rank, world):
    """Sequence-parallel self-attention = local q/k/v projection + RMSNorm + RoPE at GLOBAL token
    positions, K/V all-gather, attention of the local queries against all keys, token all-gather."""
    from flexam_amd.dist import all_gather_seq, chunk_bounds
    from flexam_amd.rope import rope_tables
    g = torch.Generator().manual_seed(0)
    b, heads, d = 2, 2, 256
    grid = (3, 2, 4)
    l = 24 + 4                                              # 4 pass-through tokens
    x = torch.randn(b, l, d, generator=g)
    wq, wk, wv = (torch.randn(d, d, generator=g) / 16 for _ in range(3))
    nq, nk = 1 + 0.1 * torch.randn(d, generator=g), 1 + 0.1 * torch.randn(d, generator=g)
    ang = O.rope_angles(1024, 128)
    q = O.rope_apply(O.rms_norm(x @ wq.t(), nq, 1e-6).view(b, l, heads, 128), grid, ang)
    k = O.rope_apply(O.rms_norm(x @ wk.t(), nk, 1e-6).view(b, l, heads, 128), grid, ang)
    v = (x @ wv.t()).view(b, l, heads, 128)
    want = O.attention(q, k, v)
    # sharded
    s, e = chunk_bounds(l, rank, world)
    cos, sin = rope_tables(grid, l, 128)

    def rope_local(t):                                      # what flexam_rmsnorm_rope does with token_offset = s
        t = t.view(b, e - s, heads, 64, 2)
        c, sn = cos[s:e].view(1, e - s, 1, 64), sin[s:e].view(1, e - s, 1, 64)
        re, im = t[..., 0], t[..., 1]
        return torch.stack([re * c - im * sn, re * sn + im * c], dim=-1).reshape(b, e - s, heads, 128)
    xl = x[:, s:e]
    ql = rope_local(O.rms_norm(xl @ wq.t(), nq, 1e-6))
    kl = rope_local(O.rms_norm(xl @ wk.t(), nk, 1e-6))
    vl = (xl @ wv.t()).view(b, e - s, heads, 128)
    kv = all_gather_seq(torch.cat([kl.flatten(2), vl.flatten(2)], dim=2))
    kf, vf = kv[:, :, :d].unflatten(2, (heads, 128)), kv[:, :, d:].unflatten(2, (heads, 128))
    out = all_gather_seq(O.attention(ql, kf, vf).flatten(2))
    return float((out - want.flatten(2)).abs().max())


def test_sequence_parallel_attention_matches_single_process():
    errs = run_world(_sp_self_attention)
    assert max(errs) < 5e-5, errs


def test_chunk_bounds_pad_like_the_reference():
    """Equal chunks of the sequence padded to a multiple of the ranks (wan_transformer3d_FlexAM.py:919-920); the pads sit at the end."""
    from flexam_amd.dist import chunk_bounds, padded_len, real_tokens, shard_rows
    assert chunk_bounds(11648, 7, 8) == (10192, 11648) and padded_len(11648, 8) == 11648 and real_tokens(11648, 7, 8) == 1456
    assert padded_len(11648, 3) == 11649 and padded_len(11648, 5) == 11650
    assert [chunk_bounds(11648, r, 3) for r in range(3)] == [(0, 3883), (3883, 7766), (7766, 11649)]
    assert [real_tokens(11648, r, 3) for r in range(3)] == [3883, 3883, 3882]
    assert [real_tokens(5, r, 4) for r in range(4)] == [2, 2, 1, 0]                  # a rank may hold pads only
    idx = torch.arange(2 * 7, dtype=torch.int32)                                     # B = 2, L = 7, three ranks: chunks of 3, the last 1 real + 2 pads
    assert shard_rows(idx, 2, 7, 0, 3).tolist() == [0, 1, 2, 7, 8, 9]
    assert shard_rows(idx, 2, 7, 2, 3).tolist() == [6, 6, 6, 13, 13, 13]             # pads repeat the last real token's entry (FX.py:930-934)
    assert shard_rows(idx, 2, 7, 1, 3, chunk=4).tolist() == [4, 5, 6, 6, 11, 12, 13, 13]    # a wider padding unit (MXFP8 key records: whole tiles per rank)
    assert shard_rows(idx, 2, 7, 2, 3, chunk=4).tolist() == [6, 6, 6, 6, 13, 13, 13, 13]    # a rank that holds pads only


def _async_gather(rank, world):
    from flexam_amd.dist import SeqGather, chunk_bounds
    ok = True
    for b in (1, 2):
        l, x = 12, 5
        full = torch.arange(b * l * x, dtype=torch.float32).view(b, l, x)
        s, e = chunk_bounds(l, rank, world)
        g = SeqGather(full[:, s:e].clone())
        ok = ok and bool(torch.equal(g.finish(), full))
        out = torch.empty(b, l, x)
        g = SeqGather(full[:, s:e].clone(), out=out)
        ok = ok and bool(torch.equal(g.finish(), full))
    return ok


def test_async_seq_gather_both_layouts():
    assert all(run_world(_async_gather))


def _shard_streams(rank, world):
    from flexam_amd.dist import shard_streams
    g = torch.Generator().manual_seed(4)
    jobs = [("control", torch.randn(1, 3, 5, 4, 4, generator=g)), ("depth", None), ("ref", torch.randn(1, 3, 1, 4, 4, generator=g))]
    jobs += [(("cos", k), torch.randn(1, 3, 5, 4, 4, generator=g)) for k in range(3)]
    calls = []

    def encode(v):                                       # stand-in for vae.encode: any deterministic map
        calls.append(tuple(v.shape))
        return v.mean(dim=1, keepdim=True) * 2 + 1
    out = shard_streams(jobs, encode)
    want = {k: (None if v is None else v.mean(dim=1, keepdim=True) * 2 + 1) for k, v in jobs}
    same = all((out[k] is None and want[k] is None) or torch.equal(out[k], want[k]) for k in want)
    return same, len(calls), sorted(str(k) for k in out)


def test_conditioning_streams_shard_round_robin_and_broadcast():
    res = run_world(_shard_streams, 2)
    assert all(r[0] for r in res)                       # every rank ends with every latent, bit-identical to a local encode
    assert [r[1] for r in res] == [3, 2]                # 5 live streams: 3 on rank 0, 2 on rank 1 -- each encoded exactly once
    assert res[0][2] == res[1][2] and len(res[0][2]) == 6


def _parallel_decode_gather(rank, world):
    from flexam_amd.wan_vae3_8 import AutoencoderKLWan3_8
    full = torch.arange(3 * 5 * 8 * 6, dtype=torch.float32).view(3, 5, 8, 6)

    class FakeEngine:                                     # stands in for the HIP decoder: returns this rank's row band
        def band_grid(self, h, w, n):
            return (n, 1)
        def decode(self, u, stripe=None):
            r, n = stripe
            return full[:, :, r * 8 // n:(r + 1) * 8 // n].contiguous()
    vae = AutoencoderKLWan3_8(c_dim=16, dec_dim=16)
    vae.enable_parallel_decode()
    out = vae._decode_one(FakeEngine(), torch.zeros(1, 1, 4, 3))
    return bool(torch.equal(out, full))


def test_parallel_vae_decode_assembles_row_bands():
    assert all(run_world(_parallel_decode_gather, 2))


def _parallel_decode_gather_tiles(rank, world):
    from flexam_amd.wan_vae3_8 import AutoencoderKLWan3_8
    full = torch.arange(3 * 5 * 8 * 6, dtype=torch.float32).view(3, 5, 8, 6)

    class FakeEngine:                                     # a 2 x 2 grid: rank = row * 2 + column (what _DecoderEngine.band_grid / decode hand out)
        def band_grid(self, h, w, n):
            return (2, 2)
        def decode(self, u, stripe=None):
            r, n = stripe
            ri, ci = divmod(r, 2)
            return full[:, :, ri * 4:(ri + 1) * 4, ci * 3:(ci + 1) * 3].contiguous()
    vae = AutoencoderKLWan3_8(c_dim=16, dec_dim=16)
    vae.enable_parallel_decode()
    out = vae._decode_one(FakeEngine(), torch.zeros(1, 1, 4, 3))
    return bool(torch.equal(out, full))


def test_parallel_vae_decode_assembles_a_tile_grid():
    assert all(run_world(_parallel_decode_gather_tiles, 4))


def _a2a_blocks_and_layouts(rank, world):
    """The all-to-all exchange of the head-parallel mode, with the send / receive layouts the engine uses:
    send [B, sp, lc, 3G] (block (b, j) -> rank j), receive [B, sp, lc, 3G] = [B, L, 3G] in token order, output chunks back to
    [sp, B, lc, G], read as A[m, j*G + c] through per-K-block offsets."""
    from flexam_amd.dist import all_to_all_blocks
    B, lc, G, C = 2, 3, 64, 64 * world
    L = lc * world
    g = torch.Generator().manual_seed(11)
    full = torch.randn(B, L, 3, C, generator=g)                                   # q|k|v of every token, all heads
    mine = full[:, rank * lc:(rank + 1) * lc]                                     # this rank's tokens
    send = torch.empty(B, world, lc, 3 * G)
    for j in range(world):                                                        # what rmsnorm_rope_scatter writes
        send[:, j] = mine[:, :, :, j * G:(j + 1) * G].reshape(B, lc, 3 * G)
    recv = torch.empty(B, world, lc, 3 * G)
    for b in range(B):
        all_to_all_blocks([recv[b, i] for i in range(world)], [send[b, j] for j in range(world)])
    got = recv.view(B, L, 3, G)
    ok = bool(torch.equal(got, full[:, :, :, rank * G:(rank + 1) * G]))         # all tokens of MY head group, token order
    out = got[:, :, 0] * 2 + 1                                                    # stand-in for attention: [B, L, G]
    recv2 = torch.empty(world, B, lc, G)
    chunks = out.view(B, world, lc, G)
    for b in range(B):
        all_to_all_blocks([recv2[j, b] for j in range(world)], [chunks[b, i] for i in range(world)])
    koff = [(kb * 64 // G) * (B * lc * G) + (kb * 64) % G for kb in range(C // 64)]
    flat = recv2.reshape(-1)
    a = torch.stack([torch.cat([flat[m * G + koff[kb]: m * G + koff[kb] + 64] for kb in range(C // 64)]) for m in range(B * lc)])
    want = (mine[:, :, 0] * 2 + 1).reshape(B * lc, C)                             # my tokens, ALL head groups
    return ok and bool(torch.equal(a, want))


def test_all_to_all_block_layouts_need_no_pack_or_unpack():
    assert all(run_world(_a2a_blocks_and_layouts, 2))


def _local_first_merge(rank, world):
    """K|V all-gather mode: softmax over {local chunk} U {chunks before} U {chunks after} merged from partial
    (un-normalised O, reference, row sum) triples equals attention over all keys."""
    import math
    from flexam_amd.dist import chunk_bounds
    g = torch.Generator().manual_seed(5)
    L, H, D = 24, 2, 16
    q, k, v = (torch.randn(1, L, H, D, generator=g) for _ in range(3))
    s, e = chunk_bounds(L, rank, world)
    ql = q[:, s:e]
    kv = torch.cat([k, v], dim=-1).flatten(2)                                     # [1, L, 2*H*D]
    send = kv[:, s:e].contiguous()
    cat = torch.empty(1, L, kv.shape[2])
    dist.all_gather_into_tensor(cat[0], send[0])                                  # one gather per CFG row, token order
    assert torch.equal(cat, kv)

    def partial(keys, vals):
        sc = torch.einsum("blhd,bmhd->bhlm", ql, keys) / math.sqrt(D) * math.log2(math.e)
        ref = sc.max(dim=-1).values
        p = torch.exp2(sc - ref.unsqueeze(-1))
        return torch.einsum("bhlm,bmhd->blhd", p, vals), ref, p.sum(-1)
    parts = [partial(k[:, s:e], v[:, s:e])]
    if s > 0:
        parts.append(partial(k[:, :s], v[:, :s]))
    if e < L:
        parts.append(partial(k[:, e:], v[:, e:]))
    m = torch.stack([p[1] for p in parts]).max(dim=0).values
    acc = sum(p[0] * torch.exp2(p[1] - m).permute(0, 2, 1).unsqueeze(-1) for p in parts)
    l = sum(p[2] * torch.exp2(p[1] - m) for p in parts)
    got = acc / l.permute(0, 2, 1).unsqueeze(-1)
    want = O.attention(ql, k, v)
    return float((got - want).abs().max())


def test_local_chunk_first_partial_softmax_merge():
    errs = run_world(_local_first_merge, 2)
    assert max(errs) < 1e-5, errs


def test_default_layout_follows_the_exchange_mode():
    """with the K|V all-gather (the default exchange) every even world size splits the CFG pair first, so N = 4 / 8
    run 2 x 2 / 2 x 4; only the all-to-all exchange with heads that divide over the ranks runs N-way token chunks with the pair
    batched; two ranks always take the CFG split (no per-block traffic), odd worlds cannot."""
    from flexam_amd import Wan2_2Transformer3DModel_FlexAM as M
    assert all(M.default_cfg_parallel(w, 24) for w in (2, 4, 8))                       # default mode = allgather
    assert all(M.default_cfg_parallel(w, 24, "allgather") for w in (2, 4, 8))
    assert M.default_cfg_parallel(2, 24, "ulysses")
    assert not M.default_cfg_parallel(4, 24, "ulysses") and not M.default_cfg_parallel(8, 24, "ulysses")
    assert M.default_cfg_parallel(4, 2, "ulysses")                                      # 2 heads do not divide over 4 ranks
    assert not M.default_cfg_parallel(3, 24) and not M.default_cfg_parallel(1, 24)


def _head_group_pieces(rank, world):
    """The K|V gather cut into G head-group pieces (flexam_amd.dit_sp.KVGather): send layout [G, B, lc, 2*C/G] (K of the
    group's heads | V of the group's heads), one all-gather per (piece, CFG row) whose rank-major concatenation is the token
    order.  Group g's attention needs ONLY piece g -- whatever the other pieces' buffers hold (here: NaN until their own gather
    is consumed, in reverse order of issue) -- and the groups together equal attention over all heads; within a piece the
    per-peer chunks are merged from partial softmaxes in EVERY arrival order."""
    import itertools
    import math
    from flexam_amd.dist import chunk_bounds
    g = torch.Generator().manual_seed(9)
    B, L, H, D, G = 2, 24, 4, 16, 2
    hg, cb = H // G, H // G * D
    q, k, v = (torch.randn(B, L, H, D, generator=g) for _ in range(3))
    s, e = chunk_bounds(L, rank, world)
    lc = e - s
    ql = q[:, s:e]
    send = torch.empty(G, B, lc, 2 * cb)
    for gi in range(G):
        send[gi, :, :, :cb] = k[:, s:e, gi * hg:(gi + 1) * hg].flatten(2)
        send[gi, :, :, cb:] = v[:, s:e, gi * hg:(gi + 1) * hg].flatten(2)
    cat = torch.full((G, B, L, 2 * cb), float("nan"))
    works = [[dist.all_gather_into_tensor(cat[gi, b], send[gi, b], async_op=True) for b in range(B)] for gi in range(G)]
    want = O.attention(ql, k, v)
    worst = 0.0

    def partial(qh, keys, vals):
        sc = torch.einsum("blhd,bmhd->bhlm", qh, keys) / math.sqrt(D) * math.log2(math.e)
        ref = sc.max(dim=-1).values
        p = torch.exp2(sc - ref.unsqueeze(-1))
        return torch.einsum("bhlm,bmhd->blhd", p, vals), ref, p.sum(-1)
    for gi in reversed(range(G)):                                   # consume the LAST piece first: pieces are independent
        for w in works[gi]:
            w.wait()
        kg = cat[gi, :, :, :cb].unflatten(2, (hg, D))
        vg = cat[gi, :, :, cb:].unflatten(2, (hg, D))
        assert torch.equal(kg, k[:, :, gi * hg:(gi + 1) * hg]) and torch.equal(vg, v[:, :, gi * hg:(gi + 1) * hg])
        qh = ql[:, :, gi * hg:(gi + 1) * hg]
        got = O.attention(qh, kg, vg)
        worst = max(worst, float((got - want[:, :, gi * hg:(gi + 1) * hg]).abs().max()))
        chunks = [chunk_bounds(L, r, world) for r in range(world)]
        for order in itertools.permutations(range(world)):          # peer chunks in every arrival order
            parts = [partial(qh, kg[:, chunks[r][0]:chunks[r][1]], vg[:, chunks[r][0]:chunks[r][1]]) for r in order]
            m = torch.stack([p[1] for p in parts]).max(dim=0).values
            acc = sum(p[0] * torch.exp2(p[1] - m).permute(0, 2, 1).unsqueeze(-1) for p in parts)
            l = sum(p[2] * torch.exp2(p[1] - m) for p in parts)
            merged = acc / l.permute(0, 2, 1).unsqueeze(-1)
            worst = max(worst, float((merged - want[:, :, gi * hg:(gi + 1) * hg]).abs().max()))
    return worst


@pytest.mark.parametrize("world", [2, 3])
def test_head_group_pieces_and_chunk_arrival_orders(world):
    errs = run_world(_head_group_pieces, world)
    assert max(errs) < 1e-5, errs


def _layout_reselection(rank, world):
    """What bench.py's layout probe does to the communicators: every candidate layout and then the winner call
    enable_multi_gpus_inference -- twice over (the probe run twice in one process)."""
    from flexam_amd.dist import live_subgroups
    from flexam_amd.wan_transformer3d_FlexAM import Wan2_2Transformer3DModel_FlexAM
    cfg = dict(O.DIT_TINY, num_layers=1)
    kw = dict(cfg)
    kw.pop("eps")
    m = Wan2_2Transformer3DModel_FlexAM(**kw)
    seen = []
    for _ in range(2):                                     # the whole probe, twice
        for cfgp in (True, True, False, False, True, None):
            m.enable_multi_gpus_inference(cfg_parallel=cfgp)
            par = m._parallel
            seen.append((par.get("cfg_size", 1), par["sp_size"], live_subgroups()))
            if par.get("cfg_size", 1) == 2:                # the cached half group is a working communicator of the right members
                t = torch.tensor([float(rank)])
                dist.all_reduce(t, group=par["sp_group"])
                half = rank // (world // 2)
                assert float(t) == sum(range(half * (world // 2), (half + 1) * (world // 2)))
    return seen


def test_cfg_half_groups_are_created_once_per_member_set():
    """r3 verdict item 4: enable_multi_gpus_inference created two new process groups on EVERY call; a layout probe of four candidates
    plus the winner left a dozen communicators alive on the first RCCL run.  Now the halves are cached by member tuple: the world
    group + 2, however often a layout is selected."""
    res = run_world(_layout_reselection, world=4)
    for seen in res:
        assert max(n for _, _, n in seen) == 2 and seen[-1][2] == 2
        assert [c for c, _, _ in seen[:6]] == [2, 2, 1, 1, 2, 2]          # None -> the default for 4 ranks with the all-gather: 2 x 2


# ----------------------------------------------------------------------------- r5: re-bound self-attention under sequence parallelism
def _rebound_usp_forward(rank, world):
    """The seam the engine offers blocks that are called as modules under sequence parallelism (DiTEngine._run_block_modules): the
    block gets this rank's token chunk, global seq_lens / grid, and its `self_attn.forward` -- here a caller's own USP forward,
    re-bound the way the reference does it (wan_transformer3d_FlexAM.py:807-815) -- reads group / rank / token offset from
    flexam_amd.dist.current_sp_context() and exchanges K|V with all_gather_seq.  Compute = the fp32 oracle; two stacked blocks'
    self-attention halves; equal to the whole-sequence result."""
    from flexam_amd.dist import (all_gather_seq, chunk_bounds, current_sp_context, get_sequence_parallel_rank,
                                 get_sequence_parallel_world_size, sequence_parallel_context)
    g = torch.Generator().manual_seed(3)
    b, heads, d = 2, 2, 256
    grid = (3, 2, 4)
    l = 24
    x = torch.randn(b, l, d, generator=g)
    layers = [dict(wq=torch.randn(d, d, generator=g) / 16, wk=torch.randn(d, d, generator=g) / 16, wv=torch.randn(d, d, generator=g) / 16,
                   nq=1 + 0.1 * torch.randn(d, generator=g), nk=1 + 0.1 * torch.randn(d, generator=g)) for _ in range(2)]
    ang = O.rope_angles(1024, 128)

    def whole(xx, p):
        q = O.rope_apply(O.rms_norm(xx @ p["wq"].t(), p["nq"], 1e-6).view(b, l, heads, 128), grid, ang)
        k = O.rope_apply(O.rms_norm(xx @ p["wk"].t(), p["nk"], 1e-6).view(b, l, heads, 128), grid, ang)
        return xx + O.attention(q, k, (xx @ p["wv"].t()).view(b, l, heads, 128)).flatten(2)
    want = whole(whole(x, layers[0]), layers[1])
    assert current_sp_context() is None and get_sequence_parallel_world_size() == world      # outside a forward: the world group

    def usp_forward(xc, seq_lens, p):                      # a caller's re-bound forward: everything it needs is in the context
        ctx = current_sp_context()
        assert ctx["size"] == get_sequence_parallel_world_size() == world and ctx["rank"] == get_sequence_parallel_rank() == rank
        lc, t0 = xc.shape[1], ctx["token_offset"]
        assert lc * ctx["size"] == ctx["seq_len"] == int(seq_lens[0])
        full_q = torch.zeros(b, l, heads, 128)
        full_k = torch.zeros(b, l, heads, 128)
        full_q[:, t0:t0 + lc] = O.rms_norm(xc @ p["wq"].t(), p["nq"], 1e-6).view(b, lc, heads, 128)
        full_k[:, t0:t0 + lc] = O.rms_norm(xc @ p["wk"].t(), p["nk"], 1e-6).view(b, lc, heads, 128)
        ql = O.rope_apply(full_q, grid, ang)[:, t0:t0 + lc]             # RoPE at the chunk's GLOBAL positions
        kl = O.rope_apply(full_k, grid, ang)[:, t0:t0 + lc]
        vl = (xc @ p["wv"].t()).view(b, lc, heads, 128)
        kv = all_gather_seq(torch.cat([kl.flatten(2), vl.flatten(2)], dim=2), ctx["group"])
        return xc + O.attention(ql, kv[:, :, :d].unflatten(2, (heads, 128)), kv[:, :, d:].unflatten(2, (heads, 128))).flatten(2)
    s, e = chunk_bounds(l, rank, world)
    xc = x[:, s:e].clone()
    with sequence_parallel_context(None, rank, world, s, l):
        for p in layers:
            xc = usp_forward(xc, torch.tensor([l] * b), p)
    assert current_sp_context() is None
    out = all_gather_seq(xc)
    return float((out - want).abs().max())


def test_rebound_self_attention_forward_under_sequence_parallel_context():
    errs = run_world(_rebound_usp_forward)
    assert max(errs) < 5e-5, errs


def _subgroups_after_reinit(rank, world):
    """Round-4 advice: the sub-communicator cache must not hand out groups of a destroyed default process group."""
    from flexam_amd.dist import clear_subgroups, live_subgroups, subgroup
    g1 = subgroup([0, 1])
    assert subgroup([0, 1]) is g1 and live_subgroups() == 1
    port = int(os.environ["MASTER_PORT"])
    dist.destroy_process_group()
    os.environ["MASTER_PORT"] = str(port + 1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    assert live_subgroups() == 0                            # a new default group: the cache starts empty
    g2 = subgroup([0, 1])
    assert g2 is not g1
    t = torch.tensor([float(rank + 1)])
    dist.all_reduce(t, group=g2)                           # and the new handle works
    clear_subgroups()
    assert live_subgroups() == 0
    return float(t)


def test_subgroup_cache_belongs_to_one_default_process_group():
    assert run_world(_subgroups_after_reinit) == [3.0, 3.0]


def test_loopback_group_collectives_keep_shapes_and_order():
    """flexam_amd.dist.LoopbackGroup (bench.py --emulate-rank): one process as rank r of N, collectives = copies of the same sizes.
    On CPU tensors the copies are synchronous; shapes, slot order and the Work protocol are what is under test."""
    from flexam_amd.dist import (LoopbackGroup, SeqGather, all_gather_into_tensor, all_gather_seq, all_to_all_blocks, group_backend,
                                 group_rank, group_size)
    g = LoopbackGroup(4, rank=2)
    assert (group_size(g), group_rank(g), group_backend(g)) == (4, 2, "loopback")
    loc = torch.arange(2 * 3 * 5, dtype=torch.float32).view(2, 3, 5)
    out = all_gather_seq(loc, g)
    assert out.shape == (2, 12, 5)
    for r in range(4):
        assert torch.equal(out[:, r * 3:(r + 1) * 3], loc)
    flat = torch.empty(4 * 6, 5)
    w = all_gather_into_tensor(flat, loc.view(6, 5), group=g, async_op=True)
    assert w.wait() and torch.equal(flat.view(4, 6, 5)[3], loc.view(6, 5))
    sg = SeqGather(loc[:1], g)
    assert torch.equal(sg.finish()[:, 9:12], loc[:1])
    ins = [torch.full((2, 2), float(i)) for i in range(4)]
    outs = [torch.empty(2, 2) for _ in range(4)]
    assert all_to_all_blocks(outs, ins, g) is None and all(float(o[0, 0]) == i for i, o in enumerate(outs))
    with pytest.raises(ValueError):
        LoopbackGroup(2, rank=2)
