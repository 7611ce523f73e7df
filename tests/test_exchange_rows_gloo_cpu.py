"""CPU, worlds of 2 and 3 under gloo: flexam_amd.dist.exchange_rows on CPU tensors -- the dist.batch_isend_irecv path RCCL runs on GPUs --
moving the row ranges dit_layout.halo_plan states, with the send [G, B, lc, 2*cb] and halo [G, B, rows, 2*cb] layouts of dit_sp.KVHalo.
Uneven ranges, a peer with one range, two or none, a rank that neither sends nor receives, waited-for and asynchronous: every row of a
rank's buffer equals the row of the sequence the plan says it is, and the rows of the allocation around the buffer stay as they were.
The all-gather form that serves gloo on device tensors (the GPU test worlds) runs in the same worlds, on CPU tensors, to the same end.
Spawning as in tests/test_dist_gloo_cpu.py.  Then the LoopbackGroup stand-in: copies of the planned sizes."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, fn, args, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ret[rank] = fn(rank, world, *args)
    finally:
        dist.destroy_process_group()


def run_world(fn, world, *args):
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, fn, args, ret)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0, f"rank exited with {p.exitcode}"
    return [ret[r] for r in range(world)]


G, B, CB = 2, 2, 3      # head groups, CFG rows, columns of one group's K|V


def _sequence(L, lc, world):
    """[G, B, world * lc, 2 * CB]: every element its own number, pad rows (from L on) NaN -- they never travel."""
    full = torch.arange(G * B * world * lc * 2 * CB, dtype=torch.float32).view(G, B, world * lc, 2 * CB) + 1.0
    full[:, :, L:] = float("nan")
    return full


def _views(plan, send, halo):
    pairs = [(g, b) for g in range(G) for b in range(B)]
    return ([(p, halo[g, b, d:d + n]) for g, b in pairs for p, _, d, n in plan.recvs],
            [(p, send[g, b, s:s + n]) for g, b in pairs for p, s, _, n in plan.sends])


def _exchange(rank, world, L, window, sink, T, async_op, gathered=False):
    from flexam_amd import hip
    from flexam_amd.dist import _exchange_rows_gathered, exchange_rows
    from flexam_amd.dit_layout import halo_plan, token_layout
    plan = halo_plan(L, world, rank, window, sink, T)
    lc, tok0 = token_layout(L, world, rank)[1:]
    full = _sequence(L, lc, world)
    send = full[:, :, tok0:tok0 + lc].contiguous()
    big = torch.full((G, B, plan.rows + 2, 2 * CB), -7.0)      # the buffer, with a row either side that nothing may touch
    halo = big[:, :, 1:1 + plan.rows]
    recvs, sends = _views(plan, send, halo)
    if gathered:         # the form that serves backends without device send / receive, here on CPU tensors
        work = _exchange_rows_gathered(recvs, sends, None, send)
    else:
        work = exchange_rows(recvs, sends, None, async_op=async_op, like=send)
    for s, d, n in plan.local:
        halo[:, :, d:d + n].copy_(send[:, :, s:s + n])
    if async_op:
        assert work.wait()
    else:
        assert work is None
    tile = hip.ATTN_KV_TILE
    s_n = -(-min(sink, L) // tile) if window[0] >= 0 else 0
    key = torch.arange(plan.rows)
    key = torch.where(key < s_n * tile, key, key + plan.gap * tile)
    ok = bool(torch.equal(halo, full[:, :, key])) and not bool(halo.isnan().any())
    ok = ok and bool((big[:, :, 0] == -7.0).all()) and bool((big[:, :, -1] == -7.0).all())
    return ok, plan.rows, len(plan.recvs), len(plan.sends)


# (L, window, sink, frame_tokens): chunks off every tile boundary, a sink and a gap; frames that straddle chunks; five keys, where a
# rank of three holds one real row; causal over chunks of whole tiles, where rank 0 of two only sends and rank 1 only receives
PLANS = [(1111, (100, 37), 70, 0), (1344, (1, 1), 0, 448), (1111, (1, 1), 300, 37), (1111, (-1, 0), 0, 0), (5, (0, 0), 0, 0),
         (1280, (-1, 0), 0, 0)]


def _exchange_all(rank, world):
    """Every plan, waited for and asynchronous, in one world (a world costs seconds to start)."""
    out = [(plan, async_op, _exchange(rank, world, *plan, async_op)) for plan in PLANS for async_op in (False, True)]
    return out + [(plan, False, _exchange(rank, world, *plan, False, gathered=True)) for plan in PLANS]


@pytest.mark.parametrize("world", [2, 3])
def test_every_received_row_is_the_senders(world):
    res = run_world(_exchange_all, world)
    for i, (plan, async_op, _) in enumerate(res[0]):
        per_rank = [r[i][2] for r in res]
        assert all(x[0] for x in per_rank), (plan, async_op, per_rank)
        if not async_op and i < 2 * len(PLANS):
            print(f"world {world}, {plan}: buffer rows {[x[1] for x in per_rank]}, ranges received {[x[2] for x in per_rank]}, "
                  f"sent {[x[3] for x in per_rank]}")


def test_the_plans_above_are_uneven_and_some_are_empty():
    """What the worlds above exercise, from the planner alone: ranges of different sizes, a peer that sends two ranges, a rank that
    receives nothing and one that sends nothing."""
    from flexam_amd.dit_layout import halo_plan
    plans = [halo_plan(L, world, r, w, s, T) for L, w, s, T in PLANS for world in (2, 3) for r in range(world)]
    sizes = {n for p in plans for *_, n in p.recvs}
    assert len(sizes) > 8
    assert any(len([1 for x in p.recvs if x[0] == peer]) == 2 for p in plans for peer in range(3))
    assert any(not p.recvs and p.sends for p in plans) and any(p.recvs and not p.sends for p in plans)
    assert halo_plan(5, 4, 3, (0, 0), 0, 0) == (0, 0, [], [], [])


def test_loopback_group_copies_the_planned_sizes():
    """LoopbackGroup: one process as rank 1 of 3; every received range is overwritten (by rows this rank sends: plumbing, not results),
    nothing else is."""
    from flexam_amd.dist import LoopbackGroup, exchange_rows
    from flexam_amd.dit_layout import halo_plan, token_layout
    L, world, rank = 1111, 3, 1
    plan = halo_plan(L, world, rank, (100, 37), 70, 0)
    lc, tok0 = token_layout(L, world, rank)[1:]
    send = _sequence(L, lc, world)[:, :, tok0:tok0 + lc].contiguous()
    halo = torch.full((G, B, plan.rows, 2 * CB), -7.0)
    recvs, sends = _views(plan, send, halo)
    group = LoopbackGroup(world, rank)
    assert exchange_rows(recvs, sends, group) is None
    written = torch.zeros(plan.rows, dtype=torch.bool)
    for _, _, d, n in plan.recvs:
        written[d:d + n] = True
    assert bool((halo[:, :, written] != -7.0).all()) and bool((halo[:, :, ~written] == -7.0).all())
    assert exchange_rows(recvs, sends, group, async_op=True).wait()
    assert exchange_rows([], [], group) is None and exchange_rows([], [], group, async_op=True).wait()
