"""CPU: dit_layout.halo_plan -- which key rows travel to a rank for its windowed self-attention call on a compact buffer
(flexam_attn_fwd_window_halo; FLEXAM_SP_HALO=1) -- held to brute force.

For every rank case of tests/attn_window_at_cases.CASES: the buffer holds every key some row of the rank sees (`allowed()`, row by row),
and every tile hip.attn_window_at_tiles says a query block visits, at the address the kernel computes for it; every buffer row is written
exactly once, by the rank itself or by one peer, and is a real key (below L); what a rank receives is what its peers send, range for
range and in the same order; the remote rows are at most the rows needed plus 3 x 63 (tile alignment at the end of the sink run and at
both ends of the window run).  Then the flagship's shape (L 11648, 8 ranks, frames of 448 tokens, windows of +-2 / +-5 / +-12 frames,
sink 0 / 448; printed), a rank that is all pads, and a window without a left bound."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_at_cases as A  # noqa: E402
from flexam_amd import hip  # noqa: E402
from flexam_amd.dit_layout import halo_plan, token_layout  # noqa: E402

TILE = hip.ATTN_KV_TILE
SLACK = 3 * (TILE - 1)
RANK_CASES = [c for c in A.CASES if c.rank is not None]


def _plan(c, rank=None):
    return halo_plan(c.Lk, c.ranks, c.rank if rank is None else rank, c.window, c.sink, c.T)


def _buffer_keys(L, sp, rank, plan):
    """[rows] int64: the global key every buffer row holds, from the plan's ranges alone; -1 = nobody writes it.  Asserts on the way that
    no row is written twice and that every source row is a real token of its holder's chunk."""
    lc = token_layout(L, sp, rank)[1]
    keys = torch.full((plan.rows,), -1, dtype=torch.int64)
    for holder, src, dst, n in [(rank, *x) for x in plan.local] + list(plan.recvs):
        assert n > 0 and 0 <= src and src + n <= lc and 0 <= dst and dst + n <= plan.rows, (holder, src, dst, n)
        assert holder * lc + src + n <= L, "a pad row is never a key"
        assert bool((keys[dst:dst + n] == -1).all()), "a buffer row written twice"
        keys[dst:dst + n] = torch.arange(holder * lc + src, holder * lc + src + n)
    return keys


def _check_plan(L, sp, rank, window, sink, T):
    """Everything the module docstring claims for one rank; returns (plan, remote rows, exact need of remote rows)."""
    plan = halo_plan(L, sp, rank, window, sink, T)
    lc, tok0 = token_layout(L, sp, rank)[1:]
    keys = _buffer_keys(L, sp, rank, plan)
    assert bool((keys >= 0).all()), "every buffer row is a planned row"
    s_n = -(-min(sink, L) // TILE) if window[0] >= 0 else 0
    # the address rule of the kernel: global key j at buffer row j below the sink tiles' end, j - 64 gap from there on
    want = torch.arange(plan.rows)
    want = torch.where(want < s_n * TILE, want, want + plan.gap * TILE)
    assert torch.equal(keys, want), "buffer rows are the sink tiles, then the tiles from s_n + gap on"
    assert plan.rows == 0 or int(keys[-1]) < L
    assert plan.rows % TILE == 0 or int(keys[-1]) == L - 1, "whole tiles, except a last tile cut at L"
    # every key some row of the rank sees is there
    seen = A.allowed(range(tok0, tok0 + lc), L, window, T, sink).any(0)
    held = torch.zeros(L, dtype=torch.bool)
    held[keys] = True
    assert bool(held[seen].all()), "a visible key is missing from the buffer"
    # every tile a query block visits lies in the buffer, whole (cut at L)
    for runs in hip.attn_window_at_tiles(lc, L, tok0, window, sink, T):
        for first, last in runs:
            for t in range(first, last + 1):
                assert t < s_n or t >= s_n + plan.gap, "a visited tile lies in the gap"
                assert bool(held[t * TILE:min((t + 1) * TILE, L)].all()), "a visited tile is not whole in the buffer"
    local = torch.zeros(L, dtype=torch.bool)
    local[tok0:min(tok0 + lc, L)] = True
    remote = sum(n for _, _, _, n in plan.recvs)
    need = int((seen & ~local).sum())
    assert remote == int((held & ~local).sum())
    assert remote <= need + SLACK, f"{remote} remote rows for {need} needed"
    return plan, remote, need


@pytest.mark.parametrize("case", RANK_CASES, ids=A.ids(RANK_CASES))
def test_plan_holds_every_visible_key_once(case):
    _check_plan(case.Lk, case.ranks, case.rank, case.window, case.sink, case.T)


def _splits():
    seen = {}
    for c in RANK_CASES:
        seen.setdefault((c.Lk, c.window, c.T, c.sink, c.ranks), c)
    return list(seen.values())


@pytest.mark.parametrize("case", _splits(), ids=A.ids(_splits()))
def test_sends_mirror_receives(case):
    plans = [_plan(case, r) for r in range(case.ranks)]
    for me, mine in enumerate(plans):
        assert all(p != me for p, *_ in mine.recvs + mine.sends)
        for peer, theirs in enumerate(plans):
            if peer == me:
                continue
            sent = [x[1:] for x in mine.sends if x[0] == peer]
            got = [x[1:] for x in theirs.recvs if x[0] == me]
            assert sent == got, f"rank {me} -> rank {peer}: sends {sent}, receives {got}"
            assert len(sent) <= 2


FLAGSHIP = dict(L=11648, sp=8, T=448)


def test_flagship_shape_and_its_planned_rows():
    L, sp, T = FLAGSHIP["L"], FLAGSHIP["sp"], FLAGSHIP["T"]
    lc = token_layout(L, sp, 0)[1]
    assert lc == 1456
    for n in (2, 5, 12):
        for sink in (0, 448):
            line = []
            for rank in range(sp):
                plan, remote, need = _check_plan(L, sp, rank, (n, n), sink, T)
                line.append(f"{remote}/{need}")
            print(f"frames +-{n}, sink {sink}: remote rows planned / needed per rank of {L - lc}: " + " ".join(line))
    # a middle rank under +-2 frames with the sink frame: about a quarter of the gather
    plan, remote, need = _check_plan(L, sp, 4, (2, 2), 448, T)
    # (rows 5824 .. 7279 lie in frames 13 .. 16: the keys of frames 11 .. 18 less the rank's own, and the sink frame)
    assert need == 8 * 448 - lc + 448 and remote == need and plan.gap > 0 and plan.rows == 9 * 448 and remote * 3 < L - lc
    # the sends of all ranks mirror the receives there too
    plans = [halo_plan(L, sp, r, (2, 2), 448, T) for r in range(sp)]
    for me in range(sp):
        for peer in range(sp):
            if peer != me:
                assert [x[1:] for x in plans[me].sends if x[0] == peer] == [x[1:] for x in plans[peer].recvs if x[0] == me]


def test_a_rank_that_is_all_pads_plans_nothing():
    case = next(c for c in RANK_CASES if c.Lk == 5 and c.rank == 3)
    plan = _plan(case)
    assert plan == (0, 0, [], [], [])
    # ... and nobody sends it anything, while rank 2 (one real row that sees its own key) holds the one tile, cut at L: keys 0 .. 3 from
    # their holders (tile alignment) and key 4 its own, which ranks 0 and 1 want for the same reason
    for r in range(4):
        assert all(p != 3 for p, *_ in _plan(case, r).sends)
    assert _plan(case, 2) == (0, 5, [(0, 4, 1)], [(0, 0, 0, 2), (1, 0, 2, 2)], [(0, 0, 4, 1), (1, 0, 4, 1)])


def test_an_unbounded_left_side_plans_a_prefix_with_gap_zero():
    for case in (c for c in RANK_CASES if c.window[0] < 0):
        plan = _plan(case)
        assert plan.gap == 0
        hi = min(case.Lk, case.q_offset + case.Lq + case.window[1])      # causal (-1, 0): the keys up to the rank's last row
        assert plan.rows == min(case.Lk, -(-hi // TILE) * TILE)
    # ... and the sink is dropped with it
    assert halo_plan(1111, 3, 0, (-1, 0), 448, 0) == halo_plan(1111, 3, 0, (-1, 0), 0, 0)


def test_the_whole_sequence_is_gap_zero_and_all_rows():
    for rank in range(4):
        plan = halo_plan(1111, 4, rank, (5000, 5000), 70, 0)
        assert (plan.gap, plan.rows) == (0, 1111)
