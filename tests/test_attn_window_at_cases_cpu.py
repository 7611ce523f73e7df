"""CPU: the cases of tests/attn_window_at_cases.py (the windowed kernel at a query offset) are not blind, the GPU-free planner
hip.attn_window_at_tiles equals enumeration, and the engine's host side (FLEXAM_SP_WINDOW) refuses, resolves and warns as it says.

Not blind, measured here (asserted against attn_window_cases.SENSITIVITY_ULPS = 8): one key added or dropped at either end of every row's
range moves every altered row by 16.4 bf16 ulps or more (the sink and frame cases, whose construction these share and which does not
depend on the row index, give 15.8 at theirs); unaltered rows stay bit-identical.  The mask evaluated at the row's index i in the call
instead of its global token q_offset + i moves at least one row by 11.0 ulps or more in every case with q_offset > 0 but five calls of
the tile-aligned 448-token frames, where it provably moves nothing (OFFSET_BLIND below says why); each of their splits has ranks that are
moved, so a kernel that ignores the offset cannot pass tests/test_attn_window_at_gpu.py on any split."""
import itertools
import os
import sys
import types
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_at_cases as A  # noqa: E402
import attn_window_cases as W  # noqa: E402
import attn_window_frames_cases as F  # noqa: E402
import attn_window_sink_cases as S  # noqa: E402
from flexam_amd import dit_layout as D  # noqa: E402
from flexam_amd import hip  # noqa: E402
from flexam_amd.dit_engine import DiTEngine  # noqa: E402


def _row_moves(got, want):
    """[Lq]: the largest |got - want| / ulp(want) over batch, head and channel of every row."""
    return ((got - want).abs() / A.bf16_ulp(want)).amax(dim=(0, 2, 3))


def test_the_cases_hold_pad_rows_empty_rows_and_an_empty_call():
    """What the table of cases promises, so that a change to it cannot quietly drop it."""
    by = {c.name: c for c in A.CASES}
    assert len(by) == len(A.CASES) == 51
    assert by["L600-w0_0-s0-r6of7-b1h2"].empty_rows().tolist() == [False] * 84 + [True] * 2
    assert not by["L600-w0_0-s5-r6of7-b1h2"].empty_rows().any() and by["L600-w0_0-s5-r6of7-b1h2"].allowed()[84:].sum() == 10
    assert not by["L1111-w-1_0-s0-r2of3-b1h2"].empty_rows().any()                  # two pad rows that still see keys
    assert by["L1111-w-1_0-s0-r2of3-b1h2"].q_offset + by["L1111-w-1_0-s0-r2of3-b1h2"].Lq == 1113
    assert by["L896-f0_0-T448-s0-r2of3-b1h2"].empty_rows().tolist() == [False] * 298 + [True]
    assert not by["L896-f0_0-T448-s448-r2of3-b1h2"].empty_rows().any()
    assert by["L5-w0_0-s0-r2of4-b1h2"].empty_rows().tolist() == [False, True] and by["L5-w0_0-s0-r3of4-b1h2"].empty_rows().all()
    a2a = by["L1111-w100_37-s70-a2aof3-b1h2"]
    assert (a2a.q_offset, a2a.Lq) == (0, 1113) and not a2a.empty_rows().any()      # (the sink shows the pad rows 70 keys)
    wide = by["L1111-w100_37-s70-r1of4-b2h3"]
    assert (wide.chunk, wide.q_offset, wide.B, wide.H) == (278, 278, 2, 3) and wide.q_offset % A.KV_TILE and wide.q_offset % A.Q_BLOCK
    assert {c.ranks for c in A.CASES if c.T == 448 and c.Lk == 1344} == {3, 4, 8}
    for c in A.CASES:                                            # every rank of each listed split but case 9's
        if c.rank is not None and c.Lk != 5:
            assert sum(1 for o in A.CASES if (o.Lk, o.window, o.T, o.sink, o.ranks) == (c.Lk, c.window, c.T, c.sink, c.ranks)) == c.ranks
        want = c.want()
        assert want.shape == (c.B, c.Lq, c.H, 128) and bool((want[:, c.empty_rows()] == 0).all()) and not want.isnan().any()


def test_a_key_at_either_end_of_any_rows_range_moves_that_row_and_no_other():
    least = float("inf")
    for c in A.CASES:
        q, k, v = c.inputs()
        want = c.want()
        assert torch.equal(A.reference(q, k, v, c.allowed()), want)          # the rows of the full sequence's reference are this call's
        for name, mask, sel in A.altered_masks(c):
            moved = _row_moves(A.reference(q, k, v, mask), want)
            assert bool((moved[~sel] == 0).all()), (c.name, name)
            if sel.any():
                least = min(least, float(moved[sel].min()))
                assert float(moved[sel].min()) >= W.SENSITIVITY_ULPS, (c.name, name, float(moved[sel].min()))
    print(f"least move of an altered row: {least:.1f} bf16 ulps")
    assert least >= W.SENSITIVITY_ULPS


# Calls of case 5 (1344 tokens in three frames of 448 = 7 key tiles, one frame either side, no sink) that a mask blind to the offset does
# not move, because it cannot: rank 1 of 8 holds rows 168 .. 335, which lie in frame 0 like rows 0 .. 167 -- the two masks are the same
# mask; the four others hold rows of the last frame, whose keys [448, 1344) mirror the keys [0, 896) rows of frame 0 see: an odd number
# of tiles and half a period of V's channels further on, the same masses per channel under this construction.  Every one of their splits
# has other ranks that are moved (asserted below), so a kernel that ignores the offset fails each split.
OFFSET_BLIND = {"L1344-f1_1-T448-s0-r2of3-b1h2", "L1344-f1_1-T448-s0-r3of4-b1h2", "L1344-f1_1-T448-s0-r1of8-b1h2",
                "L1344-f1_1-T448-s0-r6of8-b1h2", "L1344-f1_1-T448-s0-r7of8-b1h2"}


def test_the_mask_taken_at_the_rows_index_in_the_call_fails_every_case_with_an_offset():
    """... but for the five calls of OFFSET_BLIND, which are exactly 0.0 and whose splits are caught by their other ranks."""
    least, caught = float("inf"), {}
    for c in A.CASES:
        if c.q_offset == 0:
            continue
        q, k, v = c.inputs()
        blind = A.reference(q, k, v, A.allowed(range(c.Lq), c.Lk, c.window, c.T, c.sink))      # the mask a kernel deaf to q_offset applies
        moved = float(_row_moves(blind, c.want()).max())
        split = (c.Lk, c.window, c.T, c.sink, c.ranks)
        if c.name in OFFSET_BLIND:
            assert moved == 0.0, (c.name, moved)
            caught.setdefault(split, 0)
            continue
        least = min(least, moved)
        assert moved >= W.SENSITIVITY_ULPS, (c.name, moved)
        caught[split] = caught.get(split, 0) + 1
    print(f"least move of the most moved row under a mask blind to the offset: {least:.1f} bf16 ulps")
    assert all(n >= 1 for n in caught.values()), caught
    assert OFFSET_BLIND <= {c.name for c in A.CASES}


def test_the_planner_equals_enumeration_at_the_cases_and_around_them():
    for c in A.CASES:
        assert hip.attn_window_at_tiles(c.Lq, c.Lk, c.q_offset, c.window, c.sink, c.T) == A.runs_brute(c), c.name
    n = 0
    for Lk, Lq, off in ((600, 86, 516), (600, 300, 299), (333, 120, 250), (333, 335, 0), (70, 40, 200), (5, 2, 6), (1111, 278, 834), (64, 257, 63)):
        for (a, b), T, sink in itertools.product(((0, 0), (1, 1), (100, 37), (-1, 0), (0, -1), (3, 0), (64, 64), (-1, -1)), (0, 1, 7, 37, 64, 100, 448),
                                                 (0, 1, 5, 64, 70, 300)):
            got = hip.attn_window_at_tiles(Lq, Lk, off, (a, b), sink, T)
            assert got == A.runs_of(A.allowed(range(off, off + Lq), Lk, (a, b), T, sink), Lk), (Lk, Lq, off, a, b, T, sink)
            n += 1
    assert n == 8 * 8 * 7 * 6
    assert hip.attn_window_at_tiles(2, 5, 6, (0, 0)) == [[]] and hip.attn_window_at_tiles(2, 5, 6, (0, 0), sink=3) == [[(0, 0)]]
    for bad in (dict(q_offset=-1), dict(sink=-1), dict(frame_tokens=-1)):
        with pytest.raises(ValueError):
            hip.attn_window_at_tiles(**dict(dict(Lq=10, Lk=10, q_offset=0, window=(1, 1)), **bad))


def test_the_planner_equals_the_three_existing_planners_at_offset_zero_and_one_length():
    """(attn_window_sink_tiles keeps the sink under a window without a left bound, which the entry points drop: compared where they agree.)"""
    for c in W.CASES:
        assert hip.attn_window_at_tiles(c.L, c.L, 0, c.window) == [[t] for t in hip.attn_window_tiles(c.L, c.window)], c.name
    for c in S.CASES:
        assert c.window[0] >= 0
        assert hip.attn_window_at_tiles(c.L, c.L, 0, c.window, c.sink) == hip.attn_window_sink_tiles(c.L, c.window, c.sink), c.name
    for c in F.CASES:
        assert hip.attn_window_at_tiles(c.L, c.L, 0, c.window, c.sink, c.T) == hip.attn_window_frames_tiles(c.L, c.window, c.T, c.sink), c.name
    for L, (a, b), sink, T in itertools.product((70, 600, 1111), ((0, 0), (5, 3), (100, 37), (-1, 0), (0, -1), (2, 1)), (0, 5, 70, 448), (1, 37, 64, 448)):
        assert hip.attn_window_at_tiles(L, L, 0, (a, b), sink, T) == hip.attn_window_frames_tiles(L, (a, b), T, sink)
        if a >= 0:
            assert hip.attn_window_at_tiles(L, L, 0, (a, b), sink) == hip.attn_window_sink_tiles(L, (a, b), sink)


# ----------------------------------------------------------------------------- the engine's host side
SAGE = {"VIDEOX_ATTENTION_TYPE": "SAGE_ATTENTION"}
SWITCHES = ("VIDEOX_ATTENTION_TYPE", "FLEXAM_SAGE_SMOOTH_K", "FLEXAM_SAGE_SMOOTH_V", "FLEXAM_SAGE_WINDOW", "FLEXAM_SP_WINDOW", "FLEXAM_REPLAY",
            "FLEXAM_SHARE_BLOCK0", "FLEXAM_FP8_OPROJ", "FLEXAM_FP8_FFN_APRIORI")


def _engine(sp=8, rank=3, env=(), window=(-1, -1), frames=(-1, -1), L=11648):
    par = D.resolve_parallel(dict(env), 24, sp)
    return types.SimpleNamespace(fused=True, nl=30, nh=24, hd=128, dim=3072, table_limit=1 << 30, fp8=False, sp_size=sp, sp_rank=rank,
                                 sp_mode=par.sp_mode, sp_overlap_level=par.sp_overlap_level, sp_pieces=par.sp_pieces, sp_fused_qkv=par.sp_fused_qkv,
                                 cond=dict(B=2, L=L, dens_same=True), _smooth_k=None, _smooth_v=None, window=window, window_frames=frames, window_sink=448)


def _mode(e, env, monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    return DiTEngine._mode(e, 1, 2, 1, None, True, None)


def test_switch_default_off_and_the_refusal_stays_word_for_word(monkeypatch):
    assert not D.sp_window_asked({}) and not D.sp_window_asked({"FLEXAM_SP_WINDOW": "0"}) and D.sp_window_asked({"FLEXAM_SP_WINDOW": "1"})
    for kw, word in ((dict(window=(100, 37)), "window_size"), (dict(frames=(2, 2)), "window_frames")):
        for env in ({}, {"FLEXAM_SP_WINDOW": "0"}, dict(SAGE, FLEXAM_SAGE_WINDOW="1")):
            with pytest.raises(NotImplementedError) as err:
                _mode(_engine(**kw), env, monkeypatch)
            assert str(err.value) == (f"flexam_amd: {word} under sequence parallelism is not served: a rank's queries and the keys it gathers "
                                      "carry global token indices, which the windowed kernel does not take")
    # one rank, and a model without a window on eight: untouched by the switch
    for env in ({}, {"FLEXAM_SP_WINDOW": "1"}):
        assert _mode(_engine(sp=1, rank=0, window=(100, 37)), env, monkeypatch).sp == 1
        a = _mode(_engine(), env, monkeypatch)
        assert a == _mode(_engine(), {}, monkeypatch) and a.sp == 8


def test_switch_on_resolves_the_layout_of_the_unmasked_forward(monkeypatch):
    on = {"FLEXAM_SP_WINDOW": "1"}
    for sp_env in ({}, {"FLEXAM_SP_MODE": "ulysses"}, {"FLEXAM_SP_PIECES": "2"}):
        for rank in (0, 3, 7):
            plain = _mode(_engine(rank=rank, env=sp_env), {}, monkeypatch)
            for kw in (dict(window=(100, 37)), dict(frames=(2, 2))):
                m = _mode(_engine(rank=rank, env=sp_env, **kw), on, monkeypatch)
                assert m == plain and (m.sp, m.rank, m.lc, m.tok0) == (8, rank, 1456, 1456 * rank) and not m.sage
    # two ranks' modes differ (rank, tok0): their launch plans, keyed on the mode, cannot be confused
    a, b = (_mode(_engine(rank=r, frames=(2, 2)), on, monkeypatch) for r in (3, 4))
    assert a != b and a._replace(rank=4, tok0=b.tok0) == b


def test_sage_under_a_window_and_the_gather_is_cleared_with_the_existing_warning(monkeypatch):
    monkeypatch.setattr(DiTEngine, "_sage_window_warned", False)
    monkeypatch.setattr(DiTEngine, "_sage_warned", False)
    monkeypatch.setattr(DiTEngine, "_smooth_k_warned", True)
    monkeypatch.setattr(DiTEngine, "_smooth_v_warned", True)
    base = _mode(_engine(frames=(2, 2)), {"FLEXAM_SP_WINDOW": "1"}, monkeypatch)
    # without a window SAGE under the default gather is the record gather, padded to 64 x ranks
    rec = _mode(_engine(L=11650), SAGE, monkeypatch)
    assert rec.sage and rec.sage_gather and rec.Lp == 11776
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for env in (dict(SAGE, FLEXAM_SP_WINDOW="1", FLEXAM_SAGE_WINDOW="1"), dict(SAGE, FLEXAM_SP_WINDOW="1")):
            e = _engine(frames=(2, 2))
            m = _mode(e, env, monkeypatch)
            assert m == base and not m.sage and not m.sage_gather and not m.sage_fused and e._smooth_k is False and e._smooth_v is False
        m = _mode(_engine(frames=(2, 2), L=11650), dict(SAGE, FLEXAM_SP_WINDOW="1", FLEXAM_SAGE_WINDOW="1"), monkeypatch)
        assert not m.sage and m.Lp == 11656                        # padded to the ranks alone: bf16 rows are gathered
    said = [str(w.message) for w in seen]
    assert len(said) == 1 and "window_size / window_frames" in said[0] and "windowed bf16 kernel" in said[0], said
    # the all-to-all over heads on an unpadded sequence keeps SAGE with FLEXAM_SAGE_WINDOW=1 and loses it without
    ul = {"FLEXAM_SP_MODE": "ulysses"}
    monkeypatch.setattr(DiTEngine, "_sage_window_warned", True)
    assert _mode(_engine(env=ul, frames=(2, 2)), dict(SAGE, FLEXAM_SP_WINDOW="1", FLEXAM_SAGE_WINDOW="1"), monkeypatch).sage
    assert not _mode(_engine(env=ul, frames=(2, 2)), dict(SAGE, FLEXAM_SP_WINDOW="1"), monkeypatch).sage


def test_the_overlapped_gather_is_waited_for_under_a_window_and_says_so_once(monkeypatch):
    monkeypatch.setattr(DiTEngine, "_sp_window_overlap_warned", False)
    ov = {"FLEXAM_SP_OVERLAP": "1"}
    assert _mode(_engine(env=ov), {}, monkeypatch).sp_overlap_level == 1 and not DiTEngine._sp_window_overlap_warned      # no window: as ever
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for _ in range(2):
            m = _mode(_engine(env=ov, window=(100, 37)), {"FLEXAM_SP_WINDOW": "1"}, monkeypatch)
            assert m.sp_overlap_level == 0 and m.sp_pieces == 2 and m.sp_mode == "allgather"
        # the all-to-all's overlap levels are stages of the exchange, not of the softmax: untouched
        assert _mode(_engine(env={"FLEXAM_SP_MODE": "ulysses"}, window=(100, 37)), {"FLEXAM_SP_WINDOW": "1"}, monkeypatch).sp_overlap_level == 1
    said = [str(w.message) for w in seen if "FLEXAM_SP_OVERLAP" in str(w.message)]
    assert len(said) == 1 and len(seen) == 1, [str(w.message) for w in seen]
