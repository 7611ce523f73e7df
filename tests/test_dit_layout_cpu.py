"""CPU: the layout arithmetic and the switch resolution of the DiT engine (flexam_amd/dit_layout.py) on plain values -- what only the
multi-rank GPU tests (tests/test_sp_gpu.py) saw before.  Expected numbers are literals: those of the 5B clip (L = 11648) and of the
padded cases come from the expressions the engine evaluated inline before they moved."""
import pytest

from flexam_amd import dit_layout as D
from flexam_amd import hip
from flexam_amd.dist import chunk_bounds

CASES = [(11648, 8), (11648, 3), (5, 4), (130, 4)]
# (local, before, after) key counts, requested splits and slot total per rank, for one sample's 24 heads (and the pair's 48 at the clip)
RANGES_24 = {
    (11648, 8): [([1456, 0, 10192], [1, 0, 7], 8), ([1456, 1456, 8736], [1, 1, 7], 9), ([1456, 2912, 7280], [1, 5, 7], 13),
                 ([1456, 4368, 5824], [1, 7, 7], 15), ([1456, 5824, 4368], [1, 7, 7], 15), ([1456, 7280, 2912], [1, 7, 5], 13),
                 ([1456, 8736, 1456], [1, 7, 1], 9), ([1456, 10192, 0], [1, 7, 0], 8)],
    (11648, 3): [([3883, 0, 7765], [2, 0, 2], 4), ([3883, 3883, 3882], [2, 2, 2], 6), ([3882, 7766, 0], [2, 2, 0], 4)],
    (5, 4): [([2, 0, 3], [1, 0, 1], 2), ([2, 2, 1], [1, 1, 1], 3), ([1, 4, 0], [1, 1, 0], 2), ([0, 5, 0], [0, 1, 0], 1)],
    (130, 4): [([33, 0, 97], [1, 0, 1], 2), ([33, 33, 64], [1, 1, 1], 3), ([33, 66, 31], [1, 1, 1], 3), ([31, 99, 0], [1, 1, 0], 2)],
}
RANGES_48_CLIP = [([1456, 0, 10192], [2, 0, 7], 9), ([1456, 1456, 8736], [2, 2, 7], 11), ([1456, 2912, 7280], [2, 5, 7], 14),
                  ([1456, 4368, 5824], [2, 7, 7], 16), ([1456, 5824, 4368], [2, 7, 7], 16), ([1456, 7280, 2912], [2, 7, 5], 14),
                  ([1456, 8736, 1456], [2, 7, 2], 11), ([1456, 10192, 0], [2, 7, 0], 9)]


# ----------------------------------------------------------------------------- token layout
def test_token_layout_of_the_clip_and_of_padded_sequences():
    assert D.token_layout(11648, 8, 0)[:2] == (11648, 1456)
    assert D.token_layout(11648, 3, 0)[:2] == (11649, 3883)
    assert [D.key_range_sizes(5, 4, r)[0] for r in range(4)] == [2, 2, 1, 0]                    # real tokens per rank
    for L, sp in CASES:
        for r in range(sp):
            assert D.token_layout(L, sp, r)[2] == chunk_bounds(L, r, sp)[0]


def test_token_layout_under_the_record_gather_is_whole_key_tiles():
    assert hip.ATTN_KV_TILE == 64
    assert D.token_layout(11648, 8, 0, 8 * 64)[:2] == (11776, 1472) and 1472 % 64 == 0
    assert D.token_layout(100, 2, 0, 2 * 64)[0] == 128
    for r in range(8):
        Lp, lc, tok0 = D.token_layout(11648, 8, r, 8 * 64)
        assert tok0 == chunk_bounds(Lp, r, 8)[0] == r * 1472


# ----------------------------------------------------------------------------- key ranges of the overlapped gather
@pytest.mark.parametrize("L,sp", CASES)
def test_key_ranges_partition_the_real_tokens(L, sp):
    for rank in range(sp):
        Lp, lc, tok0 = D.token_layout(L, sp, rank)
        kr = D.gather_key_ranges(L, sp, rank, 24)
        n_loc, n_before, n_after = kr.sizes
        # in the gathered buffer: before = [0, n_before), local = [tok0, tok0 + n_loc), after = [tok0 + lc, tok0 + lc + n_after)
        spans = [(0, n_before), (tok0, tok0 + n_loc), (tok0 + lc, tok0 + lc + n_after)]
        spans = [s for s in spans if s[1] > s[0]]
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))                 # disjoint and in order
        keys = [t for lo, hi in spans for t in range(lo, hi)]
        assert keys == list(range(L))                                              # exactly the real tokens: no pad row, none missing
        if tok0 >= L:
            assert n_loc == 0                                                      # a rank of pads only
        assert kr.total == sum(hip.attn_effective_splits(n, s) for n, s in zip(kr.sizes, kr.splits) if n)
        assert all((n == 0) == (s == 0) == (e == 0) for n, s, e in zip(kr.sizes, kr.splits, kr.slots))
        assert (list(kr.sizes), list(kr.splits), kr.total) == RANGES_24[L, sp][rank]


def test_key_range_splits_follow_the_work_units_of_the_call():
    """The CFG pair's 48 (sample, head) units per query block ask for other splits than one sample's 24."""
    got = [D.gather_key_ranges(11648, 8, r, 48) for r in range(8)]
    assert [(list(k.sizes), list(k.splits), k.total) for k in got] == RANGES_48_CLIP


# ----------------------------------------------------------------------------- o-projection offsets behind the all-to-all
@pytest.mark.parametrize("d,G", [(3072, 1536), (3072, 768), (3072, 384), (256, 128)])
def test_a2a_koff_addresses_whole_k_blocks_inside_one_rank_block(d, G):
    rows = 7
    assert G % 64 == 0                                                             # no K block straddles two rank blocks
    koff = D.a2a_koff(d, G, rows)
    assert len(koff) == d // 64
    for kb, off in enumerate(koff):
        assert off == (kb * 64 // G) * rows * G + (kb * 64) % G
    if (d, G) == (256, 128):
        assert koff == [0, 64, 896, 960]


# ----------------------------------------------------------------------------- set_parallel's resolution
def test_parallel_defaults():
    assert D.resolve_parallel({}, 24, 8) == ("allgather", 0, 1, True)
    assert D.resolve_parallel({"FLEXAM_SP_MODE": "ulysses"}, 24, 8) == ("ulysses", 1, 1, True)
    assert D.resolve_parallel({"FLEXAM_SP_MODE": "ulysses"}, 24, 5).sp_mode == "allgather"      # heads do not divide: the gather
    assert D.resolve_parallel({"FLEXAM_SP_MODE": "ulysses", "FLEXAM_SP_OVERLAP": "2"}, 24, 8).sp_overlap_level == 2
    assert D.resolve_parallel({"FLEXAM_SP_OVERLAP": "off"}, 24, 8).sp_overlap_level == 0
    assert D.resolve_parallel({"FLEXAM_SP_OVERLAP": " Yes "}, 24, 8).sp_overlap_level == 1
    assert D.resolve_parallel({"FLEXAM_SP_FUSED_QKV": "0"}, 24, 8).sp_fused_qkv is False
    assert D.SINGLE_RANK == (None, 0, 1, True)


def test_parallel_pieces():
    ov = {"FLEXAM_SP_OVERLAP": "1"}
    assert [D.resolve_parallel(ov, 24, sp).sp_pieces for sp in (2, 3, 4, 8)] == [1, 1, 2, 2]
    assert D.resolve_parallel({}, 24, 8).sp_pieces == 1                                          # no overlap: one piece
    assert D.resolve_parallel({"FLEXAM_SP_MODE": "ulysses"}, 24, 8).sp_pieces == 1                # pieces belong to the gather
    assert D.resolve_parallel({"FLEXAM_SP_MODE": "ulysses", "FLEXAM_SP_PIECES": "3"}, 24, 8).sp_pieces == 1
    assert D.resolve_parallel(dict(ov, FLEXAM_SP_PIECES="3"), 24, 8).sp_pieces == 3
    assert D.resolve_parallel(dict(ov, FLEXAM_SP_PIECES="3"), 24, 1).sp_pieces == 1              # one rank: nothing to cut
    assert D.resolve_parallel(ov, 3, 4).sp_pieces == 1                                           # an odd head count is not halved
    with pytest.raises(ValueError, match="FLEXAM_SP_PIECES"):
        D.resolve_parallel(dict(ov, FLEXAM_SP_PIECES="5"), 24, 8)
    with pytest.raises(ValueError, match="FLEXAM_SP_PIECES"):
        D.resolve_parallel(dict(ov, FLEXAM_SP_PIECES="0"), 24, 8)
    with pytest.raises(ValueError, match="FLEXAM_SP_MODE"):
        D.resolve_parallel({"FLEXAM_SP_MODE": "ring"}, 24, 8)


# ----------------------------------------------------------------------------- the mode of a forward
SAGE = {"VIDEOX_ATTENTION_TYPE": "SAGE_ATTENTION"}


def mode(env=None, **kw):
    """The sampler's CFG pair on one latent at the 5B model, one rank, unless `kw` says otherwise."""
    a = dict(fused=True, nl=30, nh=24, hd=128, dim=3072, table_limit=1 << 30, fp8=False, sp=1, rank=0, parallel=D.SINGLE_RANK,
             B=2, L=11648, dens_same=True, bx=1, R=2, rows_per_batch=1, only_row=None, rows_shared=True, teacache=False)
    a.update(kw)
    return D.resolve_mode(env or {}, **a)


def test_mode_sizes_and_identity():
    m = mode()
    assert (m.B, m.Lp, m.lc, m.tok0, m.R, m.rows_per_batch, m.only_row) == (2, 11648, 11648, 0, 2, 1, None)
    assert (m.sp, m.rank, m.sp_mode, m.sp_pieces, m.sp_overlap_level, m.sp_fused_qkv) == (1, 0, None, 1, 0, True)
    assert m._fields == ("B", "Lp", "lc", "tok0", "R", "rows_per_batch", "only_row", "per_layer", "share0", "sage", "sage_gather",
                         "sage_fused", "fp8", "fp8_oproj", "ffn_apriori", "sp", "rank", "sp_mode", "sp_pieces", "sp_overlap_level",
                         "sp_fused_qkv", "use_plan")
    assert hash(m) == hash(mode()) and m == mode() and {m: 1}[mode()] == 1
    assert m != mode(R=4)
    assert mode(only_row=1).B == 1
    r5 = mode(sp=8, rank=5, parallel=D.resolve_parallel({}, 24, 8))
    assert (r5.Lp, r5.lc, r5.tok0) == (11648, 1456, 7280)
    assert mode(L=11647, sp=8, rank=7, parallel=D.resolve_parallel({}, 24, 8))[1:4] == (11648, 1456, 10192)


def test_mode_sage():
    gather, a2a = D.resolve_parallel({}, 24, 8), D.resolve_parallel({"FLEXAM_SP_MODE": "ulysses"}, 24, 8)
    assert not mode().sage and not mode().sage_fused
    m = mode(SAGE)
    assert m.sage and m.sage_fused and not m.sage_gather                                         # one rank
    assert mode(SAGE, nh=12).sage and not mode(SAGE, nh=12).sage_fused                            # the fused operand write: 24 heads only
    assert not mode(SAGE, fused=False).sage
    assert mode(SAGE, sp=8, parallel=a2a).sage and not mode(SAGE, sp=8, parallel=a2a).sage_gather
    assert not mode(SAGE, sp=8, parallel=a2a, L=11647).sage                                      # all-to-all: only when Lp == L
    m = mode(SAGE, sp=8, rank=1, parallel=gather)
    assert m.sage and m.sage_gather and (m.Lp, m.lc, m.tok0) == (11776, 1472, 1472)              # records travel: 64 x ranks padding
    assert mode(sp=8, rank=1, parallel=gather)[1:4] == (11648, 1456, 1456)
    for env in ({"FLEXAM_SP_OVERLAP": "1"}, {"FLEXAM_SP_OVERLAP": "1", "FLEXAM_SP_PIECES": "1"}, {"FLEXAM_SP_PIECES": "2"}):
        m = mode(SAGE, sp=8, parallel=D.resolve_parallel(env, 24, 8))
        assert not m.sage and not m.sage_gather and m.Lp == 11648                                # overlap or pieces: the bf16 kernel


def test_mode_share0_needs_every_condition():
    assert mode().share0
    for kw in (dict(B=1), dict(B=3), dict(bx=2), dict(sp=2, parallel=D.resolve_parallel({}, 24, 2)), dict(rows_shared=False),
               dict(dens_same=False), dict(teacache=True), dict(fused=False), dict(only_row=0)):
        assert not mode(**kw).share0, kw
    assert not mode({"FLEXAM_SHARE_BLOCK0": "0"}).share0


def test_mode_tables_plan_and_fp8_switches():
    at_limit = 30 * 2 * 6 * 3072 * 4
    assert not mode(table_limit=at_limit).per_layer and mode(table_limit=at_limit - 1).per_layer
    assert mode(fused=False).per_layer
    assert mode().use_plan
    for env, kw in (({}, dict(teacache=True)), ({}, dict(table_limit=at_limit - 1)), ({}, dict(fused=False)), ({"FLEXAM_REPLAY": "0"}, {})):
        assert not mode(env, **kw).use_plan, (env, kw)
    assert not mode().fp8 and not mode({"FLEXAM_FP8_OPROJ": "1"}).fp8_oproj                      # the o-projection switch needs fp8
    assert mode(fp8=True).fp8 and not mode(fp8=True).fp8_oproj and mode({"FLEXAM_FP8_OPROJ": "1"}, fp8=True).fp8_oproj
    assert mode().ffn_apriori and not mode({"FLEXAM_FP8_FFN_APRIORI": "0"}).ffn_apriori
