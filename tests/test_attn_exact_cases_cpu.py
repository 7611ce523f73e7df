"""The integer-score attention cases (tests/attn_exact_cases.py) are what tests/test_attn_exact_gpu.py takes them for -- checked
without a GPU, for every case of the GPU list: bf16-exact inputs, integer scores within 120 binades of the row maximum, a reference
that moves in the ramp rows, and no blind key: dropping any key, or counting it twice, moves some compared output by >= 8 bf16 ulps."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_exact_cases as X  # noqa: E402


def test_log2_scale_reaches_the_kernel_as_exactly_one():
    """softmax_scale = log 2 crosses the C ABI as a float and is multiplied by 1.4426950408889634f there (attn_run): exactly 1.0f,
    so fma(s, c, -m c) is s - m on integers.  The neighbouring floats do not give 1."""
    s = np.float32(X.LN2)
    log2e = np.float32(1.4426950408889634)
    assert s * log2e == np.float32(1.0)
    assert np.nextafter(s, np.float32(0)) * log2e != np.float32(1.0)
    assert np.nextafter(s, np.float32(1)) * log2e != np.float32(1.0)


def test_case_names_are_unique_and_every_listed_instance_is_what_dispatch_gives():
    assert len({c.name for c in X.ALL}) == len(X.ALL)
    for c in X.ALL:
        for lk, n in ([(hi - lo, n) for lo, hi, n in c.sets] if c.sets else [(c.lk, c.splits[0] if c.splits else 1)]):
            got = X.dispatch(lk, c.prescaled, n > 1, bool(c.sets), c.mult, c.env)
            if c.sets and lk <= 1024:
                assert got in ("<1,true>", "<1,false>")              # the short key sets of a partial case
            else:
                assert got == c.instance, (c.name, got)
    assert {c.instance for c in X.ALL} == {"<0,false>", "<1,false>", "<0,true>", "<1,true>", "FULL", "SHORT"}


def test_partial_cases_have_a_key_set_above_1024_keys_and_one_below_and_no_aligned_bound():
    for c in X.PARTIAL:
        sizes = [hi - lo for lo, hi, _ in c.sets]
        assert max(sizes) > 1024 and min(sizes) <= 1024 and sum(sizes) == c.lk
        assert sorted(k for lo, hi, _ in c.sets for k in range(lo, hi)) == list(range(c.lk))
        assert all(b % X.KV_TILE for lo, hi, _ in c.sets for b in (lo, hi) if 0 < b)


def test_split_cases_cover_one_to_five_tiles_per_range_and_the_shifted_tile_alone():
    per = {(c.instance, -(-X.tiles(c.lk) // c.splits[0])) for c in X.SPLIT}
    for inst in ("FULL", "<0,false>"):
        assert {n for i, n in per if i == inst} >= {1, 2, 3, 4, 5}
    alone = [c for c in X.SPLIT if c.instance == "FULL" and c.lk % 64 and c.range_starts()[-1] == 64 * (X.tiles(c.lk) - 1)]
    assert alone                                                     # a last range that is only the shifted window
    for c in X.SPLIT:
        units = c.B * c.H * -(-c.lq // X.Q_BLOCK)
        assert 0 <= c.splits[1] < units
    assert {dict(c.env).get("FLEXAM_ATTN_FUSED_TAIL") for c in X.SPLIT if c.splits[1] > 0} == {"0", "1"}


@pytest.mark.parametrize("case", X.ALL, ids=X.ids(X.ALL))
def test_case_is_exact_and_no_key_is_blind(case):
    q, k, v = case.inputs()
    assert all(X.bf16_exact(t) for t in (q, k, v))
    s = X.scores(q, k, case.mult)
    assert torch.equal(s, s.round())
    assert float((s.amax(-1, keepdim=True) - s).max()) <= 120.0
    want = case.want(q, k, v)
    assert torch.isfinite(want).all() and float(want.abs().min()) >= 1.0        # |v| >= 1, one sign per channel: no cancellation
    if case.special and not case.sets:
        kind = X.row_kinds(case.lq)
        moves = X.reference_moves(s)[:, :, kind == 0]
        need = 2 if case.lk >= 96 else 1 if case.lk >= 64 else 0
        print(f"{case.name}: the reference moves {int(moves.min())} .. {int(moves.max())} times in the rising-ramp rows")
        assert int(moves.min()) >= need
        last = s[:, :, kind == 2]                                                # rows whose maximum is the last real key
        assert bool((last.argmax(-1) == case.lk - 1).all())
        assert bool((s[:, :, kind == 1].argmax(-1) < 64).all())                  # falling ramp: the maximum in the first tile
    if case.lk == 1:
        return
    drop, twice, at_drop, at_twice = X.sensitivity(q, k, v, case.mult)
    print(f"{case.name}: least-sensitive key moves an output by {drop:.1f} ulps when dropped (b, h, key = {at_drop}), "
          f"{twice:.1f} ulps when counted twice {at_twice}")
    assert drop >= X.SENSITIVITY_ULPS and twice >= X.SENSITIVITY_ULPS


def test_sensitivity_sees_a_key_no_row_looks_at():
    """The measure itself: once no row points at positions 7 and 39 of a tile, the keys there are reported blind."""
    q, k, v = X.build(300, 100, special=False)
    assert min(X.sensitivity(q, k, v)[:2]) >= X.SENSITIVITY_ULPS
    q[..., 7] = 0.0
    q[..., 39] = 0.0
    drop, twice, at_drop, at_twice = X.sensitivity(q, k, v)
    assert drop < X.SENSITIVITY_ULPS and twice < X.SENSITIVITY_ULPS
    assert at_drop[2] in (7, 39, 71) and at_twice[2] in (7, 39, 71)


def test_reference_is_softmax_attention():
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(1, n, 2, 128, generator=g, dtype=torch.float64) for n in (5, 9, 9))
    want = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), scale=math.log(2.0))
    torch.testing.assert_close(X.reference(q, k, v), want.transpose(1, 2), rtol=1e-12, atol=1e-12)
    both = X.reference_lastkey(q, k, v, 4)
    s = X.scores(q, k, 4)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    torch.testing.assert_close(both, torch.einsum("bhlm,bmhd->blhd", p / p.sum(-1, keepdim=True), v), rtol=1e-12, atol=1e-12)
