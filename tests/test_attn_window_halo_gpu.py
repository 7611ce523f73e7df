"""GPU: the windowed bf16 kernel at a query offset on a COMPACT key buffer (attn_window_halo_kernel of csrc/attn.hip,
flexam_attn_fwd_window_halo): what a rank runs when it has fetched only the halo of keys its window reaches (dit_layout.halo_plan).

For every rank case of tests/attn_window_at_cases.CASES and both forms of the kernel: K and V are packed by the plan into the middle of
a larger allocation whose other rows are NaN, the entry point is called through the C ABI, and the output is bit-equal to
flexam_attn_fwd_window_at on the full keys -- both launches visit the same tiles in the same order -- and within one bf16 ulp of the
float64 masked attention, the tolerance of tests/test_attn_window_at_gpu.py; no NaN row is ever read into the result.  key_gap_tiles = 0
with k_rows = Lk gives the bits of _at.  A buffer one tile short at its end, a gap one tile too large (with and without the rows that go
with it) and a compact buffer under a call that sees every key are FLEXAM_E_ARG, and the output is not touched: nothing was launched.

Not blind (CPU, first test): packed with gap + 1 -- every window key one tile off -- the float64 reference of at least one case moves
by more than the ulp the comparison allows."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_at_cases as A  # noqa: E402
from flexam_amd.dit_layout import halo_plan  # noqa: E402

BF = torch.bfloat16
LN2 = math.log(2.0)
TILE = A.KV_TILE
RANK_CASES = [c for c in A.CASES if c.rank is not None]
FORMS = pytest.mark.parametrize("prescaled", [False, True], ids=["scale-in-kernel", "prescaled"])


def _plan(c):
    return halo_plan(c.Lk, c.ranks, c.rank, c.window, c.sink, c.T)


def _s_n(c):
    return -(-min(c.sink, c.Lk) // TILE) if c.window[0] >= 0 else 0


def _buffer_keys(c, gap, rows):
    """The global key of every buffer row under the kernel's address rule (clamped to the last key: a wrong gap may point past it)."""
    key = torch.arange(rows)
    return torch.where(key < _s_n(c) * TILE, key, key + gap * TILE)


def _pack(c, t, gap, rows, margin=TILE + 5):
    """t [B, Lk, H, 128] -> the rows the plan names, in the middle of an allocation of NaN rows: (the view, the allocation)."""
    big = torch.full((t.shape[0], rows + 2 * margin, t.shape[2], 128), float("nan"), dtype=t.dtype)
    big[:, margin:margin + rows] = t[:, _buffer_keys(c, gap, rows)]
    return big[:, margin:margin + rows], big


def test_a_gap_one_tile_too_large_moves_the_float64_reference():
    """CPU: the comparison below is not blind to the address rule.  With the window tiles packed from s_n + gap + 1 on and read as if
    packed from s_n + gap, row i's window keys are those of one tile further: the reference under THAT reading differs from want()."""
    moved = 0
    for c in RANK_CASES:
        plan = _plan(c)
        last = _s_n(c) * TILE + (plan.rows - _s_n(c) * TILE) + (plan.gap + 1) * TILE      # one behind the last key the shifted buffer names
        if plan.rows <= _s_n(c) * TILE or last > c.Lk:
            continue                                                   # no window tiles, or no tile further to take them from
        q, k, v = c.inputs()
        src = _buffer_keys(c, plan.gap + 1, plan.rows)                 # what the shifted buffer holds ...
        dst = _buffer_keys(c, plan.gap, plan.rows)                     # ... and where the kernel believes it is
        k2, v2 = k.clone(), v.clone()
        k2[:, dst], v2[:, dst] = k[:, src], v[:, src]
        got = A.reference(q, k2, v2, c.allowed())
        err = (got - c.want()).abs() / A.bf16_ulp(c.want())
        moved += bool((err > 1.0).any())
    assert moved >= 1, "no case tells a buffer packed one tile off from the right one"
    print(f"{moved} cases move by more than 1 bf16 ulp under gap + 1")


@pytest.fixture(scope="module")
def H():
    from flexam_amd import hip
    hip.load_library()
    return hip


def _scale(H, prescaled):
    return H._softmax_scale(None if prescaled else LN2, prescaled, 128)


def _halo_call(H, c, q, kc, vc, out, gap, k_rows, prescaled, Lk=None):
    """The C ABI, not the wrapper: the status, and the message of a refusal."""
    lib = H.load_library()
    st = lib.flexam_attn_fwd_window_halo(q.data_ptr(), q.stride(0), q.stride(1), kc.data_ptr(), kc.stride(0), kc.stride(1), vc.data_ptr(),
                                         vc.stride(0), vc.stride(1), out.data_ptr(), out.stride(0), out.stride(1), c.B, c.H, c.Lq,
                                         c.Lk if Lk is None else Lk, 128, _scale(H, prescaled), *H.attn_window(c.window), c.T, c.sink,
                                         c.q_offset, gap, k_rows, torch.cuda.current_stream().cuda_stream)
    return st, lib.flexam_last_error()


@pytest.mark.gpu
@FORMS
@pytest.mark.parametrize("case", RANK_CASES, ids=A.ids(RANK_CASES))
def test_compact_buffer_gives_the_bits_of_the_full_keys(H, case, prescaled):
    from flexam_amd import abi
    from test_attn_window_gpu import _check
    E_ARG = abi.CONSTANTS["FLEXAM_E_ARG"]
    c, plan = case, _plan(case)
    q, k, v = (t.to(BF) for t in c.inputs())
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    full = H.attn_fwd_window(qd, kd, vd, c.window, sink=c.sink, frame_tokens=c.T, q_offset=c.q_offset,
                             softmax_scale=None if prescaled else LN2, prescaled=prescaled)
    kbig, vbig = (_pack(c, t, plan.gap, plan.rows)[1].cuda() for t in (k, v))
    margin = (kbig.shape[1] - plan.rows) // 2
    kc, vc = kbig[:, margin:margin + plan.rows], vbig[:, margin:margin + plan.rows]
    if plan.rows == 0:                                   # (a rank of pads: a pointer the call never follows)
        kc, vc = kbig[:, margin:margin + 1], vbig[:, margin:margin + 1]
    out = torch.full_like(full, -768.0)
    st, msg = _halo_call(H, c, qd, kc, vc, out, plan.gap, plan.rows, prescaled)
    torch.cuda.synchronize()
    assert st == 0, msg
    assert torch.equal(out, full), f"{c.name}: compact buffer (gap {plan.gap}, rows {plan.rows} of {c.Lk}) differs from the full keys"
    _check(f"{c.name} halo [{'prescaled' if prescaled else 'scale in kernel'}]", out, c.want())
    # the whole sequence through this entry point is flexam_attn_fwd_window_at
    out.fill_(-768.0)
    st, msg = _halo_call(H, c, qd, kd, vd, out, 0, c.Lk, prescaled)
    torch.cuda.synchronize()
    assert st == 0 and torch.equal(out, full), msg
    # wrong plans: refused, and nothing launched
    if plan.gap == 0 and plan.rows == c.Lk:
        return
    out.fill_(-768.0)
    wrong = []
    if plan.rows > 0:
        wrong.append(("one tile short at the end", plan.gap, max(plan.rows - TILE, 0)))
    if plan.rows > _s_n(c) * TILE:                      # window tiles behind the sink tiles
        wrong += [("gap + 1", plan.gap + 1, plan.rows), ("one tile short at the front of the window run", plan.gap + 1, max(plan.rows - TILE, 0))]
    for what, gap, rows in wrong:
        st, msg = _halo_call(H, c, qd, kc, vc, out, gap, rows, prescaled)
        assert st == E_ARG and b"attn_fwd_window_halo" in msg, (what, st, msg)
    torch.cuda.synchronize()
    assert bool((out == -768.0).all()), "a refused call launched"


@pytest.mark.gpu
def test_wrapper_and_argument_errors(H):
    from flexam_amd import abi
    E_ARG = abi.CONSTANTS["FLEXAM_E_ARG"]
    c = next(x for x in RANK_CASES if x.sink == 70 and x.rank == 2)
    plan = _plan(c)
    assert plan.gap > 0 and plan.rows < c.Lk
    q, k, v = (t.to(BF) for t in c.inputs())
    kc, vc = (_pack(c, t, plan.gap, plan.rows)[0].contiguous().cuda() for t in (k, v))
    qd = q.cuda()
    full = H.attn_fwd_window(qd, k.cuda(), v.cuda(), c.window, sink=c.sink, q_offset=c.q_offset, prescaled=True)
    got = H.attn_fwd_window(qd, kc, vc, c.window, sink=c.sink, q_offset=c.q_offset, prescaled=True, key_gap_tiles=plan.gap, Lk=c.Lk)
    assert torch.equal(got, full)
    # k_rows: the first rows of a longer buffer
    pad = lambda t: torch.cat([t, torch.full_like(t[:, :9], float("nan"))], 1)
    got = H.attn_fwd_window(qd, pad(kc), pad(vc), c.window, sink=c.sink, q_offset=c.q_offset, prescaled=True, key_gap_tiles=plan.gap, Lk=c.Lk,
                            k_rows=plan.rows)
    assert torch.equal(got, full)
    with pytest.raises(RuntimeError, match="q_offset and the global key count"):
        H.attn_fwd_window(qd, kc, vc, c.window, sink=c.sink, key_gap_tiles=plan.gap)
    with pytest.raises(RuntimeError, match="k_rows"):
        H.attn_fwd_window(qd, kc, vc, c.window, sink=c.sink, q_offset=c.q_offset, key_gap_tiles=plan.gap, Lk=c.Lk, k_rows=plan.rows + 1)
    with pytest.raises(RuntimeError, match="attn_fwd_window_halo"):
        H.attn_fwd_window(qd, kc, vc, c.window, sink=c.sink, q_offset=c.q_offset, prescaled=True, key_gap_tiles=plan.gap + 1, Lk=c.Lk)
    out = torch.full_like(full, -768.0)
    # a call that sees every key cannot run on a compact buffer; nor can a negative gap or more rows than keys
    wide = A.Case(c.Lk, (5000, 5000), 0, c.sink, c.ranks, c.rank)
    for case, gap, rows in ((wide, plan.gap, plan.rows), (wide, 0, c.Lk - 1), (c, -1, plan.rows), (c, plan.gap, c.Lk + 1), (c, plan.gap, -1)):
        st, msg = _halo_call(H, case, qd, kc, vc, out, gap, rows, True)
        assert st == E_ARG and b"attn_fwd_window_halo" in msg, (gap, rows, st, msg)
    torch.cuda.synchronize()
    assert bool((out == -768.0).all())
