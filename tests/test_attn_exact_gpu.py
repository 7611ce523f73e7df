"""The bf16 flash-attention kernels (csrc/attn.hip) on integer scores: every compared element within 1 bf16 ulp of plain float64
softmax-attention of the same inputs.

With integer scores in exp2 units every p = exp2(s - ref) is an exact power of two whatever reference the online softmax holds, a
power of two survives the bf16 packing of P, every rescale factor is a power of two, and with small-integer V of one sign per channel
the PV sums carry only fp32 rounding (2^-24 relative per addition, no cancellation).  So the output is the float64 attention rounded
once to bf16: within 1/2 ulp, plus the two fp32 roundings of acc * (1 / l).  ONE ulp is that derived bound, not a measured one: a key
dropped or counted twice at a tile, mask, window or split-range edge, or a wrong row in the merge, moves some element by 30 ulps or
more (tests/test_attn_exact_cases_cpu.py proves that for every key of every case below), where the random-data tests of
tests/test_hip_kernels.py allow an absolute 6e-3 on outputs of rms 0.05.  Every row of every case is compared.

The scale-in-kernel instances get softmax_scale = log 2, which reaches the kernel's FMA as exactly 1.0f; the pre-scaled ones integer
q; attn_fwd_lastkey multiplicities that are powers of two, against float64 attention over the explicit copies.

Not covered here: non-integer data, i.e. the bf16 rounding of a general P and v_exp_f32 off the integers.  The random-data tests of
tests/test_hip_kernels.py keep covering those, at their tolerance.

Measured on an MI355X, max |err| / ulp per case (recorded, not asserted; correct rounding gives at most 0.5), no element of any
case more than 1 ulp off:
    scale-lk{31 .. 1111}, scale-lq{255, 256, 257, 300}   0.500   (o is a small dyadic rational in many rows: exact ties occur)
    scale-lq1 0.400, scale-lq31 0.498, scale-lk1 0.000 (o = v_0)
    pre-*, pre-nofull-*                                  0.500
    short-lk{33 .. 256}, short-lk200-all-cus             0.500   short-lk1 0.000
    full-lk{1025 .. 1345}                                0.500
    split-* (all 16)                                     0.500
    partial-scale, partial-pre                           0.500
    lastkey-*-lk{32, 65, 100}-x{2, 512}                  0.500   lastkey-*-lk1-* 0.000
    strided-full, strided-split-3                        0.500
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_exact_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENTINEL = -768.0               # exact in bf16, outside every output (|o| <= 8)


@pytest.fixture(scope="module")
def H():
    from flexam_amd import hip
    hip.load_library()
    return hip


def _dev(*ts):
    return [t.to(BF).cuda() for t in ts]


def _check(case, got, want):
    """got [B, Lq, H, 128] from the kernel, want float64: all rows, 1 bf16 ulp."""
    got = got.double().cpu()
    ulp = X.bf16_ulp(want)
    err = (got - want).abs() / ulp
    bad = ~(err <= 1.0)                                          # (a NaN is bad)
    print(f"{case.name} [{case.instance}]: max |err| / ulp {float(err.max()):.3f}, elements off by more than 1 ulp: {int(bad.sum())}")
    assert not bad.any(), (f"{case.name}: {int(bad.sum())} of {bad.numel()} elements more than 1 bf16 ulp from float64 attention, max |err| / ulp "
                           f"{float(err.nan_to_num(float('inf')).max()):.3g}; first at (b, row, head, channel) = {bad.nonzero()[0].tolist()}: got {float(got[bad][0])}, "
                           f"want {float(want[bad][0])}")


def _run(H, case, q, k, v, out=None):
    kw = dict(softmax_scale=case.scale, prescaled=case.prescaled)
    if case.mult != 1:
        return H.attn_fwd_lastkey(q, k, v, float(case.mult), out=out, **kw)
    if case.splits:
        return H.attn_fwd(q, k, v, out=out, kv_splits=case.splits[0], split_from_unit=case.splits[1], **kw)
    return H.attn_fwd(q, k, v, out=out, kv_splits=1, **kw)


def _exact(H, case, monkeypatch):
    for name, value in case.env:
        monkeypatch.setenv(name, value)
    q, k, v = case.inputs()
    want = case.want(q, k, v)
    if case.cu_budget:
        H.set_cu_budget(case.cu_budget)
    try:
        got = _run(H, case, *_dev(q, k, v))
        torch.cuda.synchronize()
    finally:
        if case.cu_budget:
            H.set_cu_budget(0)
    _check(case, got, want)


@pytest.mark.parametrize("case", X.GENERAL, ids=X.ids(X.GENERAL))
def test_scale_in_kernel_instances(H, case, monkeypatch):
    """<1,false> (Lk <= 1024) and <0,false>: tails of 1, 31, 32, 33, 63, 64, 65 keys, whole tiles, a ragged last q block, one query."""
    _exact(H, case, monkeypatch)


@pytest.mark.parametrize("case", X.PRE, ids=X.ids(X.PRE))
def test_prescaled_general_instances(H, case, monkeypatch):
    """<1,true> above 4 key tiles (SHORT not taken) and <0,true> (FLEXAM_ATTN_FULL=0): the wave-wide rescale trigger."""
    _exact(H, case, monkeypatch)


@pytest.mark.parametrize("case", X.SHORT, ids=X.ids(X.SHORT))
def test_short_context_instance(H, case, monkeypatch):
    """SHORT: 1 to 4 resident key tiles; 24 units on 8 workgroups (set_cu_budget), so a walk crosses a head boundary."""
    if case.cu_budget:
        assert H.attn_units(case.B * case.H, case.lq) > case.cu_budget
    _exact(H, case, monkeypatch)


@pytest.mark.parametrize("case", X.FULL, ids=X.ids(X.FULL))
def test_full_instance_shifted_last_tile(H, case, monkeypatch):
    """FULL: the window [Lk - 64, Lk) and mask_shift at shifts 63, 1, 0 and between, behind main loops that leave 1 to 4 tail tiles."""
    _exact(H, case, monkeypatch)


@pytest.mark.parametrize("case", X.SPLIT, ids=X.ids(X.SPLIT))
def test_split_kv_and_merge(H, case, monkeypatch):
    """Split-KV through FULL and the general instances: 1 to 5 tiles per range, a shorter last range, a last range that is only the
    shifted window, whole and split units in one launch and in two."""
    assert H.attn_effective_splits(case.lk, case.splits[0]) == len(case.range_starts()) + 1
    _exact(H, case, monkeypatch)


@pytest.mark.parametrize("case", X.PARTIAL, ids=X.ids(X.PARTIAL))
def test_partial_calls_and_merge(H, case):
    """attn_fwd_partial + attn_merge in the sequence-parallel order (local chunk, keys before, keys after); the keys after are more
    than 1024, so FULL (pre-scaled) / <0,false> run as a partial call next to <1,*> ones in the same merge."""
    q, k, v = case.inputs()
    want = case.want(q, k, v)
    qd, kd, vd = _dev(q, k, v)
    kw = dict(softmax_scale=case.scale, prescaled=case.prescaled)
    slots = sum(H.attn_effective_splits(hi - lo, n) for lo, hi, n in case.sets)
    ws = H.attn_partial_workspace(case.B, case.H, case.lq, slots, qd.device)
    n = 0
    for lo, hi, splits in case.sets:
        n += H.attn_fwd_partial(qd, kd[:, lo:hi], vd[:, lo:hi], ws, n, splits, **kw)
    assert n == slots
    out = torch.empty(case.B, case.lq, case.H, 128, device=qd.device, dtype=BF)
    H.attn_merge(out, ws, n, **kw)
    _check(case, out, want)


@pytest.mark.parametrize("case", X.LASTKEY, ids=X.ids(X.LASTKEY))
def test_weighted_last_key(H, case, monkeypatch):
    """attn_fwd_lastkey at multiplicities 2 and 512 (log2f exact) against float64 attention over the explicit copies: the bias in raw
    score units (<1,false>), in exp2 units in SHORT and in <1,true> (FLEXAM_ATTN_SHORT=0); the last key alone, ending a half tile,
    opening a tile, in mid tile."""
    _exact(H, case, monkeypatch)


@pytest.mark.parametrize("case", X.STRIDED, ids=X.ids(X.STRIDED))
def test_strided_output_leaves_the_rest_of_the_buffer_alone(H, case, monkeypatch):
    """out= a row and column slice of a larger buffer: the attended rows exact, every other element still the sentinel (the qi < Lq
    store guard of a ragged last q block; the merge kernel's addressing)."""
    q, k, v = case.inputs()
    want = case.want(q, k, v)
    B, lq, Hh = case.B, case.lq, case.H
    big = torch.full((B, lq + 7, 3 * Hh * 128), SENTINEL, device="cuda", dtype=BF)
    out = big[:, 3:3 + lq, Hh * 128:2 * Hh * 128].unflatten(2, (Hh, 128))
    assert out.data_ptr() != big.data_ptr() and not out.is_contiguous()
    _run(H, case, *_dev(q, k, v), out=out)
    torch.cuda.synchronize()
    _check(case, out, want)
    rest = big.clone()
    rest[:, 3:3 + lq, Hh * 128:2 * Hh * 128] = SENTINEL
    assert bool((rest == SENTINEL).all()), f"{case.name}: {int((rest != SENTINEL).sum())} elements outside the output view were written"
