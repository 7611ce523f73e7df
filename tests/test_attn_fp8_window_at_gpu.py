"""GPU: the windowed MXFP8 self-attention at a query offset on chunked records (flexam_attn_fwd_fp8_window_at: attn8_window_at_kernel /
attn8_window_at_oshift_kernel of csrc/attn_fp8.inc; hip.attn_fwd_fp8_chunked with a window), a rank's call under sequence parallelism
and the MXFP8 record gather, against tests/mxfp8_window_restatement.py on the masks of tests/attn_window_at_cases.py.

(a) Integer cases (tests/attn_fp8_window_at_cases.py: every rank of L = 70 on 2, 600 on 2 and 1111 on 3 ranks, lc = 64 ceil(L / (64 n));
    tests/test_attn_fp8_window_at_cases_cpu.py shows that a mask blind to the offset, a mask one key off at either end and a chunk index
    one off each move a row of every call with an offset by 8 ulps or more): EVERY element of EVERY row within 1 bf16 ulp of the
    windowed restatement of rows q_offset .. q_offset + Lq - 1; rows that see no key exactly zero (with an output shift as well).  The
    records of a pad key hold a real token's key and value, not zeros: a pad key let in moves the output.
(b) Random unit-variance data against the restatement at the bound of tests/test_attn_fp8_restated_gpu.py, rel-RMS <= 3.2e-3, whose
    smallest support is 40 keys per row (asserted: every row, pad rows included, sees 64 keys or more), every rank of L = 1111 on 3.
(c) The normalisations, byte for byte: q_offset = 0, Lq == Lk and one chunk is flexam_attn_fwd_fp8_window; a window that clips no row of
    this call, or a sink that holds every key, is flexam_attn_fwd_fp8_chunked at kv_splits = 1 (with o_shift: FLEXAM_E_ARG); a window
    without a left bound drops the sink.
(d) The argument errors.  (e) A strided `out`.

Measured on an MI355X (recorded, not asserted): (a) max |err| / ulp 0.499 .. 0.554 over the 25 calls, no element more than 1 ulp off,
the 55 empty rows of L = 70 / (3, 2) / rank 1 exactly zero without and with the output shift; the strided output 0.523.  (b) rel-RMS
against the restatement 9.8e-4 .. 1.22e-3 at (200, 100) sink 192 and 8.1e-4 .. 1.08e-3 at frames (2, 1) of 64, ranks 0 / 1 / 2."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_fp8_window_at_cases as P  # noqa: E402
import attn_window_at_cases as A  # noqa: E402
from test_attn_fp8_gpu import _inputs  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
REL_RMS = 3.2e-3            # tests/test_attn_fp8_restated_gpu.py


@pytest.fixture(scope="module")
def H():
    from flexam_amd import hip
    hip.load_library()
    return hip


def _pack_ranks(H, q, k, v, lc, ranks):
    """q, k, v [B, ranks lc, H, 128] on the device -> ([(q8, qs) of every rank], records uint8 [ranks, B, H, lc / 64, REC] rank-major)."""
    bufs = [H.attn_fp8_pack(*(t[:, r * lc:(r + 1) * lc] for t in (q, k, v))) for r in range(ranks)]
    return [(b[0], b[1]) for b in bufs], torch.stack([b[2] for b in bufs]).contiguous()


_packed = {}


def _operands(H, c):
    """The packed operands of the call's split, once per split."""
    key = (c.Lk, c.ranks, c.window, c.sink, c.T, c.B, c.H)
    if key not in _packed:
        _packed[key] = _pack_ranks(H, *(t.cuda() for t in c.padded()), c.lc, c.ranks)
    return _packed[key]


def _run(H, c, out=None):
    qbufs, recs = _operands(H, c)
    shift = c.shift()
    return H.attn_fwd_fp8_chunked(*qbufs[c.rank], recs, c.lc, c.Lk, out=out, window=c.window, sink=c.sink, frame_tokens=c.T, q_offset=c.q_offset,
                                  o_shift=None if shift is None else shift.cuda())


def _check(name, got, want, empty):
    got = got.double().cpu()
    err = (got - want).abs() / P.bf16_ulp(want)
    bad = ~(err <= 1.0)                                                # (a NaN is bad)
    print(f"{name}: max |err| / ulp {float(err.nan_to_num(float('inf')).max()):.3f}, elements off by more than 1 ulp: {int(bad.sum())}, "
          f"empty rows {int(empty.sum())}")
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.numel()} elements more than 1 bf16 ulp from the restatement; first at "
                           f"(b, row, head, channel) = {bad.nonzero()[0].tolist()}: got {float(got[bad][0])}, want {float(want[bad][0])}")
    assert bool((got[:, empty] == 0).all()), f"{name}: a row that sees no key is not zeros"


# ----------------------------------------------------------------------------- (a) integer scores
@pytest.mark.parametrize("c", P.CASES, ids=P.ids(P.CASES))
def test_integer_scores_within_one_bf16_ulp_of_the_windowed_restatement_at_the_ranks_offset(H, c):
    _check(c.name, _run(H, c), c.want(), c.empty_rows())


# ----------------------------------------------------------------------------- (b) random data
@pytest.mark.parametrize("window,sink,T", [((200, 100), 192, 0), ((2, 1), 0, 64)], ids=["w200_100-s192", "f2_1-T64"])
def test_random_data_against_the_windowed_restatement_on_every_rank(H, window, sink, T):
    L, ranks = 1111, 3
    lc = P.chunk_rows(L, ranks)
    q, k, v = _inputs(1, 2, ranks * lc, 300 + L + T)
    k[:, L:], v[:, L:] = 0, 0                                          # pad keys as the pack writes keys past L: the restatement's V blocks
    qbufs, recs = _pack_ranks(H, q, k, v, lc, ranks)
    for r in range(ranks):
        rows = range(r * lc, (r + 1) * lc)
        ok = A.allowed(rows, L, window, T, sink)
        assert int(ok.sum(dim=1).min()) >= 64                          # (the bound was set at a support of 40)
        got = H.attn_fwd_fp8_chunked(*qbufs[r], recs, lc, L, window=window, sink=sink, frame_tokens=T, q_offset=r * lc).float().cpu()
        want = P.restate(q[:, r * lc:(r + 1) * lc], k[:, :L], v[:, :L], ok).float().to(BF).float()
        rel = float((got - want).norm() / want.norm())
        print(f"L={L} rank {r} of {ranks} window={window} sink={sink} T={T}: rel-RMS vs restatement {rel:.2e}")
        assert torch.isfinite(got).all() and rel <= REL_RMS


# ----------------------------------------------------------------------------- (c) normalisations
def _raw(H, qb, recs, Lq, Lk, left, right, sink, T, off, shift=None, chunk_tiles=None, like=None):
    lib, s = H.load_library(), torch.cuda.current_stream().cuda_stream
    B, Hh = qb[0].shape[0], qb[0].shape[1]
    out = torch.full((B, Lq, Hh, 128), -768.0, device="cuda", dtype=BF)
    rc = lib.flexam_attn_fwd_fp8_window_at(qb[0].data_ptr(), qb[1].data_ptr(), recs.data_ptr(), out.data_ptr(), out.stride(0), out.stride(1), B, Hh, Lq, Lk,
                                           recs.shape[3] if chunk_tiles is None else chunk_tiles, 128, left, right, sink, T, off,
                                           None if shift is None else shift.data_ptr(), s)
    return rc, out


def test_offset_zero_one_length_and_one_chunk_is_the_windowed_launch_byte_for_byte(H):
    L = 600
    q, k, v = _inputs(2, 3, L, 11)
    bufs = H.attn_fp8_pack(q, k, v)
    recs = bufs[2].unsqueeze(0)
    shift = torch.randn(2, 3 * 128, device="cuda")
    for (left, right), sink, T, sh in (((100, 37), 70, 0, None), ((1, 1), 0, 48, None), ((-1, 0), 0, 0, None), ((100, 37), 0, 0, shift), ((-1, -1), 0, 0, None)):
        rc, out = _raw(H, bufs, recs, L, L, left, right, sink, T, 0, sh)
        assert rc == 0, H.load_library().flexam_last_error()
        assert torch.equal(out, H.attn_fwd_fp8(bufs, L, window=(left, right), sink=sink, frame_tokens=T, o_shift=sh,
                                               kv_splits=1 if (left, right) == (-1, -1) else None)), (left, right, sink, T)


def test_a_window_that_clips_no_row_of_the_call_is_the_chunked_launch_byte_for_byte(H):
    """Rank 1 of 600 keys on 2 ranks: rows 320 .. 639 (40 pad rows).  The left side clips iff it clips row 639, the right iff row 320."""
    L, ranks = 600, 2
    lc = P.chunk_rows(L, ranks)
    q, k, v = _inputs(1, 2, ranks * lc, 17)
    qbufs, recs = _pack_ranks(H, q, k, v, lc, ranks)
    lib, s = H.load_library(), torch.cuda.current_stream().cuda_stream
    plain = torch.empty(1, lc, 2, 128, device="cuda", dtype=BF)
    rc = lib.flexam_attn_fwd_fp8_chunked(qbufs[1][0].data_ptr(), qbufs[1][1].data_ptr(), recs.data_ptr(), plain.data_ptr(), plain.stride(0), plain.stride(1),
                                         1, 2, lc, L, lc // 64, 128, 1, 0, None, None, s)
    assert rc == 0, lib.flexam_last_error()
    run = lambda left, right, sink=0, T=0, shift=None: _raw(H, qbufs[1], recs, lc, L, left, right, sink, T, lc, shift)
    for args in ((639, 279), (-1, 279), (639, -1), (3, 2, 600), (3, 2, 700), (1, 0, 0, 320), (0, 0, 0, 1300)):
        rc, out = run(*args)
        assert rc == 0 and torch.equal(out, plain), args
    for args in ((638, 279), (639, 278), (3, 2, 599), (0, 0, 0, 320)):
        rc, out = run(*args)
        assert rc == 0 and not torch.equal(out, plain), args
    # the chunked call takes no output shift: refused where the window would be dropped, served where it acts
    from flexam_amd import abi
    shift = torch.randn(1, 2 * 128, device="cuda")
    rc, _ = run(639, 279, shift=shift)
    assert rc == abi.CONSTANTS["FLEXAM_E_ARG"] and b"o_shift" in lib.flexam_last_error()
    assert run(100, 37, shift=shift)[0] == 0
    with pytest.raises(RuntimeError, match="o_shift goes with a window"):
        H.attn_fwd_fp8_chunked(*qbufs[1], recs, lc, L, o_shift=shift)
    # a window without a left bound drops the sink
    assert torch.equal(run(-1, 0, 70)[1], run(-1, 0)[1]) and not torch.equal(run(100, 0, 70)[1], run(100, 0)[1])
    # the wrapper's defaults make the call it has always made
    assert torch.equal(H.attn_fwd_fp8_chunked(*qbufs[1], recs, lc, L), H.attn_fwd_fp8_chunked(*qbufs[1], recs, lc, L, window=(-1, -1), sink=5, q_offset=lc))


# ----------------------------------------------------------------------------- (d) argument errors
def test_abi_argument_errors(H):
    from flexam_amd import abi
    E_ARG, E_SHAPE = abi.CONSTANTS["FLEXAM_E_ARG"], abi.CONSTANTS["FLEXAM_E_SHAPE"]
    lib, s = H.load_library(), torch.cuda.current_stream().cuda_stream
    q8, qs, kv8 = H.attn_fp8_buffers(1, 2, 64, "cuda")
    recs = torch.stack([kv8, kv8]).contiguous()
    o = torch.empty(1, 64, 2, 128, dtype=BF, device="cuda")

    def call(a=q8.data_ptr(), b=qs.data_ptr(), c=recs.data_ptr(), op=o.data_ptr(), Lq=64, Lk=70, ct=1, hd=128, left=3, right=2, sink=0, T=0, off=64):
        return lib.flexam_attn_fwd_fp8_window_at(a, b, c, op, o.stride(0), o.stride(1), 1, 2, Lq, Lk, ct, hd, left, right, sink, T, off, None, s)
    assert call() == 0
    assert call(off=-1) == E_ARG and b"q_offset" in lib.flexam_last_error()
    assert call(sink=-1) == E_ARG and b"sink" in lib.flexam_last_error()
    assert call(T=-1) == E_ARG and b"frame_tokens" in lib.flexam_last_error()
    for ct in (0, -1):
        assert call(ct=ct) == E_ARG and b"chunk_tiles" in lib.flexam_last_error()
    for kw in (dict(a=None), dict(b=None), dict(c=None), dict(op=None)):
        assert call(**kw) == E_ARG and b"null pointer" in lib.flexam_last_error()
    assert call(a=q8.data_ptr() + 2) == E_ARG and b"misaligned" in lib.flexam_last_error()
    assert call(hd=64) == E_SHAPE and b"head_dim" in lib.flexam_last_error()
    assert call(Lq=0) == E_SHAPE and b"empty problem" in lib.flexam_last_error()
    assert call(Lk=0) == E_SHAPE and b"empty problem" in lib.flexam_last_error()
    # more keys than the chunks hold: the binding knows the number of chunks, the C ABI does not
    with pytest.raises(RuntimeError, match="do not fit 2 chunks of 1 tiles"):
        H.attn_fwd_fp8_chunked(q8, qs, recs, 64, 129, window=(3, 2), q_offset=64)
    with pytest.raises(RuntimeError, match="do not fit"):
        H.attn_fwd_fp8_chunked(q8, qs, recs, 64, 0, window=(3, 2), q_offset=64)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- (e) a strided output
def test_strided_output_leaves_the_rest_of_the_buffer_alone(H):
    """out= a row and column slice of a larger buffer; rank 2 of L = 1111 on 3 ranks: 41 pad rows behind the keys."""
    c = next(c for c in P.CASES if (c.Lk, c.rank, c.window) == (1111, 2, (200, 100)))
    big = torch.full((1, c.lc + 7, 3 * 2 * 128), -768.0, device="cuda", dtype=BF)
    out = big[:, 3:3 + c.lc, 256:512].unflatten(2, (2, 128))
    _run(H, c, out=out)
    torch.cuda.synchronize()
    _check(c.name + ", strided out", out, c.want(), c.empty_rows())
    rest = big.clone()
    rest[:, 3:3 + c.lc, 256:512] = -768.0
    assert bool((rest == -768.0).all())
