"""GPU: windowed self-attention at a query offset -- the call a rank makes under sequence parallelism: Lq rows that are the global tokens
q_offset .. q_offset + Lq - 1 against the first Lk tokens as keys, pad rows included -- in the HIP kernel (attn_window_at_kernel of
csrc/attn.hip, flexam_attn_fwd_window_at, hip.attn_fwd_window(..., q_offset=)).

Exact cases (tests/attn_window_at_cases.py; tests/test_attn_window_at_cases_cpu.py proves that one key too many or too few at either end
of any row's range moves that row by more than 8 bf16 ulps, and that the mask taken at the row's index in the call instead of its global
token moves a row of every case with an offset by as much): every rank of every split, both forms of the kernel (scale in kernel with
softmax_scale = log 2; pre-scaled q), every element within ONE bf16 ulp of the float64 masked attention of the full sequence; rows that
see no key exactly zero.  Then the byte-for-byte identities of the entry point's normalisations, a strided output, random data against
fp32 masked attention at the bound the sibling tests apply (2 bf16 ulps + 6e-3) and the C ABI's errors.  The rows of a rank's call are
held to the reference and to nothing else: different unit boundaries change the fp32 order, so no bit-equality across ranks is claimed.

Measured on an MI355X (recorded, not asserted; correct rounding gives at most 0.5): max |err| / ulp over the 51 calls 0.499, both forms
alike, no element more than 1 ulp off, every empty row exactly zero; strided output 0.456.  Random data: max |err| 7.0e-4 to 9.1e-4 over
the three ranks and both forms."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_at_cases as A  # noqa: E402
import attn_window_frames_cases as F  # noqa: E402
from test_attn_window_gpu import _assert_bf16_close, _check, _dev  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LN2 = math.log(2.0)


@pytest.fixture(scope="module")
def H():
    from flexam_amd import hip
    hip.load_library()
    return hip


def _kw(prescaled):
    return dict(softmax_scale=None if prescaled else LN2, prescaled=prescaled)


FORMS = pytest.mark.parametrize("prescaled", [False, True], ids=["scale-in-kernel", "prescaled"])


def _run(H, case, prescaled, **kw):
    return H.attn_fwd_window(*_dev(*case.inputs()), case.window, sink=case.sink, frame_tokens=case.T, q_offset=case.q_offset, **_kw(prescaled), **kw)


@FORMS
@pytest.mark.parametrize("case", A.CASES, ids=A.ids(A.CASES))
def test_exact_cases(H, case, prescaled):
    got = _run(H, case, prescaled)
    torch.cuda.synchronize()
    assert got.shape == (case.B, case.Lq, case.H, 128)
    _check(f"{case.name} [{'prescaled' if prescaled else 'scale in kernel'}]", got, case.want())
    empty = case.empty_rows()
    assert bool((got[:, empty.cuda()] == 0).all()), "a row that sees no key is zeros"


@FORMS
def test_offset_zero_and_one_length_is_the_sibling_entry_point_byte_for_byte(H, prescaled):
    q, k, v = _dev(*F.build(600, 2, 3))
    kw = _kw(prescaled)
    for window, T, sink in (((100, 37), 0, 0), ((100, 37), 0, 70), ((-1, 0), 0, 0), ((1, 0), 100, 70), ((1, 1), 48, 0)):
        old = H.attn_fwd_window(q, k, v, window, sink=sink, frame_tokens=T, **kw)
        assert torch.equal(H.attn_fwd_window(q, k, v, window, sink=sink, frame_tokens=T, q_offset=0, **kw), old), (window, T, sink)
        # ... and through the new entry point itself, which hip.attn_fwd_window does not call at offset 0 and one length
        out = torch.empty_like(old)
        from flexam_amd.hip import _call, _ptr, _softmax_scale
        _call("flexam_attn_fwd_window_at", _ptr(q, BF), q.stride(0), q.stride(1), _ptr(k, BF), k.stride(0), k.stride(1), _ptr(v, BF), v.stride(0),
              v.stride(1), _ptr(out, BF), out.stride(0), out.stride(1), 2, 3, 600, 600, 128, _softmax_scale(kw["softmax_scale"], prescaled, 128),
              *H.attn_window(window), T, sink, 0)
        assert torch.equal(out, old), (window, T, sink)


@FORMS
def test_a_window_that_clips_no_row_of_the_call_is_attn_fwd_byte_for_byte(H, prescaled):
    """Rows 278 .. 555 of 1111 keys: a side clips a row of THIS call or it does not, whatever it does to rows of other ranks."""
    qa, k, v = _dev(*F.build(1111, 1, 2))
    q = qa[:, 278:556]
    kw = _kw(prescaled)
    plain = H.attn_fwd(q, k, v, kv_splits=1, **kw)
    run = lambda window, T=0, sink=0, off=278: H.attn_fwd_window(q, k, v, window, sink=sink, frame_tokens=T, q_offset=off, **kw)
    for window, T, sink in (((-1, -1), 0, 0), ((555, 832), 0, 0), ((555, -1), 0, 70), ((-1, 832), 0, 0), ((5000, 5000), 0, 70), ((1, 2), 278, 0),
                            ((0, 0), 2000, 0), ((100, 37), 0, 1111), ((1, 1), 37, 5000)):
        assert torch.equal(run(window, T, sink), plain), (window, T, sink)
    # one key of one row masked on either side: the windowed kernel ran
    assert not torch.equal(run((554, 832)), plain) and not torch.equal(run((555, 831)), plain)
    # at offset 0 the same rows clip nothing under a window that clipped them at 278
    assert torch.equal(run((277, 1110), off=0), H.attn_fwd(q, k, v, kv_splits=1, **kw))
    assert not torch.equal(run((277, 1110)), plain)


def test_strided_output_leaves_the_rest_of_the_buffer_alone(H):
    """out= a row and column slice of a larger buffer; case 6 (frames of 37, sink 300), rank 3: a ragged last block that ends in a pad row."""
    case = next(c for c in A.CASES if c.T == 37 and c.rank == 3)
    assert (case.Lk, case.sink, case.Lq, case.q_offset + case.Lq) == (1111, 300, 278, 1112)
    big = torch.full((1, case.Lq + 7, 3 * 2 * 128), -768.0, device="cuda", dtype=BF)
    out = big[:, 3:3 + case.Lq, 256:512].unflatten(2, (2, 128))
    _run(H, case, True, out=out)
    torch.cuda.synchronize()
    _check("frames of 37, sink 300, rank 3 of 4, strided out", out, case.want())
    rest = big.clone()
    rest[:, 3:3 + case.Lq, 256:512] = -768.0
    assert bool((rest == -768.0).all())


def _masked_fp32(q, k, v, ok, scale=None):
    """fp32 masked attention [B, Lq, H, 128] of bf16 inputs, natural softmax with scale (default 1 / sqrt(128)); every row sees a key."""
    q, k, v = (t.float().transpose(1, 2) for t in (q, k, v))
    s = q @ k.transpose(-1, -2) * (128 ** -0.5 if scale is None else scale)
    s = s.masked_fill(~ok.to(s.device), float("-inf"))
    return (s.softmax(-1) @ v).transpose(1, 2)


@pytest.fixture(scope="module")
def random_case():
    g = torch.Generator().manual_seed(1500)
    return tuple(torch.randn(1, 1500, 2, 128, generator=g).to(BF) for _ in range(3))


@FORMS
@pytest.mark.parametrize("rank", [0, 1, 2])
def test_random_data_against_fp32_masked_attention(H, random_case, rank, prescaled):
    """Lk = 1500 over three ranks, frames of 448 tokens (the last one ragged), one frame either side, the leading frame always visible;
    N(0, 1) data."""
    q, k, v = random_case
    rows = range(rank * 500, rank * 500 + 500)
    ok = A.allowed(rows, 1500, (1, 1), 448, 448)
    q = q[:, rows.start:rows.stop]
    kw = dict(sink=448, frame_tokens=448, q_offset=rows.start)
    if prescaled:
        qs = (q.float() * (128 ** -0.5 * 1.4426950408889634)).to(BF)
        want = _masked_fp32(qs, k, v, ok, scale=0.6931471805599453)          # of the q the kernel was given
        got = H.attn_fwd_window(qs.cuda(), k.cuda(), v.cuda(), (1, 1), prescaled=True, **kw)
    else:
        want = _masked_fp32(q, k, v, ok)
        got = H.attn_fwd_window(q.cuda(), k.cuda(), v.cuda(), (1, 1), **kw)
    _assert_bf16_close(got, want, 2.0, 6e-3, f"attention windowed in frames with a sink at offset {rows.start}, random data")


def test_unequal_lengths_without_an_offset_are_still_refused(H):
    q = torch.zeros(1, 64, 2, 128, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError, match="share one length"):
        H.attn_fwd_window(q, q[:, :32], q[:, :32], (1, 1))


# ----------------------------------------------------------------------------- the C ABI
def test_abi_argument_errors(H):
    from flexam_amd import abi
    E_ARG, E_SHAPE = abi.CONSTANTS["FLEXAM_E_ARG"], abi.CONSTANTS["FLEXAM_E_SHAPE"]
    lib = H.load_library()
    q = torch.zeros(1, 64, 2, 128, dtype=BF, device="cuda")
    o = torch.empty_like(q)
    s = torch.cuda.current_stream().cuda_stream

    def new(qp, kp, vp, op, Lq=32, Lk=64, hd=128, T=7, sink=5, off=16):
        return lib.flexam_attn_fwd_window_at(qp, 64 * 256, 256, kp, 64 * 256, 256, vp, 64 * 256, 256, op, 64 * 256, 256, 1, 2, Lq, Lk, hd, 0.1, 3, 2, T, sink, off, s)

    def old(qp, kp, vp, op, L=64, hd=128):
        return lib.flexam_attn_fwd_window_sink(qp, 64 * 256, 256, kp, 64 * 256, 256, vp, 64 * 256, 256, op, 64 * 256, 256, 1, 2, L, hd, 0.1, 3, 2, 5, s)

    def both(*args, **kw):
        """(status, message) of the new entry point, held to its sibling's."""
        a = (old(*args, **kw), lib.flexam_last_error())
        b = (new(*args, **kw), lib.flexam_last_error())
        assert a == b, (a, b)
        return b
    p = q.data_ptr()
    assert new(p, p, p, o.data_ptr()) == 0 and new(p, p, p, o.data_ptr(), sink=0) == 0 and new(p, p, p, o.data_ptr(), sink=1000) == 0
    assert new(p, p, p, o.data_ptr(), T=0) == 0 and new(p, p, p, o.data_ptr(), T=64) == 0 and new(p, p, p, o.data_ptr(), T=1 << 30) == 0
    assert new(p, p, p, o.data_ptr(), off=0) == 0 and new(p, p, p, o.data_ptr(), off=40) == 0 and new(p, p, p, o.data_ptr(), off=1000) == 0
    assert new(p, p, p, o.data_ptr(), Lq=64, Lk=32, off=0) == 0
    for off in (-1, -278):
        assert new(p, p, p, o.data_ptr(), off=off) == E_ARG and b"q_offset" in lib.flexam_last_error()
    assert new(p, p, p, o.data_ptr(), T=-1) == E_ARG and b"frame_tokens" in lib.flexam_last_error()
    for sink in (-1, -448):
        assert new(p, p, p, o.data_ptr(), sink=sink) == E_ARG and b"sink" in lib.flexam_last_error()
    assert new(p, p, p, o.data_ptr(), off=1 << 30) == E_SHAPE and b"q_offset" in lib.flexam_last_error()
    for Lq, Lk in ((0, 64), (32, 0), (-1, 64)):
        assert new(p, p, p, o.data_ptr(), Lq=Lq, Lk=Lk) == E_SHAPE and b"empty problem" in lib.flexam_last_error()
    for args in ((None, p, p, o.data_ptr()), (p, None, p, o.data_ptr()), (p, p, None, o.data_ptr()), (p, p, p, None)):
        st, msg = both(*args)
        assert st == E_ARG and b"null pointer" in msg
    st, msg = both(p, p, p, o.data_ptr(), hd=64)
    assert st == E_SHAPE and b"head_dim" in msg
    st, msg = both(p + 2, p, p, o.data_ptr())
    assert st == E_ARG and b"misaligned" in msg
    with pytest.raises(RuntimeError, match="q_offset"):
        H.attn_fwd_window(q[:, :32], q, q, (1, 1), q_offset=-3)
    with pytest.raises(RuntimeError, match="sink"):
        H.attn_fwd_window(q[:, :32], q, q, (1, 1), sink=-1, q_offset=16)
    torch.cuda.synchronize()
