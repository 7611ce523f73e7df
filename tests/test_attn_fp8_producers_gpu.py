"""The producers of the MXFP8 self-attention's operands, byte for byte: flexam_rmsnorm_rope_mx (RMSNorm + RoPE + MX quantisation of q and
k in one pass, the kernel behind every self-attention of the 5B model under SAGE_ATTENTION) against the float64 restatement and the
admissible sets of tests/rmsnorm_rope_mx_restatement.py -- every scale byte and every code of every valid row, at the place the header's
layout formulas put it, and not one byte written anywhere else -- and flexam_attn_fp8_pack in the two forms the DiT engine uses: from
strided views of the [M, 9216] q|k|v buffer, and V only into buffers that already hold Q and K."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rmsnorm_rope_mx_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from flexam_amd import hip
    hip.load_library()
    return hip


def _filled_buffers(H, B, L, fill=R.FILL):
    bufs = H.attn_fp8_buffers(B, R.HEADS, L, "cuda")
    for t in bufs:
        t.view(torch.uint8).fill_(fill)
    return bufs


def _bytes(bufs):
    """(q8, qs bytes [B, H, lq_pad, 4], records) on the CPU."""
    q8, qs, kv8 = (t.cpu() for t in bufs)
    return q8, qs.view(torch.uint8).reshape(tuple(qs.shape) + (4,)), kv8


def _on_gpu(c):
    """The case's q, k [M, 3072] and v [B, L, 24, 128] in the form it names, and its weights and tables."""
    qkv = c.qkv.cuda()
    if c.form == "qkv":                                    # the engine's: column views of one [M, 9216] buffer
        q, k = qkv[:, :R.C], qkv[:, R.C:2 * R.C]
        v = qkv.view(c.B, c.L, 3 * R.C)[:, :, 2 * R.C:].unflatten(2, (R.HEADS, R.HD))
    else:                                                  # buffers of their own, row pitches 3072 + 8 and 3072 + 64
        q = torch.zeros(c.M, R.C + 8, dtype=torch.bfloat16, device="cuda")[:, :R.C]
        k = torch.zeros(c.M, R.C + 64, dtype=torch.bfloat16, device="cuda")[:, :R.C]
        q.copy_(qkv[:, :R.C])
        k.copy_(qkv[:, R.C:2 * R.C])
        v = qkv[:, 2 * R.C:].reshape(c.B, c.L, R.HEADS, R.HD)
    return q, k, v, c.wq.cuda(), c.wk.cuda(), c.cos[:c.L + c.offset].cuda(), c.sin[:c.L + c.offset].cuda()


def _produce(H, c, bufs):
    q, k, v, wq, wk, cos, sin = _on_gpu(c)
    H.rmsnorm_rope_mx(q, wq, k, wk, bufs, cos, sin, c.L, c.offset, eps=c.eps)
    return v


@pytest.mark.parametrize("name", list(R.CASES))
def test_fused_producer_writes_admissible_bytes_in_place_and_nothing_else(H, name):
    """Every scale byte and code of the rows below L admissible (the first violating row, head, block and byte named otherwise), the
    inputs leaving less than 1e-3 of them a choice; the buffers start as 0xA5 everywhere, and whatever the producer has no business
    writing -- Q rows and scales from L on, K rows and scales past L in the last tile, the V image, the V scales, the records' unused
    tail -- is still 0xA5 afterwards.  Then the V-only pack into the same buffers: the V half equals the restated bytes, every Q and K
    byte stays.

    Measured on an MI355X: nothing refused; of the 3168 M bytes of an operand, 3 of q and 3 of k differ from the nominal ones (those of
    y itself) in `ragged`, none in the other cases; ambiguous codes 1.6e-4 .. 2.3e-4 of all, ambiguous scale bytes none."""
    c = R.case_inputs(name)
    for a in R.case_admissible(name):
        assert a.ambiguous_codes <= R.AMBIGUOUS_CAP and a.ambiguous_scales <= R.AMBIGUOUS_CAP
    bufs = _filled_buffers(H, c.B, c.L)
    v = _produce(H, c, bufs)
    after_fused = _bytes(bufs)
    verdicts = R.check_operands(name, *after_fused)
    for which, a, vd in zip("qk", R.case_admissible(name), verdicts):
        print(f"{name} {which}: {vd.off_nominal} bytes off the nominal ones, {vd.bad_scales} scale bytes and {vd.bad_codes} codes refused; "
              f"ambiguous shares: codes {a.ambiguous_codes:.3g}, scale bytes {a.ambiguous_scales:.3g}")
    for vd in verdicts:
        assert vd.bad_scales == 0 and vd.bad_codes == 0, vd.first
    # the all-zero row: scale byte 1, codes zero (of either sign: 0 c - 0 s is -0 where c < 0 < s)
    for (codes, scales), rows in zip((R.q_rows_inv(*after_fused[:2], c.L), R.k_record_inv(after_fused[2], c.L)), (c.rows_q, c.rows_k)):
        if "zero" in rows:
            b, tok = divmod(rows["zero"], c.L)
            assert int(scales[b, tok].min()) == 1 == int(scales[b, tok].max()) and int((codes[b, tok] & 127).max()) == 0
    written = R.fused_writes(c.B, c.L)
    for what, buf, w in zip(("q8", "qs", "kv8"), after_fused, written):
        stray = (buf != R.FILL) & ~w
        assert not bool(stray.any()), f"{what}: {int(stray.sum())} bytes written outside the valid rows, the first at {stray.nonzero()[0].tolist()}"
    assert int(written[0].sum()) == c.M * R.C and int(written[1].sum()) == c.M * R.HEADS * 4 and int(written[2].sum()) == c.M * R.HEADS * 132

    H.attn_fp8_pack(None, None, v, bufs)
    q8, qs, kv8 = _bytes(bufs)
    v_img, v_sc = R.v_record(v.cpu())
    assert torch.equal(kv8[..., R.REC_V:R.REC_KS], v_img) and torch.equal(kv8[..., R.REC_VS:R.REC_END], v_sc)
    assert torch.equal(q8, after_fused[0]) and torch.equal(qs, after_fused[1])
    for lo, hi in ((0, R.REC_V), (R.REC_KS, R.REC_VS), (R.REC_END, R.REC_BYTES)):
        assert torch.equal(kv8[..., lo:hi], after_fused[2][..., lo:hi]), (lo, hi)


def test_pack_from_the_engines_strided_views(H):
    """flexam_attn_fp8_pack as the DiT engine calls it: q, k and v [B, L, 24, 128] views into one [B L, 9216] buffer (batch stride
    9216 L, row stride 9216), two samples, a ragged last tile -- every byte of the three buffers against the restated layouts, the
    zero rows past L included (codes 0, scale byte 1) and the records' unused tail untouched."""
    B, L = 2, 150
    g = torch.Generator().manual_seed(150)
    x = torch.randn(B * L, 3 * R.C, generator=g)
    x[L + 7, R.C + 5 * R.HD + 32: R.C + 5 * R.HD + 64] *= 37.0         # an outlier block of k, second sample
    x[L - 1, :2 * R.C] = 0.0                                           # a zero row of q and k, next to the first sample's padding
    qkv = x.to(torch.bfloat16).cuda()
    q, k, v = (qkv.view(B, L, 3 * R.C)[:, :, i * R.C:(i + 1) * R.C].unflatten(2, (R.HEADS, R.HD)) for i in range(3))
    assert q.stride() == (3 * R.C * L, 3 * R.C, R.HD, 1)
    got = _bytes(H.attn_fp8_pack(q, k, v, _filled_buffers(H, B, L)))
    want = R.pack_bytes(q.cpu(), k.cpu(), v.cpu(), tail=R.FILL)
    for what, a, b in zip(("q8", "qs", "kv8"), got, want):
        assert a.shape == b.shape
        assert torch.equal(a, b), f"{what}: {int((a != b).sum())} bytes differ, the first at {(a != b).nonzero()[0].tolist()}"


@pytest.mark.parametrize("splits", [None, (2, 0)])
def test_attention_is_indifferent_to_the_padding_rows_scale_bytes(H, splits):
    """The two producers disagree on padding rows: the pack kernel writes scale byte 1 for its zero rows, the fused producer leaves
    the buffers' 0.  The attention kernel must not care: on the `ragged` operands, made in zero-initialised buffers, the rows below L
    come out bit-identical with the padding rows' Q scale bytes and the last tile's K scale bytes past L at 0 and at 1."""
    c = R.case_inputs("ragged")
    bufs = H.attn_fp8_buffers(c.B, R.HEADS, c.L, "cuda")
    H.attn_fp8_pack(None, None, _produce(H, c, bufs), bufs)
    kw = {} if splits is None else dict(kv_splits=splits[0], split_from_unit=splits[1])
    qs = bufs[1].view(torch.uint8).view(c.B, R.HEADS, R.lq_pad(c.L), 4)[:, :, c.L:]
    ks = bufs[2][:, :, -1, R.REC_KS + 4 * (c.L % R.TILE):R.REC_VS]
    assert qs.numel() == c.B * R.HEADS * 56 * 4 and ks.numel() == c.B * R.HEADS * 56 * 4 and int(qs.max()) == 0 == int(ks.max())
    left_at_zero = H.attn_fwd_fp8(bufs, c.L, **kw).clone()
    qs.fill_(1)
    ks.fill_(1)
    set_to_one = H.attn_fwd_fp8(bufs, c.L, **kw)
    assert bool(torch.isfinite(left_at_zero.float()).all()) and float(left_at_zero.float().abs().max()) > 0
    assert torch.equal(left_at_zero, set_to_one)


def test_fused_producer_refuses_what_it_cannot_do(H):
    """The wrapper's refusals and the C side's, none of which may launch anything: the buffers stay untouched."""
    c = R.case_inputs("tile-plus-one")
    M, L = c.M, c.L
    q, k, _, wq, wk, cos, sin = _on_gpu(c)
    bufs = _filled_buffers(H, 1, L)

    def c_side(q=q, k=k, bufs=bufs, M=M, heads=R.HEADS, width=R.C, tokens=L):
        H._call("flexam_rmsnorm_rope_mx", H._ptr(q), q.stride(0), H._ptr(wq), H._ptr(k), k.stride(0), H._ptr(wk), *(H._raw(t) for t in bufs),
                M, width, c.eps, H._ptr(cos), H._ptr(sin), tokens, 0, heads, R.HD)

    # heads other than 24: 12 heads of 128 pass the wrapper's own shape check (its buffers are those of 12 heads), not the library's
    bufs12 = H.attn_fp8_buffers(1, 12, L, "cuda")
    with pytest.raises(RuntimeError, match="24 heads of 128"):
        H.rmsnorm_rope_mx(q[:, :12 * R.HD], wq, k[:, :12 * R.HD], wk, bufs12, cos, sin, L, heads=12)
    with pytest.raises(RuntimeError, match="do not tile"):
        H.rmsnorm_rope_mx(q, wq, k, wk, bufs, cos, sin, L, heads=12)
    with pytest.raises(RuntimeError, match="24 heads of 128"):
        c_side(heads=12, width=12 * R.HD)
    with pytest.raises(RuntimeError, match="24 heads of 128"):
        c_side(heads=12)
    # rows that do not tile the batches
    with pytest.raises(RuntimeError, match="do not tile"):
        H.rmsnorm_rope_mx(q, wq, k, wk, bufs, cos, sin, 7)
    with pytest.raises(RuntimeError, match="bad sizes"):
        c_side(tokens=7)
    # a row pitch that is not a multiple of 8 elements (16 bytes), of q and of k
    odd = torch.zeros(M, R.C + 4, dtype=torch.bfloat16, device="cuda")[:, :R.C]
    with pytest.raises(RuntimeError, match="bad sizes"):
        H.rmsnorm_rope_mx(odd, wq, k, wk, bufs, cos, sin, L)
    with pytest.raises(RuntimeError, match="bad sizes"):
        H.rmsnorm_rope_mx(q, wq, odd, wk, bufs, cos, sin, L)
    # buffers of another (B, L): the byte images cannot be size-checked by the library, so the wrapper must
    for B2, L2 in ((1, L - 1), (2, L), (1, 300)):
        with pytest.raises(RuntimeError, match="operand buffers are not attn_fp8_buffers"):
            H.rmsnorm_rope_mx(q, wq, k, wk, H.attn_fp8_buffers(B2, R.HEADS, L2, "cuda"), cos, sin, L)
    with pytest.raises(RuntimeError, match="operand buffers are not attn_fp8_buffers"):
        H.attn_fp8_pack(None, None, torch.zeros(1, L, R.HEADS, R.HD, dtype=torch.bfloat16, device="cuda"), H.attn_fp8_buffers(1, R.HEADS, L + 64, "cuda"))
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == R.FILL).all()) for t in bufs) and all(int(t.view(torch.uint8).max()) == 0 for t in bufs12)
