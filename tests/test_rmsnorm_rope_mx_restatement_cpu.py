"""CPU: the restatement of flexam_rmsnorm_rope_mx and of the MXFP8 operand layouts (tests/rmsnorm_rope_mx_restatement.py) that
tests/test_attn_fp8_producers_gpu.py holds the kernels to.  A plain float32 torch emulation of the kernel's documented arithmetic must
pass its checker on every GPU case's inputs; the inputs themselves must leave the checker little freedom (the ambiguous shares); and
the emulation with one planted fault -- of the arithmetic or of the store pattern -- must be refused, each of them."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rmsnorm_rope_mx_restatement as R  # noqa: E402
from mxfp8_restatement import mx_quant  # noqa: E402

ARITHMETIC_FAULTS = ["offset+1", "sin-sign", "pair-swapped", "amax-8", "amax-16", "no-eps"]
LAYOUT_FAULTS = ["k-swizzle-dropped-on-odd-row-pairs", "k-chunk-halves-exchanged", "q-pitch-L", "k-scales-in-wrong-tile"]


def emulate(x, w, cos, sin, tokens_per_batch, token_offset, eps, fault=None):
    """The kernel's documented arithmetic in plain float32 torch: x [M, 3072] bf16 -> codes [M, 24, 4, 32], scale bytes [M, 24, 4]."""
    xf = x.float()
    M = xf.shape[0]
    ms = (xf * xf).sum(dim=-1, keepdim=True) / float(R.C)
    rn = torch.rsqrt(ms if fault == "no-eps" else ms + torch.tensor(eps, dtype=torch.float32))
    y = xf * rn * w
    tok = token_offset + (fault == "offset+1") + torch.arange(M) % tokens_per_batch
    c, s = cos[tok][:, None, :], sin[tok][:, None, :]
    if fault == "sin-sign":
        s = -s
    re, im = y.view(M, R.HEADS, R.HD // 2, 2).unbind(-1)
    even, odd = re * c - im * s, re * s + im * c
    if fault == "pair-swapped":
        even, odd = odd, even
    y = torch.stack([even, odd], dim=-1).reshape(M, R.HEADS, 4, 32)
    if fault in ("amax-8", "amax-16"):          # the block maximum taken over a lane's own 8 channels / two lanes' 16: every group is
        n = int(fault[5:])                      # quantised under its own scale, the first group's byte is the one stored
        codes, scales = mx_quant(y.reshape(M, R.HEADS, 4, 32 // n, n))
        return codes.reshape(M, R.HEADS, 4, 32), scales[..., 0]
    return mx_quant(y)


def write_operands(c, q, k, fault=None):
    """(codes, scales) of q and k, rows m = b L + token -> the operand buffers (q8, qs bytes, records) of case c, everything the
    producer does not write = R.FILL."""
    B, L, H = c.B, c.L, R.HEADS
    (qc, qsc), (kc, ksc) = ((t.reshape((B, L) + tuple(t.shape[1:])) for t in pair) for pair in (q, k))
    q8, qs = R.q_rows(qc, qsc, fill=R.FILL)
    if fault == "q-pitch-L":                    # row (b H + h) L + token instead of (b H + h) lq_pad + token
        q8, qs = torch.full_like(q8, R.FILL), torch.full_like(qs, R.FILL)
        q8.view(-1, R.HD)[:B * H * L] = qc.reshape(B, L, H, R.HD).movedim(2, 1).reshape(-1, R.HD)
        qs.view(-1, 4)[:B * H * L] = qsc.movedim(2, 1).reshape(-1, 4)
    offsets = R.K_OFFSETS
    if fault == "k-swizzle-dropped-on-odd-row-pairs":
        r, ch = torch.arange(R.TILE)[:, None], torch.arange(R.HD)[None, :]
        offsets = torch.where(((r >> 1) & 1) == 1, r * R.HD + ch, offsets)
    if fault == "k-chunk-halves-exchanged":
        offsets = offsets ^ 8
    k_img, k_sc = R.k_record(kc, ksc, fill=R.FILL, offsets=offsets)
    if fault == "k-scales-in-wrong-tile":
        k_sc = k_sc.roll(1, dims=2)
    filler = torch.full_like(k_img, R.FILL)
    return q8, qs, R.records(k_img, k_sc, filler, filler[..., :2 * R.HD], fill=R.FILL)


def _emulated(c, fault=None):
    f = fault if fault in ARITHMETIC_FAULTS else None
    return tuple(emulate(c.qkv[:, i * R.C:(i + 1) * R.C], w, c.cos, c.sin, c.L, c.offset, c.eps, f) for i, w in ((0, c.wq), (1, c.wk)))


def test_scale_rule_equals_the_pack_kernels():
    """e8m0_byte (float64) against the rule of mxfp8_restatement.mx_quant at float32 numbers: powers of two times 448, their
    neighbours, zero (byte 1, the lower clamp), random magnitudes and the largest ones (the upper clamp is out of float32's reach)."""
    p = 448.0 * torch.pow(2.0, torch.arange(-140.0, 120.0))
    a = torch.cat([p, torch.nextafter(p.float(), torch.tensor(0.0)).double(), torch.nextafter(p.float(), torch.tensor(1e38)).double(),
                   torch.rand(4096, generator=torch.Generator().manual_seed(0)).double() * 100, torch.tensor([0.0, 3e38])]).float()
    want = mx_quant(a[:, None])[1].long()
    assert torch.equal(R.e8m0_byte(a.double()), want), a[R.e8m0_byte(a.double()) != want][:8]
    assert int(want.min()) == 1 and int(want[-2]) == 1 and int(want[-1]) == 247


def test_layout_builders_spell_the_headers_formulas_and_invert():
    g = torch.Generator().manual_seed(3)
    B, L, H = 2, 70, 3
    codes = torch.randint(0, 256, (B, L, H, 4, 32), generator=g).to(torch.uint8)
    scales = torch.randint(0, 256, (B, L, H, 4), generator=g).to(torch.uint8)
    q8, qs = R.q_rows(codes, scales, fill=7)
    assert q8.shape == (B, H, 256, 128) and qs.shape == (B, H, 256, 4) and int(q8[:, :, L:].min()) == 7 == int(qs[:, :, L:].max())
    k_img, k_sc = R.k_record(codes, scales, fill=7)
    assert k_img.shape == (B, H, 2, 8192) and k_sc.shape == (B, H, 2, 256)
    for b, tok, h, ch in ((0, 0, 0, 0), (1, 69, 2, 127), (0, 37, 1, 40), (1, 64, 0, 8), (0, 3, 2, 95), (1, 6, 1, 16)):
        t, r = tok // 64, tok % 64
        assert q8[b, h, tok, ch] == codes[b, tok, h, ch // 32, ch % 32] and qs[b, h, tok, ch // 32] == scales[b, tok, h, ch // 32]
        assert k_img[b, h, t, r * 128 + 16 * ((ch // 16) ^ ((r >> 1) & 7)) + ch % 16] == codes[b, tok, h, ch // 32, ch % 32]
        assert k_sc[b, h, t, 4 * r + ch // 32] == scales[b, tok, h, ch // 32]
    assert int(k_img[:, :, 1].reshape(B, H, 64, 128)[:, :, 6:].min()) == 7       # keys 70 .. 127: every byte of their rows
    rec = R.records(k_img, k_sc, torch.zeros_like(k_img), torch.zeros(B, H, 2, 256), fill=9)
    assert rec.shape[-1] == R.REC_BYTES == 18432 and (R.REC_V, R.REC_KS, R.REC_VS, R.REC_END) == (8192, 16384, 16640, 16896)
    assert int(rec[..., R.REC_END:].min()) == 9
    for got, want in zip(R.q_rows_inv(q8, qs, L) + R.k_record_inv(rec, L), (codes, scales, codes, scales)):
        assert torch.equal(got, want)
    # V: byte e of the chunk (2 b + h) of channel d, at chunk position (2 b + h) ^ ((d >> 2) & 3), is key 32 b + (e & 3) + 8 (e >> 2) + 4 h
    v = torch.randn(B, L, H, 128, generator=g).to(torch.bfloat16)
    v_img, v_sc = R.v_record(v)
    vt = torch.zeros(B, H, 128, 128)
    vt[:, :, :L] = v.float().permute(0, 2, 1, 3)
    vt = vt.reshape(B, H, 2, 64, 128)
    for d, b, h in ((0, 0, 0), (5, 1, 0), (127, 1, 1), (66, 0, 1)):
        keys = [32 * b + (e & 3) + 8 * (e >> 2) + 4 * h for e in range(16)]
        wv, sv = mx_quant(vt[:, :, :, 32 * b:32 * b + 32, d])
        pos = (2 * b + h) ^ ((d >> 2) & 3)
        assert torch.equal(v_img[..., d * 64 + 16 * pos: d * 64 + 16 * pos + 16], wv[..., [kk - 32 * b for kk in keys]]), (d, b, h)
        assert torch.equal(v_sc[..., 2 * d + b], sv)
    vc, vs = R.v_record_inv(R.records(k_img, k_sc, v_img, v_sc))
    assert torch.equal(vs.reshape(B, H, 2, 256), v_sc) and torch.equal(vc[0, 1, 1, 5], mx_quant(vt[0, 1, 1, :32].t())[0][:, 5])


@pytest.mark.parametrize("name", list(R.CASES))
def test_inputs_leave_the_checker_little_freedom(name):
    """The condition under which the byte check is worth its name: at most 1e-3 of the codes and of the scale bytes of a case's inputs
    have more than one admissible value.  Every case holds the rows the issue asks for."""
    c = R.case_inputs(name)
    for a, which in zip(R.case_admissible(name), "qk"):
        print(f"{name} {which}: ambiguous codes {a.ambiguous_codes:.3g}, ambiguous scale bytes {a.ambiguous_scales:.3g}")
        assert a.ambiguous_codes <= R.AMBIGUOUS_CAP and a.ambiguous_scales <= R.AMBIGUOUS_CAP
    rows = {**c.rows_k, **c.rows_q}
    assert set(rows) == {"zero", "quiet", "block", "scaled"}
    q, k = c.qkv[:, :R.C].float(), c.qkv[:, R.C:2 * R.C].float()
    assert float(q[c.rows_q["zero"]].abs().max()) == 0 and all(3e-4 < float(q[r].square().mean().sqrt()) < 3e-3 for r in c.rows_q["quiet"])
    assert float(k[c.rows_k["scaled"]].abs().max()) > 2.0 ** 7 and float(k[c.rows_k["block"], -32:].abs().max()) > 37.0


@pytest.mark.parametrize("name", list(R.CASES))
def test_float32_emulation_is_admissible_everywhere(name):
    c = R.case_inputs(name)
    q, k = _emulated(c)
    bufs = write_operands(c, q, k)
    for v in R.check_operands(name, *bufs):
        print(name, "bytes off the nominal ones:", v.off_nominal)
        assert v.bad_scales == 0 and v.bad_codes == 0, v.first
    zq, zk = c.rows_q.get("zero"), c.rows_k.get("zero")
    assert int(q[1][zq].max()) == 1 and int((q[0][zq] & 127).max()) == 0          # the all-zero row: scale byte 1, codes 0
    assert zk is None or (int(k[1][zk].max()) == 1 and int((k[0][zk] & 127).max()) == 0)
    written = R.fused_writes(c.B, c.L)
    for buf, w in zip(bufs, written):
        assert bool((buf[~w] == R.FILL).all())


@pytest.mark.parametrize("fault", ARITHMETIC_FAULTS + LAYOUT_FAULTS)
@pytest.mark.parametrize("name", ["tile-plus-one", "ragged"])
def test_planted_faults_are_refused(name, fault):
    """On one sample of two tiles and on two samples of four with a token offset (the other two cases have a single key row 0 per tile
    or five faultless tiles more: nothing these do not show)."""
    c = R.case_inputs(name)
    q, k = _emulated(c, fault)
    vq, vk = R.check_operands(name, *write_operands(c, q, k, fault))
    print(name, fault, "q:", vq.bad_scales, vq.bad_codes, "k:", vk.bad_scales, vk.bad_codes, "|", vq.first or vk.first)
    if fault.startswith("k-"):
        assert vq.first is None and vk.first is not None
    elif fault.startswith("q-"):
        assert vk.first is None and vq.first is not None
    else:
        assert vq.first is not None and vk.first is not None
    if fault == "no-eps" and name == "tile-plus-one":       # visible on the quiet rows and the zero row only
        bad = {int(m) for a, (codes, scales) in zip(R.case_admissible(name), (q, k))
               for m in ((scales.long() < a.e_lo) | (scales.long() > a.e_hi)).nonzero()[:, 0]}
        assert bad <= set(c.rows_q["quiet"]) | {c.rows_q["zero"]}
