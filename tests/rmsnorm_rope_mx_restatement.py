"""A torch (CPU, float64) restatement of flexam_rmsnorm_rope_mx, the fused RMSNorm + RoPE producer of the MXFP8 self-attention's Q and K
operands (rmsnorm_rope_mx_kernel in csrc/attn_fp8.inc), and of the byte layouts of the operand buffers -- the yardstick of
tests/test_attn_fp8_producers_gpu.py.  Written from include/flexam_hip.h and the kernel's comment, not from the kernel body; the e4m3
rounding and the scale rule are those of tests/mxfp8_restatement.py.

  values    y = x rsqrt(mean(x^2) + eps) w over the 3072 channels of a row (eps as the float32 the entry point takes); the pairs
            (2j, 2j + 1) of each 128-channel head rotated by row token_offset + m % tokens_per_batch, column j, of the float32 cos / sin
            tables (taken as given, promoted to float64): even = re c - im s, odd = re s + im c;
  operands  one E8M0 scale per 32 channels (the smallest power of two with amax / scale <= 448, bytes 1 .. 253) and e4m3 codes of
            y / scale; Q rows [B][H][lq_pad][128] with four scale bytes per row, K row r of a 64-key tile with its 16-byte chunk c at
            chunk position c ^ ((r >> 1) & 7) of the record and its scales at REC_KS + 4 r + block; V (written by flexam_attn_fp8_pack)
            transposed, channel d's 16-byte chunk 2 b + h at position (2 b + h) ^ ((d >> 2) & 3), byte e = key 32 b + (e & 3) + 8 (e >> 2)
            + 4 h, one scale per channel and 32-key half tile at REC_VS + 2 d + b.

The admissible set.  The kernel computes in float32 with a reduction order, a hardware rsqrt and FMA contraction that are the compiler's
choice, so its bytes are not determined; its float32 value is, to within delta * mag of y, where mag = |re c| + |im s| (even outputs) and
|re s| + |im c| (odd outputs) is the quantity float32 rounding error scales with.  Count of delta, in units of u = 2^-24 (one rounding
to nearest):
   16   the sum of squares: 24 adds per thread and at most 8 steps of the 128-thread reduction, all terms non-negative (the squares of
        bf16 numbers are exact in float32), so at most 32 u on the sum, halved by the square root;
    3   the division by C and the addition of eps: one rounding each (up to 5 u together should the division not be correctly rounded),
        halved by the square root;
    4   v_rsq_f32, about 2 ulp = 4 u;
    2   the two multiplies x rn w;
    3   the rotation: two products and one subtraction / addition (2 u mag when contracted), relative to mag;
    2   the scale rule's amax * (1 / 448): the rounded constant and the product (scale bytes only)
  = 30 u < 32 u, hence DELTA = 2^-19.
A scale byte is admissible if it is the E8M0 byte of some amax in [max_j(|y_j| - delta mag_j), max_j(|y_j| + delta mag_j)] of its block.
A code is admissible if, under the kernel's own (admissible) scale byte e, it lies between the codes of the smallest and the largest
float32 number in [y - delta mag, y + delta mag] times 2^(127 - e); 0x00 and 0x80 count as one code only where that interval contains
zero.  An element or block is AMBIGUOUS when its set has more than one member (codes: under the nominal scale byte, that of y itself):
the share of ambiguous elements says how much freedom the check leaves, and the tests cap it."""
import functools
import math
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mxfp8_restatement import e4m3_code, mx_quant  # noqa: E402

from flexam_amd import hip  # noqa: E402

HEADS, HD, QBLK, TILE, REC_BYTES = 24, hip.ATTN_HEAD_DIM, hip.ATTN_Q_BLOCK, hip.ATTN_KV_TILE, hip.ATTN8_REC_BYTES
C = HEADS * HD
# a record: [K image][V^T image][K scales, 4 per key][V scales, 2 per channel][unused]
REC_V, REC_KS, REC_VS, REC_END = TILE * HD, 2 * TILE * HD, 2 * TILE * HD + 4 * TILE, 2 * TILE * HD + 4 * TILE + 2 * HD
DELTA = 2.0 ** -19
AMBIGUOUS_CAP = 1e-3
FILL = 0xA5


def lq_pad(L):
    return -(-L // QBLK) * QBLK


def tiles(L):
    return -(-L // TILE)


# ----------------------------------------------------------------------------- values
def reference(x, w, cos, sin, tokens_per_batch, token_offset, eps):
    """x [M, 3072] bf16, w [3072] float32, cos / sin [T, 64] float32 -> float64 y [M, 24, 4, 32] and the per-element magnitude `mag`."""
    xd = x.double().cpu()
    M = xd.shape[0]
    eps = float(torch.tensor(eps, dtype=torch.float32))
    y = xd * torch.rsqrt((xd * xd).mean(dim=-1, keepdim=True) + eps) * w.double().cpu()
    tok = token_offset + torch.arange(M) % tokens_per_batch
    c, s = cos.double().cpu()[tok][:, None, :], sin.double().cpu()[tok][:, None, :]
    re, im = y.view(M, HEADS, HD // 2, 2).unbind(-1)
    out = torch.stack([re * c - im * s, re * s + im * c], dim=-1)
    mag = torch.stack([(re * c).abs() + (im * s).abs(), (re * s).abs() + (im * c).abs()], dim=-1)
    return out.reshape(M, HEADS, 4, 32), mag.reshape(M, HEADS, 4, 32)


def e8m0_byte(amax):
    """float64 amax >= 0 -> the E8M0 byte of the smallest power of two 2^e with amax 2^-e <= 448, as int64, clamped to 1 .. 253 (the
    rule of mxfp8_restatement.mx_quant, without its float32 rounding of amax / 448)."""
    m, ex = torch.frexp(amax.double() / 448.0)                   # amax / 448 = m 2^ex, m in [0.5, 1)
    e = ex.long() + 126 + (m != 0.5).long()
    return torch.where(amax == 0, torch.ones_like(e), e).clamp(1, 253)


def _f32_at_least(x):
    """The smallest float32 >= x (float64), as float32."""
    f = x.float()
    return torch.where(f.double() < x, torch.nextafter(f, torch.full_like(f, math.inf)), f)


def _f32_at_most(x):
    f = x.float()
    return torch.where(f.double() > x, torch.nextafter(f, torch.full_like(f, -math.inf)), f)


def _rank(code):
    """e4m3 codes in the order of their values: +-(code & 127), both zeros 0."""
    c = code.long()
    m = c & 127
    return torch.where((c & 128) != 0, -m, m)


class Admissible:
    """The admissible scale bytes and codes of one operand (q or k) of one call; rows m = b * tokens_per_batch + token."""

    def __init__(self, x, w, cos, sin, tokens_per_batch, token_offset, eps, delta=DELTA):
        self.y, mag = reference(x, w, cos, sin, tokens_per_batch, token_offset, eps)
        self.tol = delta * mag
        a = self.y.abs()
        self.e_lo = e8m0_byte((a - self.tol).amax(dim=-1).clamp(min=0))
        self.e_hi = e8m0_byte((a + self.tol).amax(dim=-1))
        self.e_nom = e8m0_byte(a.amax(dim=-1))
        self.zero_in = (self.y - self.tol <= 0) & (self.y + self.tol >= 0)
        lo, hi = self._code_ranks(self.e_nom)
        self.code_nom = e4m3_code(self.y * torch.pow(2.0, 127.0 - self.e_nom.double()).unsqueeze(-1))
        self.ambiguous_codes = float((lo != hi).double().mean())
        self.ambiguous_scales = float((self.e_lo != self.e_hi).double().mean())

    def _code_ranks(self, e):
        inv = torch.pow(2.0, 127.0 - e.double()).unsqueeze(-1).float()
        lo = _rank(e4m3_code(_f32_at_least(self.y - self.tol) * inv))
        hi = _rank(e4m3_code(_f32_at_most(self.y + self.tol) * inv))
        return lo, hi

    def check(self, codes, scales, name=""):
        """codes uint8 [M, 24, 4, 32], scales uint8 [M, 24, 4] as read back from the operand buffers -> a verdict: the number of
        inadmissible scale bytes and codes, the number of bytes off the nominal ones, and `first`, a sentence naming the first
        violating (row, head, block, byte), or None.  The codes of a block whose scale byte is refused are judged under the nominal one."""
        e = scales.long()
        bad_s = (e < self.e_lo) | (e > self.e_hi)
        lo, hi = self._code_ranks(torch.where(bad_s, self.e_nom, e))
        got = _rank(codes)
        neg = (codes.long() & 128) != 0
        bad_c = (got < lo) | (got > hi) | ((got == 0) & ~self.zero_in & (neg != (self.y < 0)))
        first = None
        if bool(bad_s.any()):
            m, h, b = (int(i) for i in bad_s.nonzero()[0])
            first = (f"{name} scale byte of row {m} head {h} block {b}: got {int(e[m, h, b])}, admissible {int(self.e_lo[m, h, b])} .. "
                     f"{int(self.e_hi[m, h, b])} (block amax {float(self.y[m, h, b].abs().max())!r})")
        elif bool(bad_c.any()):
            m, h, b, j = (int(i) for i in bad_c.nonzero()[0])
            first = (f"{name} code of row {m} head {h} block {b} byte {j}: got 0x{int(codes[m, h, b, j]):02x} under scale byte "
                     f"{int(e[m, h, b])}, admissible ranks {int(lo[m, h, b, j])} .. {int(hi[m, h, b, j])}, nominal 0x{int(self.code_nom[m, h, b, j]):02x} "
                     f"under {int(self.e_nom[m, h, b])} (y {float(self.y[m, h, b, j])!r} +- {float(self.tol[m, h, b, j])!r})")
        return types.SimpleNamespace(bad_scales=int(bad_s.sum()), bad_codes=int(bad_c.sum()), first=first,
                                     off_nominal=int((scales.long() != self.e_nom).sum()) + int((codes != self.code_nom).sum()))


# ----------------------------------------------------------------------------- layouts
def _k_offsets():
    """[64 rows, 128 channels] -> byte of the record's K image: chunk c = ch / 16 of row r at chunk position c ^ ((r >> 1) & 7)."""
    r, ch = torch.arange(TILE)[:, None], torch.arange(HD)[None, :]
    return r * HD + 16 * ((ch >> 4) ^ ((r >> 1) & 7)) + (ch & 15)


def _v_offsets():
    """[64 keys, 128 channels] -> byte of the record's V^T image, from its start."""
    off = torch.empty(TILE, HD, dtype=torch.long)
    d = torch.arange(HD)
    for b in range(2):
        for h in range(2):
            for e in range(16):
                off[32 * b + (e & 3) + 8 * (e >> 2) + 4 * h] = d * TILE + 16 * ((2 * b + h) ^ ((d >> 2) & 3)) + e
    return off


K_OFFSETS, V_OFFSETS = _k_offsets(), _v_offsets()


def _tile_rows(t, L, fill):
    """[B, L, H, ...] -> [B, H, T, 64, ...], rows past L = fill."""
    B, H, T = t.shape[0], t.shape[2], tiles(L)
    out = torch.full((B, T * TILE, H) + tuple(t.shape[3:]), fill, dtype=t.dtype)
    out[:, :L] = t
    return out.movedim(2, 1).reshape((B, H, T, TILE) + tuple(t.shape[3:]))


def q_rows(codes, scales, fill=0):
    """codes uint8 [B, L, H, 4, 32], scales uint8 [B, L, H, 4] -> q8 [B, H, lq_pad, 128], qs bytes [B, H, lq_pad, 4]; rows past L = fill."""
    B, L, H = codes.shape[:3]
    q8 = torch.full((B, H, lq_pad(L), HD), fill, dtype=torch.uint8)
    qs = torch.full((B, H, lq_pad(L), 4), fill, dtype=torch.uint8)
    q8[:, :, :L] = codes.reshape(B, L, H, HD).movedim(2, 1)
    qs[:, :, :L] = scales.movedim(2, 1)
    return q8, qs


def q_rows_inv(q8, qs, L):
    """q8 [B, H, lq_pad, 128], qs (int32 [B, H, lq_pad] or its bytes) -> codes [B, L, H, 4, 32], scales [B, L, H, 4] of the rows below L."""
    B, H = q8.shape[:2]
    qs = qs.view(torch.uint8).reshape(B, H, -1, 4)
    return q8[:, :, :L].movedim(1, 2).reshape(B, L, H, 4, 32), qs[:, :, :L].movedim(1, 2)


def k_record(codes, scales, fill=0, offsets=K_OFFSETS):
    """codes uint8 [B, L, H, 4, 32], scales uint8 [B, L, H, 4] -> K image [B, H, T, 8192], K scales [B, H, T, 256]; rows past L = fill."""
    B, L, H = codes.shape[:3]
    rows = _tile_rows(codes.reshape(B, L, H, HD), L, fill)                      # [B, H, T, 64, 128]
    img = torch.empty(B, H, tiles(L), TILE * HD, dtype=torch.uint8)
    img[..., offsets.flatten()] = rows.reshape(B, H, tiles(L), TILE * HD)
    return img, _tile_rows(scales, L, fill).reshape(B, H, tiles(L), 4 * TILE)


def k_record_inv(kv8, L):
    """records [B, H, T, REC_BYTES] -> codes [B, L, H, 4, 32], scales [B, L, H, 4] of the keys below L."""
    B, H, T = kv8.shape[:3]
    rows = kv8[..., :REC_V][..., K_OFFSETS.flatten()].reshape(B, H, T * TILE, HD)[:, :, :L]
    sc = kv8[..., REC_KS:REC_VS].reshape(B, H, T * TILE, 4)[:, :, :L]
    return rows.movedim(1, 2).reshape(B, L, H, 4, 32), sc.movedim(1, 2)


def v_record(v):
    """v [B, L, H, 128] bf16 -> V^T image [B, H, T, 8192], V scales [B, H, T, 256] as flexam_attn_fp8_pack quantises and lays them out:
    keys past L are zeros, one scale per channel d and half tile b at 2 d + b."""
    B, L, H, _ = v.shape
    T = tiles(L)
    vt = _tile_rows(v.float().cpu(), L, 0.0)                                    # [B, H, T, key, d]
    codes, sc = mx_quant(vt.reshape(B, H, T, 2, 32, HD).transpose(-1, -2))      # [B, H, T, b, d, 32 keys], [B, H, T, b, d]
    codes = codes.transpose(-1, -2).reshape(B, H, T, TILE * HD)                 # [.., key, d] flattened
    img = torch.empty(B, H, T, TILE * HD, dtype=torch.uint8)
    img[..., V_OFFSETS.flatten()] = codes
    return img, sc.transpose(-1, -2).reshape(B, H, T, 2 * HD)


def v_record_inv(kv8):
    """records [B, H, T, REC_BYTES] -> codes [B, H, T, 64 keys, 128 channels], scales [B, H, T, 128 channels, 2 half tiles]."""
    B, H, T = kv8.shape[:3]
    return kv8[..., REC_V:REC_KS][..., V_OFFSETS.flatten()].reshape(B, H, T, TILE, HD), kv8[..., REC_VS:REC_END].reshape(B, H, T, HD, 2)


def records(k_img, k_sc, v_img, v_sc, fill=0):
    """The four parts -> records [B, H, T, REC_BYTES], the unused tail = fill."""
    rec = torch.full(tuple(k_img.shape[:3]) + (REC_BYTES,), fill, dtype=torch.uint8)
    rec[..., :REC_V], rec[..., REC_V:REC_KS], rec[..., REC_KS:REC_VS], rec[..., REC_VS:REC_END] = k_img, v_img, k_sc, v_sc
    return rec


def pack_bytes(q, k, v, tail=0):
    """What flexam_attn_fp8_pack writes for q, k, v [B, L, H, 128] bf16: (q8, qs bytes, records).  Rows past L are zero rows (codes 0,
    scale byte 1) up to lq_pad for Q and to the end of the last tile for K and V; the records' unused tail = `tail` (never written)."""
    B, L, H, _ = v.shape

    def rows(t, n):
        x = torch.zeros(B, n, H, 4, 32)
        x[:, :L] = t.float().cpu().reshape(B, L, H, 4, 32)
        return mx_quant(x)

    return q_rows(*rows(q, lq_pad(L))) + (records(*k_record(*rows(k, tiles(L) * TILE)), *v_record(v), fill=tail),)


def fused_writes(B, L):
    """Masks (q8, qs bytes, records; True = written) of the bytes flexam_rmsnorm_rope_mx writes at this shape: Q rows and K keys below L."""
    ones = torch.ones(B, L, HEADS, 4, 32, dtype=torch.uint8), torch.ones(B, L, HEADS, 4, dtype=torch.uint8)
    k_img, k_sc = k_record(*ones)
    return tuple(t.bool() for t in q_rows(*ones) + (records(k_img, k_sc, torch.zeros_like(k_img), torch.zeros(B, HEADS, tiles(L), 2 * HD)),))


# ----------------------------------------------------------------------------- the cases of the GPU test
# q and k [B * L, 3072] bf16 rows: `qkv` = column views of one [B * L, 9216] buffer (the engine's form), `separate` = buffers of their own
# with row pitches 3072 + 8 and 3072 + 64.  token_offset as given, tokens_per_batch = L.
CASES = {
    "ragged": dict(B=2, L=200, offset=5, form="qkv"),             # lq_pad 256, 4 tiles, the last one 8 rows
    "tile-plus-one": dict(B=1, L=65, offset=0, form="separate"),
    "two-q-blocks": dict(B=1, L=257, offset=3, form="qkv"),       # lq_pad 512, 5 tiles
    "one-token": dict(B=3, L=1, offset=0, form="qkv"),            # tokens_per_batch = 1
}
EPS = 1e-6


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """The inputs of a case (CPU tensors, not to be modified): qkv [M, 9216] bf16 (q | k | v columns), wq, wk [3072], cos, sin
    [L + offset + 1, 64] (one row more than the call reads), drawn as test_fused_rmsnorm_rope_writes_the_same_operands_as_the_two_step_path
    draws them, plus in q and in k: one all-zero row (the last but one), two quiet rows (|x| ~ 1e-3, so eps carries
    weight), one 32-channel block times 37 and one row times 2^7.  The three rows of `one-token` cannot hold all of that twice: there q
    has the zero row and the quiet rows, k the scaled row and the outlier block."""
    c = CASES[name]
    B, L, M = c["B"], c["L"], c["B"] * c["L"]
    g = torch.Generator().manual_seed(21 + 1000 * L + B)
    x = torch.randn(M, 3 * C, generator=g) * 1.5
    wq = torch.rand(C, generator=g) * 0.2 + 0.05
    wk = torch.rand(C, generator=g) + 0.5
    ang = torch.rand(L + c["offset"] + 1, HD // 2, generator=g) * 6.28
    quiet = torch.randn(2, 2 * C, generator=g) * 1e-3
    q, k = x[:, :C], x[:, C:2 * C]
    if M >= 8:
        rows_q = rows_k = dict(zero=M - 2, quiet=(0, M // 2 + 1), block=7, scaled=M // 2)
    else:
        rows_q, rows_k = dict(zero=0, quiet=(1, 2)), dict(block=1, scaled=0)
    for t, rows, col, (head, blk) in ((q, rows_q, 0, (1, 1)), (k, rows_k, C, (HEADS - 1, 3))):
        if "quiet" in rows:
            for i, r in enumerate(rows["quiet"]):
                t[r] = quiet[i, col:col + C]
        if "block" in rows:
            t[rows["block"], head * HD + 32 * blk: head * HD + 32 * blk + 32] *= 37.0
        if "scaled" in rows:
            t[rows["scaled"]] *= 2.0 ** 7
        if "zero" in rows:
            t[rows["zero"]] = 0.0
    return types.SimpleNamespace(name=name, B=B, L=L, M=M, offset=c["offset"], form=c["form"], eps=EPS, qkv=x.to(torch.bfloat16), wq=wq, wk=wk,
                                 cos=ang.cos(), sin=ang.sin(), rows_q=rows_q, rows_k=rows_k)


@functools.lru_cache(maxsize=None)
def case_admissible(name):
    """(Admissible of q, Admissible of k) of a case: computed once, shared by every test that needs it."""
    c = case_inputs(name)
    return tuple(Admissible(c.qkv[:, i * C:(i + 1) * C], w, c.cos, c.sin, c.L, c.offset, c.eps) for i, w in ((0, c.wq), (1, c.wk)))


def check_operands(name, q8, qs, kv8):
    """The operand buffers (CPU) of a case after flexam_rmsnorm_rope_mx -> (verdict of q, verdict of k) over the rows below L."""
    c = case_inputs(name)
    aq, ak = case_admissible(name)
    flat = lambda t: t.reshape((c.M,) + tuple(t.shape[2:]))                     # [B, L, H, ..] -> rows m = b L + token
    qc, qsc = q_rows_inv(q8, qs, c.L)
    kc, ksc = k_record_inv(kv8, c.L)
    return aq.check(flat(qc), flat(qsc), "q"), ak.check(flat(kc), flat(ksc), "k")
