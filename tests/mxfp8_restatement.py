"""A torch (CPU, float64) restatement of the MXFP8 self-attention in csrc/attn_fp8.inc, the yardstick of
tests/test_attn_fp8_restated_gpu.py, and of the e4m3 rounding every fp8 kernel here applies (v_cvt_pk_fp8_f32).

It restates the arithmetic the kernel's header documents, independently of the kernel:
  operands  Q and K: e4m3 values with one E8M0 scale per 32 channels of a row; V: one scale per channel and 32-key half tile (the
            MX block of the P.V product); zero rows past L (what flexam_attn_fp8_pack writes);
  scores    float64 dot products of the dequantised rows, in exp2 units (q carries softmax_scale * log2 e);
  walk      per query row, over the half tiles of a key range in order: ref0 = floor(max of the first half tile's VALID keys) - 6;
            a half tile whose maximum exceeds ref + 8.5 moves the reference by delta = floor(max - ref - 6), capped so that
            rd = ref - ref0 <= 96, then clamps its scores to ref + 8.5 (bites at the cap only); the row sum l is multiplied by
            2^-delta on a move; p = exp2(s - ref) as a float32 value; l adds the unrounded p, O adds e4m3(p) * 2^rd * v, so O stays
            in the units of ref0; keys past Lk contribute nothing;
  ranges    the split plan of the call: tiles_per_split = ceil(tiles / S), units (b H + h) ceil(Lq / 256) + q_block before
            split_from_unit take all keys in one range; a split unit's partials (O 2^-rd, ref, l) are merged with weights
            2^(ref_s - max ref), as attn_merge_kernel does (here in float64);
  output    O 2^-rd / l (float64; the caller rounds it to bf16).
With `quant=False` the operands are taken as given and P is not rounded (nor made float32): the walk is then exact softmax attention.
Only the query rows asked for are evaluated (vectorised over rows, a loop over half tiles), so production shapes stay cheap."""
import math

import torch

QBLK, KVBLK, HALF = 256, 64, 32
REF_HEAD, RESCALE_THR, RD_MAX = 6.0, 8.5, 96.0


# ----------------------------------------------------------------------------- e4m3 (OCP float8_e4m3fn)
def e4m3_table():
    """float64 values of the non-negative finite codes 0..126 (code 127 is NaN): subnormals m 2^-9, normals (1 + m/8) 2^(e-7)."""
    c = torch.arange(127)
    e, m = c >> 3, (c & 7).double()
    return torch.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * torch.pow(2.0, (e - 7).double()))


_T = e4m3_table()


def e4m3_code(x):
    """float32 values -> uint8 e4m3 codes: round to nearest, ties to the even code, subnormals kept, magnitudes above 464 -> NaN (0x7F),
    the sign bit of x carried (also onto zero).  The rule v_cvt_pk_fp8_f32 applies in the kernels and torch's float8_e4m3fn cast
    applies (tests/test_mxfp8_restatement_cpu.py pins the two against each other; the GPU tests pin the hardware to it)."""
    x = x.float().double()
    a = x.abs()
    lo = (torch.searchsorted(_T, a, right=True) - 1).clamp(0, 126)
    hi = (lo + 1).clamp(max=126)
    mid = (_T[lo] + _T[hi]) / 2
    up = (a > mid) | ((a == mid) & (hi % 2 == 0) & (hi != lo))
    code = torch.where(up, hi, lo)
    code = torch.where(a > 464.0, torch.full_like(code, 127), code)
    code = torch.where(torch.isnan(a), torch.full_like(code, 127), code)
    return (code | (torch.signbit(x).long() << 7)).to(torch.uint8)


def e4m3_value(codes):
    """uint8 e4m3 codes -> float64 values (NaN for 0x7F / 0xFF)."""
    c = codes.long()
    v = torch.cat([_T, torch.tensor([math.nan], dtype=torch.float64)])[c & 127]
    return torch.where((c & 128) != 0, -v, v)


def e4m3(x):
    """float32 values rounded to e4m3, as float64."""
    return e4m3_value(e4m3_code(x))


# ----------------------------------------------------------------------------- MX operands
def mx_quant(x32):
    """OCP MX block quantisation as the pack kernel does it: x32 [..., 32] fp32 -> (e4m3 bytes [..., 32] uint8, E8M0 byte [...] uint8),
    scale = the smallest power of two with amax / scale <= 448."""
    amax = x32.abs().amax(dim=-1)
    t = (amax / 448.0).float()
    bits = t.view(torch.int32)
    e = ((bits >> 23) & 255) + ((bits & 0x7FFFFF) != 0).int()
    e = e.clamp(1, 253)
    inv = ((254 - e) << 23).view(torch.float32)
    q = (x32 * inv.unsqueeze(-1)).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, e.to(torch.uint8)


def mx_dequant(q, e):
    return e4m3_value(q) * torch.pow(2.0, e.double() - 127.0).unsqueeze(-1)


def _pad_keys(x, n):
    """[B, L, H, 128] -> float32 [B, H, n, 128] with zero rows past L."""
    B, L, H, D = x.shape
    out = torch.zeros(B, H, n, D)
    out[:, :, :L] = x.float().cpu().permute(0, 2, 1, 3)
    return out


def dequant_rows(x):
    """q or k [B, L, H, 128] bf16 -> float64 [B, H, L, 128]: e4m3 with one E8M0 scale per 32 channels of a row."""
    B, L, H, D = x.shape
    xf = _pad_keys(x, L).reshape(B, H, L, 4, 32)
    return mx_dequant(*mx_quant(xf)).reshape(B, H, L, D)


def dequant_v(v):
    """v [B, L, H, 128] bf16 -> float64 [B, H, L, 128]: e4m3 with one scale per channel and 32-key half tile (zero keys past L)."""
    B, L, H, D = v.shape
    n = -(-L // KVBLK) * KVBLK
    vf = _pad_keys(v, n).reshape(B, H, n // HALF, HALF, D).transpose(-1, -2)        # [B, H, half tile, d, 32 keys]
    return mx_dequant(*mx_quant(vf)).transpose(-1, -2).reshape(B, H, n, D)[:, :, :L]


# ----------------------------------------------------------------------------- the online softmax of one key range
def range_pass(s, v, lo, hi, lk, quant=True):
    """s [R, >= hi'] float64 scores of R query rows, v [>= hi', 128] float64 values (hi' = min(hi, lk)); keys [lo, hi) (lo a multiple of
    64) with those at or past `lk` masked -> (O 2^-rd [R, 128], ref [R], l [R]) in the units of the range's last reference."""
    R = s.shape[0]
    halves = -(-(hi - lo) // HALF)
    o = torch.zeros(R, v.shape[1], dtype=torch.float64)
    l = torch.zeros(R, dtype=torch.float64)
    rd = torch.zeros(R, dtype=torch.float64)
    ref = None
    for g in range(halves):
        a, b = lo + HALF * g, min(lo + HALF * (g + 1), lk, hi)
        if b <= a:
            continue
        sc = s[:, a:b]
        mx = sc.amax(dim=1)
        if ref is None:
            ref = torch.floor(mx) - REF_HEAD
        else:
            move = mx - ref > RESCALE_THR
            delta = torch.where(move, torch.minimum(torch.floor(mx - ref - REF_HEAD), RD_MAX - rd), torch.zeros_like(rd))
            ref, rd = ref + delta, rd + delta
            l = l * torch.pow(2.0, -delta)
            sc = torch.where(move[:, None], torch.minimum(sc, (ref + RESCALE_THR)[:, None]), sc)
        p = torch.pow(2.0, sc - ref[:, None])
        if quant:
            p = p.float().double()
            pq = e4m3(p)
        else:
            pq = p
        l = l + p.sum(dim=1)
        o = o + (pq * torch.pow(2.0, rd)[:, None]) @ v[a:b]
    return o * torch.pow(2.0, -rd)[:, None], ref, l


def split_ranges(lk, kv_splits):
    """Key ranges [lo, hi) of a unit cut into kv_splits ranges (empty trailing ranges dropped, as attn_run does)."""
    tiles = -(-lk // KVBLK)
    tps = -(-tiles // kv_splits)
    return [(t * KVBLK, min((t + tps) * KVBLK, tiles * KVBLK)) for t in range(0, tiles, tps)]


def attend_rows(s, v, lk, ranges, quant=True):
    """Output rows (float64 [R, 128]) of one (batch, head) over the given key ranges, partials merged as attn_merge_kernel does."""
    parts = [range_pass(s, v, lo, hi, lk, quant) for lo, hi in ranges]
    if len(parts) == 1:
        o, _, l = parts[0]
        return o / l[:, None]
    m = torch.stack([p[1] for p in parts]).amax(dim=0)
    w = [torch.pow(2.0, p[1] - m) for p in parts]
    o = sum(wi[:, None] * p[0] for wi, p in zip(w, parts))
    l = sum(wi * p[2] for wi, p in zip(w, parts))
    return o / l[:, None]


def attention(q, k, v, rows, lk=None, kv_splits=1, split_from_unit=None, quant=True):
    """q [B, Lq, H, 128], k / v [B, Lk, H, 128] (bf16 as handed to the pack; a chunked call: the concatenated keys), the query rows to
    evaluate (a list of indices < Lq, the same for every batch and head), the call's split plan (kv_splits, split_from_unit: units
    before it run unsplit; None = every unit split) -> float64 [B, len(rows), H, 128].  quant=False: operands as given, P unrounded."""
    B, Lq, H, D = q.shape
    lk = k.shape[1] if lk is None else lk
    rows = torch.as_tensor(rows, dtype=torch.long)
    if quant:
        qd, kd, vd = dequant_rows(q), dequant_rows(k), dequant_v(v)
    else:
        qd, kd, vd = (t.double().cpu().permute(0, 2, 1, 3) for t in (q, k, v))
    q_blocks = -(-Lq // QBLK)
    from_unit = 0 if split_from_unit is None else split_from_unit
    whole = [(0, lk)]
    split = split_ranges(lk, kv_splits) if kv_splits > 1 else whole
    out = torch.empty(B, len(rows), H, D, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            s = qd[b, h, rows] @ kd[b, h, :lk].t()
            units = (b * H + h) * q_blocks + rows // QBLK
            for is_split in (False, True):
                sel = (units >= from_unit) == is_split
                if kv_splits == 1 and is_split:
                    sel = torch.zeros_like(sel)
                if kv_splits == 1 and not is_split:
                    sel = torch.ones_like(sel)
                if sel.any():
                    out[b, sel, h] = attend_rows(s[sel], vd[b, h, :lk], lk, split if is_split else whole, quant)
    return out
