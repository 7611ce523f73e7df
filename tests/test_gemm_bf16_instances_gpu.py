"""Every instance of the bf16 GEMM that launch() in csrc/gemm.hip can select -- gemm_bf16_kernel<EPI, OutT, MT, TAIL, WMW, NTW, W8>, its
TAIL twin and gemm_splitk_finish_kernel<EPI, OutT, MT, WMW, NTW> -- against exact restatements of its arithmetic.

Data.  a and w hold integers in -2..2 and the bias lies on a 1/4 grid, so the pre-epilogue value y = a.w + b is exact in float32 whatever
the tile, the K order or the split (asserted: y, computed in float64 on the device, round-trips through float32).  Rows of a cycle through
four densities: three sparse ones that give y a variance of 2, 9 and 36 -- |y| spread over roughly -12..12, the region where GELU bends,
both tails and zero -- and a dense one (|y| up to a few hundred: every lane's fragment of every K block carries data, GELU saturated).
Gates lie on a 1/2 grid and x0 is integer, so x0 + bf16(y) g is exact in float32 (asserted) whether the multiply-add is fused or not.
  NONE, bf16 out   bf16(y), bit for bit;            NONE, fp32 out   y, bit for bit;
  GELU_TANH        within 1 bf16 ulp of bf16(gelu64(y)), the rule of test_gemm_fp8_instances_gpu.py (gemm_checks.gelu_misses);
  GATE_RESIDUAL    fp32(x0 + bf16(y) g), bit for bit: no gate, a gate row per output row (gate_row), a gate row per batch of rows
                   (rows_per_batch, a batch boundary inside a row tile), and bias = None.
Views.  A, W and the gate table are slices of wider buffers whose margins hold NaN (lda, ldw != K): a stray read poisons the output.  C
(bf16 / fp32) and X (fp32) are slices at a column offset with sentinels above, below, left and right, intact after every call; `c_odd`
cases give the bf16 C a row stride of 4 mod 8 and a column offset of 4 (rows only 8-byte aligned under the 16-byte stores).
Every form is launched twice with flexam_set_cu_budget(8) -- identical bits -- and once with all CUs, a different split-K plan -- the
same bits again.

With 8 CUs the planner (plan_split, restated in _plan and asserted per shape) reaches, at a few hundred rows: several units per workgroup,
tail tiles cut into S = 2 or 4 K slices at K = 2048 with their finish kernel, launches whose whole tiles are none (split_full == 0:
the TAIL = false kernel is not launched), and the tall 160-wide tiles (tiles_tall >= 4 G = 32).  Instances, by <MT, WMW, NTW>; each
stands for the EPI / OutT forms (NONE, bf16), (NONE, float), (GELU, bf16), (GATE_RESIDUAL, bf16) of the TAIL = false kernel and of the
finish kernel, and for the one TAIL = true kernel <EPI_NONE, float, MT, true, WMW, NTW>:
  <4..8, 2, 4>        32 MT x 256 tiles      test_256_wide_instances (FLEXAM_GEMM_MT forces MT), _shapes_256
  <6, 2, 3>           192 x 192              test_192_wide_instance (FLEXAM_GEMM_N192=2), _SHAPES_192
  <4, 4, 5>           256 x 160              test_160_wide_instances, _SHAPES_160 rows marked short
  <6, 4, 5>           384 x 160, plain       test_160_wide_instances, _SHAPES_160 rows marked tall; test_tall_160_wide_tiles_at_the_full_cu_count
  <5, 4, 5>           320 x 160, gated       the same rows (launch() takes MT = 5 for EPI_GATE_RESIDUAL)
  <4..8, 2, 4, W8>, <6, 2, 3, W8>            test_w8_instances_equal_the_bf16_ones_on_upcast_weights
a_koff (per-K-block A offsets, tail slices starting at kb0 != 0): test_a_koff_in_every_family."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_checks import _margins_untouched, _strided, dev, gelu_misses  # noqa: E402

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
C16_SENTINEL, C32_SENTINEL, X_SENTINEL = 1232.0, 1234.5, -7.5
ALL_FORMS = ("bf16", "f32", "gelu", "res_none", "res_row", "res_rpb", "res_nobias")
G8 = 8                                              # the CU budget every shape below is planned for


@pytest.fixture(scope="module")
def H():
    from flexam_amd import hip
    hip.device_check()
    return hip


def _plan(tiles, nk, G=G8, n_slabs=256):
    """plan_split (csrc/gemm_tile.h) restated: (whole tiles run by the TAIL = false kernel, tail tiles, K slices per tail tile)."""
    rem, S, best = tiles % G, 1, 1.0
    s = 2
    while rem and s <= 8 and s <= nk // 8 and rem * s <= n_slabs:
        passes = (rem * s + G - 1) // G
        c = passes * (1.0 / s + 4.0 / nk) + (4.0 + 0.03 * rem * s) / nk
        if c < best - 0.05:
            best, S = c, s
        s += 1
    return (tiles - rem, rem, S) if S > 1 else (tiles, 0, 1)


def _tiles(m, n, bm, bn):
    return -(-m // bm) * -(-n // bn)


def _a_ints(m, cols, k, g):
    """[m, cols] integers in -2..2; row i keeps a fraction var / (4 k) of them, var = 2, 9, 36 (the variance of a.w over k terms of
    variance 2 x 2), or all of them (i % 4 == 3)."""
    a = torch.randint(-2, 3, (m, cols), generator=g).float()
    var = torch.tensor([2.0, 9.0, 36.0, 0.0])[torch.arange(m) % 4]
    dens = torch.where(var > 0, var / (4.0 * k), torch.ones(m)).clamp(max=1.0)
    return a * (torch.rand(m, cols, generator=g) < dens[:, None]).float()


class _Problem:
    """Operands in poisoned buffers and the exact expectations of every form, on the device."""

    def __init__(self, m, n, k, seed, c_odd=False, koff=False, w8=False):
        g = torch.Generator().manual_seed(seed)
        self.m, self.n, self.k, self.c_odd = m, n, k, c_odd
        cols = k + 128 if koff else k                                  # a_koff: A is a base view two K blocks wider than K
        a = _a_ints(m, cols, k, g)
        w = torch.randint(-2, 3, (n, k), generator=g).float()
        b = torch.randint(-8, 9, (n,), generator=g).float() / 4
        self.abuf, self.a = _strided(m, cols, cols + 24, BF, NAN, c0=8)
        self.wbuf, self.w = _strided(n, k, k + 40, BF, NAN, c0=16)
        self.a.copy_(a.to(dev()))
        self.w.copy_(w.to(dev()))
        self.w8 = None
        if w8:                                                         # the same integers as e4m3 bytes; margins 0x7F (e4m3 NaN), ldw in bytes
            self.w8buf, w8 = _strided(n, k, k + 48, torch.uint8, 0x7F, c0=16)
            w8.copy_(w.to(torch.float8_e4m3fn).view(torch.uint8).to(dev()))
            self.w8 = w8.view(torch.float8_e4m3fn)                     # H.gemm / H.gemm_gate_residual take the e4m3-W entry points by dtype
        self.bias = b.to(dev())
        a64 = a.to(dev()).double()
        self.kw = {}
        if koff:
            # K-block kb of the operand is the 64 columns at table[kb] of the base view: a permutation of the base's blocks that is not
            # the identity, one block used twice, starts that are multiples of 8 but not of 64
            nk = k // 64
            blocks = torch.randperm(nk + 1, generator=g)[:nk]
            blocks[nk // 2 + 1] = blocks[3]
            table = blocks * 64 + 8 * (torch.arange(nk) % 3)
            assert not torch.equal(table, torch.arange(nk) * 64) and int(table.max()) + 64 <= cols
            a64 = torch.cat([a64[:, o:o + 64] for o in table.tolist()], dim=1)
            self.kw = dict(a_koff=table.to(dev()))
        acc = a64 @ w.to(dev()).double().t()
        y = acc + self.bias.double()
        assert bool((y.float().double() == y).all())                   # exact in float32
        if m * n >= 10000:                                             # both tails, the bend and zero are all there
            sparse = y[torch.arange(m, device=dev()) % 4 != 3]
            assert float((sparse.abs() <= 12).double().mean()) > 0.9
            assert bool((sparse < -3).any() and (sparse > 3).any() and (sparse.abs() < 1).any())
        self.y = y
        nb = 3
        self.gbuf, self.gate = _strided(nb, n, n + 8, F32, NAN, c0=4)
        self.gate.copy_((torch.randint(-4, 5, (nb, n), generator=g).float() / 2).to(dev()))
        self.rows = torch.randint(0, nb, (m,), generator=g, dtype=torch.int32).to(dev())
        rpb = -(-m // nb)
        self.rpb = rpb + 5 if rpb % 16 == 0 else rpb                   # a batch boundary inside a row tile of 16
        self.x0 = torch.randint(-5, 6, (m, n), generator=g).float().to(dev())
        ybf = y.float().to(BF).double()
        g64, x64 = self.gate.double(), self.x0.double()
        res = {"res_none": x64 + ybf, "res_row": x64 + ybf * g64[self.rows.long()],
               "res_rpb": x64 + ybf * g64[torch.arange(m, device=dev()) // self.rpb],
               "res_nobias": x64 + acc.float().to(BF).double()}
        for v in res.values():
            assert bool((v.float().double() == v).all())               # one value in float32, fused multiply-add or not
        self.want = {"bf16": y.float().to(BF), "f32": y.float(), **{f: v.float() for f, v in res.items()}}

    def out_geometry(self, form):
        """(dtype, ld, c0, sentinel) of the output buffer of `form`."""
        n = self.n
        if form in ("bf16", "gelu"):
            return (BF, (n + 40) // 8 * 8 + 4, 4, C16_SENTINEL) if self.c_odd else (BF, (n + 47) // 8 * 8, 8, C16_SENTINEL)
        return (F32, n + 12, 4, C32_SENTINEL if form == "f32" else X_SENTINEL)

    def launch(self, H, form, w):
        """One launch of `form` into a fresh sentinel-filled buffer; returns the whole buffer."""
        dt, ld, c0, sentinel = self.out_geometry(form)
        buf, v = _strided(self.m, self.n, ld, dt, sentinel, c0=c0)
        assert v.data_ptr() % 16 == 0
        if form in ("bf16", "f32", "gelu"):
            H.gemm(self.a, w, self.bias, out=v, epilogue=H.EPI_GELU_TANH if form == "gelu" else H.EPI_NONE, m=self.m, k=self.k, **self.kw)
            return buf
        v.copy_(self.x0)
        if form == "res_none":
            H.gemm_gate_residual(self.a, w, self.bias, v, **self.kw)
        elif form == "res_row":
            H.gemm_gate_residual(self.a, w, self.bias, v, self.gate, self.rows, **self.kw)
        elif form == "res_rpb":
            H.gemm_gate_residual(self.a, w, self.bias, v, self.gate, None, rows_per_batch=self.rpb, **self.kw)
        else:
            H.gemm_gate_residual(self.a, w, None, v, **self.kw)
        return buf

    def check(self, form, buf, what):
        dt, ld, c0, sentinel = self.out_geometry(form)
        v = buf[1:1 + self.m, c0:c0 + self.n]
        tag = f"{what} {self.m}x{self.n}x{self.k} {form}"
        if form == "gelu":
            bad = gelu_misses(v, self.y)
            assert not bad.any(), f"{tag}: {int(bad.sum())} outputs more than 1 bf16 ulp from gelu64; first y = {float(self.y[bad][0])}, got {float(v[bad][0])}"
        else:
            bad = ~(v == self.want[form])
            assert not bad.any(), (f"{tag}: {int(bad.sum())} outputs differ; first at {bad.nonzero()[0].tolist()}: "
                                   f"got {float(v[bad][0])}, want {float(self.want[form][bad][0])}")
        assert _margins_untouched(buf, self.m, self.n, sentinel, c0=c0), f"{tag}: wrote outside the view"


def _run(H, P, what, forms=ALL_FORMS, w8=False):
    """Every form twice with 8 CUs (checked; identical bits), once with all CUs (another split-K plan; the same bits)."""
    try:
        H.set_cu_budget(G8)
        assert H.num_cus() == G8
        first = {f: P.launch(H, f, P.w) for f in forms}
        again = {f: P.launch(H, f, P.w) for f in forms}
        if w8:
            first8 = {f: P.launch(H, f, P.w8) for f in forms}
            again8 = {f: P.launch(H, f, P.w8) for f in forms}
    finally:
        H.set_cu_budget(0)
    assert H.num_cus() > G8
    full = {f: P.launch(H, f, P.w) for f in forms}
    for f in forms:
        P.check(f, first[f], what)
        assert torch.equal(first[f].view(torch.uint8), again[f].view(torch.uint8)), f"{what} {f}: two launches differ"
        assert torch.equal(first[f].view(torch.uint8), full[f].view(torch.uint8)), f"{what} {f}: the plans for 8 CUs and for all CUs differ"
        if w8:
            assert torch.equal(first[f].view(torch.uint8), first8[f].view(torch.uint8)), f"{what} {f}: e4m3 W differs from the upcast weights"
            assert torch.equal(first8[f].view(torch.uint8), again8[f].view(torch.uint8)), f"{what} {f}: two e4m3-W launches differ"


# ----------------------------------------------------------------------------- 256-wide tiles: <MT, 2, 4>, MT = 4..8, bm = 32 MT
def _shapes_256(mt):
    """(m, n, k, c_odd, (whole tiles, tail tiles, slices)) -- the plan for 8 CUs."""
    bm = 32 * mt
    return [(3 * bm + 17, 388, 128, True, (8, 0, 1)),         # 4 x 2 tiles, N ragged (388 % 8 == 4) and edge rows; one unit per workgroup, 2 K blocks
            (2 * bm - 5, 388, 2048, True, (0, 4, 2)),         # 2 x 2 tiles, all of them tail tiles of 2 slices: split_full == 0, TAIL and finish kernels only
            (5 * bm + 9, 644, 2048, False, (16, 2, 4)),       # 6 x 3 tiles: 16 whole (2 units per workgroup, counted hand-over), 2 cut in 4
            (30 * bm + 5, 388, 128, False, (62, 0, 1)),       # 31 x 2 tiles on 8 workgroups: 7-8 units each, the prefetch under the epilogue
            (5, 4, 64, True, (1, 0, 1))]                      # one partial tile, one K block: the smallest legal problem


@pytest.mark.parametrize("shape_i", range(5))
@pytest.mark.parametrize("mt", [4, 5, 6, 7, 8])
def test_256_wide_instances(H, mt, shape_i, monkeypatch):
    monkeypatch.setenv("FLEXAM_GEMM_MT", str(mt))
    monkeypatch.setenv("FLEXAM_GEMM_N160", "0")              # N = 4 would take the narrow 160-wide route
    m, n, k, c_odd, plan = _shapes_256(mt)[shape_i]
    assert _plan(_tiles(m, n, 32 * mt, 256), k // 64) == plan
    _run(H, _Problem(m, n, k, 1000 * mt + shape_i, c_odd), f"MT={mt}")


# ----------------------------------------------------------------------------- the 192 x 192 tile: <6, 2, 3>
_SHAPES_192 = [(7, 192, 128, True, (1, 0, 1)),               # less than one tile
               (7, 192, 2048, False, (0, 1, 4)),              # ... cut in 4: tail and finish only
               (7, 576, 128, False, (3, 0, 1)),
               (7, 576, 2048, True, (0, 3, 2)),
               (192 * 2 + 7, 192, 128, False, (3, 0, 1)),    # interior tiles (the LDS-staged epilogues with shadow lanes) above an edge tile
               (192 * 2 + 7, 192, 2048, True, (0, 3, 2)),
               (192 * 2 + 7, 576, 128, True, (9, 0, 1)),     # 3 x 3 tiles: a second unit for one workgroup
               (192 * 2 + 7, 576, 2048, False, (8, 1, 4)),
               (192 * 5 + 9, 192, 128, False, (6, 0, 1)),
               (192 * 5 + 9, 192, 2048, False, (6, 0, 1)),   # 6 tiles: no split pays, 32 K blocks per unit
               (192 * 5 + 9, 576, 128, False, (18, 0, 1)),   # 6 x 3 tiles, 2-3 units per workgroup
               (192 * 5 + 9, 576, 2048, True, (16, 2, 4))]


@pytest.mark.parametrize("shape_i", range(len(_SHAPES_192)))
def test_192_wide_instance(H, shape_i, monkeypatch):
    monkeypatch.setenv("FLEXAM_GEMM_N192", "2")
    m, n, k, c_odd, plan = _SHAPES_192[shape_i]
    assert _plan(_tiles(m, n, 192, 192), k // 64) == plan
    _run(H, _Problem(m, n, k, 192000 + shape_i, c_odd), "192-wide")


# ----------------------------------------------------------------------------- 160-wide tiles: <4, 4, 5> short, <6, 4, 5> / <5, 4, 5> tall
TALL_M = 320 * 20 + 11       # 17 x 2 = 34 tiles of 384 rows (>= 4 G = 32: the tall instances), 21 x 2 = 42 tiles of 320 rows: 2 tail tiles either way
_SHAPES_160 = [  # (m, n, k, c_odd, tile rows of the plain forms, plan of the plain forms)
    (777, 160, 64, False, 256, (4, 0, 1)),                   # short: 4 x 1 tiles, one K block
    (777, 160, 2048, False, 256, (0, 4, 2)),                 # short: tail and finish only
    (300, 320, 64, True, 256, (4, 0, 1)),                    # short: 2 x 2 tiles
    (300, 320, 2048, True, 256, (0, 4, 2)),
    (2100, 320, 2048, False, 256, (16, 2, 4)),               # short: 9 x 2 tiles, whole ones (2 units per workgroup) and cut ones in one launch
    (300, 96, 64, False, 256, (2, 0, 1)),                    # short, the narrow route (N <= 160): a partial tile column
    (300, 96, 2048, False, 256, (0, 2, 4)),
    (41, 12, 64, True, 256, (1, 0, 1)),                      # short, narrow, N ragged (12 % 8 == 4), less than one tile
    (41, 12, 2048, True, 256, (0, 1, 4)),
    (TALL_M, 320, 64, False, 384, (34, 0, 1)),               # tall: 4-5 units per workgroup
    (TALL_M, 320, 2048, True, 384, (32, 2, 4))]              # tall: with their TAIL and finish kernels


@pytest.mark.parametrize("shape_i", range(len(_SHAPES_160)))
def test_160_wide_instances(H, shape_i, monkeypatch):
    monkeypatch.delenv("FLEXAM_GEMM_N160", raising=False)
    m, n, k, c_odd, bm, plan = _SHAPES_160[shape_i]
    tall = -(-m // 384) * -(-n // 160) >= 4 * G8               # launch(): tiles_tall >= 4 flexam_num_cus()
    assert tall == (bm == 384)
    assert _plan(_tiles(m, n, bm, 160), k // 64) == plan
    if tall:                                                   # the gated residual runs 320-row tiles: <5, 4, 5>
        assert _plan(_tiles(m, n, 320, 160), k // 64) == ((42, 0, 1) if k == 64 else (40, 2, 4))
    _run(H, _Problem(m, n, k, 160000 + shape_i, c_odd), "160-wide")


# ----------------------------------------------------------------------------- a_koff, once per family
@pytest.mark.parametrize("family,m,n,bm,bn,plan", [("256", 5 * 160 + 9, 644, 160, 256, (16, 2, 4)), ("192", 192 * 5 + 9, 576, 192, 192, (16, 2, 4)),
                                                   ("160", 2100, 320, 256, 160, (16, 2, 4)), ("160", TALL_M, 320, 384, 160, (32, 2, 4))])
def test_a_koff_in_every_family(H, family, m, n, bm, bn, plan, monkeypatch):
    """Per-K-block A offsets over a base view at K = 2048: whole tiles walk the table from 0, the four slices of a tail tile from kb0 =
    8, 16, 24.  Exact against the product with the gathered columns."""
    k = 2048
    if family == "256":
        monkeypatch.setenv("FLEXAM_GEMM_MT", "5")
    if family == "192":
        monkeypatch.setenv("FLEXAM_GEMM_N192", "2")
    assert _plan(_tiles(m, n, bm, bn), k // 64) == plan
    _run(H, _Problem(m, n, k, 7000 + m, koff=True), f"a_koff {family}", forms=("f32", "gelu", "res_row"))


# ----------------------------------------------------------------------------- e4m3 W: <MT, 2, 4, W8>, <6, 2, 3, W8>
@pytest.mark.parametrize("mt", [4, 5, 6, 7, 8, 192])
def test_w8_instances_equal_the_bf16_ones_on_upcast_weights(H, mt, monkeypatch):
    """flexam_gemm_w8 / flexam_gemm_w8_gate_residual on e4m3 weights: bit for bit what the bf16 calls give on the upcast weights (which are
    checked against the restatement here as well), on the ragged shape and on the shape with whole and cut tiles."""
    if mt == 192:
        monkeypatch.setenv("FLEXAM_GEMM_N192", "2")
        shapes = [(192 * 2 + 7, 576, 128, True, (9, 0, 1)), (192 * 5 + 9, 576, 2048, False, (16, 2, 4))]
        bm, bn = 192, 192
    else:
        monkeypatch.setenv("FLEXAM_GEMM_MT", str(mt))
        shapes = [_shapes_256(mt)[0], _shapes_256(mt)[2]]
        bm, bn = 32 * mt, 256
    for i, (m, n, k, c_odd, plan) in enumerate(shapes):
        assert _plan(_tiles(m, n, bm, bn), k // 64) == plan
        _run(H, _Problem(m, n, k, 8000 + 10 * mt + i, c_odd, w8=True), f"W8 {mt}", w8=True)


def test_w8_still_refuses_the_160_wide_widths(H, monkeypatch):
    from flexam_amd.abi import CONSTANTS
    monkeypatch.delenv("FLEXAM_GEMM_N160", raising=False)
    a = torch.zeros(64, 64, dtype=BF, device=dev())
    for n in (320, 160, 96):
        w = torch.zeros(n, 64, dtype=torch.uint8, device=dev())
        c = torch.full((64, n), C16_SENTINEL, dtype=BF, device=dev())
        x = torch.full((64, n), X_SENTINEL, device=dev())
        with pytest.raises(RuntimeError, match=f"code {CONSTANTS['FLEXAM_E_SHAPE']}:"):
            H.gemm_w8(a, w, out=c)
        with pytest.raises(RuntimeError, match=f"code {CONSTANTS['FLEXAM_E_SHAPE']}:"):
            H.gemm_w8_gate_residual(a, w, None, x)
        assert bool((c == C16_SENTINEL).all()) and bool((x == X_SENTINEL).all())       # nothing ran


# ----------------------------------------------------------------------------- the tall 160-wide tiles the way production reaches them
def test_tall_160_wide_tiles_at_the_full_cu_count(H, monkeypatch):
    """All CUs, N = 160, K = 64 and M just above 4 num_cus() 384 rows (the VAE encoder's 160-channel convolutions over ~400 000 rows):
    launch() takes <6, 4, 5> (384 x 160) for the plain forms and <5, 4, 5> (320 x 160) for the gated residual.  The whole bf16, fp32 and
    gate_row results are exact; the float64 reference is computed on the device."""
    monkeypatch.delenv("FLEXAM_GEMM_N160", raising=False)
    H.set_cu_budget(0)
    n, k = 160, 64
    m = 4 * H.num_cus() * 384 - 383 + 76                       # ceil(m / 384) = 4 num_cus(): the threshold itself, with a partial last tile
    assert -(-m // 384) == 4 * H.num_cus()
    P = _Problem(m, n, k, 160160, c_odd=True)
    for form in ("bf16", "f32", "res_row"):
        P.check(form, P.launch(H, form, P.w), "all CUs, tall 160-wide")
