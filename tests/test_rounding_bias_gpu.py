"""GPU: every kernel with a bf16 output, on general data, held to NO LEAN: the mean signed error against an unrounded float64 reference
of the same bf16-representable inputs is within 0.05 bf16 ulp, overall and in each of the 16 classes of output column modulo 16 (and,
where the elements of a row class are independent, in each of the 64 classes of output row modulo 64).  tests/rounding_bias.py derives
the bound and holds the data sets; tests/test_rounding_bias_cpu.py proves that a truncated P, a truncated output, and an output
truncated in one column of 16 or one row of 64 each read -0.35 or lower.  The distance tests (1 .. 4 ulps) and the exact tests (data
whose intermediate values are representable) cannot see any of those.

Every case is one kernel call (or one per form); the float64 reference runs on the device (RMSNorm + RoPE's, reused from
tests/test_dit_row_kernels_gpu.py, builds its angle table on the host).  Attention: B = 1, H = 2, head dim 128, Lq = 600, at flat
(score std 1 in exp2 units) and peaked (std 6: the deferred rescale moves) logits; each instance is pinned with
attn_exact_cases.dispatch.  The MXFP8 attention is out of scope (its P is e4m3 and l counts flushed keys by design;
tests/mxfp8_restatement.py restates it).

Measured on an MI355X (recorded, not asserted), per case: overall mean / worst column class / worst row class (- where not asserted),
flat logits | peaked logits; every figure in bf16 ulp:
    attn_fwd <1,false> Lk 200          -0.0019 / -0.0095 / -0.0287 | -0.0057 / -0.0118 / -
    attn_fwd SHORT, <1,true> Lk 200    -0.0021 / -0.0070 / -0.0235 | -0.0017 / -0.0065 / -      (the two instances: the same figures)
    attn_fwd <0,false> Lk 1100         -0.0004 / -0.0053 / +0.0113 | -0.0052 / -0.0109 / -
    attn_fwd FULL, <0,true> Lk 1100    +0.0010 / -0.0052 / +0.0184 | +0.0038 / +0.0085 / -
    split 3: FULL                      +0.0005 / -0.0051 / +0.0180 | +0.0008 / +0.0064 / -
    split 3: <0,false>                 +0.0000 / -0.0056 / +0.0143 | -0.0028 / -0.0066 / -
    partial x 3 + merge                -0.0003 / -0.0062 / +0.0176 | +0.0022 / +0.0066 / -
    attn_fwd_lastkey <1,false>         -0.0034 / -0.0081 / -       | +0.0047 / +0.0091 / -      (row classes, not asserted: -0.0491)
    attn_fwd_lastkey SHORT             -0.0026 / -0.0088 / -       | +0.0037 / +0.0089 / -      (row classes, not asserted: -0.0310)
    window (300, 100) pre-scaled       -0.0010 / -0.0047 / -0.0117 | -0.0025 / -0.0055 / -
    window (300, 100) scale in kernel  -0.0006 / +0.0077 / -0.0120 | +0.0018 / +0.0057 / -
    window + sink 70                   -0.0005 / +0.0050 / +0.0104 | -0.0064 / -0.0100 / -
    frames of 100, (1, 0), sink 70     -0.0019 / -0.0056 / -0.0150 | -0.0027 / -0.0052 / -
GEMMs, overall mean / worst column class / worst row class, EPI_NONE | EPI_GELU_TANH (0.31 % excluded, e4m3 weights 0.33 .. 0.34 %).  The
three M = 300 plans agree to one unit of the 4th digit (the sums differ only in fp32 order), so one line stands for them: finish kernel
alone (8 CUs, all CUs), whole-tile kernel alone (8 CUs, MT = 4); M = 1300 runs whole and tail tiles in one call:
    gemm bf16 M 300    -0.0003 / -0.0063 / -0.0169 | +0.0009 / +0.0074 / +0.0182
    gemm bf16 M 1300   -0.0001 / -0.0026 / -0.0047 | +0.0001 / +0.0027 / +0.0079
    gemm w8   M 300    -0.0010 / -0.0068 / -0.0120 | +0.0013 / +0.0094 / -0.0163
    gemm w8   M 1300   -0.0003 / -0.0028 / -0.0084 | +0.0003 / +0.0034 / +0.0078
    gemm fp8  M 300    +0.0011 / +0.0053 / +0.0198 | +0.0001 / -0.0077 / -0.0143
    gemm fp8  M 1300   -0.0006 / -0.0023 / -0.0076 | -0.0004 / -0.0033 / -0.0079
Row kernels, overall mean / worst column class (/ worst row class), share excluded:
    ln_modulate plain -0.0035 / -0.0074, 0.30 %             modulated -0.0003 / +0.0066, 0.39 %
    rmsnorm_rope q -0.0004 / +0.0023, 0.32 %                k -0.0002 / +0.0024, 0.31 %
    t5_norm +0.0003 / -0.0050                               mul_bf16 -0.0059 / -0.0080
    softmax_bias_rows bias -0.0003 / -0.0060 / -0.0151      no bias -0.0007 / -0.0052 / -0.0143
    softmax_rows +0.0003 / +0.0058                          groupnorm_silu_cl +0.0008 / +0.0075, 0.35 %
Nothing leaned: no kernel was changed.  (ln_modulate plain and mul_bf16 read as the CPU's round-to-nearest-even of the same data does,
-0.0035 and -0.0059: inputs on the bf16 grid repeat values within a row, so their roundings are not independent.)
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_exact_cases as X  # noqa: E402
import attn_window_cases as W  # noqa: E402
import attn_window_frames_cases as WF  # noqa: E402
import attn_window_sink_cases as WS  # noqa: E402
import rounding_bias as RB  # noqa: E402
import test_dit_row_kernels_gpu as DR  # noqa: E402
from gemm_checks import _gelu64  # noqa: E402
from test_gemm_bf16_instances_gpu import _plan, _tiles  # noqa: E402
from test_text_encoder_kernels_gpu import softmax_ref  # noqa: E402
from test_vae_row_kernels_gpu import padded_rows  # noqa: E402

pytestmark = pytest.mark.gpu
BF, F32, F64, U8, F8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8, torch.float8_e4m3fn
DEV = "cuda:0"
SHARPS = list(RB.SHARP)


@pytest.fixture(scope="module")
def H():
    from flexam_amd import hip
    hip.device_check()
    return hip


# ----------------------------------------------------------------------------- bf16 attention (csrc/attn.hip)
@pytest.fixture(scope="module")
def attn():
    """case(lq, lk, sharp, prescaled, mult, mask name) -> (q, k, v, want) on the device; every reference is computed once."""
    made = {}
    masks = {"window": lambda: W.allowed(WIN_L, WINDOW), "sink": lambda: WS.allowed(WIN_L, WINDOW, SINK),
             "frames": lambda: WF.allowed(WIN_L, FRAME_WINDOW, FRAME_TOKENS, SINK)}

    def case(lq, lk, sharp, prescaled, mult=1, mask=None):
        key = (lq, lk, sharp, prescaled, mult, mask)
        if key not in made:
            q, k, v = RB.attn_data(1000 * lk + 10 * SHARPS.index(sharp) + prescaled, lq, lk, sharp, prescaled, DEV)
            made[key] = (q, k, v, RB.attn_reference(q, k, v, prescaled, mult, masks[mask]() if mask else None))
        return made[key]
    return case


def _kw(prescaled):
    return dict(softmax_scale=None if prescaled else RB.SOFTMAX_SCALE, prescaled=prescaled)


def _no_lean(got, want, sharp, what, rows=True):
    """got [B, L, H, 128] bf16 from the kernel; the row classes only where many keys carry a row: at flat logits, and not with a
    weighted last key (tests/rounding_bias.py)."""
    torch.cuda.synchronize()
    return RB.assert_no_lean(RB.attn_rows_last(got.double()), RB.attn_rows_last(want), rows=rows and sharp == "flat", what=f"{what} [{sharp}]",
                             row_floor=RB.SMALL_ROW_FLOOR)


INSTANCES = [("<1,false>", 200, False, ()), ("SHORT", 200, True, ()), ("<1,true>", 200, True, X.NO_SHORT),
             ("<0,false>", 1100, False, ()), ("FULL", 1100, True, ()), ("<0,true>", 1100, True, X.NO_FULL)]


@pytest.mark.parametrize("sharp", SHARPS)
@pytest.mark.parametrize("inst,lk,prescaled,env", INSTANCES, ids=[i[0] for i in INSTANCES])
def test_attention_instances(H, attn, monkeypatch, inst, lk, prescaled, env, sharp):
    """One pass over the keys through each of the six instances: Lk = 200 (3 whole tiles and 8 keys) and 1100 (17 tiles and 12 keys)."""
    assert X.dispatch(lk, prescaled, False, False, 1, env) == inst
    for name, value in env:
        monkeypatch.setenv(name, value)
    q, k, v, want = attn(RB.ATTN_LQ, lk, sharp, prescaled)
    _no_lean(H.attn_fwd(q, k, v, kv_splits=1, **_kw(prescaled)), want, sharp, f"attn_fwd {inst} Lk={lk}")


@pytest.mark.parametrize("sharp", SHARPS)
@pytest.mark.parametrize("inst,prescaled", [("FULL", True), ("<0,false>", False)], ids=["FULL", "<0,false>"])
def test_attention_split_kv_and_merge(H, attn, inst, prescaled, sharp):
    """Lk = 1100 in 3 key ranges (6, 6 and 6 tiles) and the merge that writes the bf16 output."""
    assert X.dispatch(1100, prescaled, True, False, 1, ()) == inst and H.attn_effective_splits(1100, 3) == 3
    q, k, v, want = attn(RB.ATTN_LQ, 1100, sharp, prescaled)
    _no_lean(H.attn_fwd(q, k, v, kv_splits=3, **_kw(prescaled)), want, sharp, f"attn_fwd split 3 {inst}")


SETS = ((130, 420, 1), (0, 130, 1), (420, 1100, 2))


@pytest.mark.parametrize("sharp", SHARPS)
def test_attention_partial_calls_and_merge(H, attn, sharp):
    """attn_fwd_partial over three key sets in the sequence-parallel order, pre-scaled, then attn_merge."""
    q, k, v, want = attn(RB.ATTN_LQ, 1100, sharp, True)
    assert all(X.dispatch(hi - lo, True, n > 1, True, 1, ()) == "<1,true>" for lo, hi, n in SETS)
    slots = sum(H.attn_effective_splits(hi - lo, n) for lo, hi, n in SETS)
    ws = H.attn_partial_workspace(1, RB.HEADS, RB.ATTN_LQ, slots, q.device)
    n = 0
    for lo, hi, splits in SETS:
        n += H.attn_fwd_partial(q, k[:, lo:hi], v[:, lo:hi], ws, n, splits, **_kw(True))
    assert n == slots
    out = torch.empty(1, RB.ATTN_LQ, RB.HEADS, 128, device=q.device, dtype=BF)
    H.attn_merge(out, ws, n, **_kw(True))
    _no_lean(out, want, sharp, "attn_fwd_partial x 3 + attn_merge")


MULT = 386                                      # the model's text padding count


@pytest.mark.parametrize("sharp", SHARPS)
@pytest.mark.parametrize("inst,prescaled", [("<1,false>", False), ("SHORT", True)], ids=["<1,false>", "SHORT"])
def test_attention_weighted_last_key(H, attn, inst, prescaled, sharp):
    """attn_fwd_lastkey, Lk = 100, the last key counted 386 times: the reference adds ln 386 to its logit.  That key carries three
    quarters of a row at flat logits too (386 against 99 others), the row's channels share the rounding of its p, and a row class has
    19 rows: no row classes here, as at peaked logits (under honest rounding they read up to 0.049 at flat logits)."""
    assert X.dispatch(100, prescaled, False, False, MULT, ()) == inst
    q, k, v, want = attn(RB.ATTN_LQ, 100, sharp, prescaled, mult=MULT)
    _no_lean(H.attn_fwd_lastkey(q, k, v, float(MULT), **_kw(prescaled)), want, sharp, f"attn_fwd_lastkey {inst}", rows=False)


WIN_L, WINDOW, SINK, FRAME_WINDOW, FRAME_TOKENS = 1100, (300, 100), 70, (1, 0), 100
WINDOWED = [("window", True), ("window", False), ("sink", True), ("frames", True)]


@pytest.mark.parametrize("sharp", SHARPS)
@pytest.mark.parametrize("mask,prescaled", WINDOWED, ids=[f"{m}-{'pre' if p else 'scale'}" for m, p in WINDOWED])
def test_attention_window(H, attn, mask, prescaled, sharp):
    """attn_fwd_window, Lq = Lk = 1100: window (300, 100); the same with the first 70 keys always visible; frames of 100 tokens with
    window (1, 0) and the sink.  Against float64 attention under the mask hip.attn_fwd_window's docstring states (the `allowed` of
    the three window case modules)."""
    q, k, v, want = attn(WIN_L, WIN_L, sharp, prescaled, mask=mask)
    kw = {"window": {}, "sink": dict(sink=SINK), "frames": dict(sink=SINK, frame_tokens=FRAME_TOKENS)}[mask]
    got = H.attn_fwd_window(q, k, v, FRAME_WINDOW if mask == "frames" else WINDOW, **_kw(prescaled), **kw)
    _no_lean(got, want, sharp, f"attn_fwd_window {mask} {'pre-scaled' if prescaled else 'scale in kernel'}")


# ----------------------------------------------------------------------------- GEMMs (csrc/gemm.hip, csrc/gemm_fp8.hip)
@pytest.fixture(scope="module")
def gemms(H):
    """Per (kernel, M): (run(epilogue) -> bf16 out, y float64, keep); the exclusion cap is asserted here, from the reference alone."""
    out = {}
    for m in (RB.GEMM_M, RB.GEMM_M_TALL):
        a, w, b = RB.gemm_data(5 + m, DEV, m)
        w8 = RB.e4m3_weights(w)
        (qa, sa), (qw, sw) = H.quantize_rows_fp8(a), H.quantize_rows_fp8(w)
        torch.cuda.synchronize()
        for name, run, y in (("bf16", lambda epi, a=a, w=w, b=b: H.gemm(a, w, b, epilogue=epi), RB.gemm_reference(a, w, b)),
                             ("w8", lambda epi, a=a, w8=w8, b=b: H.gemm_w8(a, w8, b, epilogue=epi), RB.gemm_reference(a, w8, b)),
                             ("fp8", lambda epi, qa=qa, sa=sa, qw=qw, sw=sw, b=b: H.gemm_fp8(qa, sa, qw, sw, b, epilogue=epi),
                              RB.gemm_reference(qa.view(F8), qw.view(F8), b, sa, sw))):
            keep = RB.keep_mask(y)
            RB.assert_cap(keep, f"gemm {name} M={m}")
            out[name, m] = (run, y, keep)
    return out


def _pick_mt(m, n, nk, G):
    """pick_mt / best_256wide / launch_cost of csrc/gemm_tile.h restated on _plan: the tile height MT = 8 .. 4 of the 256-wide family
    (a tile costs MT + 1.25; a smaller tile must win by more than 3 %), a launch lasting its whole rounds of the G CUs plus the tail
    plan_split leaves (1 unsplit, else passes (1 / S + 4 / nk) + (4 + 0.03 rem S) / nk)."""
    best, best_cost = 8, 1e30
    for mt in range(8, 3, -1):
        tiles = _tiles(m, n, 32 * mt, 256)
        _, tail, S = _plan(tiles, nk, G)
        rem = tiles % G
        cost = 0.0 if rem == 0 else 1.0 if S == 1 else -(-rem * S // G) * (1.0 / S + 4.0 / nk) + (4.0 + 0.03 * rem * S) / nk
        if (tiles // G + cost) * (mt + 1.25) < best_cost * 0.97:
            best, best_cost = mt, (tiles // G + cost) * (mt + 1.25)
    return best


# (M, CU budget, FLEXAM_GEMM_MT or None) -> (MT, (whole tiles, tail tiles, K slices per tail tile)) of the bf16- and e4m3-weight GEMMs at
# N = 512, K = 2048 (N is no multiple of 160 or 192: the 256-wide family).  Whole tiles run gemm_bf16_kernel<EPI, bf16, MT, TAIL = false>,
# whose epilogue packs bf16 through LDS; tail tiles run the TAIL = true kernel (fp32 slabs) and gemm_splitk_finish_kernel, which rounds.
# A CU budget is a multiple of 8 and M = 300 has 4 or 6 tiles, so without a switch every tile there is a tail tile: the whole-tile kernel
# is reached at that shape with FLEXAM_GEMM_MT = 4 (6 tiles on 8 CUs: no cut pays), and by the planner's own choice at M = 1300.
GEMM_PLANS = {(RB.GEMM_M, 8, None): (5, (0, 4, 2)),           # the finish kernel writes all of the output
              (RB.GEMM_M, 8, 4): (4, (6, 0, 1)),              # the whole-tile kernel writes all of it
              (RB.GEMM_M, 0, None): (4, (0, 6, 4)),           # all 256 CUs: tail tiles only, another MT and another cut
              (RB.GEMM_M_TALL, 8, None): (7, (8, 4, 2))}      # 6 x 2 tiles of 224 rows: a whole round, then 4 tiles cut in 2, in one call


@pytest.mark.parametrize("epi", ["none", "gelu"])
@pytest.mark.parametrize("kernel", ["bf16", "w8", "fp8"])
def test_gemm(H, gemms, kernel, epi, monkeypatch):
    """flexam_gemm_bf16, flexam_gemm_w8 (e4m3 weights, upcast exactly in the reference) and flexam_gemm_fp8 (quantised with
    flexam_quantize_rows_fp8; the reference is the float64 product of the dequantised codes and scales), bf16 out, EPI_NONE and
    EPI_GELU_TANH, N = 512, K = 2048, once under each plan of GEMM_PLANS (asserted against the planner's restatement; the e4m3-weight
    GEMM takes the bf16 one's plan): the split-K finish kernel alone, the whole-tile kernel's LDS-staged bf16 pack alone, both in one
    call.  The fp8 GEMM has no split-K: its one epilogue runs in every call."""
    for name in ("FLEXAM_GEMM_MT", "FLEXAM_GEMM_N160", "FLEXAM_GEMM_N192"):
        monkeypatch.delenv(name, raising=False)
    assert os.environ.get("FLEXAM_GEMM_SPLITK", "1") != "0"
    code = H.EPI_GELU_TANH if epi == "gelu" else H.EPI_NONE
    nk = RB.GEMM_K // 64
    for (m, budget, forced), (mt, plan) in GEMM_PLANS.items():
        run, y, keep = gemms[kernel, m]
        want = _gelu64(y) if epi == "gelu" else y
        if forced:
            monkeypatch.setenv("FLEXAM_GEMM_MT", str(forced))
        H.set_cu_budget(budget)
        try:
            G = H.num_cus()
            assert budget == 0 and G == 256 or G == budget
            assert (forced or _pick_mt(m, RB.GEMM_N, nk, G)) == mt and _plan(_tiles(m, RB.GEMM_N, 32 * mt, 256), nk, G) == plan
            got = run(code)
            torch.cuda.synchronize()
        finally:
            H.set_cu_budget(0)
            monkeypatch.delenv("FLEXAM_GEMM_MT", raising=False)
        RB.assert_no_lean(got, want, keep, rows=True, what=f"gemm {kernel} {epi}, M={m}, {budget or 'all'} CUs, MT={mt} {plan}",
                          row_floor=RB.SMALL_ROW_FLOOR if m == RB.GEMM_M else RB.MIN_PER_CLASS)


# ----------------------------------------------------------------------------- row kernels with a bf16 output
@pytest.mark.parametrize("modulated", [False, True], ids=["plain", "modulated"])
def test_ln_modulate(H, modulated):
    """flexam_ln_modulate, M = 64, C = 3072 (wave form, NV8 = 6), plain and with the (shift, 1 + scale) rows of a table."""
    x, tab, rows = RB.ln_data(21, DEV)
    r = rows.long()
    want = DR.ln_ref(x, 1e-6, **(dict(sh=tab[r, 0], sc=tab[r, 1]) if modulated else {}))[0]
    keep = RB.keep_mask(want)
    RB.assert_cap(keep, "ln_modulate")
    got = H.ln_modulate(x, eps=1e-6, **(dict(shift=tab[:, 0], scale=tab[:, 1], row_index=rows) if modulated else {}))
    torch.cuda.synchronize()
    RB.assert_no_lean(got, want, keep, what=f"ln_modulate {'modulated' if modulated else 'plain'}")


def test_rmsnorm_rope(H):
    """flexam_rmsnorm_rope on q and k in one call, M = 256 rows (8 sequences of 32 tokens, 24 of them rotated), C = 3072 in 24 heads
    of 128; the tables and the float64 reference of tests/test_dit_row_kernels_gpu.py."""
    from flexam_amd.rope import rope_tables
    q, k, wq, wk = RB.rms_data(22)
    wants = [DR.rope_ref(x.float(), w, RB.RMS_HD, True)[0].reshape(-1, RB.RMS_C).to(DEV) for x, w in ((q, wq), (k, wk))]
    keeps = [RB.keep_mask(w) for w in wants]
    for kp in keeps:
        RB.assert_cap(kp, "rmsnorm_rope")
    cos, sin = (t.to(DEV) for t in rope_tables(DR.GRID, RB.RMS_L, RB.RMS_HD))
    qd, kd = q.reshape(-1, RB.RMS_C).to(DEV), k.reshape(-1, RB.RMS_C).to(DEV)
    H.rmsnorm_rope(qd, wq.to(DEV), kd, wk.to(DEV), rope_cos=cos, rope_sin=sin, tokens_per_batch=RB.RMS_L, token_offset=0, head_dim=RB.RMS_HD)
    torch.cuda.synchronize()
    for name, got, want, kp in (("q", qd, wants[0], keeps[0]), ("k", kd, wants[1], keeps[1])):
        RB.assert_no_lean(got, want, kp, what=f"rmsnorm_rope {name}")


def test_t5_norm(H):
    """flexam_t5_norm, bf16 out, M = 48, C = 4096: w x rsqrt(mean(x^2) + eps), a product (no exclusion)."""
    x, w = RB.t5_data(23, DEV)
    x64 = x.double()
    want = w.double() * x64 * (x64.pow(2).mean(1, keepdim=True) + 1e-6).rsqrt()
    out = torch.empty(RB.T5_M, RB.T5_C, dtype=BF, device=DEV)
    H.t5_norm(x, w, out, eps=1e-6)
    torch.cuda.synchronize()
    RB.assert_no_lean(out, want, what="t5_norm")


@pytest.mark.parametrize("biased", [True, False], ids=["bias", "no-bias"])
def test_softmax_bias_rows(H, biased):
    """flexam_softmax_bias_rows, M = N = 512 (4096 elements in each of the 64 row classes), scale 0.125, with and without the bias."""
    s, b = RB.softmax_bias_data(24, DEV)
    want = softmax_ref(s, 0.125, b if biased else None, None)
    out = torch.empty(RB.SMB_M, RB.SMB_N + 64, dtype=BF, device=DEV)
    H.softmax_bias_rows(s, out, RB.SMB_N, 0.125, b if biased else None)
    torch.cuda.synchronize()
    RB.assert_no_lean(out[:, :RB.SMB_N], want, rows=True, what=f"softmax_bias_rows bias={biased}")


def test_mul_bf16(H):
    """flexam_mul_bf16, n = 2^18: the exact product of two bf16 values, rounded once."""
    a, b = RB.mul_data(25, DEV)
    got = H.mul_bf16(a, b)
    torch.cuda.synchronize()
    RB.assert_no_lean(got.view(-1, 1024), (a.double() * b.double()).view(-1, 1024), what="mul_bf16")


def test_softmax_rows(H):
    """flexam_softmax_rows (one form: a workgroup per row), the VAE encoder's middle attention: 450 positions, scale 640^-1/2, into
    [450, 512] bf16."""
    s = RB.softmax_rows_data(26, DEV)
    n, scale = RB.SMR_H * RB.SMR_W, RB.SMR_C ** -0.5
    out = torch.empty(n, (n + 63) // 64 * 64, dtype=BF, device=DEV)
    H.softmax_rows(s, scale, out, n)
    torch.cuda.synchronize()
    RB.assert_no_lean(out[:, :n], torch.softmax(s[:, :n].double() * scale, dim=1), what="softmax_rows")


def test_groupnorm_silu_cl(H):
    """flexam_groupnorm_silu_cl into a bf16 padded channels-last image, C = 256 in 32 groups, 2 x 16 x 24 positions; excluded by the
    pre-activation (the GroupNorm output), as GELU is by its GEMM output."""
    x, gamma, beta = RB.groupnorm_data(27)
    y = RB.groupnorm_preact(x.to(DEV), gamma.to(DEV), beta.to(DEV), RB.GN_GROUPS)            # [F, H, W, C]
    keep = RB.keep_mask(y)
    RB.assert_cap(keep, "groupnorm_silu_cl")
    dst = torch.zeros(RB.GN_F, RB.GN_H + 2, RB.GN_W + 2, RB.GN_C, dtype=BF, device=DEV)
    H.groupnorm_silu_cl(padded_rows(x).to(DEV), RB.GN_C, RB.GN_F, RB.GN_H, RB.GN_W, RB.GN_GROUPS, gamma.to(DEV), beta.to(DEV), dst)
    torch.cuda.synchronize()
    got = dst[:, 1:-1, 1:-1, :].reshape(-1, RB.GN_C)
    RB.assert_no_lean(got, RB.silu64(y).reshape(-1, RB.GN_C), keep.reshape(-1, RB.GN_C), what="groupnorm_silu_cl")
