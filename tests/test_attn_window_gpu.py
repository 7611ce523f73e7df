"""GPU: causal and sliding-window attention in the HIP kernel (attn_window_kernel of csrc/attn.hip) from the kernel call up to the model.

Exact cases (tests/attn_window_cases.py; tests/test_attn_window_cases_cpu.py proves that one key too many or too few at either edge of
any row moves that row by 8 bf16 ulps or more): integer scores in exp2 units, small positive integer V, so the output is the float64
masked attention rounded once to bf16 -- every element of every row within ONE bf16 ulp, the bound tests/test_attn_exact_gpu.py derives
for attn_fwd and applies, through both forms of the kernel (scale in kernel with softmax_scale = log 2; pre-scaled q).
Random data: against fp32 masked attention at the bound tests/test_hip_kernels.py applies to attn_fwd at like shapes (2 bf16 ulps + 6e-3).
Then the seam (attention(causal=, window_size=)), the model (fused engine and re-bound blocks against the oracle with its self-attention
masked; launch plans; sequence parallelism refused) and the C ABI's argument errors.

Measured on an MI355X, max |err| / ulp per exact case (recorded, not asserted; correct rounding gives at most 0.5; both forms alike):
L600-w100_37, L600-w-1_0, L600-w0_-1, L1111-w300_0 0.500, L600-w255_256 0.479, L70-w3_2 0.496, L70-w80_75 0.497; no element more than
1 ulp off.  Random data: max |err| 1.2e-3 (scale in kernel), 1.3e-3 (pre-scaled).  Model: rel-rms 4.2e-3, 66.7 dB, fused and re-bound."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_cases as W  # noqa: E402
from oracle import cases as C  # noqa: E402
from oracle import dit as O  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
REL_RMS, PSNR_DB = 1.5e-2, 40.0          # tests/test_dit_gpu.py: the HIP bf16 path against the fp32 oracle on the model output


@pytest.fixture(scope="module")
def H():
    from flexam_amd import hip
    hip.load_library()
    return hip


def _dev(*ts):
    return [t.to(BF).cuda() for t in ts]


def _check(name, got, want):
    """got [B, L, H, 128] from the kernel, want float64: all rows, 1 bf16 ulp (tests/test_attn_exact_gpu.py:_check)."""
    got = got.double().cpu()
    err = (got - want).abs() / W.bf16_ulp(want)
    bad = ~(err <= 1.0)                                          # (a NaN is bad)
    print(f"{name}: max |err| / ulp {float(err.max()):.3f}, elements off by more than 1 ulp: {int(bad.sum())}")
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.numel()} elements more than 1 bf16 ulp from float64 masked attention, max |err| / ulp "
                           f"{float(err.nan_to_num(float('inf')).max()):.3g}; first at (b, row, head, channel) = {bad.nonzero()[0].tolist()}: "
                           f"got {float(got[bad][0])}, want {float(want[bad][0])}")


@pytest.fixture(scope="module")
def exact():
    """Inputs and float64 reference of every case, computed once."""
    out = {}
    for c in W.CASES:
        q, k, v = c.inputs()
        out[c.name] = (q, k, v, c.want(q, k, v))
    return out


@pytest.mark.parametrize("prescaled", [False, True], ids=["scale-in-kernel", "prescaled"])
@pytest.mark.parametrize("case", W.CASES, ids=W.ids(W.CASES))
def test_exact_cases(H, exact, case, prescaled):
    q, k, v, want = exact[case.name]
    got = H.attn_fwd_window(*_dev(q, k, v), case.window, softmax_scale=None if prescaled else W.LN2, prescaled=prescaled)
    torch.cuda.synchronize()
    _check(f"{case.name} [{'prescaled' if prescaled else 'scale in kernel'}]", got, want)


@pytest.mark.parametrize("prescaled", [False, True], ids=["scale-in-kernel", "prescaled"])
def test_no_window_and_a_window_past_the_sequence_are_attn_fwd_byte_for_byte(H, exact, prescaled):
    q, k, v, _ = exact["L600-w100_37-b2h3"]
    qd, kd, vd = _dev(q, k, v)
    kw = dict(softmax_scale=None if prescaled else W.LN2, prescaled=prescaled)
    plain = H.attn_fwd(qd, kd, vd, kv_splits=1, **kw)
    for window in ((-1, -1), (599, 599), (-1, 5000), (-7, -2)):
        assert torch.equal(H.attn_fwd_window(qd, kd, vd, window, **kw), plain), window
    assert not torch.equal(H.attn_fwd_window(qd, kd, vd, (598, 599), **kw), plain)      # one key of one row masked: the windowed kernel ran


def test_strided_output_leaves_the_rest_of_the_buffer_alone(H, exact):
    """out= a row and column slice of a larger buffer, ragged last q block: the qi < Lq store guard under the backwards walk of the causal units."""
    q, k, v, want = exact["L600-w-1_0-b1h2"]
    big = torch.full((1, 607, 3 * 2 * 128), -768.0, device="cuda", dtype=BF)
    out = big[:, 3:603, 256:512].unflatten(2, (2, 128))
    H.attn_fwd_window(*_dev(q, k, v), (-1, 0), out=out, prescaled=True)
    torch.cuda.synchronize()
    _check("causal, strided out", out, want)
    rest = big.clone()
    rest[:, 3:603, 256:512] = -768.0
    assert bool((rest == -768.0).all())


def _masked_fp32(q, k, v, window, scale=None):
    """fp32 masked attention [B, L, H, 128] of bf16 inputs, natural softmax with scale (default 1 / sqrt(128))."""
    q, k, v = (t.float().transpose(1, 2) for t in (q, k, v))
    s = q @ k.transpose(-1, -2) * (128 ** -0.5 if scale is None else scale)
    s = s.masked_fill(~W.allowed(s.shape[-1], window).to(s.device), float("-inf"))
    return (s.softmax(-1) @ v).transpose(1, 2)


def _assert_bf16_close(got, want, ulps, atol, msg):
    got, want = got.float().cpu(), want.float().cpu()
    err = (got - want).abs()
    bad = err > ulps * (2.0 ** -8) * want.abs() + atol
    print(f"{msg}: max |err| {float(err.max()):.3e}")
    assert not bad.any(), f"{msg} {int(bad.sum())}/{bad.numel()} off; max err {float(err.max()):.4g}"


@pytest.fixture(scope="module")
def random_case():
    g = torch.Generator().manual_seed(1500)
    q, k, v = (torch.randn(1, 1500, 2, 128, generator=g).to(BF) for _ in range(3))
    return q, k, v, _masked_fp32(q, k, v, (448, 448))


@pytest.mark.parametrize("prescaled", [False, True], ids=["scale-in-kernel", "prescaled"])
def test_random_data_against_fp32_masked_attention(H, random_case, prescaled):
    """L = 1500, H = 2, window (448, 448): one latent frame either side of a 448-token frame; N(0, 1) data, non-integer p."""
    q, k, v, want = random_case
    if prescaled:
        qs = (q.float() * (128 ** -0.5 * 1.4426950408889634)).to(BF)
        want = _masked_fp32(qs, k, v, (448, 448), scale=0.6931471805599453)          # of the q the kernel was given
        got = H.attn_fwd_window(qs.cuda(), k.cuda(), v.cuda(), (448, 448), prescaled=True)
    else:
        got = H.attn_fwd_window(q.cuda(), k.cuda(), v.cuda(), (448, 448))
    _assert_bf16_close(got, want, 2.0, 6e-3, "windowed attention, random data")


# ----------------------------------------------------------------------------- the seam
def test_seam_serves_causal_and_window(H, exact, monkeypatch):
    from flexam_amd.attention_utils import attention
    q, k, v, _ = exact["L600-w100_37-b2h3"]
    qd, kd, vd = _dev(q, k, v)
    full = torch.tensor([600, 600])
    assert torch.equal(attention(qd, kd, vd, causal=True), H.attn_fwd_window(qd, kd, vd, (-1, 0)))
    assert torch.equal(attention(qd, kd, vd, window_size=(100, 37)), H.attn_fwd_window(qd, kd, vd, (100, 37)))
    assert torch.equal(attention(qd, kd, vd, window_size=(100, 37), causal=True), H.attn_fwd_window(qd, kd, vd, (100, 0)))
    assert torch.equal(attention(qd, kd, vd, window_size=(100, 37), softmax_scale=W.LN2, q_lens=full, k_lens=full),
                       H.attn_fwd_window(qd, kd, vd, (100, 37), softmax_scale=W.LN2))
    out = attention(qd.float(), kd.float(), vd.float(), causal=True)
    assert out.dtype == torch.float32 and torch.equal(out, H.attn_fwd_window(qd, kd, vd, (-1, 0)).float())
    # the quantised-attention switch with a mask: the bf16 windowed kernel's bytes
    monkeypatch.setenv("VIDEOX_ATTENTION_TYPE", "SAGE_ATTENTION")
    with torch.no_grad():
        assert torch.equal(attention(qd, kd, vd, window_size=(100, 37)), H.attn_fwd_window(qd, kd, vd, (100, 37)))
        assert not torch.equal(attention(qd, kd, vd), H.attn_fwd(qd, kd, vd))          # (without a mask the switch does take the MXFP8 kernel)


def test_seam_refuses_masks_whose_alignment_is_ambiguous(H, exact):
    from flexam_amd.attention_utils import attention
    q, k, v, _ = exact["L70-w3_2-b2h3"]
    qd, kd, vd = _dev(q, k, v)
    for kw in (dict(k_lens=torch.tensor([70, 50])), dict(q_lens=torch.tensor([60, 60])), dict(k_lens=torch.tensor([64, 64]))):
        for mask in (dict(causal=True), dict(window_size=(3, 2))):
            with pytest.raises(NotImplementedError, match="bottom-right"):
                attention(qd, kd, vd, **kw, **mask)
    with pytest.raises(NotImplementedError, match="bottom-right"):
        attention(qd[:, :40], kd, vd, causal=True)                                     # Lq != Lk
    with pytest.raises(NotImplementedError):
        attention(qd, kd, vd, attn_mask=torch.ones(70, 70, dtype=torch.bool, device="cuda"))
    with pytest.raises(NotImplementedError):
        attention(qd, kd, vd, dropout_p=0.1)
    with pytest.raises(RuntimeError, match="one length"):
        H.attn_fwd_window(qd[:, :40], kd, vd, (3, 2))


# ----------------------------------------------------------------------------- the model
WINDOW = (40, 40)


def _build(cfg, seed, window):
    from flexam_amd.wan_transformer3d_FlexAM import Wan2_2Transformer3DModel_FlexAM
    kw = dict(cfg)
    kw.pop("eps")
    m = Wan2_2Transformer3DModel_FlexAM(**kw, window_size=window)
    sd = C.dit_weights(cfg, seed)
    m.load_state_dict(sd, strict=True)
    return m.to("cuda:0"), sd


def _to_dev(case):
    return {k: ([u.cuda() for u in v] if isinstance(v, list) else (v.cuda() if torch.is_tensor(v) else v)) for k, v in case.items()}


def _check_model(got, want, what):
    got, want = got.float().cpu(), want.float()
    rel = ((got - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt()).item()
    p = C.psnr(got, want)
    print(f"{what}: rel-rms {rel:.3e}, psnr {p:.1f} dB")
    assert rel <= REL_RMS and p >= PSNR_DB, f"{what}: rel-rms {rel:.3e}, psnr {p:.1f} dB"


@pytest.fixture(scope="module")
def tiny():
    """DIT_TINY, its inputs, and the oracle's forward with the window applied to self-attention only (cross-attention calls the same
    oracle function: told apart by Lq == Lk), next to the unwindowed one."""
    cfg = dict(O.DIT_TINY)
    case = C.dit_case(cfg, 41)
    sd = C.dit_weights(cfg, 7)
    plain = O.attention

    def windowed(q, k, v, k_lens=None):
        if q.shape[1] != k.shape[1]:
            return plain(q, k, v, k_lens)
        assert k_lens is None and q.shape[1] > WINDOW[0] + WINDOW[1] + 1
        qt, kt, vt = (u.float().transpose(1, 2) for u in (q, k, v))
        s = qt @ kt.transpose(-1, -2) / q.shape[-1] ** 0.5
        s = s.masked_fill(~W.allowed(q.shape[1], WINDOW), float("-inf"))
        return (s.softmax(-1) @ vt).transpose(1, 2)

    full = O.dit_forward(sd, cfg, **case)
    mp = pytest.MonkeyPatch()
    mp.setattr(O, "attention", windowed)
    try:
        want = O.dit_forward(sd, cfg, **case)
    finally:
        mp.undo()
    assert (want - full).pow(2).mean().sqrt() / full.pow(2).mean().sqrt() > 3 * REL_RMS      # the mask shows at the tolerance (5.3e-2)
    return cfg, case, want, full


def test_model_with_a_window_matches_the_masked_oracle(tiny):
    cfg, case, want, _ = tiny
    m, _ = _build(cfg, 7, WINDOW)
    assert tuple(m.config["window_size"]) == WINDOW and m.blocks[0].self_attn.window_size == WINDOW
    d = _to_dev(case)
    first = m(**d).clone()
    assert m.engine().fused and m.engine().window == WINDOW and not m.engine().replay_taken
    _check_model(first, want, "fused engine, window (40, 40)")
    second = m(**d).clone()                                       # served from the launch plan
    assert m.engine().replay_taken and torch.equal(first, second)
    # re-bound self-attention forwards (the reference's multi-GPU hook point): the blocks run as modules
    calls = {"n": 0}

    def delegating(self, x, seq_lens, grid_sizes, freqs, dtype=torch.bfloat16, t=0):
        calls["n"] += 1
        return type(self).forward(self, x, seq_lens, grid_sizes, freqs, dtype, t=t)
    for blk in m.blocks:
        blk.self_attn.forward = types.MethodType(delegating, blk.self_attn)
    out = m(**d)
    assert calls["n"] == len(m.blocks) and not m.engine().fused
    _check_model(out, want, "re-bound blocks, window (40, 40)")


def test_the_window_is_part_of_the_plan_key(tiny):
    cfg, case, want, full = tiny
    d = _to_dev(case)
    a, _ = _build(cfg, 7, WINDOW)
    b, _ = _build(cfg, 7, (-1, -1))
    out_a, out_b = a(**d).clone(), b(**d).clone()
    _check_model(out_a, want, "window (40, 40)")
    _check_model(out_b, full, "no window")
    assert torch.equal(a(**d), out_a) and a.engine().replay_taken and torch.equal(b(**d), out_b) and b.engine().replay_taken
    # one engine, its window changed between two forwards: a new plan, never the other window's launches
    eng = a.engine()
    eng.window = (-1, -1)
    assert torch.equal(a(**d), out_b) and not eng.replay_taken
    eng.window = WINDOW
    assert torch.equal(a(**d), out_a) and eng.replay_taken


def test_sage_switch_with_a_window_runs_the_bf16_windowed_kernel(tiny, monkeypatch):
    from flexam_amd.dit_engine import DiTEngine
    cfg, case, want, _ = tiny
    d = _to_dev(case)
    m, _ = _build(cfg, 7, WINDOW)
    base = m(**d).clone()
    monkeypatch.setenv("VIDEOX_ATTENTION_TYPE", "SAGE_ATTENTION")
    monkeypatch.setattr(DiTEngine, "_sage_window_warned", False)
    m2, _ = _build(cfg, 7, WINDOW)
    with pytest.warns(RuntimeWarning, match="window_size"):
        out = m2(**d)
    assert not m2.engine().sage_taken and torch.equal(out, base)


def test_sequence_parallelism_with_a_window_is_refused(tiny):
    from flexam_amd.dist import sequence_parallel_context
    cfg, case, _, _ = tiny
    m, _ = _build(cfg, 7, WINDOW)
    d = _to_dev(case)
    m(**d)
    eng = m.engine()
    eng.sp_size = 2
    try:
        with pytest.raises(NotImplementedError, match="sequence parallelism"):
            m(**d)
    finally:
        eng.sp_size = 1
    sa = m.blocks[0].self_attn
    x = torch.zeros(1, 64, cfg["dim"], device="cuda")
    with sequence_parallel_context(None, 0, 2, 0, 128):
        with pytest.raises(NotImplementedError, match="sequence parallelism"):
            sa(x, None, [[2, 8, 8]], m.freqs)


# ----------------------------------------------------------------------------- the C ABI
def test_abi_argument_errors(H):
    from flexam_amd import abi
    E_ARG, E_SHAPE = abi.CONSTANTS["FLEXAM_E_ARG"], abi.CONSTANTS["FLEXAM_E_SHAPE"]
    lib = H.load_library()
    q = torch.zeros(1, 64, 2, 128, dtype=BF, device="cuda")
    o = torch.empty_like(q)
    s = torch.cuda.current_stream().cuda_stream

    def call(qp, kp, vp, op, L=64, hd=128, left=3, right=2):
        return lib.flexam_attn_fwd_window(qp, 64 * 256, 256, kp, 64 * 256, 256, vp, 64 * 256, 256, op, 64 * 256, 256, 1, 2, L, hd, 0.1, left, right, s)
    p = q.data_ptr()
    assert call(p, p, p, o.data_ptr()) == 0
    for args in ((None, p, p, o.data_ptr()), (p, None, p, o.data_ptr()), (p, p, None, o.data_ptr()), (p, p, p, None)):
        assert call(*args) == E_ARG and b"null pointer" in lib.flexam_last_error()
    assert call(p, p, p, o.data_ptr(), hd=64) == E_SHAPE and b"head_dim" in lib.flexam_last_error()
    for L in (0, -5):
        assert call(p, p, p, o.data_ptr(), L=L) == E_SHAPE and b"empty problem" in lib.flexam_last_error()
    assert call(p + 2, p, p, o.data_ptr()) == E_ARG and b"misaligned" in lib.flexam_last_error()
    with pytest.raises(RuntimeError, match="head_dim"):
        H.attn_fwd_window(q[..., :64].contiguous(), q[..., :64].contiguous(), q[..., :64].contiguous(), (3, 2))
    with pytest.raises(RuntimeError, match="packed"):
        H.attn_fwd_window(q.transpose(1, 2).contiguous().transpose(1, 2), q, q, (3, 2))
    torch.cuda.synchronize()
