"""GPU: smooth-K behind FLEXAM_SAGE_SMOOTH_K=1 (csrc/attn_fp8.inc: flexam_k_mean, flexam_rmsnorm_rope_mx_shift, flexam_attn_fp8_pack_shift)
against tests/smooth_k_restatement.py, from the kernels up to the three users of the MXFP8 self-attention: (a) the mean in both forms
within a counted bound, bit-stable; (b) the shifted fused producer in admissible bytes; (c) the shifted pack byte for byte; (d) attention on
data with a channel offset in K: the restatement's output, and the error against exact attention the offset costs and the mean removes;
(e) the attention() seam, (f) the DiT engine at 24 heads (fused producer; and with a bias in K) and (g) at 2 heads (general form): the
switch taken, the launch plan keyed on it, replay bit for bit."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp8_restatement as MX  # noqa: E402
import rmsnorm_rope_mx_restatement as R  # noqa: E402
import smooth_k_restatement as S  # noqa: E402

from oracle import cases as C  # noqa: E402
from oracle import dit as O  # noqa: E402

pytestmark = pytest.mark.gpu
REL_RMS = 3.2e-3               # the kernel against its restatement, both rounded to bf16 (tests/test_attn_fp8_restated_gpu.py)
BF = torch.bfloat16


@pytest.fixture(scope="module")
def H():
    from flexam_amd import hip
    hip.load_library()
    return hip


def _filled_buffers(H, B, heads, L):
    bufs = H.attn_fp8_buffers(B, heads, L, "cuda")
    for t in bufs:
        t.view(torch.uint8).fill_(R.FILL)
    return bufs


def _bytes(bufs):
    q8, qs, kv8 = (t.cpu() for t in bufs)
    return q8, qs.view(torch.uint8).reshape(tuple(qs.shape) + (4,)), kv8


# ----------------------------------------------------------------------------- (a) the mean
@pytest.mark.parametrize("B,L,offset,parts", [(2, 200, 5, None), (1, 65, 0, None), (3, 1, 0, None), (1, 1111, 0, 1), (1, 1111, 0, 7), (1, 1111, 0, None)])
@pytest.mark.parametrize("normed", [True, False], ids=["norm+rope", "as-given"])
def test_k_mean_within_the_counted_bound_and_bit_stable(H, B, L, offset, parts, normed):
    """hip.k_mean against the float64 mean of the float64 values (reference()'s y, or k itself), per channel within
    (DELTA + (tokens_per_part + parts + 2) 2^-24) mean_t(mag) (no DELTA and mag = |k| as given; counted in the restatement); a second
    call and a call under another CU budget give the same bits.  k is a column view of a [M, 9216] buffer where the producer's case is.
    Measured on an MI355X: the largest |err| / bound is 0.10 (one token, normed: the DELTA term alone), 0.09 as given (L = 65)."""
    c = S.mean_inputs(B, L, offset)
    want, mag = S.mean_reference(B, L, offset, normed)
    k = c.k.cuda()
    if L != 1111:                                              # the engine's form: a column view, row pitch 9216
        wide = torch.zeros(B * L, 3 * R.C, dtype=BF, device="cuda")
        wide[:, R.C:2 * R.C] = k
        k = wide[:, R.C:2 * R.C]
    args = (k, c.wk.cuda(), c.cos.cuda(), c.sin.cuda(), L, offset) if normed else (k, None, None, None, L)
    n = H.k_mean_parts(L) if parts is None else parts
    scratch = lambda: torch.full((B, n, R.C), float("nan"), device="cuda")
    got = H.k_mean(*args, eps=c.eps, scratch=scratch())
    again = H.k_mean(*args, eps=c.eps, scratch=scratch(), out=torch.full((B, R.C), float("nan"), device="cuda"))
    H.set_cu_budget(64)
    try:
        budget = H.k_mean(*args, eps=c.eps, scratch=scratch())
    finally:
        H.set_cu_budget(0)
    if parts is None:
        default = H.k_mean(*args, eps=c.eps)                   # the wrapper's own scratch
        assert torch.equal(default, got)
    assert torch.equal(got, again) and torch.equal(got, budget)
    err = (got.double().cpu() - want).abs()
    bound = S.k_mean_bound(mag, -(-L // n), n, normed)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"B={B} L={L} offset={offset} parts={n} normed={normed}: max |err| / bound {worst:.3f}, max |err| {float(err.max()):.3e}")
    assert torch.isfinite(got).all() and bool((err <= bound).all()), f"max |err| / bound {worst}"


def test_k_mean_refuses_what_it_cannot_do(H):
    k = torch.zeros(130, 256, dtype=BF, device="cuda")
    w, tab = torch.ones(256, device="cuda"), torch.ones(65, 64, device="cuda")
    with pytest.raises(RuntimeError, match="do not tile"):
        H.k_mean(k, None, None, None, 7)
    with pytest.raises(RuntimeError, match="scratch must be"):
        H.k_mean(k, None, None, None, 65, scratch=torch.zeros(2, 66, 256, device="cuda"))
    with pytest.raises(RuntimeError, match="scratch must be"):
        H.k_mean(k, None, None, None, 65, scratch=torch.zeros(1, 4, 256, device="cuda"))
    with pytest.raises(RuntimeError, match="out must be"):
        H.k_mean(k, None, None, None, 65, out=torch.zeros(2, 128, device="cuda"))
    with pytest.raises(RuntimeError, match="RoPE tables"):
        H.k_mean(k, w, None, None, 65)
    with pytest.raises(RuntimeError, match="RoPE tables must be"):
        H.k_mean(k, w, tab[:64], tab[:64], 65)
    with pytest.raises(RuntimeError, match="bad sizes"):       # the C side: parts beyond the tokens
        H._call("flexam_k_mean", H._ptr(k), 256, None, 130, 256, 1e-6, None, None, 65, 0, 128, 66, H._ptr(w), H._ptr(w))
    with pytest.raises(RuntimeError, match="at most 3072"):
        H._call("flexam_k_mean", H._ptr(k), 4096, H._ptr(w), 2, 4096, 1e-6, H._ptr(tab), H._ptr(tab), 1, 0, 128, 1, H._ptr(w), H._ptr(w))


# ----------------------------------------------------------------------------- (b) the shifted fused producer
def _shifted_on_gpu(c):
    qkv = c.qkv.cuda()
    if c.form == "qkv":
        q, k = qkv[:, :R.C], qkv[:, R.C:2 * R.C]
    else:
        q = torch.zeros(c.M, R.C + 8, dtype=BF, device="cuda")[:, :R.C]
        k = torch.zeros(c.M, R.C + 64, dtype=BF, device="cuda")[:, :R.C]
        q.copy_(qkv[:, :R.C])
        k.copy_(qkv[:, R.C:2 * R.C])
    return q, k, c.wq.cuda(), c.wk.cuda(), c.cos[:c.L + c.offset].cuda(), c.sin[:c.L + c.offset].cuda()


@pytest.mark.parametrize("name", S.SHIFTED_CASES)
def test_shifted_fused_producer_writes_admissible_bytes_and_nothing_else(H, name):
    """rmsnorm_rope_mx(..., k_shift=shift) on shifted_case(name) into 0xA5-filled buffers: Q judged as tests/test_attn_fp8_producers_gpu.py
    judges it, K against the SHIFTED admissible set -- no scale byte, no code refused; every byte outside fused_writes still 0xA5; and with
    k_shift=None the new wrapper leaves what the entry point without a shift leaves, bit for bit.  The Q half of the shifted call is a
    launch of the plain instance: its bytes are the unshifted call's.
    Measured on an MI355X: nothing refused; of K's bytes 12 (`ragged`), 1 and 4 differ from the nominal ones, of Q's 2, 0 and 0."""
    c = S.shifted_case(name)
    for a in S.shifted_admissible(name):
        assert a.ambiguous_codes <= R.AMBIGUOUS_CAP and a.ambiguous_scales <= R.AMBIGUOUS_CAP
    q, k, wq, wk, cos, sin = _shifted_on_gpu(c)
    bufs = _filled_buffers(H, c.B, R.HEADS, c.L)
    H.rmsnorm_rope_mx(q, wq, k, wk, bufs, cos, sin, c.L, c.offset, eps=c.eps, k_shift=c.shift.cuda())
    after = _bytes(bufs)
    verdicts = S.check_shifted_operands(name, *after)
    for which, vd in zip("qk", verdicts):
        print(f"{name} {which}: {vd.off_nominal} bytes off the nominal ones, {vd.bad_scales} scale bytes and {vd.bad_codes} codes refused")
    for vd in verdicts:
        assert vd.bad_scales == 0 and vd.bad_codes == 0, vd.first
    for what, buf, w in zip(("q8", "qs", "kv8"), after, R.fused_writes(c.B, c.L)):
        stray = (buf != R.FILL) & ~w
        assert not bool(stray.any()), f"{what}: {int(stray.sum())} bytes written outside the valid rows, the first at {stray.nonzero()[0].tolist()}"
    # the unshifted wrapper call against the entry point it has always called, and against the shifted bytes
    plain, old = _filled_buffers(H, c.B, R.HEADS, c.L), _filled_buffers(H, c.B, R.HEADS, c.L)
    H.rmsnorm_rope_mx(q, wq, k, wk, plain, cos, sin, c.L, c.offset, eps=c.eps, k_shift=None)
    H._call("flexam_rmsnorm_rope_mx", H._ptr(q), q.stride(0), H._ptr(wq), H._ptr(k), k.stride(0), H._ptr(wk), *(H._raw(t) for t in old),
            c.M, R.C, c.eps, H._ptr(cos), H._ptr(sin), c.L, c.offset, R.HEADS, R.HD)
    for a, b, s in zip(_bytes(plain), _bytes(old), after):
        assert torch.equal(a, b)
    assert torch.equal(_bytes(plain)[0], after[0]) and torch.equal(_bytes(plain)[1], after[1])          # the Q half does not see the shift
    assert not torch.equal(_bytes(plain)[2], after[2])
    with pytest.raises(RuntimeError, match="k_shift must be"):
        H.rmsnorm_rope_mx(q, wq, k, wk, plain, cos, sin, c.L, c.offset, eps=c.eps, k_shift=c.shift.cuda()[:, :R.C - 8])


# ----------------------------------------------------------------------------- (c) the shifted pack
def test_shifted_pack_byte_for_byte(H):
    """attn_fp8_pack(q, k, v, k_shift=s) against pack_bytes(q, float(k) - s, v): B = 1, H = 2, L = 150 (three tiles, the last one ragged),
    an outlier block in k, a zero row; rows past L are zero rows (codes 0, scale byte 1), not -s; Q and V bytes are the unshifted call's."""
    B, L, Hh = 1, 150, 2
    g = torch.Generator().manual_seed(150)
    q, k, v = (torch.randn(B, L, Hh, 128, generator=g) for _ in range(3))
    s = torch.randn(B, Hh * 128, generator=g) * 3.0
    k = k + s.view(B, 1, Hh, 128)
    k[0, 77, 1, 32:64] *= 37.0
    k[0, L - 1] = 0.0
    q, k, v = (t.to(BF).cuda() for t in (q, k, v))
    got = _bytes(H.attn_fp8_pack(q, k, v, _filled_buffers(H, B, Hh, L), k_shift=s.cuda()))
    want = R.pack_bytes(q.cpu(), S.shifted_k(k, s), v.cpu(), tail=R.FILL)
    for what, a, b in zip(("q8", "qs", "kv8"), got, want):
        assert a.shape == b.shape
        assert torch.equal(a, b), f"{what}: {int((a != b).sum())} bytes differ, the first at {(a != b).nonzero()[0].tolist()}"
    codes, scales = R.k_record_inv(got[2][:, :, -1:], 64)          # the last tile: keys 128 .. 191, real ones up to 149
    assert int(codes[:, L - 128:].max()) == 0 and int(scales[:, L - 128:].min()) == 1 == int(scales[:, L - 128:].max())
    plain = _bytes(H.attn_fp8_pack(q, k, v, _filled_buffers(H, B, Hh, L)))
    assert torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])
    assert torch.equal(plain[2][..., R.REC_V:R.REC_KS], got[2][..., R.REC_V:R.REC_KS]) and torch.equal(plain[2][..., R.REC_VS:], got[2][..., R.REC_VS:])
    assert not torch.equal(plain[2][..., :R.REC_V], got[2][..., :R.REC_V])
    with pytest.raises(RuntimeError, match="k_shift must be"):
        H.attn_fp8_pack(q, k, v, k_shift=s.cuda().double())
    with pytest.raises(RuntimeError, match="k_shift needs its k"):
        H.attn_fp8_pack(None, None, v, k_shift=s.cuda())


# ----------------------------------------------------------------------------- (d) attention on data with an offset in K
def _rows(L, seed, n=48):
    if L <= 320:
        return list(range(L))
    g = torch.Generator().manual_seed(seed)
    fixed = {0, 1, 31, 32, 63, 64, 255, 256, L - 65, L - 64, L - 2, L - 1}
    return sorted(fixed | set(torch.randint(0, L, (n,), generator=g).tolist()))


@pytest.mark.parametrize("B,Hh,L", [(1, 2, 300), (2, 3, 1111)])
def test_attention_on_an_offset_in_k(H, B, Hh, L):
    """offset_case (an offset ~ N(0, 8^2) per head and channel in K), the default split plan.  With k_shift = k_mean(k) the kernel's
    output is the restatement's on float(k) - mean_gpu, within REL_RMS after both are rounded to bf16; against exact attention it is
    within the format's 6.5e-2, and the unshifted call is at least twice as far.
    Measured on an MI355X: L = 300 (plan (1, 4)): 6.4e-4 from the restatement, smooth 5.43e-2, plain 2.13e-1 (the CPU restatement's own
    figures); B = 2, H = 3, L = 1111 (plan (2, 0)): 1.06e-3, 5.38e-2, 2.26e-1."""
    q, k, v = (t.cuda() for t in S.offset_case(B, Hh, L, seed=L))
    mean = H.k_mean(k.view(B * L, Hh * 128), None, None, None, L)
    assert float((mean.double().cpu().view(B, 1, Hh, 128) - S.token_mean(k.cpu())).abs().max()) <= float(S.k_mean_bound(k.double().abs().max().cpu(), -(-L // H.k_mean_parts(L)), H.k_mean_parts(L), False))
    smooth = H.attn_fwd_fp8(H.attn_fp8_pack(q, k, v, k_shift=mean), L).float().cpu()
    plain = H.attn_fwd_fp8(H.attn_fp8_pack(q, k, v), L).float().cpu()
    rows = _rows(L, L)
    Sp, from_unit = H.attn_split_plan(B * Hh, L, L, H.num_cus())
    want = MX.attention(q, S.shifted_k(k, mean), v, rows, kv_splits=Sp, split_from_unit=from_unit if Sp > 1 else None).float().to(BF).float()
    exact = MX.attention(q, k, v, rows, quant=False)
    rel = S.rel_rms(smooth[:, rows], want)
    e_smooth, e_plain = S.rel_rms(smooth[:, rows], exact), S.rel_rms(plain[:, rows], exact)
    print(f"B={B} H={Hh} L={L} plan {(Sp, from_unit)}: vs restatement {rel:.2e}; vs exact attention: smooth {e_smooth:.3e}, plain {e_plain:.3e}")
    assert torch.isfinite(smooth).all() and rel <= REL_RMS
    assert e_smooth <= S.FORMAT_BOUND
    assert e_plain >= 2 * e_smooth


# ----------------------------------------------------------------------------- (e) the attention() seam
def test_attention_seam_reads_the_switch(H, monkeypatch):
    """attention(q, k, v, attention_type="SAGE_ATTENTION"): with FLEXAM_SAGE_SMOOTH_K=1 the hand-made chain k_mean -> shifted pack -> MXFP8
    attention, bit for bit, and not what the switch off gives; off (and unset): the unshifted chain, bit for bit."""
    from flexam_amd.attention_utils import attention
    B, Hh, L = 1, 2, 300
    q, k, v = (t.cuda() for t in S.offset_case(B, Hh, L))
    q = (q.float() / (128 ** -0.5 * S.LOG2E)).to(BF)             # attention() applies softmax_scale * log2 e itself
    qs = (q.float() * (128 ** -0.5 * S.LOG2E)).to(BF)
    chain_off = H.attn_fwd_fp8(H.attn_fp8_pack(qs, k, v), L)
    chain_on = H.attn_fwd_fp8(H.attn_fp8_pack(qs, k, v, k_shift=H.k_mean(k.view(B * L, Hh * 128), None, None, None, L)), L)
    with torch.no_grad():
        monkeypatch.delenv("FLEXAM_SAGE_SMOOTH_K", raising=False)
        unset = attention(q, k, v, attention_type="SAGE_ATTENTION")
        monkeypatch.setenv("FLEXAM_SAGE_SMOOTH_K", "0")
        off = attention(q, k, v, attention_type="SAGE_ATTENTION")
        monkeypatch.setenv("FLEXAM_SAGE_SMOOTH_K", "1")
        on = attention(q, k, v, attention_type="SAGE_ATTENTION")
        flash = attention(q, k, v, attention_type="FLASH_ATTENTION")
    assert torch.equal(unset, chain_off) and torch.equal(off, chain_off)
    assert torch.equal(on, chain_on) and not torch.equal(on, off)
    assert torch.equal(flash, H.attn_fwd(q, k, v))                # the switch belongs to the quantised kernel alone


# ----------------------------------------------------------------------------- (f), (g) the engine
def _model(cfg, sd):
    from flexam_amd.wan_transformer3d_FlexAM import Wan2_2Transformer3DModel_FlexAM
    kw = dict(cfg)
    kw.pop("eps")
    m = Wan2_2Transformer3DModel_FlexAM(**kw)
    m.load_state_dict(sd, strict=True)
    return m.to("cuda:0")


def _forward(m, dcase, smooth, sage=True, replay=None):
    """One forward under the given switches -> (output on the CPU, sage_smooth_taken, replay_taken)."""
    env = {"VIDEOX_ATTENTION_TYPE": "SAGE_ATTENTION" if sage else None, "FLEXAM_SAGE_SMOOTH_K": smooth, "FLEXAM_REPLAY": replay}
    saved = {k: os.environ.get(k) for k in env}
    try:
        for k, val in env.items():
            os.environ.pop(k, None) if val is None else os.environ.__setitem__(k, val)
        out = m(**dcase).float().cpu()
    finally:
        for k, val in saved.items():
            os.environ.pop(k, None) if val is None else os.environ.__setitem__(k, val)
    e = m.engine()
    assert bool(e.sage_taken) == sage
    return out, bool(e.sage_smooth_taken), bool(e.replay_taken)


def _switch_and_replay_checks(m, dcase):
    """The checks (f) and (g) share: the switch is taken and changes the output; a replayed forward and a FLEXAM_REPLAY=0 forward equal
    the recording one bit for bit; flipping the switch between forwards of one clip takes effect both ways (the plan key).
    -> (plain, smoothed)."""
    plain, taken, _ = _forward(m, dcase, None)
    assert not taken
    on, taken, replayed = _forward(m, dcase, "1")
    assert taken and not replayed                                  # the unsmoothed plan is there and is NOT what ran
    assert not torch.equal(on, plain)
    again, taken, replayed = _forward(m, dcase, "1")
    assert taken and replayed and torch.equal(again, on)
    direct, taken, replayed = _forward(m, dcase, "1", replay="0")
    assert taken and not replayed and torch.equal(direct, on)
    off, taken, replayed = _forward(m, dcase, "0")
    assert not taken and replayed and torch.equal(off, plain)
    back, taken, replayed = _forward(m, dcase, "1")
    assert taken and replayed and torch.equal(back, on)
    return plain, on


def _stats(got, want):
    rel = float((got - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt())
    return rel, C.psnr(got, want)


@functools.lru_cache(maxsize=None)
def _five_b():
    """(cfg, state dict, case, case on the GPU) of the one-layer model at the 5B width on the config-1 latent [2, 48, 3, 16, 16]: made
    once, shared by the tests below and not modified by them."""
    cfg = dict(O.DIT_5B, num_layers=1)
    case = C.dit_case(cfg, 17)
    dcase = {k: ([u.cuda() for u in v] if isinstance(v, list) else (v.cuda() if torch.is_tensor(v) else v)) for k, v in case.items()}
    return cfg, C.dit_weights(cfg, 13), case, dcase


def test_engine_fused_producer_at_24_heads():
    """A one-layer model at the 5B width (24 heads: k_mean from the raw k -> the shifted fused producer -> V pack) on the config-1 latent,
    SAGE_ATTENTION on.  The switch is taken, the smoothed output differs from the unsmoothed one and meets the quantised variant's
    tolerance against the fp32 oracle (rel-RMS 2.5e-2, PSNR 38 dB, tests/test_full_width_gpu.py); replay and the plan key as
    _switch_and_replay_checks says.  Measured on an MI355X: plain 4.065e-3 / 65.6 dB, smoothed 4.057e-3 / 65.7 dB."""
    cfg, sd, case, dcase = _five_b()
    m = _model(cfg, sd)
    plain, on = _switch_and_replay_checks(m, dcase)
    assert m.engine().nh == 24 and m.engine().fused
    with torch.no_grad():
        want = O.dit_forward(sd, cfg, **case)
    for what, out in (("plain", plain), ("smoothed", on)):
        rel, p = _stats(out, want)
        print(f"one-layer 5B-width model, MXFP8 self-attention, {what}: rel-rms {rel:.3e}, psnr {p:.1f} dB")
    rel, p = _stats(on, want)
    assert rel <= 2.5e-2 and p >= 38.0


@pytest.mark.parametrize("bias,logit_std,ratio", [(8.0, None, 1.0), (32.0, 32.0, 2.0)], ids=["bias-8", "bias-32-logits-restored"])
def test_engine_with_a_bias_in_k(bias, logit_std, ratio):
    """The same model with a self_attn.k.bias ~ N(0, (bias s)^2), s = the std of Wk x for unit-variance x (what the LayerNorm in front
    hands the projection; the modulation's 1 + scale left out): plain and smoothed SAGE against the bf16-kernel forward of THAT model,
    plain >= ratio x smoothed.
    bias-8, smoothed <= plain.  Measured on an MI355X: plain 1.639e-3, smoothed 1.567e-3 -- within 10 % of each other, and a larger
    bias ALONE does not part them (64 s: 1.631e-3 / 1.562e-3): the bias sits in FRONT of WanRMSNorm, which holds the row's RMS at 1, so
    the offset grows at the expense of the keys' own part -- the logits between tokens shrink to N(0, 1/8^2), the softmax flattens and
    K's quantisation error stops mattering either way.
    bias-32-logits-restored, plain >= 2 x smoothed: what it takes is the offset BESIDE keys that still tell tokens apart, as in the
    restatement's data: the bias at 32 s and norm_q / norm_k scaled by oracle.cases.scale_self_attention_logits(sd, 32), which puts the
    keys' own logits back at ~N(0, 1): plain 5.10e-2, smoothed 2.30e-2 (at 8 s and 8: 1.06e-2 / 5.80e-3, ratio 1.8; without a bias at
    logit_std 8: 1.83e-2 / 1.76e-2, nothing to remove and nothing lost)."""
    cfg, sd, _, dcase = _five_b()
    sd2 = {k: v.clone() for k, v in sd.items()}
    wk = sd2["blocks.0.self_attn.k.weight"].float()
    s = float(wk.pow(2).sum(dim=1).mean().sqrt())
    sd2["blocks.0.self_attn.k.bias"] = torch.randn(wk.shape[0], generator=torch.Generator().manual_seed(8)) * (bias * s)
    if logit_std is not None:
        C.scale_self_attention_logits(sd2, logit_std)
    m = _model(cfg, sd2)
    base, _, _ = _forward(m, dcase, None, sage=False)
    plain, _, _ = _forward(m, dcase, None)
    on, taken, _ = _forward(m, dcase, "1")
    assert taken
    e_plain, e_on = S.rel_rms(plain, base), S.rel_rms(on, base)
    print(f"k.bias {bias:g} x std(Wk x) = {bias * s:.3f}, logit_std {logit_std}: against the bf16-kernel forward, plain {e_plain:.3e}, smoothed {e_on:.3e}")
    assert e_plain >= ratio * e_on


def test_engine_general_form_at_2_heads():
    """The tiny model (dim 256, 2 heads: rmsnorm_rope -> k_mean of the normed K as given -> the shifted pack): the switch is taken, changes
    the output, and the replay / plan-key checks of the 24-head test hold.  Measured on an MI355X against the fp32 oracle: plain
    4.524e-3 / 66.2 dB, smoothed 4.485e-3 / 66.3 dB."""
    cfg = dict(O.DIT_TINY)
    sd = C.dit_weights(cfg, 7)
    case = C.dit_case(cfg, 41)
    dcase = {k: ([u.cuda() for u in v] if isinstance(v, list) else (v.cuda() if torch.is_tensor(v) else v)) for k, v in case.items()}
    m = _model(cfg, sd)
    plain, on = _switch_and_replay_checks(m, dcase)
    assert m.engine().nh == 2 and m.engine().fused
    with torch.no_grad():
        want = O.dit_forward(sd, cfg, **case)
    for what, out in (("plain", plain), ("smoothed", on)):
        rel, p = _stats(out, want)
        print(f"tiny model, MXFP8 self-attention, {what}: rel-rms {rel:.3e}, psnr {p:.1f} dB")
    assert _stats(on, want)[1] >= 38.0
