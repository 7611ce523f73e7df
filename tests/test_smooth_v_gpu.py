"""GPU: smooth-V behind FLEXAM_SAGE_SMOOTH_V=1 (csrc/attn_fp8.inc, csrc/attn.hip: flexam_attn_fp8_pack_shift_kv, flexam_attn_fwd_fp8_oshift)
against tests/smooth_v_restatement.py, from the kernels up to the three users of the MXFP8 self-attention: (a) the V-shifted pack byte for
byte, in all its forms; (b) attention on data with a channel offset in V, on both final writers (the kernel's epilogue and the split-KV
merge): the restatement's output, and the centred error the offset costs and the mean removes; (c) the attention() seam; (d) the DiT engine
at 24 heads (fused producer, V-only pack; and with a bias in V) and at 2 heads (general pack): the switch taken, the launch plan keyed on it,
replay bit for bit; (e) the register footprint of the new attention symbol."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mxfp8_restatement as MX  # noqa: E402
import rmsnorm_rope_mx_restatement as R  # noqa: E402
import smooth_k_restatement as SK  # noqa: E402  (k_mean_bound: the counted bound of flexam_k_mean)
import smooth_v_restatement as SV  # noqa: E402

from oracle import cases as C  # noqa: E402
from oracle import dit as O  # noqa: E402

pytestmark = pytest.mark.gpu
REL_RMS = 3.2e-3               # the kernel against its restatement, both rounded to bf16 (tests/test_smooth_k_gpu.py: the same arithmetic + one fp32 add)
# the same comparison after centring (the token mean of V taken out of both sides): twice the figure measured on an MI355X, by shape's L.
# Not derived: the two sides differ by rare bf16 rounding-boundary flips, each a whole ulp of the UNcentred element, which weigh more
# once the offset is gone from the denominator
CENTRED_REL_RMS = {300: 2 * 5.065e-3, 1111: 2 * 1.107e-2}
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


K_PART = (slice(0, R.REC_V), slice(R.REC_KS, R.REC_VS))           # the K image and the K scales of a record
V_PART = (slice(R.REC_V, R.REC_KS), slice(R.REC_VS, R.REC_END))   # the V^T image and the V scales


def _same(a, b, parts):
    return all(torch.equal(a[..., p], b[..., p]) for p in parts)


# ----------------------------------------------------------------------------- (a) the V-shifted pack
def test_v_shifted_pack_byte_for_byte(H):
    """attn_fp8_pack(q, k, v, v_shift=s) against pack_bytes(q, k, float(v) - s): B = 1, H = 2, L = 150 (three tiles, the last one ragged),
    an outlier block in v, a zero row.  V columns past L are zero codes, with scale byte 1 where a half tile holds no key at all, not -s;
    Q and K bytes are the unshifted call's; the V-only call writes the same V bytes and nothing else; both shifts together are the two
    shifts applied separately; what cannot be done is refused."""
    B, L, Hh = 1, 150, 2
    g = torch.Generator().manual_seed(151)
    q, k, v = (torch.randn(B, L, Hh, 128, generator=g) for _ in range(3))
    s = torch.randn(B, Hh * 128, generator=g) * 3.0
    ks = torch.randn(B, Hh * 128, generator=g) * 2.0
    v = v + s.view(B, 1, Hh, 128)
    v[0, 77, 1, 32:64] *= 37.0
    v[0, L - 1] = 0.0
    q, k, v = (t.to(BF).cuda() for t in (q, k, v))
    got = _bytes(H.attn_fp8_pack(q, k, v, _filled_buffers(H, B, Hh, L), v_shift=s.cuda()))
    want = R.pack_bytes(q.cpu(), k.cpu(), SV.shifted_v(v, s), tail=R.FILL)
    for what, a, b in zip(("q8", "qs", "kv8"), got, want):
        assert a.shape == b.shape
        assert torch.equal(a, b), f"{what}: {int((a != b).sum())} bytes differ, the first at {(a != b).nonzero()[0].tolist()}"
    codes, scales = R.v_record_inv(got[2])                         # [B, H, T, 64 keys, 128], [B, H, T, 128, 2 half tiles]
    assert int(codes[:, :, -1, L - 128:].max()) == 0               # the last tile: keys 128 .. 191, real ones up to 149
    assert int(scales[:, :, -1, :, 1].min()) == 1 == int(scales[:, :, -1, :, 1].max())
    plain = _bytes(H.attn_fp8_pack(q, k, v, _filled_buffers(H, B, Hh, L)))
    assert torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1]) and _same(plain[2], got[2], K_PART)
    assert not _same(plain[2], got[2], V_PART[:1])
    # the V-only call (the engine's fused producer writes Q and K itself)
    only = _bytes(H.attn_fp8_pack(None, None, v, _filled_buffers(H, B, Hh, L), v_shift=s.cuda()))
    assert _same(only[2], got[2], V_PART)
    assert bool((only[0] == R.FILL).all()) and bool((only[1] == R.FILL).all()) and all(bool((only[2][..., p] == R.FILL).all()) for p in K_PART)
    # both shifts: K as the K-shifted call writes it, V as the V-shifted one
    both = _bytes(H.attn_fp8_pack(q, k, v, _filled_buffers(H, B, Hh, L), k_shift=ks.cuda(), v_shift=s.cuda()))
    konly = _bytes(H.attn_fp8_pack(q, k, v, _filled_buffers(H, B, Hh, L), k_shift=ks.cuda()))
    assert torch.equal(both[0], got[0]) and torch.equal(both[1], got[1])
    assert _same(both[2], konly[2], K_PART) and _same(both[2], got[2], V_PART) and not _same(both[2], got[2], K_PART[:1])
    assert _same(konly[2], plain[2], V_PART)
    # refusals
    with pytest.raises(RuntimeError, match="v_shift must be"):
        H.attn_fp8_pack(q, k, v, v_shift=s.cuda().double())
    with pytest.raises(RuntimeError, match="v_shift must be"):
        H.attn_fp8_pack(q, k, v, v_shift=s.cuda()[:, :128])
    with pytest.raises(RuntimeError, match="v_shift must be"):
        H.attn_fp8_pack(q, k, v, v_shift=s)                        # on the CPU
    with pytest.raises(RuntimeError, match="k_shift must be"):
        H.attn_fp8_pack(q, k, v, k_shift=ks.cuda().view(-1), v_shift=s.cuda())
    with pytest.raises(RuntimeError, match="k_shift needs its k"):
        H.attn_fp8_pack(None, None, v, k_shift=ks.cuda(), v_shift=s.cuda())
    bufs = _filled_buffers(H, B, Hh, L)
    with pytest.raises(RuntimeError, match="needs its k"):         # the C side says the same
        H._call("flexam_attn_fp8_pack_shift_kv", None, 0, 0, None, 0, 0, H._ptr(v), v.stride(0), v.stride(1), *(H._raw(t) for t in bufs),
                B, Hh, L, 128, H._ptr(ks.cuda()), H._ptr(s.cuda()))
    with pytest.raises(RuntimeError, match="o_shift must be"):
        H.attn_fwd_fp8(bufs, L, o_shift=s.cuda().to(BF))
    with pytest.raises(RuntimeError, match="o_shift must be"):
        H.attn_fwd_fp8(bufs, L, o_shift=s.cuda().view(Hh, 128))


# ----------------------------------------------------------------------------- (b) attention on data with an offset in V
def _rows(L, seed, n=48):
    if L <= 320:
        return list(range(L))
    g = torch.Generator().manual_seed(seed)
    fixed = {0, 1, 31, 32, 63, 64, 255, 256, L - 65, L - 64, L - 2, L - 1}
    return sorted(fixed | set(torch.randint(0, L, (n,), generator=g).tolist()))


@pytest.mark.parametrize("B,Hh,L", [(1, 2, 300), (2, 3, 1111)])
def test_attention_on_an_offset_in_v(H, B, Hh, L):
    """offset_case_v (an offset ~ N(0, 4^2) per head and channel in V), the default split plan: L = 300 ends in the kernel's own epilogue,
    B = 2, H = 3, L = 1111 in the split-KV merge (plan (2, 0) on 256 CUs).  With v_shift = o_shift = k_mean(v) the kernel's output is
    the restatement's smooth_output rounded to bf16 within REL_RMS, and within CENTRED_REL_RMS once the token mean of V is taken out of
    both; against exact attention, e = the centred error and f = the floor of exact attention rounded to bf16,
    e_plain^2 - f^2 >= 4 (e_smooth^2 - f^2), as on the CPU.  With v_shift = o_shift = 0 the output is the plain call's, bit for bit.
    Measured on an MI355X.  L = 300 (plan (1, 4)): 9.51e-5 from the restatement, centred 5.065e-3; centred against exact attention smooth
    1.173e-1, plain 2.405e-1, floor 8.913e-2, ratio above the floor 8.59 (the CPU restatement's own figures).  B = 2, H = 3, L = 1111 (plan
    (2, 0), 60 rows): 1.06e-4, centred 1.107e-2; smooth 2.046e-1, plain 3.224e-1, floor 1.762e-1, ratio 6.74."""
    q, k, v = (t.cuda() for t in SV.offset_case_v(B, Hh, L, 4.0))
    mean = H.k_mean(v.view(B * L, Hh * 128), None, None, None, L)
    parts = H.k_mean_parts(L)
    assert float((mean.double().cpu().view(B, 1, Hh, 128) - SV.token_mean(v)).abs().max()) <= float(SK.k_mean_bound(v.double().abs().max().cpu(), -(-L // parts), parts, False))
    smooth = H.attn_fwd_fp8(H.attn_fp8_pack(q, k, v, v_shift=mean), L, o_shift=mean).float().cpu()
    plain_bf = H.attn_fwd_fp8(H.attn_fp8_pack(q, k, v), L)
    zero = torch.zeros_like(mean)
    assert torch.equal(H.attn_fwd_fp8(H.attn_fp8_pack(q, k, v, v_shift=zero), L, o_shift=zero), plain_bf)
    plain = plain_bf.float().cpu()
    rows = _rows(L, L)
    Sp, from_unit = H.attn_split_plan(B * Hh, L, L, H.num_cus())
    want = SV.bf16(SV.smooth_output(q, k, v, mean, rows, kv_splits=Sp, split_from_unit=from_unit if Sp > 1 else None))
    exact = MX.attention(q, k, v, rows, quant=False)
    rel = SV.rel_rms(smooth[:, rows], want)
    rel_c = SV.centred_error(smooth[:, rows], want, v)
    e_smooth, e_plain = SV.centred_error(smooth[:, rows], exact, v), SV.centred_error(plain[:, rows], exact, v)
    floor = SV.centred_error(SV.bf16(exact), exact, v)
    print(f"B={B} H={Hh} L={L} plan {(Sp, from_unit)}: vs restatement {rel:.2e}, centred {rel_c:.3e}; centred vs exact attention: "
          f"smooth {e_smooth:.3e}, plain {e_plain:.3e}, floor {floor:.3e}, ratio above the floor {SV.excess_ratio(e_plain, e_smooth, floor):.2f}")
    assert torch.isfinite(smooth).all() and rel <= REL_RMS
    assert rel_c <= CENTRED_REL_RMS[L]
    assert e_plain ** 2 - floor ** 2 >= 4 * (e_smooth ** 2 - floor ** 2)


# ----------------------------------------------------------------------------- (c) the attention() seam
def test_attention_seam_reads_the_switch(H, monkeypatch):
    """attention(q, k, v, attention_type="SAGE_ATTENTION"): with FLEXAM_SAGE_SMOOTH_V=1 the hand-made chain k_mean(v) -> V-shifted pack ->
    MXFP8 attention with the output shift, bit for bit, and not what the switch off gives; off (and unset): the unshifted chain; with
    FLEXAM_SAGE_SMOOTH_K=1 as well: the chain with both shifts.  FLASH_ATTENTION does not read the switch."""
    from flexam_amd.attention_utils import attention
    B, Hh, L = 1, 2, 300
    q, k, v = (t.cuda() for t in SV.offset_case_v(B, Hh, L, 4.0))
    q = (q.float() / (128 ** -0.5 * SV.LOG2E)).to(BF)            # attention() applies softmax_scale * log2 e itself
    qs = (q.float() * (128 ** -0.5 * SV.LOG2E)).to(BF)
    vm = H.k_mean(v.view(B * L, Hh * 128), None, None, None, L)
    km = H.k_mean(k.view(B * L, Hh * 128), None, None, None, L)
    chain_off = H.attn_fwd_fp8(H.attn_fp8_pack(qs, k, v), L)
    chain_v = H.attn_fwd_fp8(H.attn_fp8_pack(qs, k, v, v_shift=vm), L, o_shift=vm)
    chain_kv = H.attn_fwd_fp8(H.attn_fp8_pack(qs, k, v, k_shift=km, v_shift=vm), L, o_shift=vm)
    with torch.no_grad():
        monkeypatch.delenv("FLEXAM_SAGE_SMOOTH_K", raising=False)
        monkeypatch.delenv("FLEXAM_SAGE_SMOOTH_V", raising=False)
        unset = attention(q, k, v, attention_type="SAGE_ATTENTION")
        monkeypatch.setenv("FLEXAM_SAGE_SMOOTH_V", "0")
        off = attention(q, k, v, attention_type="SAGE_ATTENTION")
        monkeypatch.setenv("FLEXAM_SAGE_SMOOTH_V", "1")
        on = attention(q, k, v, attention_type="SAGE_ATTENTION")
        flash = attention(q, k, v, attention_type="FLASH_ATTENTION")
        monkeypatch.setenv("FLEXAM_SAGE_SMOOTH_K", "1")
        both = attention(q, k, v, attention_type="SAGE_ATTENTION")
    assert torch.equal(unset, chain_off) and torch.equal(off, chain_off)
    assert torch.equal(on, chain_v) and not torch.equal(on, off)
    assert torch.equal(both, chain_kv) and not torch.equal(both, on)
    assert torch.equal(flash, H.attn_fwd(q, k, v))                # the switch belongs to the quantised kernel alone


# ----------------------------------------------------------------------------- (d) the engine
def _model(cfg, sd):
    from flexam_amd.wan_transformer3d_FlexAM import Wan2_2Transformer3DModel_FlexAM
    kw = dict(cfg)
    kw.pop("eps")
    m = Wan2_2Transformer3DModel_FlexAM(**kw)
    m.load_state_dict(sd, strict=True)
    return m.to("cuda:0")


def _forward(m, dcase, smooth, sage=True, replay=None):
    """One forward under the given switches -> (output on the CPU, sage_smooth_v_taken, replay_taken)."""
    env = {"VIDEOX_ATTENTION_TYPE": "SAGE_ATTENTION" if sage else None, "FLEXAM_SAGE_SMOOTH_V": smooth, "FLEXAM_SAGE_SMOOTH_K": None,
           "FLEXAM_REPLAY": replay}
    saved = {k: os.environ.get(k) for k in env}
    try:
        for k, val in env.items():
            os.environ.pop(k, None) if val is None else os.environ.__setitem__(k, val)
        out = m(**dcase).float().cpu()
    finally:
        for k, val in saved.items():
            os.environ.pop(k, None) if val is None else os.environ.__setitem__(k, val)
    e = m.engine()
    assert bool(e.sage_taken) == sage and not e.sage_smooth_taken
    return out, bool(e.sage_smooth_v_taken), bool(e.replay_taken)


def _switch_and_replay_checks(m, dcase):
    """The switch is taken and changes the output; a replayed forward and a FLEXAM_REPLAY=0 forward equal the recording one bit for bit;
    flipping the switch between forwards of one clip takes effect both ways (the plan key).  -> (plain, smoothed)."""
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


def _on_gpu(case):
    return {k: ([u.cuda() for u in v] if isinstance(v, list) else (v.cuda() if torch.is_tensor(v) else v)) for k, v in case.items()}


@functools.lru_cache(maxsize=None)
def _five_b():
    """(cfg, state dict, case, case on the GPU) of the one-layer model at the 5B width on the config-1 latent [2, 48, 3, 16, 16]: made
    once, shared by the tests below and not modified by them."""
    cfg = dict(O.DIT_5B, num_layers=1)
    case = C.dit_case(cfg, 17)
    return cfg, C.dit_weights(cfg, 13), case, _on_gpu(case)


def test_engine_fused_producer_at_24_heads():
    """A one-layer model at the 5B width (24 heads: the fused producer writes Q and K, k_mean of the V columns -> the V-only shifted pack ->
    the attention with the output shift) on the config-1 latent, SAGE_ATTENTION on.  The switch is taken, the smoothed output differs
    from the unsmoothed one and meets the quantised variant's tolerance against the fp32 oracle (rel-RMS 2.5e-2, PSNR 38 dB); replay
    and the plan key as _switch_and_replay_checks says.  Measured on an MI355X: plain 4.065e-3 / 65.6 dB, smoothed 4.066e-3 / 65.6 dB
    (the oracle's weights put no offset into V: nothing to remove, nothing lost)."""
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


def test_engine_with_a_bias_in_v():
    """The same model with a self_attn.v.bias ~ N(0, (4 s)^2), s = the std of Wv x for unit-variance x (what the LayerNorm in front hands
    the projection; the modulation's 1 + scale left out) -- no norm follows V, so the bias IS a channel offset all keys share.  Plain and
    smoothed SAGE against the bf16-kernel forward of THAT model: smoothed <= plain.  No more is asserted: the ratio depends on how much
    of the model's output error the self-attention's V carries.  Measured on an MI355X (bias std 3.999): plain 3.794e-3, smoothed
    2.572e-3."""
    cfg, sd, _, dcase = _five_b()
    sd2 = {k: v.clone() for k, v in sd.items()}
    wv = sd2["blocks.0.self_attn.v.weight"].float()
    s = float(wv.pow(2).sum(dim=1).mean().sqrt())
    sd2["blocks.0.self_attn.v.bias"] = torch.randn(wv.shape[0], generator=torch.Generator().manual_seed(4)) * (4.0 * s)
    m = _model(cfg, sd2)
    base, _, _ = _forward(m, dcase, None, sage=False)
    plain, _, _ = _forward(m, dcase, None)
    on, taken, _ = _forward(m, dcase, "1")
    assert taken
    e_plain, e_on = SV.rel_rms(plain, base), SV.rel_rms(on, base)
    print(f"v.bias 4 x std(Wv x) = {4.0 * s:.3f}: against the bf16-kernel forward, plain {e_plain:.3e}, smoothed {e_on:.3e}")
    assert e_on <= e_plain


def test_engine_general_form_at_2_heads():
    """The tiny model (dim 256, 2 heads: rmsnorm_rope -> k_mean of the V columns -> the general pack with v_shift -> the attention with the
    output shift): the switch is taken, changes the output, the replay / plan-key checks of the 24-head test hold, and the smoothed
    output meets the same tolerance against the fp32 oracle.  Measured on an MI355X: plain 4.524e-3 / 66.2 dB, smoothed 4.537e-3 /
    66.2 dB."""
    cfg = dict(O.DIT_TINY)
    sd = C.dit_weights(cfg, 7)
    case = C.dit_case(cfg, 41)
    m = _model(cfg, sd)
    plain, on = _switch_and_replay_checks(m, _on_gpu(case))
    assert m.engine().nh == 2 and m.engine().fused
    with torch.no_grad():
        want = O.dit_forward(sd, cfg, **case)
    for what, out in (("plain", plain), ("smoothed", on)):
        rel, p = _stats(out, want)
        print(f"tiny model, MXFP8 self-attention, {what}: rel-rms {rel:.3e}, psnr {p:.1f} dB")
    rel, p = _stats(on, want)
    assert rel <= 2.5e-2 and p >= 38.0


# ----------------------------------------------------------------------------- (e) the new attention symbol
def test_the_oshift_kernel_is_there_and_fits_two_waves_per_simd():
    """tools/kernel_resources.py on the library the tests run: the MXFP8 kernel with the output shift is one symbol of its own -- its name
    holds neither `attn8_fwd_kernel` nor `attn_fwd_kernel`, whose counts tests/test_isa_resources_cpu.py pins -- with vgpr + agpr <= 256 at
    512 threads, and neither it nor the shifted pack and merge instances spill (that file's no-spill test covers them as it covers all)."""
    import kernel_resources as KR
    res = KR.kernel_resources()
    mine = {n: v for n, v in res.items() if "attn8_oshift_kernel" in n}
    assert len(mine) == 1, sorted(mine)
    (name, v), = mine.items()
    assert "attn8_fwd_kernel" not in name and "attn_fwd_kernel" not in name
    assert v["vgpr_count"] + v["agpr_count"] <= 256 and not v["vgpr_spill_count"] and not v["private_segment_fixed_size"], v
    for fam, n in (("attn8_pack_kernel", 4), ("attn_merge_kernel", 2)):
        inst = {k: r for k, r in res.items() if fam in k}
        assert len(inst) == n and not any(r["vgpr_spill_count"] or r["private_segment_fixed_size"] for r in inst.values()), inst
