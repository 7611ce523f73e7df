"""GPU: the windowed MXFP8 self-attention (flexam_attn_fwd_fp8_window: attn8_window_kernel / attn8_window_oshift_kernel of
csrc/attn_fp8.inc; FLEXAM_SAGE_WINDOW=1) from the kernel call up to the model, against tests/mxfp8_window_restatement.py.

(a) Integer cases (WR.integer_case: operands that pack losslessly, integer scores, every p a power of two; what is left is fp32
    accumulation of sums without cancellation and the output's bf16 rounding): EVERY element of EVERY row within 1 bf16 ulp of the
    windowed restatement.  tests/test_attn_fp8_window_cpu.py shows that a mask one key off moves these operands' rows by 8 ulps or more,
    that the edge rows of the narrow window carry their maximum on their last visible key with 2^32 times its weight on the key
    behind it, and that rows of (100, 37) at L = 600 start two tiles or more behind their unit and still reach the rd = 96 cap.
(b) Random data (unit-variance logits) against the restatement at the bound of tests/test_attn_fp8_restated_gpu.py, rel-RMS <= 3.2e-3,
    whose smallest support is 40 keys per row: only windows in which every row sees 40 keys or more (asserted).  The rel-RMS against
    exact masked attention is printed beside it, without a bound.
(c) Normalisations (bytes of hip.attn_fwd_fp8 at kv_splits = 1; a sink under a window without a left bound is dropped) and the ABI's
    argument errors.
(d) The tiny model of tests/test_attn_window_gpu.py with window_size = (L/4, L/4), with a sink, and with window_frames, under
    SAGE_ATTENTION and FLEXAM_SAGE_WINDOW=1: sage_taken, no window warning, replay on and off alike, not the bf16 windowed forward,
    and rel-RMS against it at most TWICE that of the unwindowed SAGE forward against the unwindowed bf16 forward, measured in the same
    module (a row that averages over a quarter of the keys averages the e4m3 error over a quarter of the terms: at most sqrt(4) more);
    smooth-K and smooth-V on top stay within it; the module seam too.  attention() with the switch on is hip.attn_fwd_fp8 with the
    window, bit for bit, and with it off what it returned before.

Measured on an MI355X (recorded, not asserted): (a) max |err| / ulp 0.51 .. 0.55 over the 17 cases, no element more than 1 ulp off.
(b) rel-RMS against the restatement 7.7e-4 .. 1.2e-3, against exact masked attention 5.3e-2 (the format's error).  The logits are
unit-variance, as the bound's cases of 40 keys are: at sharpness 3 a row rests on a handful of keys, one e4m3 code of a dominant p
that falls on the other side of a rounding midpoint moves its whole row by 6 %, and the figure is a count of such rare events -- four
seeds each gave 1.2e-3 .. 3.6e-3 at (200, 100) / L = 1111 and 8.8e-4 .. 6.5e-3 at (100, 39) / L = 600, the unwindowed kernel at L = 100
and 300 5.5e-4 .. 1.6e-3, and the restatement against itself with 2^-20 relative noise on the scores 1.1e-4 .. 9.0e-3 over six seeds (the largest unwindowed).
(d) SAGE windowed against bf16 windowed 3.27e-3 / 3.19e-3 / 3.22e-3 (window, with sink, frames; the seam within 1 %), unwindowed SAGE
against unwindowed bf16 2.86e-3; with smooth-K 3.23e-3 / 3.18e-3 / 3.20e-3, with smooth-V 3.24e-3 / 3.19e-3 / 3.16e-3."""
import os
import sys
import types
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp8_window_restatement as WR  # noqa: E402
from oracle import cases as C  # noqa: E402
from oracle import dit as O  # noqa: E402
from test_attn_fp8_gpu import _inputs  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
REL_RMS = 3.2e-3            # tests/test_attn_fp8_restated_gpu.py


@pytest.fixture(scope="module")
def H():
    from flexam_amd import hip
    hip.load_library()
    return hip


def _run(H, q, k, v, window, sink=0, T=0, o_shift=None):
    return H.attn_fwd_fp8(H.attn_fp8_pack(q, k, v), q.shape[1], window=window, sink=sink, frame_tokens=T, o_shift=o_shift)


# ----------------------------------------------------------------------------- (a) integer scores
INTEGER_CASES = [
    # name, B, H, L, window, sink, frame tokens, with o_shift
    ("L70-tokens-3_2", 2, 3, 70, (3, 2), 0, 0, False),                  # one ragged tile; the maximum on the last visible key
    ("L70-tokens-3_2-sink5", 1, 2, 70, (3, 2), 5, 0, False),
    ("L70-causal", 1, 2, 70, (-1, 0), 0, 0, False),
    ("L70-anticausal", 1, 2, 70, (0, -1), 0, 0, False),
    ("L70-frames-1_1-T7-sink5", 1, 2, 70, (1, 1), 5, 7, False),
    ("L70-frames-0_0-T7", 1, 2, 70, (0, 0), 0, 7, False),
    ("L70-frames-block-causal-T7", 1, 2, 70, (-1, 0), 0, 7, False),
    ("L600-100_37-sink70", 2, 3, 600, (100, 37), 70, 0, False),         # a sink edge inside a tile; window rows behind the sink tiles
    ("L600-100_37-oshift", 1, 2, 600, (100, 37), 0, 0, True),           # rows that start late and reach the cap; the output shift
    ("L1111-200_100-sink192", 1, 2, 1111, (200, 100), 192, 0, False),   # a unit of 10 tiles: the 4-unrolled main loop runs
    ("L1111-64_64-sink128", 1, 2, 1111, (64, 64), 128, 0, False),       # a gap between the sink tiles and the window tiles
    ("L600-causal-sink70-dropped", 1, 2, 600, (-1, 0), 70, 0, False),   # no left bound: units that grow, the sink dropped
    ("L1111-frames-2_1-T64", 1, 2, 1111, (2, 1), 0, 64, False),         # tile-aligned frames
    ("L1111-frames-0_0-T200-sink128", 1, 2, 1111, (0, 0), 128, 200, False),
    ("L1111-frames-block-causal-T200", 1, 2, 1111, (-1, 0), 0, 200, False),
    ("L600-frames-1_1-T48", 1, 2, 600, (1, 1), 0, 48, False),           # frame boundaries inside tiles
    ("L600-frames-0_0-T48", 1, 2, 600, (0, 0), 0, 48, False),
]


@pytest.mark.parametrize("name,B,Hh,L,window,sink,T,shifted", INTEGER_CASES, ids=[c[0] for c in INTEGER_CASES])
def test_integer_scores_within_one_bf16_ulp_of_the_windowed_restatement(H, name, B, Hh, L, window, sink, T, shifted):
    q, k, v = (t.to(BF).cuda() for t in WR.integer_case(B, Hh, L, window, L + sink + T, T))
    shift = None
    if shifted:          # whole numbers of the channel's own sign: nothing cancels in O / l + shift
        sign = torch.sign(v[0, 0].float()).reshape(1, Hh * 128)
        shift = (sign * (1 + torch.arange(Hh * 128, device="cuda") % 5).float()).expand(B, -1).contiguous()
    got = _run(H, q, k, v, window, sink, T, shift).double().cpu()
    ok = WR.mask(L, window, 0 if window[0] < 0 else sink, T)          # (a window without a left bound drops the sink)
    want = WR.attention(q, k, v, ok)
    if shifted:
        want = want + shift.double().cpu().view(B, 1, Hh, 128)
    err = (got - want).abs() / WR.bf16_ulp(want)
    bad = ~(err <= 1.0)                                                # (a NaN is bad)
    print(f"{name}: max |err| / ulp {float(err.nan_to_num(float('inf')).max()):.3f}, elements off by more than 1 ulp: {int(bad.sum())}")
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.numel()} elements more than 1 bf16 ulp from the restatement; first at "
                           f"(b, row, head, channel) = {bad.nonzero()[0].tolist()}: got {float(got[bad][0])}, want {float(want[bad][0])}")


# ----------------------------------------------------------------------------- (b) random data
RANDOM_CASES = [(1, 2, 600, (100, 39), 0, 0, 1.0), (1, 2, 1111, (200, 100), 192, 0, 1.0), (2, 3, 600, (100, 37), 70, 0, 1.0),
                (1, 2, 1111, (2, 1), 0, 64, 1.0), (1, 2, 600, (1, 1), 0, 48, 1.0)]


@pytest.mark.parametrize("B,Hh,L,window,sink,T,sharp", RANDOM_CASES)
def test_random_data_against_the_windowed_restatement(H, B, Hh, L, window, sink, T, sharp):
    ok = WR.mask(L, window, sink, T)
    assert int(ok.sum(dim=1).min()) >= 40                              # the support the bound was set at
    q, k, v = _inputs(B, Hh, L, 300 + L + T, sharp=sharp)
    got = _run(H, q, k, v, window, sink, T).float().cpu()
    want = WR.attention(q, k, v, ok).float().to(BF).float()
    rel = float((got - want).norm() / want.norm())
    exact = WR.masked_softmax(q, k, v, ok).float()
    print(f"B={B} H={Hh} L={L} window={window} sink={sink} T={T} sharp={sharp}: rel-RMS vs restatement {rel:.2e}; vs exact masked attention "
          f"{float((got - exact).norm() / exact.norm()):.2e}")
    assert torch.isfinite(got).all() and rel <= REL_RMS


# ----------------------------------------------------------------------------- (c) normalisations, argument errors
def test_normalisations_are_the_launches_they_name(H):
    L = 600
    q, k, v = _inputs(2, 3, L, 11)
    bufs = H.attn_fp8_pack(q, k, v)
    plain = H.attn_fwd_fp8(bufs, L, kv_splits=1)
    lib, s = H.load_library(), torch.cuda.current_stream().cuda_stream

    def raw(left, right, sink, T, shift=None):
        out = torch.empty_like(plain)
        rc = lib.flexam_attn_fwd_fp8_window(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), out.data_ptr(), out.stride(0), out.stride(1),
                                            2, 3, L, 128, left, right, sink, T, None if shift is None else shift.data_ptr(), s)
        assert rc == 0, lib.flexam_last_error()
        return out
    assert torch.equal(raw(-1, -1, 0, 0), plain) and torch.equal(raw(-1, -1, 70, 48), plain)          # no bound
    assert torch.equal(raw(L - 1, L, 0, 0), plain)                                                     # both sides reach past the sequence
    assert torch.equal(H.attn_fwd_fp8(bufs, L, window=(3, 2), sink=L), plain)                          # the sink holds every key
    assert torch.equal(H.attn_fwd_fp8(bufs, L, window=(0, 0), frame_tokens=L), plain)                  # one frame holds every key
    assert not torch.equal(H.attn_fwd_fp8(bufs, L, window=(0, 0), frame_tokens=L - 1), plain)
    shift = torch.randn(2, 3 * 128, device="cuda")
    assert torch.equal(raw(-1, -1, 0, 0, shift), H.attn_fwd_fp8(bufs, L, kv_splits=1, o_shift=shift))
    # a window without a left bound drops the sink
    assert torch.equal(H.attn_fwd_fp8(bufs, L, window=(-1, 0), sink=70), H.attn_fwd_fp8(bufs, L, window=(-1, 0)))
    assert torch.equal(H.attn_fwd_fp8(bufs, L, window=(-1, 0), sink=70, frame_tokens=48), H.attn_fwd_fp8(bufs, L, window=(-1, 0), frame_tokens=48))
    assert not torch.equal(H.attn_fwd_fp8(bufs, L, window=(100, 0), sink=70), H.attn_fwd_fp8(bufs, L, window=(100, 0)))
    with pytest.raises(RuntimeError, match="whole work units"):
        H.attn_fwd_fp8(bufs, L, kv_splits=2, window=(100, 37))


def test_abi_argument_errors(H):
    from flexam_amd import abi
    E_ARG, E_SHAPE = abi.CONSTANTS["FLEXAM_E_ARG"], abi.CONSTANTS["FLEXAM_E_SHAPE"]
    lib, s = H.load_library(), torch.cuda.current_stream().cuda_stream
    q8, qs, kv8 = H.attn_fp8_buffers(1, 2, 64, "cuda")
    o = torch.empty(1, 64, 2, 128, dtype=BF, device="cuda")

    def call(a=q8.data_ptr(), b=qs.data_ptr(), c=kv8.data_ptr(), op=o.data_ptr(), L=64, hd=128, left=3, right=2, sink=0, T=0):
        return lib.flexam_attn_fwd_fp8_window(a, b, c, op, o.stride(0), o.stride(1), 1, 2, L, hd, left, right, sink, T, None, s)
    assert call() == 0
    assert call(sink=-1) == E_ARG and b"sink" in lib.flexam_last_error()
    assert call(T=-1) == E_ARG and b"frame_tokens" in lib.flexam_last_error()
    for kw in (dict(a=None), dict(b=None), dict(c=None), dict(op=None)):
        assert call(**kw) == E_ARG and b"null pointer" in lib.flexam_last_error()
    assert call(a=q8.data_ptr() + 2) == E_ARG and b"misaligned" in lib.flexam_last_error()
    assert call(hd=64) == E_SHAPE and b"head_dim" in lib.flexam_last_error()
    assert call(L=0) == E_SHAPE and b"empty problem" in lib.flexam_last_error()
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- (d) the seam and the model
def test_attention_seam_takes_the_windowed_mxfp8_launch_only_with_the_switch(H, monkeypatch):
    from flexam_amd.attention_utils import attention
    L, window = 600, (100, 37)
    q, k, v = (t * s for t, s in zip(_inputs(2, 3, L, 21), (8.0, 1.0, 1.0)))          # (attention() applies head_dim^-0.5 itself)
    scale = 128 ** -0.5 * 1.4426950408889634
    monkeypatch.delenv("VIDEOX_ATTENTION_TYPE", raising=False)
    with torch.no_grad():
        bf16 = H.attn_fwd_window(q, k, v, window)
        monkeypatch.delenv("FLEXAM_SAGE_WINDOW", raising=False)
        assert torch.equal(attention(q, k, v, window_size=window, attention_type="SAGE_ATTENTION"), bf16)      # what it returns today
        monkeypatch.setenv("FLEXAM_SAGE_WINDOW", "1")
        want = H.attn_fwd_fp8(H.attn_fp8_pack((q.float() * scale).to(BF), k, v), L, window=window)
        assert torch.equal(attention(q, k, v, window_size=window, attention_type="SAGE_ATTENTION"), want) and not torch.equal(want, bf16)
        assert torch.equal(attention(q, k, v, causal=True, attention_type="SAGE_ATTENTION"),
                           H.attn_fwd_fp8(H.attn_fp8_pack((q.float() * scale).to(BF), k, v), L, window=(-1, 0)))
        assert torch.equal(attention(q, k, v, window_size=window), bf16)               # the switch alone asks for nothing
        assert torch.equal(attention(q, k, v, window_size=window, attention_type="FLASH_ATTENTION"), bf16)
    assert torch.equal(attention(q, k, v, window_size=window, attention_type="SAGE_ATTENTION"), bf16)          # with grad: the bf16 kernel


def _build(cfg, sd, **mask):
    from flexam_amd.wan_transformer3d_FlexAM import Wan2_2Transformer3DModel_FlexAM
    kw = dict(cfg)
    kw.pop("eps")
    m = Wan2_2Transformer3DModel_FlexAM(**kw, **mask)
    m.load_state_dict(sd, strict=True)
    return m.to("cuda:0")


def _rebind(m):
    """The reference's multi-GPU hook point: re-bound self-attention forwards make the blocks run as modules."""
    def delegating(self, x, seq_lens, grid_sizes, freqs, dtype=torch.bfloat16, t=0):
        return type(self).forward(self, x, seq_lens, grid_sizes, freqs, dtype, t=t)
    for blk in m.blocks:
        blk.self_attn.forward = types.MethodType(delegating, blk.self_attn)


def _rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


SWITCHES = ("VIDEOX_ATTENTION_TYPE", "FLEXAM_SAGE_WINDOW", "FLEXAM_SAGE_SMOOTH_K", "FLEXAM_SAGE_SMOOTH_V", "FLEXAM_REPLAY")


@pytest.fixture(scope="module")
def tiny():
    """DIT_TINY (256 tokens: 4 frames of 8 x 8), its inputs on the device, and the yardstick of the model tests: the rel-RMS of the
    UNWINDOWED SAGE forward against the unwindowed bf16 forward, fused engine and module seam, on the paths the parent has."""
    cfg = dict(O.DIT_TINY)
    case = C.dit_case(cfg, 41)
    sd = C.dit_weights(cfg, 7)
    d = {k: ([u.cuda() for u in v] if isinstance(v, list) else (v.cuda() if torch.is_tensor(v) else v)) for k, v in case.items()}
    mp = pytest.MonkeyPatch()
    base = {}
    try:
        for name in SWITCHES:
            mp.delenv(name, raising=False)
        for seam in (False, True):
            outs = []
            for sage in (False, True):
                mp.setenv("VIDEOX_ATTENTION_TYPE", "SAGE_ATTENTION" if sage else "FLASH_ATTENTION")
                m = _build(cfg, sd)
                if seam:
                    _rebind(m)
                with torch.no_grad():
                    outs.append(m(**d).clone())
                assert m.engine().fused == (not seam) and (seam or m.engine().sage_taken == sage)
            base[seam] = _rel(outs[1], outs[0])
    finally:
        mp.undo()
    return cfg, sd, d, base


MASKS = [dict(window_size=(64, 64)), dict(window_size=(64, 64), window_sink=32), dict(window_frames=(1, 0))]


@pytest.mark.parametrize("mask", MASKS, ids=["window", "window-sink", "frames"])
def test_model_with_a_window_runs_the_windowed_mxfp8_kernel_under_the_switch(tiny, mask, monkeypatch):
    cfg, sd, d, base = tiny
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    with torch.no_grad():
        bf16 = _build(cfg, sd, **mask)(**d).clone()
        m_seam = _build(cfg, sd, **mask)
        _rebind(m_seam)
        bf16_seam = m_seam(**d).clone()
        monkeypatch.setenv("VIDEOX_ATTENTION_TYPE", "SAGE_ATTENTION")
        monkeypatch.setenv("FLEXAM_SAGE_WINDOW", "1")
        m = _build(cfg, sd, **mask)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            first = m(**d).clone()
            eng = m.engine()
            assert eng.fused and eng.sage_taken and not eng.replay_taken
            second = m(**d).clone()                                   # served from the launch plan
            assert eng.replay_taken and torch.equal(first, second)
            monkeypatch.setenv("FLEXAM_REPLAY", "0")
            third = m(**d).clone()
            assert not eng.replay_taken and eng.sage_taken and torch.equal(first, third)
            monkeypatch.delenv("FLEXAM_REPLAY")
            seam = m_seam(**d).clone()
            assert not m_seam.engine().fused
        assert not [str(w.message) for w in seen if "window" in str(w.message)]
        assert not torch.equal(first, bf16) and not torch.equal(seam, bf16_seam)
        rel, rel_seam = _rel(first, bf16), _rel(seam, bf16_seam)
        print(f"{mask}: SAGE windowed vs bf16 windowed rel-RMS {rel:.3e} (fused), {rel_seam:.3e} (seam); unwindowed SAGE vs bf16 "
              f"{base[False]:.3e} (fused), {base[True]:.3e} (seam)")
        assert rel <= 2 * base[False] and rel_seam <= 2 * base[True]
        for switch, taken in (("FLEXAM_SAGE_SMOOTH_K", "sage_smooth_taken"), ("FLEXAM_SAGE_SMOOTH_V", "sage_smooth_v_taken")):
            monkeypatch.setenv(switch, "1")
            out, out_seam = m(**d).clone(), m_seam(**d).clone()
            monkeypatch.delenv(switch)
            r, r_seam = _rel(out, bf16), _rel(out_seam, bf16_seam)
            print(f"{mask} + {switch}: rel-RMS {r:.3e} (fused), {r_seam:.3e} (seam)")
            assert eng.sage_taken and getattr(eng, taken) and not torch.equal(out, first)
            assert r <= 2 * base[False] and r_seam <= 2 * base[True]
