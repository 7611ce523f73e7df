"""GPU: windowed self-attention with the window counted in frames -- query i sees the frames i // T - a .. i // T + b whole, and the first
`sink` keys -- in the HIP kernel (attn_window_kernel of csrc/attn.hip with AttnParams::win_frame, flexam_attn_fwd_window_frames) from the
kernel call up to the model's window_frames.

Exact cases (tests/attn_window_frames_cases.py; tests/test_attn_window_frames_cases_cpu.py proves that one key too many or too few at
either end of any row's range moves that row by 15.8 bf16 ulps or more, and that the cases reach one-run and two-run query blocks, frames
below, at and above a key tile and above a query block, ragged last frames and blocks): scores of 0 and 1 in exp2 units, V of 0 and 1, so
the output is the float64 masked attention rounded once to bf16 -- every element within ONE bf16 ulp, through both forms of the kernel
(scale in kernel with softmax_scale = log 2; pre-scaled q).  Then the byte-for-byte identities of attn_run's normalisations, a strided
output, random data against fp32 masked attention at the bound tests/test_attn_window_gpu.py and tests/test_attn_window_sink_gpu.py apply
(2 bf16 ulps + 6e-3), the model (fused engine, launch plans, re-bound blocks against the oracle with its self-attention masked by the same
rule; the SAGE fallback, the sequence-parallel refusals, the refusal of a sequence that is not whole frames) and the C ABI's errors.

The model tests: DIT_TINY's grid has 64 tokens per frame, exactly one key tile, and 256 tokens, one query block.  They pin the plumbing
(constructor to kernel call, T from the grid, the plan key), NOT the mask inside a tile: the exact cases pin the mask.

Measured on an MI355X, max |err| / ulp per exact case in the order of CASES (recorded, not asserted; correct rounding gives at most 0.5;
both forms alike): 0.467, 0.495, 0.409, 0.467, 0.470, 0.487, 0.462, 0.333, 0.495, 0.493, 0.470, 0.480; strided output 0.480; no element
more than 1 ulp off.  Random data: max |err| 8.2e-4 (scale in kernel) / 9.1e-4 (pre-scaled).  Model (self-attention logits at a standard
deviation of 3, see LOGIT_STD): removing the mask moves the oracle's output by rel-rms 7.2e-2; HIP against the masked oracle rel-rms
4.5e-3, 66.2 dB, fused and re-bound."""
import math
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_frames_cases as F  # noqa: E402
from test_attn_window_gpu import REL_RMS, _assert_bf16_close, _check, _check_model, _dev, _to_dev  # noqa: E402
from oracle import cases as C  # noqa: E402
from oracle import dit as O  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LN2 = math.log(2.0)


@pytest.fixture(scope="module")
def H():
    from flexam_amd import hip
    hip.load_library()
    return hip


@pytest.fixture(scope="module")
def exact():
    """Inputs and float64 reference of every case, computed once."""
    out = {}
    for c in F.CASES:
        q, k, v = c.inputs()
        out[c.name] = (q, k, v, c.want(q, k, v))
    return out


def _kw(prescaled):
    return dict(softmax_scale=None if prescaled else LN2, prescaled=prescaled)


FORMS = pytest.mark.parametrize("prescaled", [False, True], ids=["scale-in-kernel", "prescaled"])


@FORMS
@pytest.mark.parametrize("case", F.CASES, ids=F.ids(F.CASES))
def test_exact_cases(H, exact, case, prescaled):
    q, k, v, want = exact[case.name]
    got = H.attn_fwd_window(*_dev(q, k, v), case.window, sink=case.sink, frame_tokens=case.T, **_kw(prescaled))
    torch.cuda.synchronize()
    _check(f"{case.name} [{'prescaled' if prescaled else 'scale in kernel'}]", got, want)


@FORMS
def test_identities_are_byte_for_byte(H, exact, prescaled):
    q, k, v, _ = exact["L600-f1_0-T100-s70-b2h3"]
    qd, kd, vd = _dev(q, k, v)
    kw = _kw(prescaled)
    run = lambda window, T, sink=0: H.attn_fwd_window(qd, kd, vd, window, sink=sink, frame_tokens=T, **kw)
    # frame_tokens = 0 is the token-window call
    assert torch.equal(run((100, 37), 0), H.attn_fwd_window(qd, kd, vd, (100, 37), **kw))
    assert torch.equal(run((100, 37), 0, 70), H.attn_fwd_window(qd, kd, vd, (100, 37), sink=70, **kw))
    # frames of one token: the same mask and the same walk as the token window
    for window, sink in (((100, 37), 0), ((100, 37), 70), ((3, 0), 1), ((0, 200), 64), ((-1, 0), 0), ((0, -1), 0)):
        assert torch.equal(run(window, 1, sink), H.attn_fwd_window(qd, kd, vd, window, sink=sink, **kw)), (window, sink)
    # one frame that holds every key, no bound on either side (as given, or because it reaches the first and the last frame from every
    # row), a sink that holds every key: flexam_attn_fwd
    plain = H.attn_fwd(qd, kd, vd, kv_splits=1, **kw)
    for window, T, sink in (((0, 0), 600, 0), ((1, 0), 601, 70), ((0, 0), 5000, 0), ((-1, -1), 100, 0), ((-1, -1), 100, 70), ((5, 5), 100, 0),
                            ((5, -1), 100, 70), ((1, 1), 300, 0), ((1, 0), 100, 600), ((0, 0), 100, 5000)):
        assert torch.equal(run(window, T, sink), plain), (window, T, sink)
    # nothing lies to the left of a window without a left bound: the sink is dropped
    for sink in (1, 70, 599):
        assert torch.equal(run((-1, 0), 100, sink), run((-1, 0), 100)), sink
    # a window one frame narrower differs, and only in the rows whose window changed: on the left the rows of frame 0 have none to lose
    # (and the sink shows the rows of frame 1 the 70 keys of frame 0 they keep: they change too, by the 30 they lose)
    wide = run((1, 0), 100, 70)
    assert not torch.equal(wide, plain)
    narrow = run((0, 0), 100, 70)
    assert torch.equal(narrow[:, :100], wide[:, :100])
    assert all(not torch.equal(narrow[:, f * 100:(f + 1) * 100], wide[:, f * 100:(f + 1) * 100]) for f in range(1, 6))
    right = run((1, 1), 100, 70)                                  # on the right the rows of the last frame have none to gain
    assert torch.equal(right[:, 500:], wide[:, 500:])
    assert all(not torch.equal(right[:, f * 100:(f + 1) * 100], wide[:, f * 100:(f + 1) * 100]) for f in range(5))


def test_strided_output_leaves_the_rest_of_the_buffer_alone(H, exact):
    """out= a row and column slice of a larger buffer; L = 1111 has a ragged last query block, T = 37 frames that straddle every tile and
    block boundary, and three blocks whose tiles have a gap behind the sink."""
    case = F.CASES[11]
    assert (case.L, case.T, F.GAP_BLOCKS[11]) == (1111, 37, 3) and case.L % F.Q_BLOCK
    q, k, v, want = exact[case.name]
    big = torch.full((1, case.L + 7, 3 * 2 * 128), -768.0, device="cuda", dtype=BF)
    out = big[:, 3:3 + case.L, 256:512].unflatten(2, (2, 128))
    H.attn_fwd_window(*_dev(q, k, v), case.window, out=out, prescaled=True, sink=case.sink, frame_tokens=case.T)
    torch.cuda.synchronize()
    _check("frames of 37, sink 300, strided out", out, want)
    rest = big.clone()
    rest[:, 3:3 + case.L, 256:512] = -768.0
    assert bool((rest == -768.0).all())


def _masked_fp32(q, k, v, ok, scale=None):
    """fp32 masked attention [B, L, H, 128] of bf16 inputs, natural softmax with scale (default 1 / sqrt(128))."""
    q, k, v = (t.float().transpose(1, 2) for t in (q, k, v))
    s = q @ k.transpose(-1, -2) * (128 ** -0.5 if scale is None else scale)
    s = s.masked_fill(~ok.to(s.device), float("-inf"))
    return (s.softmax(-1) @ v).transpose(1, 2)


@pytest.fixture(scope="module")
def random_case():
    g = torch.Generator().manual_seed(1500)
    return tuple(torch.randn(1, 1500, 2, 128, generator=g).to(BF) for _ in range(3))


@FORMS
def test_random_data_against_fp32_masked_attention(H, random_case, prescaled):
    """L = 1500, H = 2, frames of 448 tokens (the last one ragged), one frame either side, the leading frame always visible; N(0, 1) data."""
    q, k, v = random_case
    ok = F.allowed(1500, (1, 1), 448, 448)
    if prescaled:
        qs = (q.float() * (128 ** -0.5 * 1.4426950408889634)).to(BF)
        want = _masked_fp32(qs, k, v, ok, scale=0.6931471805599453)          # of the q the kernel was given
        got = H.attn_fwd_window(qs.cuda(), k.cuda(), v.cuda(), (1, 1), prescaled=True, sink=448, frame_tokens=448)
    else:
        want = _masked_fp32(q, k, v, ok)
        got = H.attn_fwd_window(q.cuda(), k.cuda(), v.cuda(), (1, 1), sink=448, frame_tokens=448)
    _assert_bf16_close(got, want, 2.0, 6e-3, "attention windowed in frames with a sink, random data")


# ----------------------------------------------------------------------------- the model
FRAMES, SINK, T_TINY = (1, 0), 64, 64            # DIT_TINY: 256 tokens in 4 frames of 8 x 8, the first is the reference image
# The seeded weights give self-attention logits ~N(0, 1): rows so flat that hiding half of the keys moves the oracle's output by rel-rms
# 3.1e-2 only (3.0e-2 to 3.5e-2 over other seeds, 4.1e-2 with 8 frames), under 3 x the model tolerance.  With the logits at a standard
# deviation of 3 (oracle.cases.scale_self_attention_logits; the benchmark's peaked-rows line uses 6) a row rests on fewer keys and the
# mask moves the output by 7.2e-2 -- worked out on the oracle alone, on the CPU.
LOGIT_STD = 3.0


def _weights(cfg):
    sd = C.dit_weights(cfg, 7)
    C.scale_self_attention_logits(sd, LOGIT_STD)
    return sd


def _build(cfg, sd, frames, sink=0):
    from flexam_amd.wan_transformer3d_FlexAM import Wan2_2Transformer3DModel_FlexAM
    kw = dict(cfg)
    kw.pop("eps")
    m = Wan2_2Transformer3DModel_FlexAM(**kw, window_frames=frames, window_sink=sink)
    m.load_state_dict(sd, strict=True)
    return m.to("cuda:0")


def _oracle(sd, cfg, case, ok):
    """The oracle's forward with its self-attention masked by `ok` [L, L], None = no mask (cross-attention calls the same function:
    told apart by Lq == Lk)."""
    plain = O.attention

    def masked(q, k, v, k_lens=None):
        if q.shape[1] != k.shape[1] or ok is None:
            return plain(q, k, v, k_lens)
        assert k_lens is None and q.shape[1] == ok.shape[0]
        qt, kt, vt = (u.float().transpose(1, 2) for u in (q, k, v))
        s = qt @ kt.transpose(-1, -2) / q.shape[-1] ** 0.5
        s = s.masked_fill(~ok, float("-inf"))
        return (s.softmax(-1) @ vt).transpose(1, 2)

    mp = pytest.MonkeyPatch()
    mp.setattr(O, "attention", masked)
    try:
        return O.dit_forward(sd, cfg, **case)
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def tiny():
    cfg = dict(O.DIT_TINY)
    case = C.dit_case(cfg, 41)
    sd = _weights(cfg)
    want = _oracle(sd, cfg, case, F.allowed(256, FRAMES, T_TINY, SINK))
    other = _oracle(sd, cfg, case, F.allowed(256, (0, 0), T_TINY, 0))
    unmasked = _oracle(sd, cfg, case, None)
    moved = float((want - unmasked).pow(2).mean().sqrt() / unmasked.pow(2).mean().sqrt())
    print(f"oracle: removing the mask moves the output by rel-rms {moved:.3e}")
    assert moved > 3 * REL_RMS, moved                              # the mask shows at the tolerance
    return cfg, case, want, other, sd


def test_model_with_a_frame_window_and_a_sink_matches_the_masked_oracle(tiny):
    """Fused engine; launch plans (the second call is replayed and bit-equal); re-bound blocks.  64 tokens per frame are one key tile:
    this pins the plumbing, the exact cases pin the mask inside a tile."""
    cfg, case, want, _, sd = tiny
    m = _build(cfg, sd, FRAMES, SINK)
    assert tuple(m.config["window_frames"]) == FRAMES and all(b.self_attn.window_frames == FRAMES and b.self_attn.window_sink == SINK for b in m.blocks)
    assert not hasattr(m.blocks[0].cross_attn, "window_frames")
    d = _to_dev(case)
    first = m(**d).clone()
    eng = m.engine()
    assert eng.fused and eng.window == (-1, -1) and eng.window_frames == FRAMES and eng.window_sink == SINK and not eng.replay_taken
    assert eng._window_frames() == (FRAMES, T_TINY)
    _check_model(first, want, "fused engine, window_frames (1, 0), sink 64")
    second = m(**d).clone()                                       # served from the launch plan
    assert m.engine().replay_taken and torch.equal(first, second)
    calls = {"n": 0}

    def delegating(self, x, seq_lens, grid_sizes, freqs, dtype=torch.bfloat16, t=0):
        calls["n"] += 1
        return type(self).forward(self, x, seq_lens, grid_sizes, freqs, dtype, t=t)
    for blk in m.blocks:
        blk.self_attn.forward = types.MethodType(delegating, blk.self_attn)
    out = m(**d)
    assert calls["n"] == len(m.blocks) and not m.engine().fused
    _check_model(out, want, "re-bound blocks, window_frames (1, 0), sink 64")


def test_the_frame_window_is_part_of_the_plan_key(tiny):
    """Two models sharing weights but differing in window_frames do not replay each other's plan."""
    cfg, case, want, other, sd = tiny
    d = _to_dev(case)
    a, b = _build(cfg, sd, FRAMES, SINK), _build(cfg, sd, (0, 0), 0)
    out_a, out_b = a(**d).clone(), b(**d).clone()
    _check_model(out_a, want, "window_frames (1, 0), sink 64")
    _check_model(out_b, other, "window_frames (0, 0), no sink")
    assert not torch.equal(out_a, out_b)
    eng = a.engine()
    assert torch.equal(a(**d), out_a) and eng.replay_taken
    eng.window_frames, eng.window_sink = (0, 0), 0                # a new plan, never the other window's launches
    assert torch.equal(a(**d), out_b) and not eng.replay_taken
    eng.window_frames, eng.window_sink = FRAMES, SINK
    assert torch.equal(a(**d), out_a) and eng.replay_taken


def test_sage_switch_with_a_frame_window_runs_the_bf16_windowed_kernel(tiny, monkeypatch):
    from flexam_amd.dit_engine import DiTEngine
    cfg, case, _, _, sd = tiny
    d = _to_dev(case)
    base = _build(cfg, sd, FRAMES, SINK)(**d).clone()
    monkeypatch.setenv("VIDEOX_ATTENTION_TYPE", "SAGE_ATTENTION")
    monkeypatch.setenv("FLEXAM_SAGE_SMOOTH_K", "1")
    monkeypatch.setenv("FLEXAM_SAGE_SMOOTH_V", "1")
    monkeypatch.setattr(DiTEngine, "_sage_window_warned", False)
    m2 = _build(cfg, sd, FRAMES, SINK)
    with pytest.warns(RuntimeWarning, match="window_frames") as rec:
        out = m2(**d)
        m2(**d)
    assert len([w for w in rec if "window_frames" in str(w.message)]) == 1          # the one warning
    eng = m2.engine()
    assert not eng.sage_taken and not eng._smooth_k and not eng._smooth_v and torch.equal(out, base)


def test_sequence_parallelism_and_ragged_frames_are_refused(tiny):
    from flexam_amd.dist import sequence_parallel_context
    cfg, case, _, _, sd = tiny
    m = _build(cfg, sd, FRAMES, SINK)
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
    # a sequence that is not whole frames: 120 tokens on a grid of 64 per frame; and seq_lens shorter than the sequence
    with pytest.raises(NotImplementedError, match="120.*64"):
        sa(torch.zeros(1, 120, cfg["dim"], device="cuda"), None, [[2, 8, 8]], m.freqs)
    with pytest.raises(NotImplementedError, match="seq_lens"):
        sa(torch.zeros(1, 128, cfg["dim"], device="cuda"), torch.tensor([100]), [[2, 8, 8]], m.freqs)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the C ABI
def test_abi_argument_errors(H):
    from flexam_amd import abi
    E_ARG, E_SHAPE = abi.CONSTANTS["FLEXAM_E_ARG"], abi.CONSTANTS["FLEXAM_E_SHAPE"]
    lib = H.load_library()
    q = torch.zeros(1, 64, 2, 128, dtype=BF, device="cuda")
    o = torch.empty_like(q)
    s = torch.cuda.current_stream().cuda_stream

    def new(qp, kp, vp, op, L=64, hd=128, T=7, sink=5):
        return lib.flexam_attn_fwd_window_frames(qp, 64 * 256, 256, kp, 64 * 256, 256, vp, 64 * 256, 256, op, 64 * 256, 256, 1, 2, L, hd, 0.1, 3, 2, T, sink, s)

    def old(qp, kp, vp, op, L=64, hd=128):
        return lib.flexam_attn_fwd_window_sink(qp, 64 * 256, 256, kp, 64 * 256, 256, vp, 64 * 256, 256, op, 64 * 256, 256, 1, 2, L, hd, 0.1, 3, 2, 5, s)

    def both(*args, **kw):
        """(status, message) of the new entry point, held to its sibling's."""
        a = (old(*args, **kw), lib.flexam_last_error())
        b = (new(*args, **kw), lib.flexam_last_error())
        assert a == b, (a, b)
        return b
    p = q.data_ptr()
    assert new(p, p, p, o.data_ptr()) == 0 and new(p, p, p, o.data_ptr(), sink=0) == 0 and new(p, p, p, o.data_ptr(), sink=1000) == 0
    assert new(p, p, p, o.data_ptr(), T=1) == 0 and new(p, p, p, o.data_ptr(), T=64) == 0 and new(p, p, p, o.data_ptr(), T=1 << 30) == 0
    for T in (0, -1):
        assert new(p, p, p, o.data_ptr(), T=T) == E_ARG and b"frame_tokens" in lib.flexam_last_error()
    for sink in (-1, -448):
        assert new(p, p, p, o.data_ptr(), sink=sink) == E_ARG and b"sink" in lib.flexam_last_error()
    for args in ((None, p, p, o.data_ptr()), (p, None, p, o.data_ptr()), (p, p, None, o.data_ptr()), (p, p, p, None)):
        st, msg = both(*args)
        assert st == E_ARG and b"null pointer" in msg
    st, msg = both(p, p, p, o.data_ptr(), hd=64)
    assert st == E_SHAPE and b"head_dim" in msg
    st, msg = both(p + 2, p, p, o.data_ptr())
    assert st == E_ARG and b"misaligned" in msg
    with pytest.raises(RuntimeError, match="frame_tokens"):
        H.attn_fwd_window(q, q, q, (1, 1), frame_tokens=-3)
    with pytest.raises(RuntimeError, match="sink"):
        H.attn_fwd_window(q, q, q, (1, 1), sink=-1, frame_tokens=7)
    torch.cuda.synchronize()
