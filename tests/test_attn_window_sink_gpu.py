"""GPU: windowed self-attention with a sink -- the first `sink` keys visible to every query -- in the HIP kernel (attn_window_kernel of
csrc/attn.hip with AttnParams::win_sink, flexam_attn_fwd_window_sink) from the kernel call up to the model's window_sink.

Exact cases (tests/attn_window_sink_cases.py; tests/test_attn_window_sink_cases_cpu.py proves that one key too many or too few at either
edge of the window or at the sink of any row moves that row by 35 bf16 ulps or more, and that the cases reach one-run and two-run query
blocks): scores of 0 and 1 in exp2 units, V of 0 and 1, so the output is the float64 masked attention rounded once to bf16 -- every
element within ONE bf16 ulp, through both forms of the kernel (scale in kernel with softmax_scale = log 2; pre-scaled q).  Then the
byte-for-byte normalisations of attn_run, a strided output, random data against fp32 masked attention at the bound
tests/test_attn_window_gpu.py applies (2 bf16 ulps + 6e-3), the model (fused engine, launch plans, re-bound blocks against the oracle with
its self-attention masked by the same rule; the SAGE fallback and the sequence-parallel refusals unchanged) and the C ABI's errors.

Measured on an MI355X, max |err| / ulp per exact case in the order of CASES (recorded, not asserted; correct rounding gives at most 0.5;
both forms alike): 0.498, 0.499, 0.498, 0.499, 0.467, 0.499, 0.495, 0.498, 0.470; strided output 0.499; no element more than 1 ulp off.
Random data: max |err| 1.1e-3 (both forms).  Model: the sink moves the oracle's output by rel-rms 5.6e-2 against the window alone (window
(40, 40), that of tests/test_attn_window_gpu.py: no narrower one was needed for 3 x the model tolerance); HIP against the masked oracle rel-rms 4.2e-3, 66.7 dB, fused and re-bound.
256 tokens are one query block, so the model tests exercise no gap between runs of tiles: the kernel cases do."""
import math
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_sink_cases as S  # noqa: E402
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
    for c in S.CASES:
        q, k, v = c.inputs()
        out[c.name] = (q, k, v, c.want(q, k, v))
    return out


def _kw(prescaled):
    return dict(softmax_scale=None if prescaled else LN2, prescaled=prescaled)


FORMS = pytest.mark.parametrize("prescaled", [False, True], ids=["scale-in-kernel", "prescaled"])


@FORMS
@pytest.mark.parametrize("case", S.CASES, ids=S.ids(S.CASES))
def test_exact_cases(H, exact, case, prescaled):
    q, k, v, want = exact[case.name]
    got = H.attn_fwd_window(*_dev(q, k, v), case.window, sink=case.sink, **_kw(prescaled))
    torch.cuda.synchronize()
    _check(f"{case.name} [{'prescaled' if prescaled else 'scale in kernel'}]", got, want)


@FORMS
def test_normalisations_are_byte_for_byte_the_launches_they_name(H, exact, prescaled):
    q, k, v, _ = exact["L600-w100_37-s70-b2h3"]
    qd, kd, vd = _dev(q, k, v)
    kw = _kw(prescaled)
    windowed = H.attn_fwd_window(qd, kd, vd, (100, 37), **kw)
    assert torch.equal(H.attn_fwd_window(qd, kd, vd, (100, 37), sink=0, **kw), windowed)
    for sink in (1, 70, 599):                                  # nothing lies to the left of a window without a left bound
        assert torch.equal(H.attn_fwd_window(qd, kd, vd, (-1, 37), sink=sink, **kw), H.attn_fwd_window(qd, kd, vd, (-1, 37), **kw)), sink
    plain = H.attn_fwd(qd, kd, vd, kv_splits=1, **kw)
    for sink in (600, 609, 5000):                              # the sink holds every key
        assert torch.equal(H.attn_fwd_window(qd, kd, vd, (100, 37), sink=sink, **kw), plain), sink
    for window in ((-1, -1), (599, 599), (-1, 5000)):          # no bound on either side, whatever the sink
        for sink in (1, 70):
            assert torch.equal(H.attn_fwd_window(qd, kd, vd, window, sink=sink, **kw), plain), (window, sink)
    # one key more for the rows past 100: the sink does reach the kernel
    one = H.attn_fwd_window(qd, kd, vd, (100, 37), sink=1, **kw)
    assert not torch.equal(one, windowed) and torch.equal(one[:, :101], windowed[:, :101]) and not torch.equal(one[:, 101:], windowed[:, 101:])
    assert not torch.equal(H.attn_fwd_window(qd, kd, vd, (100, 37), sink=599, **kw), plain)


def test_strided_output_leaves_the_rest_of_the_buffer_alone(H, exact):
    """out= a row and column slice of a larger buffer; L = 1111 has a ragged last query block and three blocks whose tiles have a gap."""
    case = S.CASES[1]
    assert S.GAP_BLOCKS[1] == 3 and case.L % S.Q_BLOCK
    q, k, v, want = exact[case.name]
    big = torch.full((1, case.L + 7, 3 * 2 * 128), -768.0, device="cuda", dtype=BF)
    out = big[:, 3:3 + case.L, 256:512].unflatten(2, (2, 128))
    H.attn_fwd_window(*_dev(q, k, v), case.window, out=out, prescaled=True, sink=case.sink)
    torch.cuda.synchronize()
    _check("sink 192, strided out", out, want)
    rest = big.clone()
    rest[:, 3:3 + case.L, 256:512] = -768.0
    assert bool((rest == -768.0).all())


def _masked_fp32(q, k, v, window, sink, scale=None):
    """fp32 masked attention [B, L, H, 128] of bf16 inputs, natural softmax with scale (default 1 / sqrt(128))."""
    q, k, v = (t.float().transpose(1, 2) for t in (q, k, v))
    s = q @ k.transpose(-1, -2) * (128 ** -0.5 if scale is None else scale)
    s = s.masked_fill(~S.allowed(s.shape[-1], window, sink).to(s.device), float("-inf"))
    return (s.softmax(-1) @ v).transpose(1, 2)


@pytest.fixture(scope="module")
def random_case():
    g = torch.Generator().manual_seed(1500)
    return tuple(torch.randn(1, 1500, 2, 128, generator=g).to(BF) for _ in range(3))


@FORMS
def test_random_data_against_fp32_masked_attention(H, random_case, prescaled):
    """L = 1500, H = 2, window (448, 448), sink 448: one latent frame either side, the leading frame always visible; N(0, 1) data."""
    q, k, v = random_case
    if prescaled:
        qs = (q.float() * (128 ** -0.5 * 1.4426950408889634)).to(BF)
        want = _masked_fp32(qs, k, v, (448, 448), 448, scale=0.6931471805599453)          # of the q the kernel was given
        got = H.attn_fwd_window(qs.cuda(), k.cuda(), v.cuda(), (448, 448), prescaled=True, sink=448)
    else:
        want = _masked_fp32(q, k, v, (448, 448), 448)
        got = H.attn_fwd_window(q.cuda(), k.cuda(), v.cuda(), (448, 448), sink=448)
    _assert_bf16_close(got, want, 2.0, 6e-3, "windowed attention with a sink, random data")


# ----------------------------------------------------------------------------- the model
WINDOW, SINK = (40, 40), 64            # DIT_TINY: 256 tokens, the first 64 are the reference image


def _build(cfg, seed, window, sink):
    from flexam_amd.wan_transformer3d_FlexAM import Wan2_2Transformer3DModel_FlexAM
    kw = dict(cfg)
    kw.pop("eps")
    m = Wan2_2Transformer3DModel_FlexAM(**kw, window_size=window, window_sink=sink)
    m.load_state_dict(C.dit_weights(cfg, seed), strict=True)
    return m.to("cuda:0")


def _oracle(sd, cfg, case, window, sink):
    """The oracle's forward with its self-attention masked by the rule (cross-attention calls the same function: told apart by Lq == Lk)."""
    plain = O.attention

    def masked(q, k, v, k_lens=None):
        if q.shape[1] != k.shape[1]:
            return plain(q, k, v, k_lens)
        assert k_lens is None and q.shape[1] > window[0] + window[1] + 1 + sink
        qt, kt, vt = (u.float().transpose(1, 2) for u in (q, k, v))
        s = qt @ kt.transpose(-1, -2) / q.shape[-1] ** 0.5
        s = s.masked_fill(~S.allowed(q.shape[1], window, sink), float("-inf"))
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
    sd = C.dit_weights(cfg, 7)
    want, window_only = _oracle(sd, cfg, case, WINDOW, SINK), _oracle(sd, cfg, case, WINDOW, 0)
    moved = float((want - window_only).pow(2).mean().sqrt() / window_only.pow(2).mean().sqrt())
    print(f"oracle: the sink moves the output by rel-rms {moved:.3e} against the window alone")
    assert moved > 3 * REL_RMS, moved                              # the sink shows at the tolerance
    return cfg, case, want, window_only


def test_model_with_a_window_and_a_sink_matches_the_masked_oracle(tiny):
    cfg, case, want, _ = tiny
    m = _build(cfg, 7, WINDOW, SINK)
    assert m.config["window_sink"] == SINK and m.window_sink == SINK and all(b.self_attn.window_sink == SINK for b in m.blocks)
    assert not hasattr(m.blocks[0].cross_attn, "window_sink")
    d = _to_dev(case)
    first = m(**d).clone()
    assert m.engine().fused and m.engine().window == WINDOW and m.engine().window_sink == SINK and not m.engine().replay_taken
    _check_model(first, want, "fused engine, window (40, 40), sink 64")
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
    _check_model(out, want, "re-bound blocks, window (40, 40), sink 64")


def test_the_sink_is_part_of_the_plan_key(tiny):
    cfg, case, want, window_only = tiny
    d = _to_dev(case)
    a, b = _build(cfg, 7, WINDOW, SINK), _build(cfg, 7, WINDOW, 0)
    out_a, out_b = a(**d).clone(), b(**d).clone()
    _check_model(out_a, want, "window (40, 40), sink 64")
    _check_model(out_b, window_only, "window (40, 40), no sink")
    assert not torch.equal(out_a, out_b)
    eng = a.engine()
    assert torch.equal(a(**d), out_a) and eng.replay_taken
    eng.window_sink = 0                                           # a new plan, never the other sink's launches
    assert torch.equal(a(**d), out_b) and not eng.replay_taken
    eng.window_sink = SINK
    assert torch.equal(a(**d), out_a) and eng.replay_taken


def test_a_sink_without_a_window_does_nothing(tiny):
    cfg, case, _, _ = tiny
    d = _to_dev(case)
    assert torch.equal(_build(cfg, 7, (-1, -1), SINK)(**d), _build(cfg, 7, (-1, -1), 0)(**d))


def test_sage_switch_with_a_window_and_a_sink_runs_the_bf16_windowed_kernel(tiny, monkeypatch):
    from flexam_amd.dit_engine import DiTEngine
    cfg, case, _, _ = tiny
    d = _to_dev(case)
    base = _build(cfg, 7, WINDOW, SINK)(**d).clone()
    monkeypatch.setenv("VIDEOX_ATTENTION_TYPE", "SAGE_ATTENTION")
    monkeypatch.setattr(DiTEngine, "_sage_window_warned", False)
    m2 = _build(cfg, 7, WINDOW, SINK)
    with pytest.warns(RuntimeWarning, match="window_size") as rec:
        out = m2(**d)
        m2(**d)
    assert len([w for w in rec if "window_size" in str(w.message)]) == 1          # the one warning
    assert not m2.engine().sage_taken and torch.equal(out, base)


def test_sequence_parallelism_with_a_window_and_a_sink_is_refused(tiny):
    from flexam_amd.dist import sequence_parallel_context
    cfg, case, _, _ = tiny
    m = _build(cfg, 7, WINDOW, SINK)
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
    from flexam_amd.wan_transformer3d_FlexAM import Wan2_2Transformer3DModel_FlexAM
    E_ARG, E_SHAPE = abi.CONSTANTS["FLEXAM_E_ARG"], abi.CONSTANTS["FLEXAM_E_SHAPE"]
    lib = H.load_library()
    q = torch.zeros(1, 64, 2, 128, dtype=BF, device="cuda")
    o = torch.empty_like(q)
    s = torch.cuda.current_stream().cuda_stream

    def new(qp, kp, vp, op, L=64, hd=128, sink=5):
        return lib.flexam_attn_fwd_window_sink(qp, 64 * 256, 256, kp, 64 * 256, 256, vp, 64 * 256, 256, op, 64 * 256, 256, 1, 2, L, hd, 0.1, 3, 2, sink, s)

    def old(qp, kp, vp, op, L=64, hd=128):
        return lib.flexam_attn_fwd_window(qp, 64 * 256, 256, kp, 64 * 256, 256, vp, 64 * 256, 256, op, 64 * 256, 256, 1, 2, L, hd, 0.1, 3, 2, s)

    def both(*args, **kw):
        """(status, message) of the new entry point, held to the old one's."""
        a = (old(*args, **kw), lib.flexam_last_error())
        b = (new(*args, **kw), lib.flexam_last_error())
        assert a == b, (a, b)
        return b
    p = q.data_ptr()
    assert new(p, p, p, o.data_ptr()) == 0 and new(p, p, p, o.data_ptr(), sink=0) == 0 and new(p, p, p, o.data_ptr(), sink=1000) == 0
    for sink in (-1, -448):
        assert new(p, p, p, o.data_ptr(), sink=sink) == E_ARG and b"sink" in lib.flexam_last_error()
    for args in ((None, p, p, o.data_ptr()), (p, None, p, o.data_ptr()), (p, p, None, o.data_ptr()), (p, p, p, None)):
        st, msg = both(*args)
        assert st == E_ARG and b"null pointer" in msg
    st, msg = both(p, p, p, o.data_ptr(), hd=64)
    assert st == E_SHAPE and b"head_dim" in msg
    st, msg = both(p + 2, p, p, o.data_ptr())
    assert st == E_ARG and b"misaligned" in msg
    with pytest.raises(RuntimeError, match="sink"):
        H.attn_fwd_window(q, q, q, (3, 2), sink=-1)
    torch.cuda.synchronize()
    kw = dict(O.DIT_TINY)
    kw.pop("eps")
    with pytest.raises(ValueError, match="window_sink"):
        Wan2_2Transformer3DModel_FlexAM(**kw, window_size=(40, 40), window_sink=-1)
    assert Wan2_2Transformer3DModel_FlexAM(**kw, window_sink=64).config["window_sink"] == 64      # accepted without a window
