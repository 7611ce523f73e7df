"""CPU: the windowed MXFP8 self-attention (FLEXAM_SAGE_WINDOW=1; flexam_attn_fwd_fp8_window, attn8_window_kernel) without a GPU.

(a) tests/mxfp8_window_restatement.py with quant=False is exact masked softmax attention (1e-12) on every case of the three windowed
    case modules, and can tell a mask that is off by one key from the right one: the yardstick of tests/test_attn_fp8_window_gpu.py.
(b) The integer operands of the GPU test do what their description says: a row that starts late reaches the rd = 96 cap counted from
    its own start, and a mask one key too wide or too narrow moves the result.
(c) The switch: dit_layout.sage_window_asked reads one variable, default off; DiTEngine._mode keeps `sage` under a window with it and
    replaces it (with the warning) without it; smooth-K and smooth-V stay as asked; the two modes differ.
(d) Header, binding and replay table name the entry point; the built library exports it and ships both kernels at 512 threads and at
    most 256 registers, without a spill or scratch."""
import os
import sys
import types
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import attn_window_cases as W  # noqa: E402
import attn_window_frames_cases as F  # noqa: E402
import attn_window_sink_cases as S  # noqa: E402
import mxfp8_window_restatement as WR  # noqa: E402

from flexam_amd import dit_layout as D  # noqa: E402
from flexam_amd.dit_engine import DiTEngine  # noqa: E402

# (case, window, sink, T): a token window is a frame window of one-token frames, which is how altered_masks takes it
ALL = ([(c, c.window, 0, 1) for c in W.CASES] + [(c, c.window, c.sink, 1) for c in S.CASES] + [(c, c.window, c.sink, c.T) for c in F.CASES])


# ----------------------------------------------------------------------------- (a) the restatement
@pytest.mark.parametrize("case,window,sink,T", ALL, ids=[c.name for c, *_ in ALL])
def test_unquantised_restatement_is_exact_masked_attention_and_sees_a_moved_boundary(case, window, sink, T):
    q, k, v = case.inputs()
    ok = F.allowed(case.L, window, T, sink)
    assert torch.equal(ok, WR.mask(case.L, window, sink, T if T > 1 else 0))
    want = WR.masked_softmax(q, k, v, ok)
    got = WR.attention(q, k, v, ok, quant=False)
    err = float((got - want).abs().max())
    assert err <= 1e-12, err
    if bool(ok.all()):
        return                                                 # (a sink or a window that holds every key: there is no boundary to move)
    moved = [name for name, m in F.altered_masks(case.L, window, T, sink)
             if not torch.equal(m, ok) and float((WR.attention(q, k, v, m, quant=False) - want).abs().max()) > 1e-6]
    assert moved, "no mask one key away changes the result: the case is blind"


# ----------------------------------------------------------------------------- (b) the integer operands of the GPU test
def _scores(L, window, seed, frame_tokens=0):
    q, k, v = (t.to(torch.bfloat16) for t in WR.integer_case(1, 1, L, window, seed, frame_tokens))
    assert all(torch.equal(t.float(), torch.round(t.float())) and float(t.abs().max()) <= 15 for t in (q, k, v))
    qd, kd, vd = WR.R.dequant_rows(q), WR.R.dequant_rows(k), WR.R.dequant_v(v)
    assert torch.equal(qd[0, 0], q[0, :, 0].double()) and torch.equal(kd[0, 0], k[0, :, 0].double()) and torch.equal(vd[0, 0], v[0, :, 0].double())
    return qd[0, 0] @ kd[0, 0].t(), vd[0, 0]                          # (the operands pack losslessly: integer scores)


def test_integer_operands_reach_the_cap_from_a_late_start():
    L, window = 600, (100, 37)
    s, v = _scores(L, window, 5)
    trace = {}
    WR.window_pass(s, v, WR.mask(L, window), trace=trace)
    rows = torch.arange(L)
    # rows of the second q block whose own first key lies two tiles or more behind the unit's first, 256 - 100, and which end at the cap
    late = (rows >= 256 + 128) & (rows < 512) & (trace["start_key"] >= 256) & (trace["rd"] == 96.0)
    assert int(late.sum()) >= 10, int(late.sum())
    assert float(trace["rd"].max()) == 96.0


@pytest.mark.parametrize("L,window,sink", [(70, (3, 2), 0), (600, (100, 37), 70)])
def test_integer_operands_show_a_mask_off_by_one(L, window, sink):
    s, v = _scores(L, window, 7)
    ok = WR.mask(L, window, sink)
    want = WR.window_pass(s, v, ok)
    rows = torch.arange(L)
    edge = rows % 3 == 1
    lo, hi = WR.row_ranges(L, window)
    if window[0] + window[1] < 63:         # the maximum of an edge row is on its last visible key, and the key behind it outweighs it by 2^32
        for i in rows[edge & (hi + 1 < L)].tolist():
            seen = s[i][ok[i]]
            assert float(s[i, hi[i]]) == 8.0 == float(seen.max()) and int((seen == 8.0).sum()) == 1 and float(s[i, hi[i] + 1]) == 40.0
    for name, m in F.altered_masks(L, window, 1, sink):
        other = WR.window_pass(s, v, m)
        changed = (m != ok).any(dim=1)
        ulps = ((other - want).abs() / WR.bf16_ulp(want)).amax(dim=1)
        if name.startswith("add") or window[0] + window[1] < 63:      # every edge row the move touches shows it, far beyond the GPU test's 1 ulp
            assert bool((changed & edge).any()) and float(ulps[changed & edge].min()) > 8.0, (name, float(ulps[changed & edge].min()))
        else:       # (a key dropped from a wide window weighs 2^-32 of an edge row's visible 40s: the ramp and noise rows show it)
            assert int((ulps[changed] > 8.0).sum()) >= 5, (name, int((ulps[changed] > 8.0).sum()))


# ----------------------------------------------------------------------------- (c) the switch and the mode
SAGE = {"VIDEOX_ATTENTION_TYPE": "SAGE_ATTENTION"}
SWITCHES = ("VIDEOX_ATTENTION_TYPE", "FLEXAM_SAGE_WINDOW", "FLEXAM_SAGE_SMOOTH_K", "FLEXAM_SAGE_SMOOTH_V", "FLEXAM_REPLAY", "FLEXAM_SHARE_BLOCK0",
            "FLEXAM_FP8_OPROJ", "FLEXAM_FP8_FFN_APRIORI")


def test_sage_window_asked_reads_one_switch_with_default_off():
    assert not D.sage_window_asked({}) and not D.sage_window_asked({"FLEXAM_SAGE_WINDOW": "0"}) and D.sage_window_asked({"FLEXAM_SAGE_WINDOW": "1"})
    assert not D.sage_window_asked(SAGE) and not D.sage_window_asked({"FLEXAM_SAGE_SMOOTH_K": "1", "FLEXAM_SAGE_SMOOTH_V": "1"})


def _engine(**window):
    p = D.SINGLE_RANK
    return types.SimpleNamespace(fused=True, nl=30, nh=24, hd=128, dim=3072, table_limit=1 << 30, fp8=False, sp_size=1, sp_rank=0,
                                 sp_mode=p.sp_mode, sp_overlap_level=p.sp_overlap_level, sp_pieces=p.sp_pieces, sp_fused_qkv=p.sp_fused_qkv,
                                 cond=dict(B=2, L=11648, dens_same=True), _smooth_k=None, _smooth_v=None, **window)


def _mode(e, env, monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        m = DiTEngine._mode(e, 1, 2, 1, None, True, None)
    return m, [str(w.message) for w in seen if "window" in str(w.message)]


@pytest.mark.parametrize("window", [dict(window=(448, 448)), dict(window=(448, 448), window_sink=448), dict(window_frames=(2, 2))], ids=["tokens", "sink", "frames"])
def test_mode_keeps_sage_under_a_window_only_with_the_switch(window, monkeypatch):
    monkeypatch.setattr(DiTEngine, "_sage_window_warned", False)      # (put back when the test ends)
    monkeypatch.setattr(DiTEngine, "_sage_warned", True)
    e = _engine(**window)
    on = dict(SAGE, FLEXAM_SAGE_WINDOW="1")
    m_on, said = _mode(e, on, monkeypatch)
    assert m_on.sage and m_on.sage_fused and not said and e._smooth_k is False and e._smooth_v is False
    m_k, said = _mode(e, dict(on, FLEXAM_SAGE_SMOOTH_K="1"), monkeypatch)
    assert m_k == m_on and not said and e._smooth_k is True and e._smooth_v is False
    m_v, said = _mode(e, dict(on, FLEXAM_SAGE_SMOOTH_V="1", FLEXAM_SAGE_SMOOTH_K="1"), monkeypatch)
    assert m_v == m_on and not said and e._smooth_k is True and e._smooth_v is True
    # without the switch (unset, or 0): the fallback's mode and its warning, once per process; smooth-K / smooth-V off with it
    m_off, said = _mode(e, dict(SAGE, FLEXAM_SAGE_SMOOTH_K="1", FLEXAM_SAGE_SMOOTH_V="1"), monkeypatch)
    assert not m_off.sage and not m_off.sage_fused and len(said) == 1 and "bf16" in said[0] and e._smooth_k is False and e._smooth_v is False
    m_zero, said = _mode(e, dict(SAGE, FLEXAM_SAGE_WINDOW="0"), monkeypatch)
    assert m_zero == m_off and not said
    assert m_on != m_off and m_on._replace(sage=False, sage_fused=False) == m_off           # they differ in `sage` alone: two plan keys
    # the switch alone asks for nothing
    m_plain, said = _mode(e, {"FLEXAM_SAGE_WINDOW": "1"}, monkeypatch)
    assert m_plain == m_off and not said
    # and without a window it changes nothing
    e0 = _engine()
    assert _mode(e0, on, monkeypatch)[0] == _mode(e0, SAGE, monkeypatch)[0] == m_on


# ----------------------------------------------------------------------------- (d) header, binding, replay table, code objects
def test_header_binding_and_replay_table_name_the_entry_point():
    from flexam_amd import abi, gen_replay
    params = {n: p for n, _, p in abi.PROTOTYPES}["flexam_attn_fwd_fp8_window"]
    assert [n for _, n in params] == ["q8", "qs", "kv8", "o", "o_bs", "o_rs", "B", "H", "L", "head_dim", "window_left", "window_right", "sink",
                                      "frame_tokens", "o_shift", "stream"]
    assert "flexam_attn_fwd_fp8_window" in dict(abi.replayable(abi.PROTOTYPES))
    header = open(abi.HEADER).read()
    assert open(gen_replay.OUT).read() == gen_replay.generate(header), "csrc/replay_table.inc is stale: python -m flexam_amd.gen_replay"
    assert gen_replay.arg_kinds(header)["flexam_attn_fwd_fp8_window"] == "pppp" + "ii" + "iiii" + "iiii" + "p"


def test_library_exports_the_entry_point():
    import ctypes
    from flexam_amd import build
    if not os.path.exists(build.LIB):
        pytest.skip("libflexam_hip.so not built")
    assert hasattr(ctypes.CDLL(build.LIB), "flexam_attn_fwd_fp8_window")


def test_the_two_kernels_fit_two_waves_per_simd_without_spills():
    import kernel_resources as KR
    if not os.path.exists(KR.LIB):
        pytest.skip("libflexam_hip.so not built")
    if not os.path.exists(os.path.join(KR.LLVM, "clang-offload-bundler")):
        pytest.skip("ROCm LLVM tools not installed here")
    res = KR.kernel_resources()
    for sym in ("attn8_window_kernel", "attn8_window_oshift_kernel"):
        hit = {k: v for k, v in res.items() if sym in k}
        assert len(hit) == 1, (sym, list(hit))
        (name, v), = hit.items()
        assert "attn8_fwd_kernel" not in name and "attn_fwd_kernel" not in name
        assert v["max_flat_workgroup_size"] == 512 and v["vgpr_count"] + v["agpr_count"] <= 256, (name, v)
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)
