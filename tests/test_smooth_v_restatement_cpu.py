"""CPU: the claims FLEXAM_SAGE_SMOOTH_V rests on, checked on the restatement alone (tests/smooth_v_restatement.py), and where the switch
lives in the DiT engine, without a GPU.  Subtracting the token mean of V and adding it back changes nothing in exact attention; on MXFP8
operands it removes most of what an offset in V costs above the floor bf16 output has anyway, and costs nothing where there is no offset.
DiTEngine._mode reads the switch beside the mode (`sage and sp == 1` only, independent of smooth-K) and a launch plan is keyed on it."""
import contextlib
import os
import sys
import types
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp8_restatement as MX  # noqa: E402
import smooth_v_restatement as SV  # noqa: E402

from flexam_amd import dit_layout as D  # noqa: E402
from flexam_amd import hip  # noqa: E402
from flexam_amd.dit_engine import DiTEngine  # noqa: E402


def test_exact_attention_does_not_see_the_shift():
    """softmax(S).(V - 1 c^T) + c^T = softmax(S).V: the walk with quant=False (exact softmax attention in float64) on v and on
    v - mean_tokens(v) with the mean added back, all 300 rows of the offset case, and with a shift that is NOT the mean (any vector per
    batch and head is exact).  Bound 1e-6, as for the same statement about K (tests/test_smooth_k_restatement_cpu.py); float64 all the
    way, the figures are ~1e-16."""
    q, k, v = SV.offset_case_v()
    rows = list(range(q.shape[1]))
    exact = MX.attention(q, k, v, rows, quant=False)
    mean = SV.token_mean(v)
    smooth = MX.attention(q.double(), k.double(), v.double() - mean, rows, quant=False) + mean
    c = 3.0 * torch.randn(1, 1, 2, 128, generator=torch.Generator().manual_seed(1)).double()
    other = MX.attention(q.double(), k.double(), v.double() - c, rows, quant=False) + c
    print("exact attention, (v - mean) + mean against v:", SV.rel_rms(smooth, exact), "; (v - c) + c against v:", SV.rel_rms(other, exact))
    assert SV.rel_rms(smooth, exact) <= 1e-6 and SV.rel_rms(other, exact) <= 1e-6


@pytest.mark.parametrize("B,Hh,L", [(1, 2, 300), (2, 3, 1111)])
def test_the_offset_is_what_mxfp8_pays_for_and_the_mean_removes_it(B, Hh, L):
    """An offset ~ N(0, 4^2) per (head, channel) in V, unit-variance logits (offset_case_v, seed L), one key range.  e = the centred
    error of the bf16-rounded output, f = the floor (exact attention rounded to bf16): e_plain^2 - f^2 >= 4 (e_smooth^2 - f^2).
    The restatement gives over all rows, (1, 2, 300): plain 2.404e-1, smooth 1.173e-1, floor 8.913e-2, ratio 8.6; (2, 3, 1111):
    3.278e-1, 2.045e-1, 1.758e-1, ratio 7.0."""
    q, k, v = SV.offset_case_v(B, Hh, L, 4.0)
    e_plain, e_smooth, floor, _ = SV.errors(q, k, v)
    print(f"B={B} H={Hh} L={L} bias 4: plain {e_plain:.3e}, smooth {e_smooth:.3e}, floor {floor:.3e}, "
          f"ratio above the floor {SV.excess_ratio(e_plain, e_smooth, floor):.2f}")
    assert e_smooth >= floor * 0.999
    assert e_plain ** 2 - floor ** 2 >= 4 * (e_smooth ** 2 - floor ** 2)


def test_without_an_offset_nothing_is_lost():
    """bias 0 at (1, 2, 300): e_smooth <= 1.05 e_plain.  The restatement gives 6.916e-2 against 6.843e-2 (+1 %)."""
    e_plain, e_smooth, floor, _ = SV.errors(*SV.offset_case_v(1, 2, 300, 0.0))
    print(f"bias 0: plain {e_plain:.3e}, smooth {e_smooth:.3e}, floor {floor:.3e}")
    assert e_smooth <= 1.05 * e_plain


# ----------------------------------------------------------------------------- the mode (in the style of tests/test_smooth_k_mode_cpu.py)
SAGE = {"VIDEOX_ATTENTION_TYPE": "SAGE_ATTENTION"}
SWITCHES = ("VIDEOX_ATTENTION_TYPE", "FLEXAM_SAGE_SMOOTH_K", "FLEXAM_SAGE_SMOOTH_V", "FLEXAM_REPLAY", "FLEXAM_SHARE_BLOCK0", "FLEXAM_FP8_OPROJ",
            "FLEXAM_FP8_FFN_APRIORI")


def _engine(sp=1, rank=0, parallel=D.SINGLE_RANK, fused=True):
    e = types.SimpleNamespace(fused=fused, nl=30, nh=24, hd=128, dim=3072, table_limit=1 << 30, fp8=False, sp_size=sp, sp_rank=rank,
                              sp_mode=parallel.sp_mode, sp_overlap_level=parallel.sp_overlap_level, sp_pieces=parallel.sp_pieces,
                              sp_fused_qkv=parallel.sp_fused_qkv, cond=dict(B=2, L=11648, dens_same=True), _smooth_k=None, _smooth_v=None,
                              _ws_gen=0, sp_group=None, launched=[])
    e._blocks = lambda m, ws, e0, dens0: e.launched.append(("blocks", e._smooth_v))
    e._head = lambda m, ws: None
    return e


def _mode(e, env, monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    return DiTEngine._mode(e, 1, 2, 1, None, True, None)


def test_smooth_v_asked_reads_one_switch_with_default_off():
    assert not D.smooth_v_asked({}) and not D.smooth_v_asked({"FLEXAM_SAGE_SMOOTH_V": "0"}) and D.smooth_v_asked({"FLEXAM_SAGE_SMOOTH_V": "1"})
    assert not D.smooth_v_asked(SAGE) and not D.smooth_v_asked({"FLEXAM_SAGE_SMOOTH_K": "1"}) and not D.smooth_k_asked({"FLEXAM_SAGE_SMOOTH_V": "1"})


def test_mode_reports_smooth_v_only_for_sage_on_one_rank(monkeypatch):
    monkeypatch.setattr(DiTEngine, "_smooth_v_warned", False)      # (all three flags: put back when the test ends)
    monkeypatch.setattr(DiTEngine, "_smooth_k_warned", True)
    monkeypatch.setattr(DiTEngine, "_sage_warned", True)
    on = dict(SAGE, FLEXAM_SAGE_SMOOTH_V="1")
    e = _engine()
    m_on = _mode(e, on, monkeypatch)
    assert m_on.sage and e._smooth_v is True and e._smooth_k is False          # independent of smooth-K
    m_off = _mode(e, SAGE, monkeypatch)
    assert e._smooth_v is False
    assert m_on == m_off and hash(m_on) == hash(m_off)              # resolve_mode's result does not see the switch
    _mode(e, dict(on, FLEXAM_SAGE_SMOOTH_K="1"), monkeypatch)       # the two compose
    assert e._smooth_v is True and e._smooth_k is True
    _mode(e, dict(SAGE, FLEXAM_SAGE_SMOOTH_K="1"), monkeypatch)
    assert e._smooth_v is False and e._smooth_k is True
    _mode(e, {"FLEXAM_SAGE_SMOOTH_V": "1"}, monkeypatch)             # without SAGE_ATTENTION: the bf16 kernel, nothing to smooth
    assert e._smooth_v is False
    _mode(e, dict(on, FLEXAM_SAGE_SMOOTH_V="0"), monkeypatch)
    assert e._smooth_v is False
    e = _engine(fused=False)                                        # blocks called as modules: the seam reads the switch itself
    assert not _mode(e, on, monkeypatch).sage and e._smooth_v is False
    # sequence parallelism: quantised attention runs, the smoothing does not; said once per process
    for env in ({}, {"FLEXAM_SP_MODE": "ulysses"}):
        e = _engine(sp=8, rank=1, parallel=D.resolve_parallel(env, 24, 8))
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            m = _mode(e, on, monkeypatch)
            assert m.sage and m.sp == 8 and e._smooth_v is False
            _mode(e, on, monkeypatch)
        said = [w for w in seen if "FLEXAM_SAGE_SMOOTH_V" in str(w.message)]
        assert len(said) == (1 if not env else 0), [str(w.message) for w in seen]
        assert all(issubclass(w.category, RuntimeWarning) for w in said)


def test_a_plan_is_keyed_on_the_switch(monkeypatch):
    """_record_or_replay with the recorder patched: the first forward of each switch value records (the blocks are issued), a repeat
    replays, and the two plans sit under two keys that differ in nothing but the switch."""
    runs = []

    @contextlib.contextmanager
    def record():
        yield types.SimpleNamespace(launches=0, run=lambda: runs.append("replayed"))

    monkeypatch.setattr(hip, "record", record)
    monkeypatch.setattr(hip, "num_cus", lambda: 256)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(cuda_stream=0))
    e = _engine()
    e.cond["cos"] = torch.zeros(4)
    m = _mode(e, SAGE, monkeypatch)
    ws = {"row_index": None, ("tabs", m.R, m.per_layer): dict(blk=torch.zeros(1), head=torch.zeros(1))}
    for smooth, want_launched, want_runs in ((False, 1, 0), (True, 2, 0), (True, 2, 1), (False, 2, 2)):
        e._smooth_v = smooth
        DiTEngine._record_or_replay(e, m, ws, None, None)
        assert (len(e.launched), len(runs)) == (want_launched, want_runs), (smooth, e.launched, runs)
    assert e.launched == [("blocks", False), ("blocks", True)] and e.replay_taken
    k0, k1 = list(e.cond["_plans"])
    diff = [i for i, (a, b) in enumerate(zip(k0, k1)) if a != b]
    assert len(k0) == len(k1) and len(diff) == 1 and {k0[diff[0]], k1[diff[0]]} == {False, True} and k0[0] == k1[0] == m
    e._smooth_k = True                                              # and smooth-K on top is a third plan: the two are separate words of the key
    DiTEngine._record_or_replay(e, m, ws, None, None)
    assert len(e.cond["_plans"]) == 3 and len(e.launched) == 3
