"""CPU: where FLEXAM_SAGE_SMOOTH_K lives in the DiT engine, without a GPU: DiTEngine._mode reads it (beside the mode, never in it: the
field tuple of _Mode is pinned by tests/test_dit_layout_cpu.py), it holds for `sage and sp == 1` only, resolve_mode does not see it, and
a launch plan recorded with one value is never replayed with the other.  The engine is a stub holding the attributes _mode and
_record_or_replay read; the recorder and the two CUDA queries of the plan key are patched."""
import contextlib
import types
import warnings

import torch

from flexam_amd import dit_layout as D
from flexam_amd import hip
from flexam_amd.dit_engine import DiTEngine

SAGE = {"VIDEOX_ATTENTION_TYPE": "SAGE_ATTENTION"}
SWITCHES = ("VIDEOX_ATTENTION_TYPE", "FLEXAM_SAGE_SMOOTH_K", "FLEXAM_REPLAY", "FLEXAM_SHARE_BLOCK0", "FLEXAM_FP8_OPROJ", "FLEXAM_FP8_FFN_APRIORI")


def _engine(sp=1, rank=0, parallel=D.SINGLE_RANK, fused=True):
    e = types.SimpleNamespace(fused=fused, nl=30, nh=24, hd=128, dim=3072, table_limit=1 << 30, fp8=False, sp_size=sp, sp_rank=rank,
                              sp_mode=parallel.sp_mode, sp_overlap_level=parallel.sp_overlap_level, sp_pieces=parallel.sp_pieces,
                              sp_fused_qkv=parallel.sp_fused_qkv, cond=dict(B=2, L=11648, dens_same=True), _smooth_k=None, _ws_gen=0,
                              sp_group=None, launched=[])
    e._blocks = lambda m, ws, e0, dens0: e.launched.append(("blocks", e._smooth_k))
    e._head = lambda m, ws: None
    return e


def _mode(e, env, monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    return DiTEngine._mode(e, 1, 2, 1, None, True, None)


def test_smooth_k_asked_reads_one_switch_with_default_off():
    assert not D.smooth_k_asked({}) and not D.smooth_k_asked({"FLEXAM_SAGE_SMOOTH_K": "0"}) and D.smooth_k_asked({"FLEXAM_SAGE_SMOOTH_K": "1"})
    assert not D.smooth_k_asked(SAGE)


def test_mode_reports_smooth_k_only_for_sage_on_one_rank(monkeypatch):
    monkeypatch.setattr(DiTEngine, "_smooth_k_warned", False)      # (both flags: put back when the test ends)
    monkeypatch.setattr(DiTEngine, "_sage_warned", True)
    on = dict(SAGE, FLEXAM_SAGE_SMOOTH_K="1")
    e = _engine()
    m_on = _mode(e, on, monkeypatch)
    assert m_on.sage and e._smooth_k is True
    m_off = _mode(e, SAGE, monkeypatch)
    assert e._smooth_k is False
    assert m_on == m_off and hash(m_on) == hash(m_off)              # resolve_mode's result does not see the switch
    assert m_on == D.resolve_mode(on, fused=True, nl=30, nh=24, hd=128, dim=3072, table_limit=1 << 30, fp8=False, sp=1, rank=0,
                                  parallel=D.SINGLE_RANK, B=2, L=11648, dens_same=True, bx=1, R=2, rows_per_batch=1, only_row=None,
                                  rows_shared=True, teacache=False)
    _mode(e, {"FLEXAM_SAGE_SMOOTH_K": "1"}, monkeypatch)             # without SAGE_ATTENTION: the bf16 kernel, nothing to smooth
    assert e._smooth_k is False
    _mode(e, dict(on, FLEXAM_SAGE_SMOOTH_K="0"), monkeypatch)
    assert e._smooth_k is False
    e = _engine(fused=False)                                        # blocks called as modules: the seam reads the switch itself
    assert not _mode(e, on, monkeypatch).sage and e._smooth_k is False
    # sequence parallelism: quantised attention runs (records gathered, or all tokens of a rank's heads), the smoothing does not; said once
    for env in ({}, {"FLEXAM_SP_MODE": "ulysses"}):
        e = _engine(sp=8, rank=1, parallel=D.resolve_parallel(env, 24, 8))
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            m = _mode(e, on, monkeypatch)
            assert m.sage and m.sp == 8 and e._smooth_k is False
            _mode(e, on, monkeypatch)
        said = [w for w in seen if "FLEXAM_SAGE_SMOOTH_K" in str(w.message)]
        assert len(said) == (1 if not env else 0), [str(w.message) for w in seen]          # once per PROCESS: the second layout stays silent


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
        e._smooth_k = smooth
        DiTEngine._record_or_replay(e, m, ws, None, None)
        assert (len(e.launched), len(runs)) == (want_launched, want_runs), (smooth, e.launched, runs)
    assert e.launched == [("blocks", False), ("blocks", True)] and e.replay_taken
    k0, k1 = list(e.cond["_plans"])
    assert k0 != k1 and [a == b for a, b in zip(k0, k1)].count(False) == 1 and k0[0] == k1[0] == m
    assert {k0[-1], k1[-1]} == {False, True}
