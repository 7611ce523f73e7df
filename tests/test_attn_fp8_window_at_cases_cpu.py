"""CPU: the cases of tests/attn_fp8_window_at_cases.py (the windowed MXFP8 kernel at a query offset on chunked records) hold what they
promise and are not blind, on the restatement alone; and the engine's host side (FLEXAM_SP_SAGE_WINDOW) resolves, falls back and warns as
it says.

Not blind (asserted against attn_window_cases.SENSITIVITY_ULPS = 8, for every call with q_offset > 0): the mask taken at the row's index
in the call instead of its global token, one key added or dropped at either end of every row's range (each of the four alterations that
applies to some row of the call), and chunk c read where chunk c + 1 is meant each move some row of the restatement by 8 bf16 ulps or
more.  The least such move is printed per kind; measured: 418 ulps (row index for global token), 24 / 32 / 26 / 13 (add hi + 1, drop hi,
add lo - 1, drop lo), 176 (chunk c for c + 1)."""
import os
import sys
import types
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_fp8_window_at_cases as P  # noqa: E402
import attn_window_at_cases as A  # noqa: E402
import attn_window_cases as W  # noqa: E402
import mxfp8_window_restatement as WR  # noqa: E402
from flexam_amd import dit_layout as D  # noqa: E402
from flexam_amd.dit_engine import DiTEngine  # noqa: E402


def _most_moved(got, want):
    """The largest |got - want| / ulp(want) over every element."""
    return float(((got - want).abs() / P.bf16_ulp(want)).max())


def test_the_cases_hold_the_shapes_pad_rows_and_empty_rows_they_name():
    by = {c.name: c for c in P.CASES}
    assert len(by) == len(P.CASES) == 5 * 2 + 3 * 2 + 3 * 3
    assert [(c.lc, c.chunk_tiles) for c in (by["L70-w3_2-s0-r1of2"], by["L600-w100_37-s70-r1of2"], by["L1111-w200_100-s192-r2of3"])] == \
        [(64, 1), (320, 5), (384, 6)]
    # L = 70: rank 1 is 6 real rows and 58 pad rows; under (3, 2) without a sink the rows from global token 73 on see no key
    r1 = by["L70-w3_2-s0-r1of2"]
    assert r1.q_offset == 64 and r1.empty_rows().tolist() == [False] * 9 + [True] * 55
    assert by["L70-w3_2-s0-r1of2-oshift"].empty_rows().tolist() == r1.empty_rows().tolist() and by["L70-w3_2-s0-r1of2-oshift"].shift() is not None
    assert not by["L70-w3_2-s5-r1of2"].empty_rows().any() and not by["L70-w-1_0-s0-r1of2"].empty_rows().any()
    # L = 600: a gap between the sink tiles and the window tiles on rank 1 (rows 320 .. 575 see keys from 220 on: tiles 0, 1 and 3 ..)
    assert A.runs_of(by["L600-w100_37-s70-r1of2"].allowed(), 600)[0] == [(0, 1), (3, 9)]
    assert A.runs_of(by["L600-w-1_0-s70-r1of2"].allowed(), 600) == [[(0, 8)], [(0, 9)]]          # units that grow; the sink dropped
    r2 = by["L1111-w200_100-s192-r2of3"]
    assert r2.q_offset + r2.lc - r2.Lk == 41 and not r2.empty_rows().any()
    for c in P.CASES:
        q, k, v = c.inputs()
        assert q.shape == (c.B, c.lc, c.H, 128) and k.shape == v.shape == (c.B, c.Lk, c.H, 128) and c.lc % 64 == 0
        want = c.want()
        assert not want.isnan().any() and bool((want[:, c.empty_rows()] == 0).all())
        if c.shifted:
            assert bool((want[:, ~c.empty_rows()] != 0).all())
    # rows q_offset .. q_offset + Lq - 1 of the full-sequence mask: where the call's rows are real tokens, WR.mask's rows
    for c in (by["L600-w100_37-s70-r1of2"], by["L1111-f2_1-T64-s0-r1of3"], by["L70-f1_1-T7-s5-r0of2"]):
        n = min(c.q_offset + c.lc, c.Lk) - c.q_offset
        assert torch.equal(c.allowed()[:n], WR.mask(c.Lk, c.window, c.sink, c.T)[c.q_offset:c.q_offset + n])


def test_every_call_at_an_offset_fails_under_a_blind_mask_a_key_off_and_a_chunk_off():
    least = {}
    for c in P.CASES:
        if c.q_offset == 0:
            continue
        want = c.want()
        moved = {"row index for global token": _most_moved(c.want(ok=A.allowed(range(c.lc), c.Lk, c.window, c.T, c.sink)), want)}
        for name, mask, sel in A.altered_masks(c):
            if sel.any():
                moved[name] = _most_moved(c.want(ok=mask), want)
        assert {"add hi+1", "drop hi"} & set(moved) or c.window[1] < 0, c.name
        k, v = P.chunk_shifted_keys(c)
        moved["chunk c for c + 1"] = _most_moved(c.want(k=k, v=v), want)
        for kind, m in moved.items():
            assert m >= W.SENSITIVITY_ULPS, (c.name, kind, m)
            least[kind] = min(least.get(kind, float("inf")), m)
    print("least move of the most moved row, bf16 ulps: " + ", ".join(f"{k}: {m:.1f}" for k, m in least.items()))
    assert set(least) == {"row index for global token", "add hi+1", "drop hi", "add lo-1", "drop lo", "chunk c for c + 1"}


# ----------------------------------------------------------------------------- the engine's host side
SAGE = {"VIDEOX_ATTENTION_TYPE": "SAGE_ATTENTION"}
ALL4 = dict(SAGE, FLEXAM_SP_WINDOW="1", FLEXAM_SAGE_WINDOW="1", FLEXAM_SP_SAGE_WINDOW="1")
SWITCHES = ("VIDEOX_ATTENTION_TYPE", "FLEXAM_SAGE_SMOOTH_K", "FLEXAM_SAGE_SMOOTH_V", "FLEXAM_SAGE_WINDOW", "FLEXAM_SP_WINDOW", "FLEXAM_SP_SAGE_WINDOW",
            "FLEXAM_SP_HALO", "FLEXAM_REPLAY", "FLEXAM_SHARE_BLOCK0", "FLEXAM_FP8_OPROJ", "FLEXAM_FP8_FFN_APRIORI")


def _engine(sp=8, rank=3, env=(), window=(-1, -1), frames=(-1, -1), L=11648):
    par = D.resolve_parallel(dict(env), 24, sp)
    e = types.SimpleNamespace(fused=True, nl=30, nh=24, hd=128, dim=3072, table_limit=1 << 30, fp8=False, sp_size=sp, sp_rank=rank,
                              sp_mode=par.sp_mode, sp_overlap_level=par.sp_overlap_level, sp_pieces=par.sp_pieces, sp_fused_qkv=par.sp_fused_qkv,
                              cond=dict(B=2, L=L, dens_same=True, grid=(26, 16, 28)), _smooth_k=None, _smooth_v=None, window=window, window_frames=frames,
                              window_sink=448)
    e._window_frames = types.MethodType(DiTEngine._window_frames, e)
    e._window_mask = types.MethodType(DiTEngine._window_mask, e)
    return e


def _mode(e, env, monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    return DiTEngine._mode(e, 1, 2, 1, None, True, None)


def _quiet(monkeypatch, **flags):
    for name in ("_sage_window_warned", "_sage_warned", "_smooth_k_warned", "_smooth_v_warned", "_sp_halo_warned", "_sp_window_overlap_warned"):
        monkeypatch.setattr(DiTEngine, name, flags.get(name, True))


def test_the_switch_acts_only_on_top_of_the_other_three():
    assert D.sp_sage_window_asked(ALL4)
    for missing in ("VIDEOX_ATTENTION_TYPE", "FLEXAM_SP_WINDOW", "FLEXAM_SAGE_WINDOW", "FLEXAM_SP_SAGE_WINDOW"):
        assert not D.sp_sage_window_asked({k: v for k, v in ALL4.items() if k != missing})
    assert not D.sp_sage_window_asked(dict(ALL4, FLEXAM_SP_SAGE_WINDOW="0"))


def test_with_the_switch_the_mode_is_the_record_gather_of_the_unmasked_model(monkeypatch):
    _quiet(monkeypatch, _sage_window_warned=False)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for L in (11648, 11650):
            plain = _mode(_engine(L=L), SAGE, monkeypatch)
            assert plain.sage and plain.sage_gather
            for kw in (dict(window=(100, 37)), dict(frames=(2, 2))):
                m = _mode(_engine(L=L, **kw), ALL4, monkeypatch)
                assert m == plain and m.sage and m.sage_gather and m.lc % 64 == 0 and (m.sp_mode, m.sp_overlap_level, m.sp_pieces) == ("allgather", 0, 1)
        assert (plain.Lp, plain.lc) == (11776, 1472)
        # the overlapped gather is waited for under a window (the engine forces level 0), so the record gather resolves there too
        m = _mode(_engine(env={"FLEXAM_SP_OVERLAP": "1", "FLEXAM_SP_PIECES": "1"}, frames=(2, 2)), ALL4, monkeypatch)
        assert m.sage_gather and m.sp_overlap_level == 0
    assert not [str(w.message) for w in seen if "SAGE_ATTENTION is ignored" in str(w.message)]
    # a flipped switch is another mode: launch plans, keyed on the mode, cannot be confused
    _quiet(monkeypatch)
    assert _mode(_engine(frames=(2, 2)), {k: v for k, v in ALL4.items() if k != "FLEXAM_SP_SAGE_WINDOW"}, monkeypatch) != \
        _mode(_engine(frames=(2, 2)), ALL4, monkeypatch)


def test_without_the_switch_nothing_changes_and_where_the_record_gather_does_not_resolve_the_fallback_warns(monkeypatch):
    _quiet(monkeypatch)
    base = _mode(_engine(frames=(2, 2)), {"FLEXAM_SP_WINDOW": "1"}, monkeypatch)
    for env in ({k: v for k, v in ALL4.items() if k != "FLEXAM_SP_SAGE_WINDOW"}, dict(ALL4, FLEXAM_SP_SAGE_WINDOW="0"),
                {k: v for k, v in ALL4.items() if k != "FLEXAM_SAGE_WINDOW"}):
        m = _mode(_engine(frames=(2, 2)), env, monkeypatch)
        assert m == base and not m.sage and m.lc == 1456
    _quiet(monkeypatch, _sage_window_warned=False)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        pieces = {"FLEXAM_SP_PIECES": "2"}
        m = _mode(_engine(env=pieces, frames=(2, 2)), ALL4, monkeypatch)
        assert m == _mode(_engine(env=pieces, frames=(2, 2)), {"FLEXAM_SP_WINDOW": "1"}, monkeypatch) and not m.sage and not m.sage_gather
    said = [str(w.message) for w in seen]
    assert len(said) == 1 and "window_size / window_frames" in said[0] and "windowed bf16 kernel" in said[0], said
    # the all-to-all over heads: as without the switch (SAGE kept on an unpadded sequence)
    ul = {"FLEXAM_SP_MODE": "ulysses"}
    assert _mode(_engine(env=ul, frames=(2, 2)), ALL4, monkeypatch) == \
        _mode(_engine(env=ul, frames=(2, 2)), {k: v for k, v in ALL4.items() if k != "FLEXAM_SP_SAGE_WINDOW"}, monkeypatch)


def test_smooth_k_and_v_stay_ignored_and_the_halo_is_ignored_with_a_reason_of_its_own(monkeypatch):
    _quiet(monkeypatch, _smooth_k_warned=False, _smooth_v_warned=False, _sp_halo_warned=False)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        e = _engine(frames=(2, 2))
        m = _mode(e, dict(ALL4, FLEXAM_SAGE_SMOOTH_K="1", FLEXAM_SAGE_SMOOTH_V="1", FLEXAM_SP_HALO="1"), monkeypatch)
        assert m.sage_gather and e._smooth_k is False and e._smooth_v is False and e._sp_halo is False and e.halo_rows is None
    said = [str(w.message) for w in seen]
    assert len(said) == 3, said
    assert sum("FLEXAM_SAGE_SMOOTH_K=1 is ignored under sequence parallelism" in s for s in said) == 1
    assert sum("FLEXAM_SAGE_SMOOTH_V=1 is ignored under sequence parallelism" in s for s in said) == 1
    halo = [s for s in said if "FLEXAM_SP_HALO=1 is ignored" in s]
    assert len(halo) == 1 and "the MXFP8 record gather moves whole chunks" in halo[0] and "all-to-all" not in halo[0]
    # without the new switch the halo acts as it did
    _quiet(monkeypatch)
    e = _engine(frames=(2, 2))
    _mode(e, {k: v for k, v in dict(ALL4, FLEXAM_SP_HALO="1").items() if k != "FLEXAM_SP_SAGE_WINDOW"}, monkeypatch)
    assert e._sp_halo is True
