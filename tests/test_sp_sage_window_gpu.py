"""GPU: a windowed model with SAGE_ATTENTION under the K|V gather exchanges MXFP8 records and runs the windowed MXFP8 kernel at each
rank's query offset (FLEXAM_SP_SAGE_WINDOW=1 on top of FLEXAM_SP_WINDOW=1, SAGE_ATTENTION and FLEXAM_SAGE_WINDOW=1;
flexam_attn_fwd_fp8_window_at through dit_sp.RecordGather).  Worlds of 2, 3 and 4 ranks over gloo on the one test GPU, spawned once each
through test_sp_gpu.run_world with a worker of this module modelled on tests/test_sp_window_gpu.py's; the model, its weights, inputs and
masks are that module's.  DIT_TINY's 256 tokens are padded to 64 x ranks: 128 rows a rank on 2, 64 on 4, and 384 rows on 3 ranks, where
rank 2 holds pad rows only.

Per case with all four switches (mode allgather-wait-p1-sage, both MASKS): the MXFP8 kernel was taken and no window fallback warned
about; the second forward is replayed and bit-equal; every rank ends with the same bits; the output is NOT the bf16 windowed gather's of
the same world; rel-RMS < 4e-3 against the single-process windowed MXFP8 forward (test_sp_window_gpu._single(..., sage_window=True):
existing code, the yardstick tests/test_sp_gpu.py and tests/test_sp_window_gpu.py hold the SAGE layouts to; that module's oracle check
shows that a mask blind to the offset moves the output by 1.1e-1 or more).  Then: the switch flipped between forwards of one model
records a plan of its own and gives the bf16 gather's bits, and flipped back replays the first plan; with FLEXAM_SP_SAGE_WINDOW unset
the same call is the bf16 gather bit for bit; with two head-group pieces the fallback and its warning run; FLEXAM_SP_HALO=1 on top is
ignored with a reason of its own and changes no bit.

Measured on an MI355X (recorded, not asserted): against the single-process windowed MXFP8 forward rel-rms 0 in all six cases (the
same records, the same tiles in the same order: the same bits); against the bf16 windowed gather of the same world 1.05e-2 (frames) and
1.07e-2 (tokens) in worlds of 2, 3 and 4 ranks."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_sp_gpu as SP  # noqa: E402
import test_sp_window_gpu as W  # noqa: E402
from test_sp_gpu import rel_rms, run_world  # noqa: E402
from test_sp_window_gpu import MASKS, _single  # noqa: E402

pytestmark = pytest.mark.gpu

SW = {"FLEXAM_SP_WINDOW": "1"}
SAGE_SW = dict(SW, FLEXAM_SAGE_WINDOW="1")
ALL = dict(SAGE_SW, FLEXAM_SP_SAGE_WINDOW="1")
RECORDS = "allgather-wait-p1-sage"
# (world, mask, mode, switches beyond the mode's, flip FLEXAM_SP_SAGE_WINDOW off and on again behind the two forwards)
CASES = ([(w, mask, RECORDS, ALL, w == 2) for w in (2, 3, 4) for mask in MASKS]
         + [(w, mask, "allgather-wait-p1", SW, False) for w in (2, 3, 4) for mask in MASKS]          # the bf16 windowed gather of the same world
         + [(2, "frames", RECORDS, SAGE_SW, False),                                                   # the switch unset: today's behaviour
            (2, "frames", "allgather-wait-sage", ALL, False), (2, "frames", "allgather-wait", SW, False),      # two head-group pieces
            (2, "tokens", RECORDS, dict(ALL, FLEXAM_SP_HALO="1"), False)])
SWITCHES = W.SWITCHES + ("FLEXAM_SP_SAGE_WINDOW", "FLEXAM_SP_HALO")
FALLBACK = "SAGE_ATTENTION is ignored with window_size / window_frames"


def _key(case):
    world, mask, mode, env, flip = case
    return (mask, mode, tuple(sorted(env.items())))


def _ids(cases):
    return [f"w{c[0]}-{c[1]}-{c[2]}" + "".join("+" + k.split("_", 1)[1].lower() for k in sorted(c[3])) for c in cases]


def _worker(rank, world, port, ret, cases, wide=False, backend="gloo"):
    """cases: the CASES of this world; ret[rank] = {key: (DiT output, facts) | error text}."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from flexam_amd.dit_engine import DiTEngine
        results = {}
        for case in cases:
            _, mask, mode, env, flip = case
            m = None
            try:
                for name in SWITCHES:
                    os.environ.pop(name, None)
                SP.set_mode_env(mode)
                os.environ.update(env)
                DiTEngine._sp_window_overlap_warned = DiTEngine._sage_window_warned = DiTEngine._sp_halo_warned = False
                cfg = W._cfg(False)
                m = W._build(cfg, mask)
                m.enable_multi_gpus_inference(cfg_parallel=False)
                d = W._inputs(cfg)
                with warnings.catch_warnings(record=True) as seen:
                    warnings.simplefilter("always")
                    first = m(**d).float().cpu()
                    eng = m.engine()
                    facts = dict(sp=eng.sp_size, sp_mode=eng.sp_mode, fused=eng.fused, sage=bool(eng.sage_taken), replayed_first=bool(eng.replay_taken))
                    second = m(**d).float().cpu()
                    facts.update(replayed_second=bool(eng.replay_taken), second_equal=bool(torch.equal(first, second)),
                                 warnings=[str(w.message) for w in seen if issubclass(w.category, RuntimeWarning)])
                    if flip:
                        os.environ["FLEXAM_SP_SAGE_WINDOW"] = "0"
                        off = m(**d).float().cpu()
                        facts.update(off_sage=bool(eng.sage_taken), off_replayed=bool(eng.replay_taken))
                        os.environ["FLEXAM_SP_SAGE_WINDOW"] = "1"
                        again = m(**d).float().cpu()
                        facts.update(again_sage=bool(eng.sage_taken), again_replayed=bool(eng.replay_taken), again_equal=bool(torch.equal(first, again)))
                        first = (first, off)
                results[_key(case)] = (first, facts)
            except Exception as e:                             # noqa: BLE001  raised on every rank alike (configuration): the next case still runs
                results[_key(case)] = f"{type(e).__name__}: {e}"
            del m
        ret[rank] = results
    finally:
        dist.destroy_process_group()


_WORLDS = {}


def _world(world):
    """Every case of `world` ranks, run once per session in one spawned world."""
    if world not in _WORLDS:
        saved, SP._worker = SP._worker, _worker                  # run_world spawns test_sp_gpu._worker: this module's, for the call
        try:
            _WORLDS[world] = run_world(world, [c for c in CASES if c[0] == world])
        finally:
            SP._worker = saved
    return _WORLDS[world]


def _result(case):
    """(output, facts of rank 0) of a case, every rank's output the same bits.  (A flipped case: output = (with the switch, without).)"""
    res = [r[_key(case)] for r in _world(case[0])]
    for r in res:
        assert not isinstance(r, str), r
    for out, facts in res[1:]:
        for a, b in zip(*((o if isinstance(o, tuple) else (o,)) for o in (res[0][0], out))):
            torch.testing.assert_close(a, b, rtol=0, atol=0)
        assert facts == dict(res[0][1], warnings=facts["warnings"])
    return res[0]


def _bf16_gather(world, mask):
    return _result((world, mask, "allgather-wait-p1", SW, False))[0]


SERVED = [c for c in CASES if c[2] == RECORDS and c[3] == ALL]


@pytest.mark.parametrize("case", SERVED, ids=_ids(SERVED))
def test_windowed_sage_model_under_the_record_gather_runs_the_windowed_mxfp8_kernel(case):
    world, mask, mode, env, flip = case
    out, facts = _result(case)
    off = None
    if flip:
        out, off = out
    name = _ids([case])[0]
    assert facts["sp"] == world and facts["sp_mode"] == "allgather" and facts["fused"] and facts["sage"] is True
    assert not [w for w in facts["warnings"] if FALLBACK in w or "FLEXAM_SP_HALO" in w], facts["warnings"]
    assert facts["second_equal"] and not facts["replayed_first"] and facts["replayed_second"]
    bf16 = _bf16_gather(world, mask)
    assert not torch.equal(out, bf16)
    single = _single(False, mask, sage_window=True)
    rel = rel_rms(out, single)
    print(f"{name}: vs single-process windowed MXFP8 rel-rms {rel:.2e}; vs the bf16 windowed gather {rel_rms(out, bf16):.2e}")
    assert bool(torch.isfinite(out).all()) and rel < 4e-3
    if flip:
        # the switch flipped between forwards of one model: a mode, hence a plan, of its own -- not the other's replayed
        assert facts["off_sage"] is False and facts["off_replayed"] is False and torch.equal(off, bf16)
        assert facts["again_sage"] is True and facts["again_replayed"] is True and facts["again_equal"]


def test_with_the_switch_unset_the_call_is_the_bf16_gather_bit_for_bit():
    out, facts = _result((2, "frames", RECORDS, SAGE_SW, False))
    assert facts["sage"] is False and torch.equal(out, _bf16_gather(2, "frames"))
    assert len([w for w in facts["warnings"] if FALLBACK in w]) == 1, facts["warnings"]


def test_with_two_head_group_pieces_the_fallback_and_its_warning_run():
    out, facts = _result((2, "frames", "allgather-wait-sage", ALL, False))
    assert facts["sage"] is False and torch.equal(out, _result((2, "frames", "allgather-wait", SW, False))[0])
    said = [w for w in facts["warnings"] if FALLBACK in w]
    assert len(said) == 1 and "windowed bf16 kernel" in said[0], facts["warnings"]
    assert facts["second_equal"] and facts["replayed_second"]


def test_the_halo_switch_on_top_is_ignored_with_a_reason_of_its_own_and_changes_no_bit():
    out, facts = _result((2, "tokens", RECORDS, dict(ALL, FLEXAM_SP_HALO="1"), False))
    plain = _result((2, "tokens", RECORDS, ALL, True))[0][0]
    assert facts["sage"] is True and torch.equal(out, plain)
    said = [w for w in facts["warnings"] if "FLEXAM_SP_HALO=1 is ignored" in w]
    assert len(said) == 1 and "the MXFP8 record gather moves whole chunks" in said[0] and "all-to-all" not in said[0], facts["warnings"]
