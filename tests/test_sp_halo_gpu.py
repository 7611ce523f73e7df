"""GPU: the halo exchange of windowed self-attention under sequence parallelism (FLEXAM_SP_HALO=1 on top of FLEXAM_SP_WINDOW=1): worlds
of 2, 3 and 4 ranks over gloo on the one test GPU, spawned once each through test_sp_gpu.run_world with a worker of this module, as
tests/test_sp_window_gpu.py does, whose models (DIT_TINY, 256 tokens = 4 frames of 64, and its wide forms), masks (window_frames = (1, 0)
with window_sink = 64; window_size = (100, 37) with window_sink = 70) and masked oracle this module takes.

Under the K|V gather, waited for, in one and in two head-group pieces: every rank's result with the switch is bit-equal to the same
world's result without it (a rank's call visits the same tiles in the same order; only where the rows lie differs), it is within REL_RMS
of the masked oracle, the second forward is replayed from the launch plan and bit-equal, and at least one rank of every world holds
fewer rows than the gather would hand it (eng.halo_rows < eng.halo_gather_rows = sp * lc).  SAGE_ATTENTION under it: the bf16 fallback
and its warning, the same bits.  Where the switch cannot act -- the all-to-all over heads, a model without a window -- one RuntimeWarning
and the bits of the run without it; with the switch unset no such warning."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_sp_gpu as SP  # noqa: E402
import test_sp_window_gpu as W  # noqa: E402
from test_attn_window_gpu import _check_model  # noqa: E402
from test_sp_gpu import run_world  # noqa: E402

pytestmark = pytest.mark.gpu

SW = {"FLEXAM_SP_WINDOW": "1"}
HALO = dict(SW, FLEXAM_SP_HALO="1")
SWITCHES = W.SWITCHES + ("FLEXAM_SP_HALO",)
# (world, heads or False = DIT_TINY, mask or None, mode, switches): every served layout with and without the switch
PAIRS = [(2, False, "frames", "allgather-wait"), (2, False, "frames", "allgather-wait-p1"), (2, False, "tokens", "allgather-wait"),
         (3, False, "frames", "allgather-wait-p1"), (3, False, "tokens", "allgather-wait"),
         (4, 4, "frames", "allgather-wait"), (4, 4, "tokens", "allgather-wait-p1")]
IDLE = [(2, False, "frames", "ulysses-ov0"), (2, False, None, "allgather-wait-p1")]       # the switch set where it cannot act
SAGE = (2, False, "frames", "allgather-wait-p1-sage")
CASES = ([c + (env,) for c in PAIRS for env in (SW, HALO)] + [IDLE[0] + (SW,), IDLE[0] + (HALO,), IDLE[1] + ({},), IDLE[1] + ({"FLEXAM_SP_HALO": "1"},)]
         + [SAGE + (HALO,)])


def _key(case):
    world, heads, mask, mode, env = case
    return (heads, mask, mode, tuple(sorted(env.items())))


def _ids(cases):
    return [f"w{c[0]}-h{c[1] or 2}-{c[2]}-{c[3]}" for c in cases]


def _build(cfg, mask):
    from flexam_amd import Wan2_2Transformer3DModel_FlexAM
    kw = dict(cfg)
    kw.pop("eps")
    m = Wan2_2Transformer3DModel_FlexAM(**kw, **(W.MASKS[mask] if mask else {}))
    m.load_state_dict(W._weights(cfg), strict=True)
    return m.to("cuda:0")


def _worker(rank, world, port, ret, cases, wide=False, backend="gloo"):
    """cases: the CASES of this world; ret[rank] = {key: (DiT output, facts) | error text}."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from flexam_amd.dit_engine import DiTEngine
        results = {}
        for case in cases:
            _, heads, mask, mode, env = case
            m = None
            try:
                for name in SWITCHES:
                    os.environ.pop(name, None)
                SP.set_mode_env(mode)
                os.environ.update(env)
                DiTEngine._sp_halo_warned = DiTEngine._sage_window_warned = False
                cfg = W._cfg(heads)
                m = _build(cfg, mask)
                m.enable_multi_gpus_inference(cfg_parallel=False)
                d = W._inputs(cfg)
                with warnings.catch_warnings(record=True) as seen:
                    warnings.simplefilter("always")
                    first = m(**d).float().cpu()
                    eng = m.engine()
                    facts = dict(sp=eng.sp_size, sp_mode=eng.sp_mode, fused=eng.fused, sage=bool(eng.sage_taken), replayed_first=bool(eng.replay_taken),
                                 halo_rows=eng.halo_rows, gather_rows=eng.halo_gather_rows)
                    second = m(**d).float().cpu()
                    facts.update(replayed_second=bool(eng.replay_taken), second_equal=bool(torch.equal(first, second)),
                                 warnings=[str(w.message) for w in seen if issubclass(w.category, RuntimeWarning)])
                results[_key(case)] = (first, facts)
            except Exception as e:                             # noqa: BLE001  raised on every rank alike (configuration): the next case still runs
                import traceback
                results[_key(case)] = f"{type(e).__name__}: {e}\n{traceback.format_exc()}"
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
    """(output, facts of every rank) of a case, every rank's output the same bits."""
    res = [r[_key(case)] for r in _world(case[0])]
    for r in res:
        assert not isinstance(r, str), r
    for out, _ in res[1:]:
        torch.testing.assert_close(res[0][0], out, rtol=0, atol=0)
    return res[0][0], [f for _, f in res]


def _halo_warnings(facts):
    return [w for w in facts["warnings"] if "FLEXAM_SP_HALO" in w]


@pytest.mark.parametrize("pair", PAIRS, ids=_ids(PAIRS))
def test_halo_exchange_gives_the_bits_of_the_gather(pair):
    world, heads, mask, mode = pair
    gathered, plain_facts = _result(pair + (SW,))
    out, facts = _result(pair + (HALO,))
    assert torch.equal(out, gathered), f"{_ids([pair])[0]}: the halo exchange changed the result"
    _check_model(out, W._want(heads, mask), _ids([pair])[0] + " halo")
    for f, p in zip(facts, plain_facts):
        assert f["sp"] == world and f["sp_mode"] == "allgather" and f["fused"] and not f["sage"]
        assert f["second_equal"] and not f["replayed_first"] and f["replayed_second"]
        assert f["gather_rows"] == -(-256 // world) * world and 0 <= f["halo_rows"] <= 256
        assert not _halo_warnings(f)
        # with the switch unset: no halo, no word about it
        assert p["halo_rows"] is None and p["gather_rows"] is None and not _halo_warnings(p) and p["second_equal"] and p["replayed_second"]
    rows = [f["halo_rows"] for f in facts]
    print(f"{_ids([pair])[0]}: buffer rows per rank {rows} of {facts[0]['gather_rows']} gathered")
    assert min(rows) < facts[0]["gather_rows"], rows


def test_planned_rows_of_the_worlds_above():
    """What the engines report is the planner's, and on four ranks a rank skips tiles between its sink and its window (gap > 0)."""
    from flexam_amd.dit_layout import halo_plan
    _, facts = _result((4, 4, "frames", "allgather-wait", HALO))
    plans = [halo_plan(256, 4, r, (1, 0), 64, W.T_TINY) for r in range(4)]
    assert [f["halo_rows"] for f in facts] == [p.rows for p in plans] == [64, 128, 192, 192]
    assert [p.gap for p in plans] == [0, 0, 0, 1]


@pytest.mark.parametrize("case", IDLE, ids=_ids(IDLE))
def test_where_the_switch_cannot_act_it_warns_once_and_changes_no_bit(case):
    without, with_ = (IDLE[0] + (SW,), IDLE[0] + (HALO,)) if case[2] else (IDLE[1] + ({},), IDLE[1] + ({"FLEXAM_SP_HALO": "1"},))
    plain, plain_facts = _result(without)
    out, facts = _result(with_)
    assert torch.equal(out, plain)
    for f, p in zip(facts, plain_facts):
        said = _halo_warnings(f)
        assert len(said) == 1 and ("all-to-all over heads" if case[2] else "no window_size / window_frames") in said[0], f["warnings"]
        assert f["halo_rows"] is None and not _halo_warnings(p)
        assert f["second_equal"] and f["replayed_second"]


def test_sage_under_the_halo_keeps_the_bf16_fallback_and_its_warning():
    out, facts = _result(SAGE + (HALO,))
    assert torch.equal(out, _result((2, False, "frames", "allgather-wait-p1", SW))[0])
    for f in facts:
        assert not f["sage"] and f["halo_rows"] is not None and not _halo_warnings(f)
        assert len([w for w in f["warnings"] if "SAGE_ATTENTION is ignored with window_size / window_frames" in w]) == 1, f["warnings"]
