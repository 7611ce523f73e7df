"""GPU: windowed self-attention under sequence parallelism (FLEXAM_SP_WINDOW=1): worlds of 2, 3 and 4 ranks over gloo on the one test
GPU, spawned once each through test_sp_gpu.run_world with a worker of this module, the switch set inside the workers only.

DIT_TINY (256 tokens = 4 frames of 64, two heads) and its 3- and 4-head wide forms, the weights scaled to a self-attention logit standard
deviation of 3 as tests/test_attn_window_frames_gpu.py does, under window_frames = (1, 0) with window_sink = 64 and under window_size =
(100, 37) with window_sink = 70.  Layouts: the K|V gather in one and in two pieces; the same with FLEXAM_SP_OVERLAP=1 (the warning, the
same bits); the all-to-all over heads; three ranks (256 -> 258 rows, two pads, chunks of 86 off every tile boundary); re-bound blocks;
SAGE_ATTENTION with and without FLEXAM_SAGE_WINDOW=1.  Every rank ends with the same full result (atol = 0); that result is held to the
oracle masked by the same rule (REL_RMS) and to the single-process windowed HIP result at the 4e-3 tests/test_sp_gpu.py applies to the
same comparison without a window -- the latter is this code at offset 0, so it agrees almost trivially and is not the yardstick.  A second
forward is served from the launch plan and is bit-equal.  With the switch unset the world's forward raises the existing message.

Not blind (CPU, on the oracle alone, asserted in the fixture): masking rank 1's rows of a 2-rank split as if their offset were 0 moves the
oracle's output by more than 3 x REL_RMS for both masks (the figures are printed).

Measured on an MI355X (recorded, not asserted): the blind mask moves the oracle by rel-rms 1.22e-1 (frames) and 1.11e-1 (tokens) against
3 x REL_RMS = 4.5e-2; HIP against the masked oracle rel-rms 4.5e-3 to 4.6e-3 (64.9 - 66.2 dB) in every layout; against the single-process
windowed HIP result 1.6e-3 to 1.7e-3 under the K|V gather on three ranks (unit boundaries fall elsewhere) and 0 behind the all-to-all
and on the other worlds of the tiny model, where a rank's call walks the same tiles in the same order."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_at_cases as A  # noqa: E402
import test_sp_gpu as SP  # noqa: E402
from test_attn_window_gpu import REL_RMS, _check_model  # noqa: E402
from test_sp_gpu import _wide_cfg, rel_rms, run_world  # noqa: E402
from oracle import cases as C  # noqa: E402
from oracle import dit as O  # noqa: E402

pytestmark = pytest.mark.gpu

LOGIT_STD = 3.0
T_TINY = 64
MASKS = {"frames": dict(window_frames=(1, 0), window_sink=64), "tokens": dict(window_size=(100, 37), window_sink=70)}
REFUSAL = "under sequence parallelism is not served: a rank's queries and the keys it gathers carry global token indices"
# (world, heads or False = DIT_TINY, mask, mode, extra switches).  Modes as tests/test_sp_gpu.py spells them (set_mode_env).
SW = {"FLEXAM_SP_WINDOW": "1"}
SAGE_SW = dict(SW, FLEXAM_SAGE_WINDOW="1")
CASES = [
    (2, False, "frames", "allgather-wait-p1", SW), (2, False, "frames", "allgather-wait", SW), (2, False, "tokens", "allgather-wait", SW),
    (2, False, "tokens", "allgather", SW),                        # FLEXAM_SP_OVERLAP=1: warned about, the waited-for form runs
    (2, False, "frames", "allgather-rebound", SW), (2, False, "tokens", "allgather-rebound", SW),
    (2, False, "frames", "allgather-wait-p1-sage", SW),           # SAGE without FLEXAM_SAGE_WINDOW: the bf16 windowed gather
    (2, False, "frames", "allgather-wait-p1-sage", SAGE_SW),      # ... and with it: the record gather has no mask, the same
    (2, False, "frames", "allgather-wait-p1", {}),                # the switch unset: refused
    (3, False, "frames", "allgather-wait-p1", SW), (3, False, "tokens", "allgather-wait", SW), (3, False, "tokens", "allgather-rebound", SW),
    (3, 3, "tokens", "ulysses-ov0", SW), (3, 3, "frames", "ulysses-ov1", SW),      # 258 padded rows of a head against 256 keys
    (4, 4, "frames", "ulysses-ov0", SW), (4, 4, "tokens", "ulysses-ov1", SW), (4, 4, "tokens", "allgather-wait", SW),
    (4, 4, "frames", "ulysses-ov0-sage", SW), (4, 4, "frames", "ulysses-ov0-sage", SAGE_SW),
]


def _key(case):
    world, heads, mask, mode, env = case
    return (heads, mask, mode, tuple(sorted(env.items())))


def _ids(cases):
    return [f"w{c[0]}-h{c[1] or 2}-{c[2]}-{c[3]}" + "".join("+" + k.split("_", 1)[1].lower() for k in sorted(c[4])) for c in cases]


def _cfg(heads):
    return _wide_cfg(heads) if heads else dict(O.DIT_TINY)


def _weights(cfg):
    sd = C.dit_weights(cfg, 7)
    C.scale_self_attention_logits(sd, LOGIT_STD)
    return sd


def _build(cfg, mask, devname="cuda:0"):
    from flexam_amd import Wan2_2Transformer3DModel_FlexAM
    kw = dict(cfg)
    kw.pop("eps")
    m = Wan2_2Transformer3DModel_FlexAM(**kw, **MASKS[mask])
    m.load_state_dict(_weights(cfg), strict=True)
    return m.to(devname)


def _inputs(cfg, devname="cuda:0"):
    case = C.dit_case(cfg, 41)
    return {k: ([u.to(devname) for u in v] if isinstance(v, list) else (v.to(devname) if torch.is_tensor(v) else v)) for k, v in case.items()}


SWITCHES = ("FLEXAM_SP_WINDOW", "FLEXAM_SAGE_WINDOW", "VIDEOX_ATTENTION_TYPE")


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
                DiTEngine._sp_window_overlap_warned = DiTEngine._sage_window_warned = False
                cfg = _cfg(heads)
                m = _build(cfg, mask)
                if "rebound" in mode:
                    SP._rebind_and_wrap(m)
                m.enable_multi_gpus_inference(cfg_parallel=False)
                d = _inputs(cfg)
                with warnings.catch_warnings(record=True) as seen:
                    warnings.simplefilter("always")
                    first = m(**d).float().cpu()
                    eng = m.engine()
                    facts = dict(sp=eng.sp_size, sp_mode=eng.sp_mode, fused=eng.fused, sage=bool(eng.sage_taken), replayed_first=bool(eng.replay_taken))
                    second = m(**d).float().cpu()
                    facts.update(replayed_second=bool(eng.replay_taken), second_equal=bool(torch.equal(first, second)),
                                 warnings=[str(w.message) for w in seen if issubclass(w.category, RuntimeWarning)])
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
    """(output, facts of rank 0) of a case, every rank's output the same bits."""
    res = [r[_key(case)] for r in _world(case[0])]
    for r in res:
        assert not isinstance(r, str), r
    for out, facts in res[1:]:
        torch.testing.assert_close(res[0][0], out, rtol=0, atol=0)
        assert facts == dict(res[0][1], warnings=facts["warnings"])
    return res[0]


def _mask_of(mask, rows=range(256)):
    kw = MASKS[mask]
    if "window_frames" in kw:
        return A.allowed(rows, 256, kw["window_frames"], T_TINY, kw["window_sink"])
    return A.allowed(rows, 256, kw["window_size"], 0, kw["window_sink"])


def _oracle(sd, cfg, case, ok):
    """The oracle's forward with its self-attention masked by `ok` [L, L] (cross-attention calls the same function: told apart by Lq == Lk)."""
    plain = O.attention

    def masked(q, k, v, k_lens=None):
        if q.shape[1] != k.shape[1]:
            return plain(q, k, v, k_lens)
        qt, kt, vt = (u.float().transpose(1, 2) for u in (q, k, v))
        s = qt @ kt.transpose(-1, -2) / q.shape[-1] ** 0.5
        return (s.masked_fill(~ok, float("-inf")).softmax(-1) @ vt).transpose(1, 2)

    mp = pytest.MonkeyPatch()
    mp.setattr(O, "attention", masked)
    try:
        return O.dit_forward(sd, cfg, **case)
    finally:
        mp.undo()


_WANT = {}


def _want(heads, mask):
    """The masked oracle's output for a width and a mask, once.  For DIT_TINY also the proof that the test is not blind to the offset."""
    if (heads, mask) not in _WANT:
        cfg = _cfg(heads)
        sd, case = _weights(cfg), C.dit_case(cfg, 41)
        want = _oracle(sd, cfg, case, _mask_of(mask))
        if not heads:
            blind = torch.cat([_mask_of(mask, range(128)), _mask_of(mask, range(128))])      # rank 1 of 2 masked as if its offset were 0
            moved = rel_rms(_oracle(sd, cfg, case, blind), want)
            print(f"oracle, {mask}: rank 1's rows masked at offset 0 move the output by rel-rms {moved:.3e}")
            assert moved > 3 * REL_RMS, (mask, moved)
        _WANT[heads, mask] = want
    return _WANT[heads, mask]


_SINGLE = {}


def _single(heads, mask, rebound=False, sage_window=False):
    """The single-process windowed HIP result of the same model: this code at offset 0."""
    key = (heads, mask, rebound, sage_window)
    if key not in _SINGLE:
        mp = pytest.MonkeyPatch()
        try:
            for name in SWITCHES:
                mp.delenv(name, raising=False)
            if sage_window:
                mp.setenv("VIDEOX_ATTENTION_TYPE", "SAGE_ATTENTION")
                mp.setenv("FLEXAM_SAGE_WINDOW", "1")
            cfg = _cfg(heads)
            m = _build(cfg, mask)
            if rebound:
                SP._rebind_and_wrap(m)
            with torch.no_grad():
                _SINGLE[key] = m(**_inputs(cfg)).float().cpu()
            assert m.engine().fused != rebound and bool(m.engine().sage_taken) == sage_window
        finally:
            mp.undo()
    return _SINGLE[key]


SERVED = [c for c in CASES if c[4]]


@pytest.mark.parametrize("case", SERVED, ids=_ids(SERVED))
def test_windowed_model_under_sequence_parallelism_matches_the_masked_oracle(case):
    world, heads, mask, mode, env = case
    out, facts = _result(case)
    name = _ids([case])[0]
    sage_kept = "-sage" in mode and "FLEXAM_SAGE_WINDOW" in env and mode.startswith("ulysses")
    assert facts["sp"] == world and facts["sp_mode"] == mode.split("-")[0] and facts["fused"] == ("rebound" not in mode) and facts["sage"] == sage_kept
    if sage_kept:
        # the windowed MXFP8 kernel on the rank's heads, one length: against the same kernel on one rank (the same quantisation of the same
        # rows, only the bf16 hop through the exchange differs), as tests/test_sp_gpu.py holds the unmasked SAGE layouts
        rel = rel_rms(out, _single(heads, mask, sage_window=True))
        print(f"{name}: vs single-process windowed MXFP8 rel-rms {rel:.2e}")
        assert rel < 4e-3 and not torch.equal(out, _result((world, heads, mask, mode, SW))[0])
    else:
        _check_model(out, _want(heads, mask), name)
        rel = rel_rms(out, _single(heads, mask, rebound="rebound" in mode))
        print(f"{name}: vs single-process windowed HIP rel-rms {rel:.2e}")
        assert rel < 4e-3
    # launch plan: the second forward of the fused engine is replayed, bit-equal either way
    assert facts["second_equal"] and not facts["replayed_first"] and facts["replayed_second"] == facts["fused"]
    said = [w for w in facts["warnings"] if "FLEXAM_SP_OVERLAP" in w]
    assert len(said) == (1 if mode == "allgather" else 0), facts["warnings"]
    said = [w for w in facts["warnings"] if "SAGE_ATTENTION is ignored with window_size / window_frames" in w]
    assert len(said) == (1 if "-sage" in mode and not sage_kept else 0), facts["warnings"]


def test_the_overlap_switch_and_the_sage_switches_change_no_bit_of_the_gather():
    waited, _ = _result((2, False, "tokens", "allgather-wait", SW))
    assert torch.equal(_result((2, False, "tokens", "allgather", SW))[0], waited)
    one_piece, _ = _result((2, False, "frames", "allgather-wait-p1", SW))
    for env in (SW, SAGE_SW):
        assert torch.equal(_result((2, False, "frames", "allgather-wait-p1-sage", env))[0], one_piece)
    # without FLEXAM_SAGE_WINDOW the all-to-all runs the bf16 windowed kernel as well
    assert torch.equal(_result((4, 4, "frames", "ulysses-ov0-sage", SW))[0], _result((4, 4, "frames", "ulysses-ov0", SW))[0])


def test_with_the_switch_unset_the_forward_raises_the_existing_message():
    for r in _world(2):
        got = r[_key((2, False, "frames", "allgather-wait-p1", {}))]
        assert isinstance(got, str) and got.startswith("NotImplementedError: flexam_amd: window_frames " + REFUSAL), got
