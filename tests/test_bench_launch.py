"""`python bench.py --gpus N` as the driver calls it (no torch.distributed.run environment): the parent starts the N ranks
itself without touching the GPU, forwards rank 0's JSON line and carries the self-check of the multi-rank exchange.
CPU: the launcher's refusal path, and --emulate-rank refused without --full.  GPU (one device): two and four ranks share cuda:0 under gloo -- the rank code path RCCL
drives on a multi-GPU node; such a line is marked invalid as a measurement, its `check` is real."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--frames", "9", "--height", "256", "--width", "256", "--layers", "2", "--steps", "2", "--warmup", "1", "--no-vae", "--no-cpu-baseline",
         "--no-kernel-timing"]


def _run(args, env_extra, timeout=900):
    env = dict(os.environ, **env_extra)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True, text=True, timeout=timeout)


def test_launcher_refuses_more_ranks_than_gpus_without_touching_them():
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("this host has the GPUs: nothing to refuse")
    r = _run(["--gpus", "2", *SMALL], {"FLEXAM_BENCH_ONE_DEVICE": "0"}, timeout=300)
    assert r.returncode != 0
    assert "--gpus 2 but only" in (r.stderr + r.stdout)


@pytest.mark.gpu
@pytest.mark.parametrize("world,env", [(2, {}), (4, {}), (4, {"FLEXAM_CFG_PARALLEL": "0"}), (4, {"FLEXAM_SP_MODE": "ulysses"})])
def test_bench_spawns_its_own_ranks_and_validates_the_exchange(world, env):
    r = _run(["--gpus", str(world), *SMALL], {"FLEXAM_BENCH_ONE_DEVICE": "1", "FLEXAM_BENCH_BACKEND": "gloo", **env})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == world and res["launch"]["attempt"] == "default" and not res["launch"]["fallback"]
    chk = res["check"]
    print(world, env, res["config"]["parallelism"], chk)
    assert chk["ok"] and chk["ranks_agree"] and chk["ranks"] == world and chk["worst_rank_rel_rms"] <= chk["tolerance"]
    assert "invalid" in res and "code-path validation" in res["invalid"]      # one device / gloo: not a measurement
    assert res["finite"]
    if world >= 4 and not env:             # nothing pinned: two steps of every candidate layout were timed and the fastest one ran
        lp = res["layout_probe"]
        assert len(lp["candidates"]) == 5 and lp["chosen"] in [c["layout"] for c in lp["candidates"]]
        assert all(c["ms_per_step"] > 0 and c["wall_sec"] > 0 for c in lp["candidates"])
        assert lp["communicators"] <= 3, lp                 # world + the two CFG halves, however many layouts were selected
    else:
        assert "layout_probe" not in res


@pytest.mark.gpu
def test_launcher_falls_back_to_the_conservative_exchange_when_the_check_fails():
    """A failed self-check of the first attempt (forced here) must cost one more attempt with FLEXAM_SP_PIECES=1 FLEXAM_SP_OVERLAP=0,
    not the measurement: the forwarded line is the second attempt's, says so, and keeps the first attempt's verdict."""
    r = _run(["--gpus", "4", *SMALL], {"FLEXAM_BENCH_ONE_DEVICE": "1", "FLEXAM_BENCH_BACKEND": "gloo", "FLEXAM_BENCH_TEST_HOOKS": "1", "FLEXAM_BENCH_FORCE_CHECK_FAIL": "1", "FLEXAM_BENCH_LAYOUT_FORCE": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["launch"]["fallback"] and res["launch"]["attempt"].startswith("FLEXAM_SP_PIECES=1")
    first = res["launch"]["earlier_attempts"][0]
    assert first["attempt"] == "default" and first["check"]["ok"] is False and first["check"]["ranks_agree"]
    assert res["check"]["ok"] and "waited for before attention" in res["config"]["parallelism"]


def _torchrun(world, args, env_extra, timeout=900):
    """The other way the driver may start it: `python -m torch.distributed.run ... bench.py --gpus N` (ranks are not bench.py's children)."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, **env_extra)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "FLEXAM_BENCH_SPAWNED"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(world), *args]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.gpu
def test_ranks_started_by_torchrun_remeasure_on_the_conservative_exchange_when_the_check_fails():
    """Under the caller's own torch.distributed.run there is no parent to start a second attempt: a failed self-check (forced) makes the
    SAME processes switch to FLEXAM_SP_PIECES=1 FLEXAM_SP_OVERLAP=0, measure again and check again; the line keeps the first verdict."""
    r = _torchrun(4, SMALL, {"FLEXAM_BENCH_ONE_DEVICE": "1", "FLEXAM_BENCH_BACKEND": "gloo", "FLEXAM_BENCH_TEST_HOOKS": "1", "FLEXAM_BENCH_FORCE_CHECK_FAIL": "1", "FLEXAM_BENCH_LAYOUT_FORCE": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["launch"]["fallback"] and res["launch"]["attempt"].startswith("FLEXAM_SP_PIECES=1")
    first = res["launch"]["earlier_attempts"][0]
    assert first["attempt"] == "default" and first["check"]["ok"] is False and first["ms_per_step"] > 0
    par = res["config"]["parallelism"]          # the conservative form of whichever layout the probe had picked
    assert res["check"]["ok"] and res["check"]["ranks_agree"]
    assert "waited for before attention" in par or par.rstrip().endswith("all-to-all over heads (q|k|v out, attention output back)")
    r = _torchrun(2, SMALL, {"FLEXAM_BENCH_ONE_DEVICE": "1", "FLEXAM_BENCH_BACKEND": "gloo"})       # and the plain case: no launch object, check ok
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln][0])
    assert "launch" not in res and res["check"]["ok"] and res["n_gpus"] == 2


@pytest.mark.gpu
def test_bench_under_rccl_when_the_box_has_two_gpus():
    """The driver's own multi-GPU command on real devices (skipped on one-GPU boxes): two ranks, RCCL, the self-check, no fallback."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    # (never executed in any build round -- no such box: like tests/test_nccl_gpu.py a failure of this FIRST contact is reported as XFAIL
    #  with its reason instead of stopping a `pytest -x` run; FLEXAM_TEST_NCCL_STRICT=1 makes it a failure)
    try:
        r = _run(["--gpus", "2", *SMALL], {"HSA_ENABLE_IPC_MODE_LEGACY": "0"})
        assert r.returncode == 0, r.stderr[-3000:]
        res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
        assert res["n_gpus"] == 2 and res["rccl_ranks"] == 2 and res["check"]["ok"] and "invalid" not in res
    except Exception as e:                                   # noqa: BLE001
        if os.environ.get("FLEXAM_TEST_NCCL_STRICT") == "1":
            raise
        pytest.xfail(f"first execution under real RCCL failed -- {type(e).__name__}: {str(e)[-1500:]}")


@pytest.mark.gpu
def test_probe_skips_a_candidate_that_raises_or_blows_its_budget_and_goes_on():
    """r3 verdict item 4: a candidate that raises is recorded in layout_probe.skipped and the probe continues (test hook: candidate 1
    raises a RuntimeError on every rank); a first step over the budget skips the candidate too -- with a zero budget nothing is
    measured, the default layout runs, and the line still carries a passed self-check."""
    base = {"FLEXAM_BENCH_ONE_DEVICE": "1", "FLEXAM_BENCH_BACKEND": "gloo", "FLEXAM_BENCH_TEST_HOOKS": "1"}
    r = _run(["--gpus", "4", *SMALL], {**base, "FLEXAM_BENCH_PROBE_RAISE": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    lp = res["layout_probe"]
    assert len(lp["candidates"]) == 4 and len(lp["skipped"]) == 1 and "RuntimeError" in lp["skipped"][0]["error"]
    assert lp["chosen"] in [c["layout"] for c in lp["candidates"]] and res["check"]["ok"] and lp["communicators"] <= 3
    r = _run(["--gpus", "4", *SMALL], {**base, "FLEXAM_BENCH_PROBE_BUDGET": "0"})
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    lp = res["layout_probe"]
    assert lp["candidates"] == [] and len(lp["skipped"]) == 5 and lp["chosen"].startswith("none measured")
    assert res["check"]["ok"] and res["config"]["parallelism"].startswith("cfg2 x sp2")


@pytest.mark.gpu
def test_probe_retries_a_candidate_whose_first_touch_was_over_budget():
    """Round-4 advice: the first candidate that touches a communicator can exceed the first-step budget for reasons that have nothing
    to do with its step time (lazy communicator set-up on a cold node).  The budget now covers denoise_step(0) only, and a candidate
    that is over it is measured once more at the end (test hook: candidate 0 sleeps past a 2 s budget on its first try only)."""
    r = _run(["--gpus", "4", *SMALL], {"FLEXAM_BENCH_ONE_DEVICE": "1", "FLEXAM_BENCH_BACKEND": "gloo", "FLEXAM_BENCH_TEST_HOOKS": "1",
                                      "FLEXAM_BENCH_PROBE_SLOW_FIRST": "0", "FLEXAM_BENCH_PROBE_BUDGET": "2"})
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    lp = res["layout_probe"]
    assert len(lp["candidates"]) == 5 and "skipped" not in lp, lp
    retried = [c for c in lp["candidates"] if c["retried"]]
    assert len(retried) == 1 and retried[0]["layout"].startswith("cfg2 x sp2, K|V all-gather") and lp["candidates"][-1] is not None
    assert lp["budget_covers"].startswith("denoise_step(0) only") and res["check"]["ok"]


@pytest.mark.gpu
def test_one_gpu_line_carries_an_emulated_rank_of_four():
    """`bench.py --emulate-rank N` on one GPU: one rank's share of an N-GPU step per layout through the real engine, collectives as
    same-size device copies (flexam_amd.dist.LoopbackGroup); the line keeps its single-GPU measurement and gains `emulated_ranks`."""
    r = _run(["--gpus", "1", *[a for a in SMALL if a != "--no-vae"], "--no-clip", "--full", "--emulate-rank", "4"], {})
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    em = res["emulated_ranks"]
    assert res["n_gpus"] == 1 and "invalid" not in res and em["world"] == 4
    # with the VAE timed: the clip one rank would see -- its share of the 8 conditioning streams, 50 rank steps, its tile of the decode
    cp = em["predicted_sec_per_clip_no_comm"]
    # (no size relation asserted: at this debug size every part is launch-bound)
    assert cp["vae_decode_tile_sec"] > 0 and cp["vae_encode_sec"] > 0 and set(cp["per_layout"]) == {row["layout"] for row in em["layouts"]}
    assert all(v > 0 for v in cp["per_layout"].values()) and cp["single_gpu_sec_per_clip"] > 0
    names = [row["layout"] for row in em["layouts"]]
    assert names[0].startswith("cfg2 x sp2, K|V all-gather") and names[1].startswith("cfg1 x sp4, all-to-all over heads")
    assert names[2].startswith("cfg2 x sp2, all-to-all over heads") and "FLEXAM_SP_OVERLAP=1" in names[3] and "FLEXAM_SP_OVERLAP=2" in names[4] and len(names) == 5
    assert all(row["host_share_of_step"] > 0 and row["ms_per_step_compute_only"] > 0 for row in em["layouts"])
    assert set(em["predicted_scaling_compute_only"]) == set(names) and "idle" in em["host_enqueue_note"]
    assert any(row["replayed_launches"] for row in em["layouts"])            # launch plans: the timed steps re-issue the recorded launches
    # the link model: the same rank steps with every collective holding its side stream for bytes-per-link / an assumed rate
    lt = em["predicted_scaling_at_link_GBps"]
    assert set(lt) == set(names) and "ASSUMED" in em["link_time_note"]
    for row in em["layouts"]:
        at = row["ms_per_step_at_link_GBps"]
        assert set(at) == {"50", "75"} and at["50"] > 0 and at["75"] > 0      # (a debug-size step is launch-bound: nothing to compare the legs with)
    row = em["layouts"][0]
    assert row["sp_size"] == 2 and row["cfg_size"] == 2 and row["samples_per_rank"] == 1 and row["tokens_per_rank"] * 2 == 256 and row["ms_per_step"] > 0
    row = em["layouts"][1]
    assert row["sp_size"] == 4 and row["cfg_size"] == 1 and row["samples_per_rank"] == 2 and row["tokens_per_rank"] * 4 == 256 and row["ms_per_step"] > 0
    assert set(em["predicted_scaling_no_comm"]) == set(names) and "NOT a multi-GPU measurement" in em["what"]
    # and without the flag a debug-size run (not the headline workload) does not emulate, not even under --full
    r = _run(["--gpus", "1", *SMALL, "--full"], {})
    assert r.returncode == 0 and "emulated_ranks" not in json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])


def test_emulate_rank_needs_full():
    """An emulated rank runs after the timed region, which a plain run leaves out: asking for one without --full is refused before
    any GPU work, never silently dropped."""
    r = _run(["--gpus", "1", *SMALL, "--emulate-rank", "4"], {}, timeout=300)
    assert r.returncode != 0
    assert "--emulate-rank runs after the timed region: it needs --full" in r.stderr


FULL_ONLY = ("host_enqueue_ms_per_step", "configs1_same_process", "roofline", "kernels", "cpu_baseline", "emulated_ranks", "vae_decode_sec",
             "vae_encode_sec_per_stream", "conditioning_encode_sec_8_streams", "conditioning_raster", "clip_end_to_end", "sec_per_clip",
             "sec_per_clip_from_tracks")


@pytest.mark.gpu
def test_plain_line_is_lean_and_full_adds_the_rest():
    """A plain run measures only its headline: with none of the --no-* switches it still times no kernels, runs no CPU baseline, VAE,
    rasteriser or clip, and (for a --mask line) no configs[1] steps.  --full brings all of them back into the same line."""
    r = _run(["--gpus", "1", *[a for a in SMALL if not a.startswith("--no-")], "--mask", "blob"], {})
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert res["finite"] and res["steps"] == 2 and res["warmup"] == 1 and res["ms_per_step"] * res["value"] == pytest.approx(1e3)
    assert res["metric"] == "denoise-steps/sec" and res["unit"] == "denoise-steps/sec" and res["higher_is_better"] and res["dtype"] == "bf16"
    assert not [k for k in FULL_ONLY if k in res], res
    r = _run(["--gpus", "1", *[a for a in SMALL if not a.startswith("--no-")], "--full"], {})
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert res["finite"] and res["host_enqueue_ms_per_step"] > 0
    assert res["kernels"] and res["roofline"] and res["cpu_baseline"]["value"] > 0 and res["cpu_baseline"]["legs"]
    assert res["vae_decode_sec"] > 0 and res["conditioning_raster"]["sec"] > 0 and res["clip_end_to_end"]["finite"] and res["sec_per_clip"] > 0
    assert "emulated_ranks" not in res and "configs1_same_process" not in res       # debug size: not the headline; motion: no second config


@pytest.mark.gpu
def test_dump_outputs_holds_the_last_timed_step(tmp_path):
    """`bench.py --dump-outputs DIR`: the latents the last TIMED step returned, float32, as DIR/latents.npy.  One warm-up step + three timed
    steps and three warm-up steps + one timed step run the same step indices on the same seeded inputs, so they dump the same latents;
    the line counts exactly the timed steps and carries ms_per_step."""
    import numpy as np
    got = {}
    for warmup, steps in ((1, 3), (3, 1)):
        d = tmp_path / f"w{warmup}s{steps}"
        r = _run(["--gpus", "1", *SMALL, "--warmup", str(warmup), "--steps", str(steps), "--dump-outputs", str(d)], {})
        assert r.returncode == 0, r.stderr[-3000:]
        res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
        assert res["steps"] == steps and res["warmup"] == warmup and res["finite"]
        assert res["ms_per_step"] > 0 and res["ms_per_step"] * res["value"] == pytest.approx(1e3)
        assert res["dump_outputs"]["arrays"] == {"latents.npy": [48, 3, 16, 16]} and os.listdir(d) == ["latents.npy"]
        a = np.load(d / "latents.npy")
        assert a.dtype == np.float32 and np.isfinite(a).all() and a.nbytes <= 64 << 20
        got[(warmup, steps)] = a
    assert np.array_equal(got[(1, 3)], got[(3, 1)])


@pytest.mark.gpu
def test_logit_scale_line_says_what_it_measured():
    """`bench.py --logit-scale S`: norm_q / norm_k x sqrt(S) on the random-init model (peaked softmax rows); a variant line, never the headline."""
    r = _run(["--gpus", "1", *SMALL, "--logit-scale", "6"], {})
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert res["logit_scale"]["std_asked"] == 6.0 and "logits scaled to std ~6" in res["config"]["workload"] and "not the headline" in res["config"]["workload"]
    assert res["finite"] and "emulated_ranks" not in res
