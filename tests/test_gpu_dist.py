"""N > 1 on the device path without a multi-GPU node: two ranks share the one
GPU of the box (gloo transport, collectives staged through host memory) and run the device SMC and
parallel tempering of a small FFI problem; populations, betas and recorded likelihoods must equal
the 1-rank run BIT FOR BIT -- the proposal streams are keyed by the global chain id, the stage
decisions are computed identically on every rank.  On boxes with two GPUs the
same comparison runs over RCCL."""
import json
import os
import socket
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(nproc, backend, out):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(BEATAMD_TEST_BACKEND=backend, BEATAMD_TEST_OUT=out, OMP_NUM_THREADS="1")
    worker = os.path.join(ROOT, "tests", "_dist_gpu_worker.py")
    if nproc == 1:
        cmd = [sys.executable, worker]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), worker]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("DIST_GPU_WORKER_OK") == nproc, r.stdout[-2000:]
    return np.load(out)


def _compare(a, b):
    assert int(a["nstage_checks"]) == int(b["nstage_checks"]) >= 1
    for k in ("betas", "pop", "lp", "s", "ls", "scale"):
        assert np.array_equal(a[k], b[k]), k
    assert np.isfinite(a["lp"]).all() and a["pop"].shape[0] == 256 and a["s"].shape[0] == 128


def test_two_ranks_on_one_gpu_equal_one_rank(tmp_path):
    one = _run(1, "gloo", str(tmp_path / "w1.npz"))
    two = _run(2, "gloo", str(tmp_path / "w2.npz"))
    _compare(one, two)


def test_two_ranks_over_rccl_equal_one_rank(tmp_path):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs, found %d" % torch.cuda.device_count())
    one = _run(1, "nccl", str(tmp_path / "w1.npz"))
    two = _run(2, "nccl", str(tmp_path / "w2.npz"))
    _compare(one, two)


def _run_shard(nproc, mode, out, backend="gloo", **extra):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "BEATAMD_GF_SPLIT"):
        env.pop(k, None)
    env.update(BEATAMD_TEST_BACKEND=backend, BEATAMD_TEST_OUT=out, BEATAMD_TEST_MODE=mode, OMP_NUM_THREADS="1", **extra)
    worker = os.path.join(ROOT, "tests", "_shard_gpu_worker.py")
    if nproc == 1:
        cmd = [sys.executable, worker]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), worker]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("SHARD_GPU_WORKER_OK") == nproc, r.stdout[-2000:]
    return np.load(out)


def test_target_sharded_library_equals_the_replicated_model(tmp_path):
    """SURVEY 8(e) fallback: the seismic libraries sharded by TARGET over two ranks (3 + 2 targets; two
    ranks share the one GPU, gloo) -- every rank evaluates all chains on the rows of its targets, one all-gather per
    evaluation assembles the likelihood vectors.  Against the replicated one-rank model: every dataset's logpt and
    `like` BITWISE (each target's arithmetic does not depend on where the other targets live; `like` is summed from
    the gathered vector in the fused model's order), NaN for the chain outside the library grid; a one-rank sharded run
    and the two-rank run give the same SMC populations, likelihoods and betas (identical decisions on every rank); the
    replicated SMC run (fused step kernel) agrees to 1e-12 on the betas"""
    rep = _run_shard(1, "replicated", str(tmp_path / "rep.npz"))
    one = _run_shard(1, "targets", str(tmp_path / "s1.npz"))
    two = _run_shard(2, "targets", str(tmp_path / "s2.npz"))
    for sh in (one, two):
        assert sh["LL"].shape == rep["LL"].shape == (300, 9)
        assert np.array_equal(np.isnan(sh["LL"][:, -1]), np.isnan(rep["LL"][:, -1])) and np.isnan(rep["LL"][7, -1])
        ok = ~np.isnan(rep["LL"][:, -1])
        assert np.array_equal(sh["LL"][ok], rep["LL"][ok])
        np.testing.assert_allclose(sh["LL"][ok, -1], rep["LL"][ok, -1], rtol=1e-12)
    for k in ("pop", "lp", "betas"):
        assert np.array_equal(one[k], two[k]), k
    np.testing.assert_allclose(one["betas"], rep["betas"], rtol=1e-12)
    assert np.isfinite(two["lp"]).all() and two["pop"].shape[0] == 256


@pytest.mark.parametrize("interp", ["nearest_neighbor", "multilinear"])
def test_target_sharded_short_traces_keep_the_patch_ranges(tmp_path, interp):
    """A library of SHORT traces sharded by target: 40 targets x 128 patches x 120 samples, stacked in patch ranges
    (gfstack.hip launch_gfstack_split).  The ranges set the summation order over a target's patches; the replicated library
    picks R = 2, a block of 20 targets on its own would pick R = 4.  Every rank must stack in the replicated model's ranges,
    and every dataset's logpt and `like` must be BITWISE those of the replicated model (README), NaN for the
    chain outside the library grid"""
    env = dict(BEATAMD_TEST_SPEC="split", BEATAMD_TEST_INTERP=interp)
    rep = _run_shard(1, "replicated", str(tmp_path / "rep.npz"), **env)
    one = _run_shard(1, "targets", str(tmp_path / "s1.npz"), **env)
    two = _run_shard(2, "targets", str(tmp_path / "s2.npz"), **env)
    (rplan,) = rep["plans"]
    assert "stacked in 2 ranges of 64" in rplan, rplan
    want = rplan[rplan.index("patches stacked in"):].split(" (")[0]          # "patches stacked in 2 ranges of 64"
    for sh, n in ((one, 1), (two, 2)):
        assert len(sh["plans"]) == n
        for plan in sh["plans"]:
            assert want in plan, (want, plan)
        assert sh["LL"].shape == rep["LL"].shape == (300, 40 + 4)
        assert np.array_equal(np.isnan(sh["LL"][:, -1]), np.isnan(rep["LL"][:, -1])) and np.isnan(rep["LL"][7, -1])
        assert int(np.isnan(rep["LL"][:, -1]).sum()) == 1
        ok = ~np.isnan(rep["LL"][:, -1])
        for col in range(rep["LL"].shape[1]):
            assert np.array_equal(sh["LL"][ok, col], rep["LL"][ok, col]), (n, col)


def _bench(extra, env_extra, nproc_flag, full=False, legs_off=True):
    """one bench.py run at a reduced shape -> its line; `full`: with --full (the stage transition), `legs_off`: with the
    --no-* options of the legs"""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(env_extra)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(nproc_flag), "--steps", "4", "--warmup", "1",
           "--targets", "4", "--samples", "256"] + (["--full"] if full else []) + \
          (["--no-cpu-baseline", "--no-streaming-leg", "--no-batch-leg", "--no-narrow-leg", "--no-variant-legs"]
           if legs_off else []) + extra
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]          # rank 0 prints ONE line
    return json.loads(lines[0])


def test_bench_two_ranks_on_one_gpu_keeps_the_contract(tmp_path):
    """`bench.py --gpus 2` without a multi-GPU node -- the two ranks share the one GPU (gloo,
    collectives staged through host memory).  The driver's contract: n_gpus, global chains, value = all ranks'
    chain-steps over the slowest rank's time, a stage transition whose all-gather really had two ranks; and the
    gathered end points (proposal rows are seeded per block of 64 GLOBAL chains, the population per global chain)
    equal those of ONE rank stepping all 256 chains, bit for bit."""
    two = _bench(["--chains", "128"], {"BEATAMD_BENCH_BACKEND": "gloo"}, 2, full=True)
    one = _bench(["--chains", "256"], {}, 1, full=True)
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1 and two["steps"] == one["steps"] == 4
    assert two["config"]["global_chains"] == one["config"]["global_chains"] == 256
    assert two["config"]["chains_per_gpu"] == 128 and two["scaling"] == "weak"
    for d in (one, two):
        assert abs(d["value"] - d["config"]["global_chains"] * d["steps"] / (d["ms_per_step"] * 1e-3 * d["steps"])) \
            <= 1e-9 * d["value"]
        assert d["stage_transition_ms"] > 0 and d["stage_transition"]["gathered_chains"] == 256
    assert two["stage_transition"]["ranks_in_all_gather"] == 2 and two["stage_transition"]["backend"] == "gloo"
    assert two["stage_transition"]["population_checksum"] == one["stage_transition"]["population_checksum"]
    assert 0.0 < two["stage_transition"]["population_checksum"]["next_beta"] < 1.0


def test_bench_four_ranks_on_one_gpu(tmp_path):
    """the driver's multi-rank launch line beyond two ranks -- `bench.py --gpus 4` with all four ranks on the
    one GPU (gloo, reduced shape): seeds per block of 64 global chains (two blocks per rank), the stage all-gather over
    four ranks, value = all ranks' chain-steps over the slowest rank's time; the gathered end points equal those of ONE
    rank stepping all 512 chains bit for bit.  (Four ranks, not eight: the launcher's agent opens the GPU as well, so N
    ranks are N + 2 processes holding the device with this one; eight made ten, more than a shared node allows.)"""
    four = _bench(["--chains", "128"], {"BEATAMD_BENCH_BACKEND": "gloo"}, 4, full=True)
    one = _bench(["--chains", "512"], {}, 1, full=True)
    assert four["n_gpus"] == 4 and four["config"]["global_chains"] == one["config"]["global_chains"] == 512
    assert four["config"]["chains_per_gpu"] == 128 and four["scaling"] == "weak"
    assert four["stage_transition"]["ranks_in_all_gather"] == 4 and four["stage_transition"]["gathered_chains"] == 512
    assert four["stage_transition"]["backend"] == "gloo"
    assert four["stage_transition"]["population_checksum"] == one["stage_transition"]["population_checksum"]
    assert abs(four["value"] - 512 * four["steps"] / (four["ms_per_step"] * 1e-3 * four["steps"])) <= 1e-9 * four["value"]


def test_bench_dump_outputs_are_the_timed_path_end_state(tmp_path):
    """`bench.py --dump-outputs`: two runs with the same arguments write the same float64 arrays; one row per chain; the
    likelihood vectors are those of the dumped positions (the model re-evaluated here on the same seeded problem), the
    acceptance counts lie within the steps taken (warm-up + timed)"""
    import beat_amd
    import bench
    from beat_amd.synthetic import build_problem
    args = ["--chains", "128", "--steps", "3", "--warmup", "2", "--ndurations", "3", "--nstarttimes", "25"]
    runs = []
    for k in ("a", "b"):
        d = _bench(args + ["--dump-outputs", str(tmp_path / k), "--full-json", str(tmp_path / (k + ".json"))], {}, 1)
        assert d["steps"] == 3 and sum(json.load(open(str(tmp_path / (k + ".json"))))["region_steps"]) == 3
        runs.append({n: np.load(str(tmp_path / k / (n + ".npy"))) for n in ("positions", "likelihoods", "accepted")})
    a, b = runs
    for n in a:
        assert a[n].dtype == np.float64 and a[n].shape[0] == 128, n
        assert np.array_equal(a[n], b[n]), n
    assert ((a["accepted"] >= 0) & (a["accepted"] <= 5)).all() and a["accepted"].sum() > 0
    spec = bench.make_spec(SimpleNamespace(prior="survey", targets=4, samples=256, ndurations=3, nstarttimes=25,
                                           duration_min=0.5, duration_sampling=0.5, covariance="scalar",
                                           interp="nearest_neighbor"))
    ctx = beat_amd.get_context(0)
    prob, host = build_problem(spec, device_library=True, ctx=ctx)
    f = prob.compile(ctx)
    L = np.asarray(f.batch(a["positions"]))
    assert L.shape == a["likelihoods"].shape
    np.testing.assert_allclose(a["likelihoods"], L, rtol=1e-9, atol=1e-9)
    f.release()


def test_bench_plain_run_is_the_headline_alone(tmp_path):
    """`bench.py` without `--full` times the headline steps and nothing else: no CPU baseline, no stage transition, no
    labelled leg, although no --no-* option is given; `--full` adds the stage transition and the legs of the main library
    (the CPU baseline and the configuration legs left out here), and the timed path ends in the same arrays either way"""
    runs = {}
    for k, full in (("plain", False), ("full", True)):
        extra = ["--chains", "128", "--dump-outputs", str(tmp_path / k), "--full-json", str(tmp_path / (k + ".json"))]
        if full:
            extra += ["--no-cpu-baseline", "--no-variant-legs"]
        line = _bench(extra, {}, 1, full=full, legs_off=False)
        assert line["steps"] == 4 and line["warmup"] == 1 and line["roofline"]["kernel"]
        assert abs(line["value"] - 128 / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
        runs[k] = (line, json.load(open(str(tmp_path / (k + ".json")))))
    line, obj = runs["plain"]
    extras = ("cpu_baseline", "speedup_vs_cpu_baseline", "stage_transition", "stage_transition_ms", "roofline_streaming")
    assert not [k for k in obj if k in extras or k.endswith("_leg")], sorted(obj)
    assert line["legs"] == {} and "cpu_baseline" not in line and "stage_transition_ms" not in line
    line, obj = runs["full"]
    assert {"stage_transition", "roofline_streaming", "batch_2048_leg", "narrow_prior_leg"} <= set(obj), sorted(obj)
    assert line["stage_transition_ms"] > 0 and {"batch_2048", "narrow_prior"} <= set(line["legs"])
    for n in ("positions", "likelihoods", "accepted"):
        assert np.array_equal(np.load(str(tmp_path / "plain" / (n + ".npy"))), np.load(str(tmp_path / "full" / (n + ".npy")))), n
