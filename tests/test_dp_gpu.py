"""Data parallelism on the real kernels: two ranks (torchrun, one GPU shared through the gloo backend -- a 1-GPU box
cannot host two RCCL ranks) each run forward / fused losses / backward on their environment shard with the global 1/N normalisation
and SUM-all-reduce the flat gradient arena; the result must equal the single-process gradient over all environments."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    """a rendezvous port nobody holds (a fixed one collided once in a full-suite run: TIME_WAIT of an earlier test's store)"""
    import socket
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        return s_.getsockname()[1]


@pytest.mark.parametrize("backend", ["gloo", "rccl"])
def test_two_ranks_equal_single_process_gradient(tmp_path, backend):
    """backend "gloo": two ranks share the one GPU of the test box; "rccl": one rank per GPU over RCCL ("nccl" on ROCm) -- runs wherever
    at least two GPUs are visible (the 8-GPU scaling node), skipped on 1-GPU boxes."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if backend == "rccl" and torch.cuda.device_count() < 2:
        pytest.skip("RCCL needs one GPU per rank: fewer than 2 GPUs visible")
    T, B = 5, 4
    out = str(tmp_path / "dp.pt")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if backend == "gloo":
        env["SVLA_DIST_BACKEND"] = "gloo"
    else:
        env.pop("SVLA_DIST_BACKEND", None)
    port = _free_port()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "tests", "helpers", "dp_worker.py"), out, str(T), str(B)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    got = torch.load(out)
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import dp_worker

    m, eng, st = dp_worker.build(torch.device("cuda"), T, B)
    m.zero_grad()
    eng._sums.zero_()
    eng._accumulate(st.batch_slice(0, B), T * B, 0.25)
    want_g, want_s = m.arena.flat_g.cpu(), eng._sums.cpu()
    assert torch.allclose(got["sums"], want_s, rtol=1e-6, atol=1e-9), (got["sums"], want_s)
    # identical kernels on identical rows; only the fp32 accumulation order of the weight-gradient atomics / row split differs
    err = (got["flat_g"] - want_g).abs().max().item() / want_g.abs().max().item()
    assert err < 2e-3, err
    cos = torch.nn.functional.cosine_similarity(got["flat_g"].double(), want_g.double(), dim=0).item()
    assert cos > 0.99999, cos


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_bench_two_ranks_well_formed_line(scaling):
    """bench.py itself under two ranks (gloo: they share the test box's one GPU), launched the way the driver launches it for N > 1, so that
    the first real SCALE run cannot die on plumbing.  "strong": 7 envs sharded 4 + 3 -- uneven shards through the engine's single
    count all-reduce."""
    import json

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", SVLA_DIST_BACKEND="gloo")
    port = _free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--T", "8",
           "--envs-per-gpu", "4", "--full", "--no-cpu-baseline", "--no-secondary", "--scaling", scaling, "--global-envs", "7"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["rccl_ranks"] == 2 and out["scaling"] == scaling and out["steps"] == 1
    envs = 7 if scaling == "strong" else 8
    assert out["config"]["global_envs"] == envs and out["loss"]["env_steps"] == 8 * envs
    assert out["value"] > 0 and abs(out["value"] - 8 * envs / (out["ms_per_step"] * 1e-3)) < 1e-2 * out["value"]
    assert out["roofline"] is not None and "frac" in out["roofline"]


@pytest.mark.parametrize("variant", ["c4_fetch", "c5_mixed_fp8_bf16wire"])
def test_bench_eight_ranks_strong_scaling_fetch_plumbing(variant):
    """BASELINE configs[3] as the driver will launch it on the 8-GPU node -- `bench.py --gpus 8 --scaling strong --global-envs 250` under
    torch.distributed.run -- with the eight ranks sharing this box's one GPU through gloo (uneven shards: 250 = 2 x 32 + 6 x 31; three asynchronous
    per-tower all-reduces in flight on eight ranks; the single count all-reduce; the cost accumulator), short rollouts (T = 4).  RCCL itself needs
    one GPU per rank and has never run here; what this pins is everything else the first SCALE run of C4 could die on."""
    import json

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", SVLA_DIST_BACKEND="gloo")
    port = _free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "1", "--warmup", "1", "--T", "4",
           "--no-cpu-baseline", "--no-secondary", "--no-roofline", "--scaling", "strong"]
    # BASELINE configs[3] (Fetch, uneven shards) / configs[4] AS WRITTEN from the command line: mixed task sampler, 64-token instructions, 256 envs over the
    # eight ranks, fp8 MFMA attention in the headline run -- plus the bf16 gradient exchange, so that both new flags cross eight ranks once
    cmd += (["--global-envs", "250", "--task", "Fetch"] if variant == "c4_fetch" else
            ["--global-envs", "256", "--task", "Mixed", "--L", "64", "--fp8-attention", "--grad-allreduce-bf16", "--t5-dropout-per-row"])
    n_envs = 250 if variant == "c4_fetch" else 256
    torch.cuda.empty_cache()          # eight more processes are about to share this GPU with whatever this process has cached
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:             # eight ranks initialising HIP / gloo on ONE GPU at once is not what the code under test is about: one retry, the first error kept
        first = r.stderr[-1500:]
        cmd[cmd.index("--master-port") + 1] = str(_free_port())
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, "first attempt:\n" + first + "\nsecond attempt:\n" + r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["n_gpus"] == 8 and out["rccl_ranks"] == 8 and out["scaling"] == "strong"
    assert out["scaling_measured"] is False          # eight gloo ranks on one GPU are plumbing, not a point of a scaling curve
    assert out["config"]["global_envs"] == n_envs and out["loss"]["env_steps"] == 4 * n_envs
    if variant != "c4_fetch":
        c = out["config"]
        assert c["attention"].startswith("fp8") and c["grad_allreduce_dtype"] == "bf16" and c["t5_dropout"].startswith("per (t, b) row") and "configs[4]" in c["workload"]
    assert out["value"] > 0 and all(v == v for v in out["loss"].values() if isinstance(v, float))


def test_single_rank_through_rccl(tmp_path):
    """The RCCL code path EXECUTED on a 1-GPU box: ``SVLA_FORCE_DIST=1`` makes a single rank initialise the "nccl" (= RCCL) backend and send every
    exchange step of the engine through it -- communicator creation, the three asynchronous per-tower all-reduces of the fp32 gradient arena issued
    behind each tower's backward, the fp64 count / cost reductions, the broadcast of every parameter and buffer, the barrier.  With one rank every
    SUM is the identity, so the result must equal the non-distributed gradient of the same rows BIT FOR BIT (eval mode, same kernels, same order).
    What this cannot show is the xGMI exchange itself (that needs one GPU per rank: the "rccl" variant above)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    T, B = 5, 4
    out = str(tmp_path / "dp1.pt")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", SVLA_FORCE_DIST="1", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1",
               MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    env.pop("SVLA_DIST_BACKEND", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "dp_worker.py"), out, str(T), str(B), "--expect-backend", "nccl"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = torch.load(out)
    assert got["backend"] == "nccl" and got["world"] == 1 and got["pending"] == 3
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import dp_worker

    m, eng, st = dp_worker.build(torch.device("cuda"), T, B)
    m.zero_grad()
    eng._sums.zero_()
    eng._accumulate(st.batch_slice(0, B), T * B, 0.25)
    assert torch.allclose(got["sums"], eng._sums.cpu(), rtol=1e-6, atol=1e-9)
    # same rows, same kernels; only the arrival order of the fp32 weight-gradient atomics differs between two runs
    want_g = m.arena.flat_g.cpu()
    err = (got["flat_g"] - want_g).abs().max().item() / want_g.abs().max().item()
    assert err < 1e-4, err


def test_bench_single_rank_through_rccl():
    """bench.py with its one rank forced through RCCL (SVLA_FORCE_DIST=1): the collective pre-flight, the per-tower asynchronous all-reduces inside the
    timed update and the MAX-over-ranks clock all run on the "nccl" backend; the line says so (``collective_preflight.backend``)."""
    import json

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", SVLA_FORCE_DIST="1", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1",
               MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    env.pop("SVLA_DIST_BACKEND", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--T", "8", "--envs-per-gpu", "4",
           "--no-cpu-baseline", "--no-secondary", "--no-roofline"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["n_gpus"] == 1 and out["rccl_ranks"] == 1 and out["collective_preflight"]["backend"] == "nccl"
    assert out["collective_preflight"]["tower_ranges_checked"] == 3 and out["loss"]["env_steps"] == 32 and out["value"] > 0


def test_bench_plain_line_and_dump_outputs(tmp_path):
    """A plain bench run (no --full) prints the headline line without any of the --full legs, and --dump-outputs writes what its last timed update
    computed (float32 / float64, at most 64 MB); two runs with the same arguments (deterministic accumulation) write the same arrays."""
    import json

    import numpy as np

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--T", "8", "--envs-per-gpu", "4",
               "--deterministic", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        runs.append((line, {f.name[:-4]: np.load(f) for f in d.glob("*.npy")}))
    line, a = runs[0]
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["unit"] == "env-steps/s" and abs(line["value"] - 32 / (line["ms_per_step"] * 1e-3)) < 1e-2 * line["value"]
    assert all(line[k] is None for k in ("roofline", "cpu_baseline", "acting", "collect_then_update", "north_star_batch256", "secondary"))
    assert "parity_ok" not in line
    assert {"params", "grads", "returns", "c_returns", "adv_targ", "c_adv_targ", "info_ppo_total", "info_lagrangian_multiplier", "info_env_steps"} <= set(a)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["returns"].shape == (8, 4, 1) and a["info_env_steps"][0] == 32 and a["params"].shape == a["grads"].shape and (a["grads"] != 0).any()
    b = runs[1][1]
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]) if not k.startswith("info_") else np.allclose(a[k], b[k], rtol=1e-6, atol=1e-9), k
