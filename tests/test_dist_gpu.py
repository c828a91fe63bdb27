"""Multi-rank rehearsal of the distributed bench on one GPU: 2 ranks share cuda:0 (LIPA_SHARE_GPU=1)
over gloo (RCCL refuses two ranks on one device), so DDP's gradient-ready bucket hooks and the ZeRO-3
engine run with the real HIP kernels; the RCCL transport itself is exercised by the driver's 8-GPU run."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", ["ddp", "zero3"])
def test_bench_two_ranks_share_one_gpu(strategy):
    env = dict(os.environ, LIPA_DIST_BACKEND="gloo", LIPA_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0",
               PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--model", "qwen3-small",
                          "--steps", "2", "--warmup", "1", "--strategy", strategy, "--full", "--faithful-steps", "1",
                          "--selective-steps", "1", "--zero3-model", "qwen3-small", "--zero3-steps", "1"],
                         env=env, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["n_gpus"] == 2 and rec["config"]["dist_world_size"] == 2 and rec["config"]["dist_backend"] == "gloo"
    assert rec["value"] > 0 and rec["config"]["parallelism"].endswith("dp2")
    # gloo on one device: the wait is host time, no comm-stream events, so no overlap fraction (RCCL runs time both)
    ov = rec["comm"]["overlap_fraction"]
    assert rec["comm"]["exposed_ms_per_step"] >= 0 and (ov is None or 0.0 <= ov <= 1.0)
    if strategy == "zero3":      # the client 8-bit AdamW runs on each rank's partition (E6)
        assert rec["config"]["optimizer"] == "zero3-paged_adamw_8bit"
    else:                        # world > 1 DDP: config #4's sub-record (ZeRO-3 engine) with its collectives
        z = rec["zero3"]
        assert z["value"] > 0 and z["ms_per_step"] > 0 and "all_gather" in json.dumps(z["comm"]), z


def _zero3_losses(extra):
    env = dict(os.environ, LIPA_DIST_BACKEND="gloo", LIPA_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0",
               PYTHONPATH=ROOT)
    env.pop("LIPA_NF4_GEMM", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--model", "qwen3-small",
                          "--steps", "2", "--warmup", "1", "--strategy", "zero3", "--nf4-gemm", "w4", *extra],
                         env=env, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["config"]["nf4_gemm"] == "w4"
    return [float(x) for x in __import__("re").findall(r"loss=([0-9.]+)", out.stderr)]


@pytest.mark.gpu
def test_zero3_partitioned_nf4_bases_w4_match_replicated():
    """ZeRO-3 with the frozen NF4 bases partitioned across ranks (stage3_partition_frozen_quant) in the
    memory-lean w4 mode: the backward re-gathers the codes after release() and rebuilds the g4w pack —
    the losses match the replicated-base run."""
    rep = _zero3_losses([])
    part = _zero3_losses(["--ds-config", os.path.join(ROOT, "configs", "ds_zero3_nf4_partition.json")])
    assert len(rep) == len(part) == 2
    assert all(abs(a - b) <= 1e-3 * abs(b) for a, b in zip(part, rep)), (part, rep)
